"""Dense constraint matrices, CPU side: the generator is pinned by sha256, the
host classifies every (constraint, cone) coefficient by the reference's strict 10 % rule, and the
plain-C restatement (oracle/) reproduces the reference's own dense branches on the new fixtures
(scripts/make_golden_densea.py) -- a third summation order next to the reference's BLAS and the
device's tiles, at the project's 1e-9 bar."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from densea_util import EXPECT_DENSE, da_path, dense_a, meta
from golden_util import GOLDEN, rel_err, split_inputs, split_outputs

NAMES = ["da64", "da70x40", "da200"]


@pytest.fixture(scope="module")
def gen_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("densea")


@pytest.mark.parametrize("name", NAMES)
def test_generator_is_pinned(gen_dir, name):
    path = da_path(name, gen_dir)   # asserts the sha256
    g = meta()[name]
    with open(path) as f:
        assert int(f.readline()) == g["m"]
        f.readline()
        assert [int(x) for x in f.readline().split()] == g["dims"]


def test_boundary_fill_has_exactly_floor_entries(gen_dir):
    """f = 0.1 takes exactly floor(0.1 T) positions: not more than 10 %, so it stays sparse."""
    inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")
    from densea_util import args_of
    m, dims, b, entries = inst.dense_constraints_problem(**args_of("da70x40"))
    T = dims[0] * (dims[0] + 1) // 2
    cnt = sum(int(np.sum((np.asarray(c) == m) & (np.broadcast_to(bk, np.shape(c)) == 1))) for c, bk, *_ in entries)
    assert cnt == int(np.floor(0.1 * T)) and not cnt > 0.1 * T


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", ["0", "1"])
def test_host_classification(gen_dir, name, mode):
    """lrs_dense_a_plan (host only): the dense coefficients per cone by the reference's rule --
    the 0.1-boundary constraint and the cross constraint's five entries in cone 1 come out
    sparse -- and the path LRS_DENSE_A selects."""
    solver = importlib.import_module("ltr-lowrank-sdp_amd.solver")
    path = da_path(name, gen_dir)
    with dense_a(mode):
        for cone, want in enumerate(EXPECT_DENSE[name]):
            cons, on = solver.dense_a_plan(path, cone)
            assert cons == want, (cone, cons)
            assert on == (mode == "1" and len(want) > 0)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_alm_steps_match_reference(oracle_lib, gen_dir, name):
    z = np.load(os.path.join(GOLDEN, f"steps_{name}.npz"))
    path = da_path(name, gen_dir)
    lib = oracle_lib
    lib.oracle_alm_steps.restype = C.c_long
    lib.oracle_alm_steps.argtypes = [C.c_char_p, C.c_int, C.c_long, C.POINTER(C.c_double), C.c_long]
    nr, m = int(z["nr"]), int(z["m"])
    for K in [int(k) for k in z["ks"]]:
        assert z[f"K{K}_trips"].shape[0] == K
        out = np.zeros(2 * nr + 2 * m)
        got = lib.oracle_alm_steps(path.encode(), int(z["rank_flag"]), K, out.ctypes.data_as(C.POINTER(C.c_double)),
                                   out.size)
        assert got == nr, (K, got)
        errs = {"R": rel_err(out[:nr], z[f"K{K}_R"]), "G": rel_err(out[nr:2 * nr], z[f"K{K}_G"]),
                "cvs": rel_err(out[2 * nr:2 * nr + m], z[f"K{K}_cvs"])}
        print(name, K, errs)
        for key, e in errs.items():
            assert e < 1e-9, (K, key, e)


@pytest.mark.parametrize("name", ["da64", "da70x40"])
def test_oracle_kernels_match_reference(oracle_lib, gen_dir, name):
    z = np.load(os.path.join(GOLDEN, f"kernels_{name}.npz"))
    g = {k: z[k] for k in z.files}
    s = split_inputs(g)
    p = oracle_lib.oracle_read(da_path(name, gen_dir).encode())
    assert p, "oracle_read failed"
    inp = np.ascontiguousarray(g["inputs"], dtype=np.float64)
    out = np.zeros(inp.size * 2 + 1024)
    n = oracle_lib.oracle_kernels(p, s["rank"], inp.ctypes.data_as(C.POINTER(C.c_double)),
                                  out.ctypes.data_as(C.POINTER(C.c_double)))
    oracle_lib.oracle_free(p)
    o = split_outputs(out[:n], s["m"], s["NR"], s["dims"][0] * s["rank"])
    for key in ["q1", "q2", "cvs_rr", "grad", "rhs_cg"]:
        e = rel_err(o[key], g[key])
        print(name, key, e)
        assert e < 1e-9, (key, e)
    for key in ["p1", "p2", "pobj_rr", "pinf_rr", "lag", "tau"]:
        assert abs(o[key] - g[key]) <= 1e-9 * max(1.0, abs(g[key])), key
    assert o["rootnum"] == g["rootnum"]

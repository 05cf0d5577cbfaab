"""Rank-one dense constraint matrices, CPU side: the generator is pinned by
sha256, the host detects A = sigma a a^T among the coefficients the reference's rule types dense
(lrs_rank1_plan: pivot on the largest |A_pp|, residual bar 1e-13 max|A|) and nothing else, and the
plain-C restatement (oracle/) reproduces the reference's own dense branches on the new step
fixtures (scripts/make_golden_rank1.py) at the project's 1e-9 bar."""
import ctypes as C
import importlib

import numpy as np
import pytest

from golden_util import GOLDEN, rel_err
from rank1_util import EXPECT_DENSE, EXPECT_RANK1, EXPECT_SIGMA, args_of, env, meta, r1_path

import os

NAMES = ["r1_64", "r1_70x37", "r1_200"]


@pytest.fixture(scope="module")
def gen_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("rank1")


@pytest.fixture(scope="module")
def solver_mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.solver")


@pytest.mark.parametrize("name", NAMES)
def test_generator_is_pinned(gen_dir, name):
    path = r1_path(name, gen_dir)   # asserts the sha256
    g = meta()[name]
    with open(path) as f:
        assert int(f.readline()) == g["m"]
        f.readline()
        assert [int(x) for x in f.readline().split()] == g["dims"]


def test_generator_terms_and_boundary():
    """The term list matches the expansion; the hole term is still more than 10 % fill; the
    boundary term holds the largest rank-one pattern within floor(0.1 T) entries."""
    inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")
    (m, dims, b, entries), terms = inst.rank_one_constraints_problem(**args_of("r1_70x37"))
    (m2, _, b2, entries2), terms2 = inst.rank_one_constraints_problem(**args_of("r1_70x37"), expand=False)
    assert m == m2 and np.array_equal(b, b2) and len(entries2) == len(entries) - len(terms)
    n = dims[0]
    T = n * (n + 1) // 2
    for (con, blk, sigma, a), (_, _, _, a2) in zip(terms, terms2):
        assert np.array_equal(a, a2)
        cnt = sum(int(np.sum((np.asarray(c) == con) & (np.broadcast_to(bk, np.shape(c)) == 1))) for c, bk, *_ in entries)
        z = int(np.count_nonzero(a))
        assert cnt == z * (z + 1) // 2
        if con == m:   # the boundary term
            assert cnt <= np.floor(0.1 * T) < (z + 1) * (z + 2) // 2 and not cnt > 0.1 * T
        else:
            assert cnt > 0.1 * T
    hole = terms[args_of("r1_70x37")["hole"]][3]
    assert abs(np.count_nonzero(hole == 0.0) - 0.33 * n) <= 1


@pytest.mark.parametrize("name", NAMES)
def test_rank1_plan(solver_mod, gen_dir, name):
    """Exactly the expected constraints and sigma signs; the full random coefficient (r1_64's
    constraint 40) and the floor(0.1 T) term (r1_70x37's constraint 54: typed sparse, never
    tested) are not among them.  The path follows LRS_RANK1_A / LRS_DENSE_A."""
    path = r1_path(name, gen_dir)
    for cone in range(len(EXPECT_RANK1[name])):
        with env(LRS_RANK1_A="1", LRS_DENSE_A=None):
            cons, sig, on = solver_mod.rank1_plan(path, cone)
            dcons, don = solver_mod.dense_a_plan(path, cone)
        assert cons == EXPECT_RANK1[name][cone], (cone, cons)
        assert sig == EXPECT_SIGMA[name][cone], (cone, sig)
        assert on == (len(cons) > 0)
        assert dcons == EXPECT_DENSE[name][cone] and not don   # below the automatic threshold: no stack
        with env(LRS_RANK1_A="0", LRS_DENSE_A="1"):
            cons0, _, on0 = solver_mod.rank1_plan(path, cone)
            dcons0, don0 = solver_mod.dense_a_plan(path, cone)
        assert cons0 == [] and not on0
        assert dcons0 == EXPECT_DENSE[name][cone] and don0 == (len(dcons0) > 0)
        # unset: detected, and factored where the dense-A rule selects the cone (r1_200's 20 terms
        # hold 20 x 20 100 = 402 000 entries, past the automatic 320 000; the others stay below)
        with env(LRS_RANK1_A=None, LRS_DENSE_A=None):
            cons2, _, on2 = solver_mod.rank1_plan(path, cone)
        assert cons2 == EXPECT_RANK1[name][cone] and on2 == (name == "r1_200")
        with env(LRS_RANK1_A=None, LRS_DENSE_A="1"):    # selected: its rank-one coefficients are factored
            _, _, on3 = solver_mod.rank1_plan(path, cone)
        assert on3 == (len(cons) > 0)


def test_not_detected(solver_mod, tmp_path):
    """Dense coefficients that are not rank one within 1e-13 max|A|: a a^T + 1e-6 b b^T; a a^T with
    one entry of at least 0.1 max|A| outside the pivot row and column moved by 1e-9 relative; a
    dense matrix with a zero diagonal.  The plain a a^T and -a a^T next to them are detected."""
    inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")
    rng = np.random.default_rng(5)
    n = 24
    iu, ju = np.triu_indices(n)
    a, bb = rng.standard_normal(n), rng.standard_normal(n)
    A = np.outer(a, a)
    mats = [A + 1e-6 * np.outer(bb, bb)]
    near = A.copy()
    pv = int(np.argmax(np.abs(np.diag(A))))
    cand = [(j, k) for j in range(n) for k in range(j + 1) if j != pv and k != pv and abs(A[j, k]) >= 0.1 * np.abs(A).max()]
    j, k = cand[0]
    near[j, k] = near[k, j] = A[j, k] * (1.0 + 1e-9)
    mats.append(near)
    zd = rng.standard_normal((n, n))
    zd = zd + zd.T
    np.fill_diagonal(zd, 0.0)
    mats.append(zd)
    mats.append(A)
    mats.append(-A)
    d = np.arange(1, n + 1)
    entries = [(np.zeros(n, dtype=np.int64), 1, d, d, -np.ones(n))]
    for i, M in enumerate(mats, start=1):
        entries.append((np.full(iu.size, i, dtype=np.int64), 1, iu + 1, ju + 1, M[iu, ju]))
    path = inst.write_sdpa(str(tmp_path / "nd.dat-s"), len(mats), [n], np.array([np.trace(M) for M in mats]), entries)
    with env(LRS_RANK1_A="1", LRS_DENSE_A=None):
        cons, sig, on = solver_mod.rank1_plan(path, 0)
        dcons, _ = solver_mod.dense_a_plan(path, 0)
    assert dcons == [0, 1, 2, 3, 4]
    assert cons == [3, 4] and sig == [1.0, -1.0] and on


@pytest.mark.parametrize("name", ["da64", "da70x40", "da200"])
def test_densea_fixtures_have_no_rank_one(solver_mod, gen_dir, name):
    from densea_util import EXPECT_DENSE as DA_DENSE, da_path
    path = da_path(name, gen_dir)
    for cone in range(len(DA_DENSE[name])):
        with env(LRS_RANK1_A="1", LRS_DENSE_A=None):
            cons, _, on = solver_mod.rank1_plan(path, cone)
        assert cons == [] and not on


@pytest.mark.parametrize("name", NAMES)
def test_oracle_alm_steps_match_reference(oracle_lib, gen_dir, name):
    z = np.load(os.path.join(GOLDEN, f"steps_{name}.npz"))
    path = r1_path(name, gen_dir)
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

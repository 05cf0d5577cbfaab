"""The CPU restatement (oracle/lrsdp_oracle.c) against golden vectors written by
the reference LoRADS code itself (scripts/make_golden.py).  CPU only."""
import numpy as np
import pytest

from golden_util import KERNEL_CASES, load_solves, oracle_kernels, oracle_solve, rel_err

TOL = 1e-10   # summation-order differences only (OpenBLAS vs plain loops)


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_oracle_kernels_match_reference(oracle_lib, name):
    g, o = oracle_kernels(oracle_lib, name)
    for key in ["q1", "q2", "cvs_rr", "grad", "d_lbfgs2", "d_lbfgs1"]:
        assert rel_err(o[key], g[key]) < TOL, key
    for key in ["p1", "p2", "pobj_rr", "pinf_rr", "lag", "tau"]:
        assert abs(o[key] - g[key]) <= TOL * max(1.0, abs(g[key])), key
    assert o["rootnum"] == g["rootnum"]
    # CG to relative residual 1e-12: the RHS is exact to rounding; the iterate and
    # the iteration count move with the conditioning (theta: ill-conditioned)
    assert abs(o["cg_iters"] - g["cg_iters"]) <= max(2, 0.1 * g["cg_iters"])
    assert rel_err(o["rhs_cg"], g["rhs_cg"]) < TOL
    assert rel_err(o["u_cg"], g["u_cg"]) < 1e-6


def test_oracle_rand_matches_glibc(oracle_lib):
    import ctypes as C
    a = (C.c_int * 5)()
    oracle_lib.oracle_rand_seq(925, 5, a)
    # glibc srand(925); rand() x5 (the reference's initial point, lorads_solver.c:625)
    assert list(a) == [1026821133, 148406934, 1979500209, 155642481, 2031249410]


@pytest.mark.parametrize("case", range(7))
def test_oracle_solve_matches_reference(oracle_lib, case):
    s = load_solves()[case]
    o = oracle_solve(oracle_lib, s["instance"], s["flags"])
    r = s["result"]
    assert o["rank"] == r["rank"]
    if s["instance"].startswith("mc_"):
        # MaxCut: short phase 1, the trajectory is reproduced step for step
        assert abs(o["alm_inner"] - r["alm_inner"]) <= 2
        assert abs(o["admm_iter"] - r["admm_iter"]) <= 1
        for k in ("alm_pobj", "alm_dobj", "admm_pobj", "admm_dobj"):
            assert abs(o[k] - r[k]) <= 1e-6 * max(1.0, abs(r[k])), k
    else:
        # thousands of L-BFGS steps with rank growth: the iterates diverge at the
        # rounding level (chaotic), so compare the converged objectives inside the
        # certified accuracy of both runs (primal-dual gap), not the iterates
        tol = 10 * (r["admm_gap"] + o["admm_gap"]) + 1e-6
        for k in ("admm_pobj", "admm_dobj"):
            assert abs(o[k] - r[k]) <= tol * (1 + abs(r[k])), (k, o[k], r[k], tol)
        assert o["admm_pinf"] <= 1e-4 and r["admm_pinf"] <= 1e-4


STEP_CASES = ["mc_rand200", "mc_torus12x10", "mc_rand300w", "theta40", "theta25x3", "rsparse60", "checker_1.5",
              "mc_rand300w_r290", "mc_lp60", "mc_rand300w_r48", "mc_rand300w_r97", "mc_rand300w_r192",
              "mc_rand300w_r256"]
# n x r arrays stored as n x 4 projections (make_golden_steps.py); r48 ... r256: the 16 x 3, 64 x 2,
# 64 x 3 and 64 x 4 layouts, where tests/test_gpu_layouts.py takes the restatement as its reference
PROJ = {f"mc_rand300w_r{r}": 4 for r in (290, 48, 97, 192, 256)}


def _proj(v, n, k, seed=7):
    r = v.size // n
    return v.reshape(r, n).T @ np.random.default_rng(seed).standard_normal((r, k))


@pytest.mark.parametrize("name", STEP_CASES)
def test_oracle_alm_steps_match_reference(oracle_lib, name):
    """K inner iterations of the restatement vs the reference's own K trips
    (tests/golden/steps_*.npz, scripts/make_golden_steps.py)."""
    import ctypes as C
    import os
    from golden_util import GOLDEN, ROOT
    z = np.load(os.path.join(GOLDEN, f"steps_{name}.npz"))
    base = name[:name.rindex("_r")] if name in PROJ else name
    path = (os.path.join(ROOT, "data", "bundled", "checker_1.5.dat-s") if name == "checker_1.5"
            else os.path.join(GOLDEN, "instances", f"{base}.dat-s"))
    P = (lambda v: _proj(v, int(z["dims"][0]), PROJ[name])) if name in PROJ else (lambda v: v)
    lib = oracle_lib
    lib.oracle_alm_steps.restype = C.c_long
    lib.oracle_alm_steps.argtypes = [C.c_char_p, C.c_int, C.c_long, C.POINTER(C.c_double), C.c_long]
    nr, m = int(z["nr"]), int(z["m"])
    for K in [int(k) for k in z["ks"]]:
        if z[f"K{K}_trips"].shape[0] < K:
            continue
        out = np.zeros(2 * nr + 2 * m)
        got = lib.oracle_alm_steps(path.encode(), int(z["rank_flag"]), K, out.ctypes.data_as(C.POINTER(C.c_double)),
                                   out.size)
        assert got == nr, (K, got)
        assert rel_err(P(out[:nr]), z[f"K{K}_R"]) < 1e-9, K
        assert rel_err(P(out[nr:2 * nr]), z[f"K{K}_G"]) < 1e-9, K
        assert rel_err(out[2 * nr:2 * nr + m], z[f"K{K}_cvs"]) < 1e-9, K
        lam = z[f"K{K}_lam"]
        if np.linalg.norm(lam) > 0:
            assert rel_err(out[2 * nr + m:], lam) < 1e-9, K


@pytest.mark.parametrize("name", ["theta25x3", "mc_rand200", "rsparse60", "theta40"])
def test_oracle_admm_sweep_matches_reference(oracle_lib, name):
    """The restatement's LORADSUpdateSDPVar over every cone + LORADSUpdateDualVar against the
    reference's own run on the same inputs (tests/golden/admm_sweep_*.npz, cg_tol 1e-9): the
    bars of tests/test_capi.py's device sweep."""
    import ctypes as C
    import os
    import numpy as np
    from golden_util import GOLDEN, instance
    g = np.load(os.path.join(GOLDEN, f"admm_sweep_{name}.npz"))
    k = np.load(os.path.join(GOLDEN, f"kernels_{name}.npz"))
    vec, m, rank = k["inputs"].copy(), int(k["m"]), int(k["rank"])
    dims = [int(d) for d in k["dims"]]
    NR = sum(d * rank for d in dims)
    vec[9 * NR + 2 * m + 4] = float(g["cg_tol"])
    oracle_lib.oracle_admm_sweep.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    p = oracle_lib.oracle_read(instance(name).encode())
    out = np.zeros(2 * NR + 2 * m + 1 + len(dims))
    n = oracle_lib.oracle_admm_sweep(p, rank, vec.ctypes.data_as(C.POINTER(C.c_double)),
                                     out.ctypes.data_as(C.POINTER(C.c_double)))
    oracle_lib.oracle_free(p)
    assert n == out.size
    U, V, lam = out[:NR], out[NR:2 * NR], out[2 * NR + m:2 * NR + 2 * m]
    for key, ours in (("U", U), ("V", V), ("lam", lam)):
        assert rel_err(ours, g[key]) < 1e-6, (key, rel_err(ours, g[key]))
    cg_last = out[2 * NR + 2 * m + 1:]
    for c in range(len(dims)):
        ref = float(g["cg_last"][c])
        assert abs(cg_last[c] - ref) <= max(2, 0.25 * ref), (cg_last, g["cg_last"])
    assert abs(out[2 * NR + 2 * m] - float(g["cg_total"])) <= max(4, 0.15 * float(g["cg_total"]))


def test_oracle_lp_sweep_matches_reference(oracle_lib):
    """The restatement's LP block (the diagonal cone at rank 1; its ADMM update the column sweep of
    LORADSUpdateSDPLPVar) + LORADSUpdateDualVar against the reference on the same seeded U, V,
    lambda (tests/golden/admm_sweep_lp_mc_lp60.npz, scripts/make_golden_lp.py).  The LP block's
    own entries are a closed-form Gauss-Seidel sweep: within 1e-9 of the reference's."""
    import ctypes as C
    import os
    from golden_util import GOLDEN, instance
    g = np.load(os.path.join(GOLDEN, "admm_sweep_lp_mc_lp60.npz"))
    rank, m = int(g["rank"]), int(g["m"])
    dims = [int(d) for d in g["dims"]]
    NR = dims[0] * rank + dims[1]
    vec = np.concatenate([g["U0"], g["V0"], g["lam0"], [float(g["rho"]), float(g["cg_tol"])]])
    oracle_lib.oracle_admm_sweep_lp.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    p = oracle_lib.oracle_read(instance("mc_lp60").encode())
    assert p
    out = np.zeros(2 * NR + 2 * m + 1)
    n = oracle_lib.oracle_admm_sweep_lp(p, rank, vec.ctypes.data_as(C.POINTER(C.c_double)),
                                        out.ctypes.data_as(C.POINTER(C.c_double)))
    oracle_lib.oracle_free(p)
    assert n == out.size
    U, V = out[:NR], out[NR:2 * NR]
    cvs, lam = out[2 * NR:2 * NR + m], out[2 * NR + m:2 * NR + 2 * m]
    for key, ours in (("U", U), ("V", V), ("cvs", cvs), ("lam", lam)):
        assert rel_err(ours, g[key]) < 1e-6, (key, rel_err(ours, g[key]))
    nsdp = dims[0] * rank
    for key, ours in (("U", U), ("V", V)):
        assert rel_err(ours[nsdp:], g[key][nsdp:]) < 1e-9, (key, "LP block", rel_err(ours[nsdp:], g[key][nsdp:]))
    assert abs(out[-1] - float(g["cg_total"])) <= max(4, 0.15 * float(g["cg_total"]))


def test_oracle_lp_solve_matches_reference(oracle_lib):
    """mc_lp60 (LP slacks, a split free variable, a dense LP column) solved whole by the
    restatement: the reference's trajectory step for step (tests/golden/solves_lp.json)."""
    import json
    import os
    from golden_util import GOLDEN
    with open(os.path.join(GOLDEN, "solves_lp.json")) as f:
        s = {x["instance"]: x for x in json.load(f)}["mc_lp60"]
    o = oracle_solve(oracle_lib, s["instance"], s["flags"])
    r = s["result"]
    assert o["rank"] == r["rank"]   # the SDP cone's rank (the reference's rankElem)
    assert abs(o["alm_inner"] - r["alm_inner"]) <= 2
    assert abs(o["admm_iter"] - r["admm_iter"]) <= 1
    for k in ("alm_pobj", "alm_dobj", "admm_pobj", "admm_dobj"):
        assert abs(o[k] - r[k]) <= 1e-6 * max(1.0, abs(r[k])), k

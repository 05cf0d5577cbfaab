"""The LP block's ADMM column sweep (lrs_kernels.hip k_lp_admm) in isolation, in
both variants -- operands staged in LDS, and the global-memory walk that every context with more
than roughly 1 800 cuts runs -- against the NumPy restatement of tests/lp_util.py, which reads the
problem and the input vectors only.

Procedure of an isolated sweep: seed U, V and LAMBDA, lrs_op_admm_constr, read the constraint sums
cvs0 (checked against the longdouble A(U V^T)), run the sweep alone (lrs_op_admm_half on the LP
cone), and compare U, V and the sums with the longdouble restatement fed the device's own cvs0 bits,
so that the comparison sees the sweep and not the SDP gather.  The SDP rows of U and V must come
back bit for bit.  Solver.lp_sweep_info() says which variant the launch took; the environment
variable LRS_LP_LDS_MAX=0 forces the global-memory one.

Bar, from the restatement alone and per case: floor = the largest difference between the float64
and the longdouble restatement over u, v and the sums, each relative to max(1, max |ref|); the
device gets 8 floor + 4 eps.  The device contracts multiply-adds (the compiler's default), which
changes single roundings of the same dependency chain; a float64 restatement with emulated
contractions stayed within 1.3 floor on shapes up to 2 100 columns.  cvs0 gets the same bar with the
floor of the two A(U V^T) restatements.  The measured floors and errors are in
profiles/lp_sweep.md.  Both variants run one serial routine on the same values: their outputs must
be identical bit for bit."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import lp_util as lu
import tri_util as tu
from golden_util import GOLDEN, instance, rel_err

pytestmark = pytest.mark.gpu

KNOB = "LRS_LP_LDS_MAX"
LIMIT = 152 * 1024


@pytest.fixture(scope="module")
def solver_mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.solver")


@pytest.fixture(scope="module")
def inst_mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.instances")


def seeded_state(problem, r, seed):
    """(U0, V0, lam) as scripts/make_golden_lp.py seeds them: V = U + 0.1 noise."""
    m, dims = problem[0], problem[1]
    rng = np.random.default_rng(seed)
    NA = dims[0] * r - dims[1]
    U = rng.standard_normal(NA)
    return U, U + 0.1 * rng.standard_normal(NA), rng.standard_normal(m)


def isolated(sv, mod, r, U0, V0, lam, rho, set_rank=True):
    if set_rank:
        sv.set_rank([r, 1])
    assert sv.get_rank() == [r, 1]
    sv.set_factor(mod.U, U0)
    sv.set_factor(mod.V, V0)
    sv.set_vec(mod.LAMBDA, lam)
    sv.admm_constr()
    cvs0 = sv.get_vec(mod.CVS)
    info = sv.lp_sweep_info()
    assert info.lp_cone == 1
    sv.admm_half(rho, 1e-9, cone=1, side=0, init=False)
    return dict(cvs0=cvs0, info=info, U=sv.get_factor(mod.U), V=sv.get_factor(mod.V), cvs=sv.get_vec(mod.CVS))


def check(out, problem, cols, r, U0, V0, lam, rho, label):
    """One isolated sweep against the restatement; returns (floor, error)."""
    nsdp = problem[1][0] * r
    lo0 = lu.constr_values(problem, cols, U0, V0, r, np.float64)
    hi0 = lu.constr_values(problem, cols, U0, V0, r, np.longdouble)
    floor0, err0 = lu.rel_max(lo0, hi0), lu.rel_max(out["cvs0"], hi0)
    floor, hi = lu.sweep_floor(cols, problem[2], lam, rho, U0[nsdp:], V0[nsdp:], out["cvs0"])
    errs = [lu.rel_max(out["U"][nsdp:], hi[0]), lu.rel_max(out["V"][nsdp:], hi[1]), lu.rel_max(out["cvs"], hi[2])]
    print(f"lp_sweep {label}: staged {out['info'].staged} lds_bytes {out['info'].lds_bytes} entries "
          f"{out['info'].entries} dropped {out['info'].dense_dropped} | A(UV^T) floor {floor0:.3e} device {err0:.3e} "
          f"bar {lu.bar(floor0):.3e} | sweep floor {floor:.3e} device u {errs[0]:.3e} v {errs[1]:.3e} cvs {errs[2]:.3e} "
          f"bar {lu.bar(floor):.3e}")
    assert out["info"].entries == cols.entries and out["info"].dense_dropped == cols.dropped
    assert err0 <= lu.bar(floor0), (label, "A(UV^T)", err0, floor0)
    assert max(errs) <= lu.bar(floor), (label, errs, floor)
    assert out["U"][:nsdp].tobytes() == U0[:nsdp].tobytes() and out["V"][:nsdp].tobytes() == V0[:nsdp].tobytes()
    return floor, max(errs)


def same_bits(a, b, label):
    for key in ("cvs0", "U", "V", "cvs"):
        x, y = a[key].view(np.uint64), b[key].view(np.uint64)
        diff = np.flatnonzero(x != y)
        assert diff.size == 0, (label, key, "first differing index", int(diff[0]), a[key][diff[0]], b[key][diff[0]])


def both_variants(monkeypatch, sv, mod, problem, cols, r, seed, rho, label):
    """The case on the staged variant (the default limit), then on the global-memory one."""
    U0, V0, lam = seeded_state(problem, r, seed)
    monkeypatch.delenv(KNOB, raising=False)
    a = isolated(sv, mod, r, U0, V0, lam, rho)
    assert a["info"].staged == 1 and a["info"].lds_bytes <= LIMIT
    monkeypatch.setenv(KNOB, "0")
    b = isolated(sv, mod, r, U0, V0, lam, rho)
    assert b["info"].staged == 0 and b["info"].lds_bytes == a["info"].lds_bytes
    monkeypatch.delenv(KNOB)
    same_bits(a, b, label)
    check(a, problem, cols, r, U0, V0, lam, rho, label + " staged")
    check(b, problem, cols, r, U0, V0, lam, rho, label + " global")
    return a, b, (U0, V0, lam)


def test_knob_only_lowers_the_limit(solver_mod, monkeypatch):
    """LRS_LP_LDS_MAX is read per launch and clamped to [0, 152 KB]: a value above the limit or
    at the need leaves the staged variant, one byte less takes the other, a negative one is 0."""
    sv = solver_mod.Solver(instance("mc_lp60"))
    monkeypatch.delenv(KNOB, raising=False)
    need = sv.lp_sweep_info().lds_bytes
    assert sv.lp_sweep_info().staged == 1 and 0 < need <= LIMIT
    for val, staged in ((str(1 << 30), 1), (str(need), 1), (str(need - 1), 0), ("0", 0), ("-5", 0)):
        monkeypatch.setenv(KNOB, val)
        assert sv.lp_sweep_info().staged == staged, val
    sv.close()
    monkeypatch.delenv(KNOB)
    plain = solver_mod.Solver(instance("mc_torus12x10"))
    i = plain.lp_sweep_info()
    assert (i.lp_cone, i.staged, i.lds_bytes, i.entries, i.dense_dropped) == (-1, 0, 0, 0, 0)
    plain.close()


def test_one_column(solver_mod, inst_mod, monkeypatch):
    """One LP column, m = 5: its single entry is in 1 of 5 constraints, below the m/4 threshold."""
    problem = lu.lp_problem(3, 5, [(0.7, [(2, 1.3)])], seed=5)
    cols = lu.lp_columns(problem)
    assert cols.dense == [] and cols.entries == 1 and len(cols.slots) == 1
    sv = solver_mod.Solver(coo=inst_mod.coo_arrays(problem))
    both_variants(monkeypatch, sv, solver_mod, problem, cols, 2, 51, 1.7, "1 column m=5")
    sv.close()


def mixed_columns(n, m, n_sdp, seed, last_cost_only):
    """n columns cycling through eight shapes: no data at all, a cost only, 1 entry, a cost and 2
    entries, a cost and 3 entries one of them written twice, 4 entries, a cost and an entry in a
    constraint the SDP block is in too, one entry written twice."""
    rng = np.random.default_rng(seed)
    cols = []
    for j in range(n):
        k = j % 8
        cost = float(rng.uniform(-1.0, 1.0))
        pick = lambda q: [(int(i), float(rng.uniform(0.3, 1.5) * rng.choice([-1.0, 1.0])))
                          for i in rng.choice(m, size=q, replace=False)]
        if k == 0:
            cols.append((cost, []) if last_cost_only and j == n - 1 else (None, []))
        elif k == 1:
            cols.append((cost, []))
        elif k == 2:
            cols.append((None, pick(1)))
        elif k == 3:
            cols.append((cost, pick(2)))
        elif k == 4:
            e = pick(3)
            cols.append((cost, e + [(e[1][0], 0.25)]))
        elif k == 5:
            cols.append((None, pick(4)))
        elif k == 6:
            cols.append((cost, [(int(rng.integers(0, n_sdp)), 1.0)]))
        else:
            i = int(rng.integers(0, m))
            cols.append((None, [(i, 0.5), (i, -1.25)]))
    return cols


@pytest.mark.parametrize("odd", [False, True])
def test_257_mixed_columns(solver_mod, inst_mod, monkeypatch, odd):
    """257 columns (one past the block's 256-thread stride), m = 70, every column shape; with an
    even and an odd number of slots P (the global-memory variant's int entry starts sit behind
    2 n doubles of scratch).  A column without data: u <- v_old, v <- that value."""
    n, m, n_sdp, r = 257, 70, 6, 3
    problem = lu.lp_problem(n_sdp, m, mixed_columns(n, m, n_sdp, 257, odd), seed=70)
    cols = lu.lp_columns(problem)
    assert cols.dense == [] and len(cols.slots) == (225 if odd else 224)
    sv = solver_mod.Solver(coo=inst_mod.coo_arrays(problem))
    rho = 0.6
    a, _, (U0, V0, _) = both_variants(monkeypatch, sv, solver_mod, problem, cols, r, 2570 + odd, rho,
                                      f"257 columns m=70 P={len(cols.slots)}")
    sv.close()
    nsdp = n_sdp * r
    empty = [j for j in range(n) if j not in cols.slots]
    assert len(empty) == (32 if odd else 33)
    for j in empty:      # exact up to the rounding of (rho y) / rho, twice
        y = V0[nsdp + j]
        assert abs(a["U"][nsdp + j] - y) <= 2 * lu.EPS * abs(y) and abs(a["V"][nsdp + j] - y) <= 4 * lu.EPS * abs(y)


@pytest.fixture(scope="module")
def dense_problem():
    return build_dense_problem()


def build_dense_problem():
    """600 columns, m = 300; columns 100 and 400 sit in 75 (exactly m/4) and 120 constraints."""
    n, m = 600, 300
    rng = np.random.default_rng(600)
    cols = []
    for j in range(n):
        q = 75 if j == 100 else 120 if j == 400 else int(rng.integers(1, 4))
        ents = [(int(i), float(rng.uniform(0.2, 1.2) * rng.choice([-1.0, 1.0]))) for i in rng.choice(m, size=q, replace=False)]
        cols.append((float(rng.uniform(-1.0, 1.0)) if j % 2 or j == 400 else None, ents))   # 400 keeps a slot, 100 none
    problem = lu.lp_problem(8, m, cols, seed=300)
    return problem, lu.lp_columns(problem)


@pytest.mark.parametrize("rho", [0.01, 100.0])
def test_600_columns_two_dense(solver_mod, inst_mod, monkeypatch, dense_problem, rho):
    """Two columns in >= 25 % of the constraints: dense_dropped is their entry count, and their
    ||a||^2 is still in the update's denominator (the restatement without it is far off the bar)."""
    problem, cols = dense_problem
    assert cols.dense == [100, 400] and cols.dropped == 195
    r = 3
    sv = solver_mod.Solver(coo=inst_mod.coo_arrays(problem))
    a, _, (U0, V0, lam) = both_variants(monkeypatch, sv, solver_mod, problem, cols, r, 6000, rho,
                                        f"600 columns m=300 rho={rho:g}")
    assert a["info"].dense_dropped == 195
    sv.close()
    import copy
    bare = copy.copy(cols)
    bare.nrm2 = cols.nrm2.copy()
    bare.nrm2[cols.dense] = 0.0
    nsdp = problem[1][0] * r
    floor, hi = lu.sweep_floor(cols, problem[2], lam, rho, U0[nsdp:], V0[nsdp:], a["cvs0"])
    wrong = lu.lp_sweep(bare, problem[2], lam, rho, U0[nsdp:], V0[nsdp:], a["cvs0"], np.longdouble)
    assert lu.rel_max(wrong[0], hi[0]) > 1e6 * lu.bar(floor)


def test_mc_lp60(solver_mod, monkeypatch):
    """The reference's fixture instance on the fixture's own seeds."""
    g = np.load(os.path.join(GOLDEN, "admm_sweep_lp_mc_lp60.npz"))
    problem = lu.read_problem(instance("mc_lp60"))
    cols = lu.lp_columns(problem)
    r, rho = int(g["rank"]), float(g["rho"])
    sv = solver_mod.Solver(instance("mc_lp60"))
    outs = []
    for val, staged in ((None, 1), ("0", 0)):
        if val is None:
            monkeypatch.delenv(KNOB, raising=False)
        else:
            monkeypatch.setenv(KNOB, val)
        out = isolated(sv, solver_mod, r, g["U0"], g["V0"], g["lam0"], rho)
        assert out["info"].staged == staged and out["info"].dense_dropped == 20
        outs.append(out)
    monkeypatch.delenv(KNOB)
    sv.close()
    same_bits(outs[0], outs[1], "mc_lp60")
    for out, name in zip(outs, ("staged", "global")):
        check(out, problem, cols, r, g["U0"], g["V0"], g["lam0"], rho, "mc_lp60 " + name)


# ---- the global-memory variant at its natural size: no knob


def random_cuts(n, T, seed):
    i, j, k = tu.triples(n)
    rng = np.random.default_rng(seed)
    pick = rng.choice(i.size, size=T, replace=False)
    return np.stack([i[pick], j[pick], k[pick], rng.integers(0, 4, size=T)], axis=1).astype(np.int32)


@pytest.fixture(scope="module")
def torus():
    return build_torus()


def build_torus():
    inst =importlib.import_module("ltr-lowrank-sdp_amd.instances")
    problem = inst.maxcut_torus_problem(12, 10, 1210)
    cuts = random_cuts(120, 2100, 2100)
    assert np.unique(cuts[:, :4], axis=0).shape[0] == 2100
    return problem, cuts, inst.add_triangle_cuts(problem, cuts)


def test_2100_cuts_in_place(solver_mod, inst_mod, monkeypatch, torus):
    """The 12 x 10 torus with 2 100 cuts appended in place in two batches (carry): the sweep's
    operands no longer fit 152 KB, so every ADMM iteration of such a context runs the global-memory
    variant.  The sweep meets the bar there, gives the bits of the same problem loaded whole, and
    after dropping back to 500 cuts the rebuilt context stages again and still meets the bar."""
    monkeypatch.delenv(KNOB, raising=False)
    problem, cuts, full = torus
    r, rho = 3, 1.3
    rng = np.random.default_rng(12)
    X = rng.standard_normal((120, r))
    X /= np.linalg.norm(X, axis=1)[:, None]
    sv = solver_mod.Solver(coo=inst_mod.coo_arrays(problem))
    sv.set_rank([r])
    sv.set_factor(solver_mod.R, X.ravel(order="F"))
    assert sv.append_cuts(cuts[:1000], carry=True) == 1000
    assert sv.lp_sweep_info().staged == 1
    assert sv.append_cuts(cuts[1000:], carry=True) == 1100
    info = sv.lp_sweep_info()
    assert info.staged == 0 and info.lds_bytes > LIMIT and info.entries == 2100 and info.dense_dropped == 0
    cols = lu.lp_columns(full)
    assert cols.dense == [] and cols.entries == 2100
    U0, V0, lam = seeded_state(full, r, 21)
    a = isolated(sv, solver_mod, r, U0, V0, lam, rho, set_rank=False)
    assert a["info"].staged == 0
    check(a, full, cols, r, U0, V0, lam, rho, "torus 2100 cuts in place")
    whole = solver_mod.Solver(coo=inst_mod.coo_arrays(full))
    b = isolated(whole, solver_mod, r, U0, V0, lam, rho)
    whole.close()
    assert b["info"].staged == 0 and b["info"].lds_bytes == info.lds_bytes
    same_bits(a, b, "in place against loaded whole")
    # back to the first 500 cuts
    assert sv.drop_cuts(np.arange(2100) >= 500, carry=True) == 1600
    info = sv.lp_sweep_info()
    assert info.staged == 1 and info.lds_bytes <= LIMIT and info.entries == 500
    part = inst_mod.add_triangle_cuts(problem, cuts[:500])
    pcols = lu.lp_columns(part)
    U0, V0, lam = seeded_state(part, r, 22)
    c = isolated(sv, solver_mod, r, U0, V0, lam, rho, set_rank=False)
    sv.close()
    assert c["info"].staged == 1
    check(c, part, pcols, r, U0, V0, lam, rho, "torus dropped to 500 cuts")


def test_three_vertices_one_cut(solver_mod, inst_mod, monkeypatch):
    """n = 3 and one appended cut: m = 4, the slack column sits in 1/4 of the constraints, so the
    kept column typing drops its coefficient (dense_dropped 1, no entries, no slots): the sweep
    moves the slack by x = y / (1 + y^2) alone and leaves the constraint sums as they were
    (DESIGN.md §4.14)."""
    ei = np.arange(3)
    problem = inst_mod._maxcut_problem(3, ei, (ei + 1) % 3, np.ones(3))
    cut = np.array([[0, 1, 2, 0]], dtype=np.int32)
    full = inst_mod.add_triangle_cuts(problem, cut)
    cols = lu.lp_columns(full)
    assert cols.dense == [0] and cols.dropped == 1 and cols.entries == 0 and cols.slots == [] and cols.nrm2[0] == 1.0
    sv = solver_mod.Solver(coo=inst_mod.coo_arrays(problem))
    assert sv.append_cuts(cut, carry=False) == 1 and sv.m == 4
    info = sv.lp_sweep_info()
    assert (info.lp_cone, info.entries, info.dense_dropped) == (1, 0, 1)
    a, b, _ = both_variants(monkeypatch, sv, solver_mod, full, cols, 2, 31, 0.8, "3 vertices, 1 cut")
    sv.close()
    assert a["cvs"].tobytes() == a["cvs0"].tobytes()


def test_whole_iteration_against_the_oracle(solver_mod, inst_mod, oracle_lib, monkeypatch, torus, tmp_path):
    """One whole ADMM iteration of the 2 100-cut problem (lrs_op_admm_constr, the SDP cone's two
    CG half-steps, the LP sweep in its global-memory variant, the dual update) against the CPU
    restatement of the reference run live on the same file and seeds: U, V and lambda at the
    project's sweep bar 1e-6 (the CG at cg_tol 1e-9), the LP block at 1e-9, which
    tests/test_oracle_golden.py holds the oracle to against the reference."""
    monkeypatch.delenv(KNOB, raising=False)
    _, _, full = torus
    m, dims = full[0], full[1]
    r, rho, tol = 3, 2.0, 1e-9
    path = str(tmp_path / "torus_cuts2100.dat-s")
    inst_mod.write_sdpa(path, *full)
    U0, V0, lam0 = seeded_state(full, r, 23)
    NR = dims[0] * r - dims[1]
    vec = np.concatenate([U0, V0, lam0, [rho, tol]])
    oracle_lib.oracle_admm_sweep_lp.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    p = oracle_lib.oracle_read(path.encode())
    assert p
    out = np.zeros(2 * NR + 2 * m + 1)
    n = oracle_lib.oracle_admm_sweep_lp(p, r, vec.ctypes.data_as(C.POINTER(C.c_double)),
                                        out.ctypes.data_as(C.POINTER(C.c_double)))
    oracle_lib.oracle_free(p)
    assert n == out.size
    ref = dict(U=out[:NR], V=out[NR:2 * NR], lam=out[2 * NR + m:2 * NR + 2 * m])
    sv = solver_mod.Solver(path)
    assert sv.dims == [120, 2100]
    sv.set_rank([r, 1])
    sv.set_factor(solver_mod.U, U0)
    sv.set_factor(solver_mod.V, V0)
    sv.set_vec(solver_mod.LAMBDA, lam0)
    assert sv.lp_sweep_info().staged == 0
    sv.admm_constr()
    for side in (0, 1):
        sv.admm_half(rho, tol, cone=0, side=side, init=False)
    sv.admm_half(rho, tol, cone=1, side=0, init=False)
    sv.dual_update(rho)
    ours = dict(U=sv.get_factor(solver_mod.U), V=sv.get_factor(solver_mod.V), lam=sv.get_vec(solver_mod.LAMBDA))
    sv.close()
    nsdp = dims[0] * r
    errs = {k: rel_err(ours[k], ref[k]) for k in ref}
    lp = {k: rel_err(ours[k][nsdp:], ref[k][nsdp:]) for k in ("U", "V")}
    print(f"whole iteration, 2100 cuts, against the oracle: {errs}; LP block {lp}")
    for k, e in errs.items():
        assert e < 1e-6, (k, e)
    for k, e in lp.items():
        assert e < 1e-9, (k, "LP block", e)


# ---- whole solves: the global-memory variant inside the stream-ordered ADMM loop


KEYS = ("alm_inner", "admm_iter", "pobj", "dobj")


def _solve_mc_lp60(mod):
    sv = mod.Solver(instance("mc_lp60"))
    res = sv.solve(reoptLevel=0)
    out = (res, sv.get_factor(mod.R), sv.get_vec(mod.LAMBDA), sv.lp_sweep_info().staged)
    sv.close()
    return out


def _solve_torus_64(mod):
    sv = mod.Solver(instance("mc_torus12x10"))
    sv.solve()
    cuts = sv.separate_triangles(64, 1e-6)[0]
    assert sv.append_cuts(cuts, carry=True) == 64
    res = sv.solve_warm()
    out = (res, sv.get_factor(mod.R), sv.get_vec(mod.LAMBDA), sv.lp_sweep_info().staged)
    sv.close()
    return out


@pytest.mark.parametrize("which", ["mc_lp60", "torus64"])
def test_whole_solve_is_the_same_in_both_variants(solver_mod, monkeypatch, which):
    run = _solve_mc_lp60 if which == "mc_lp60" else _solve_torus_64
    monkeypatch.delenv(KNOB, raising=False)
    ra, Ra, la, sa = run(solver_mod)
    monkeypatch.setenv(KNOB, "0")
    rb, Rb, lb, sb = run(solver_mod)
    monkeypatch.delenv(KNOB)
    assert (sa, sb) == (1, 0)
    print(f"{which}: alm_inner {ra['alm_inner']} admm_iter {ra['admm_iter']} pobj {ra['pobj']!r} dobj {ra['dobj']!r}")
    assert ra["admm_iter"] > 0
    for key in KEYS:
        assert ra[key] == rb[key], (key, ra[key], rb[key])
    assert Ra.tobytes() == Rb.tobytes() and la.tobytes() == lb.tobytes()

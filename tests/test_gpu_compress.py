"""Rank reduction on the device (include/lrsdp.h lrs_factor_spectrum, lrs_factor_compress,
lrs_set_rank_shrink) against NumPy.

Inputs are factors with a prescribed spectrum, R = U0 diag(sqrt(w)) V0^T (QR of seeded normals): the
kept eigenvalues geometric from 1 down to 1e-3, the dropped ones geometric from 1e-9 to 1e-12, so
that the count at rel_tol = 1e-6 is three decades away from either side.

Bars (u = 2^-53).  Matrix-core products: 1e-12 max|ref|, the bar of test_gram_mfma_matches_fp64.
Eigenvalues: 64 r u w_0, the eigen-solver's bound (tests/test_sym_eig.py).  The Gram of the rotated
factor: (64 r u + 2e-12) w_0, that bound plus two products.  Solves whose trajectories differ:
objectives within 10 x the sum of the two certified gaps, pinf <= 1e-4."""
import importlib
import json
import os
import threading

import numpy as np
import pytest

from golden_util import instance

pytestmark = pytest.mark.gpu

R, D, G, U, V, S0, Y0, S1, Y1 = range(9)
LAMBDA = 0
UU = 2.0 ** -53
TOL = 1e-6

CASES = [(5, 1, 1), (17, 3, 2), (70, 19, 7), (70, 24, 16), (300, 64, 13), (300, 200, 33), (300, 290, 64),
         (520, 512, 1), (520, 512, 40)]


@pytest.fixture(scope="module")
def solver_mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.solver")


@pytest.fixture(scope="module")
def inst_mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.instances")


def rand_problem(inst_mod, n, seed=3):
    """A random unit-weight graph of 3 n edges (all pairs when fewer) as a MaxCut problem."""
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    pick = rng.choice(iu.size, size=min(3 * n, iu.size), replace=False)
    return inst_mod._maxcut_problem(n, iu[pick], ju[pick], np.ones(pick.size))


def context(solver_mod, inst_mod, n):
    if n == 300:
        return solver_mod.Solver(instance("mc_rand300w"))
    return solver_mod.Solver(coo=inst_mod.coo_arrays(rand_problem(inst_mod, n)))


def spectrum(r, k):
    kept = np.geomspace(1.0, 1e-3, k) if k > 1 else np.ones(1)
    drop = np.geomspace(1e-9, 1e-12, r - k) if r - k > 1 else np.full(r - k, 1e-9)
    return np.concatenate([kept, drop])


def factor(n, r, k, seed):
    rng = np.random.default_rng(seed)
    u0 = np.linalg.qr(rng.standard_normal((n, r)))[0]
    v0 = np.linalg.qr(rng.standard_normal((r, r)))[0]
    return (u0 * np.sqrt(spectrum(r, k))) @ v0.T


def put(sv, which, X):
    sv.set_factor(which, np.ascontiguousarray(X).ravel(order="F"))


def get(sv, which, n, r):
    return sv.get_factor(which).reshape(r, n).T


def start(sv, X):
    sv.set_rank([X.shape[1]])
    put(sv, R, X)


def amax(a):
    return float(np.abs(a).max(initial=0.0))


@pytest.mark.parametrize("n,r,k", CASES)
def test_compress_rotates_and_truncates(solver_mod, inst_mod, n, r, k):
    sv = context(solver_mod, inst_mod, n)
    X = factor(n, r, k, seed=100 * r + k)
    start(sv, X)
    g0 = sv.gram()
    w_np = np.linalg.eigvalsh(g0)[::-1]
    w0 = float(w_np[0])
    ebar = 64 * r * UU * w0
    gbar = (64 * r * UU + 2e-12) * w0
    assert int((w_np > TOL * w0).sum()) == k   # the input is what the case says
    eig_only, counts = sv.spectrum(R, TOL)
    assert counts == [k] and sv.get_rank() == [r]
    out = sv.compress(rel_tol=TOL, return_q=True)
    q, eigs, lost = out["q"][0], out["eigs"][0], out["lost"][0]
    # 3. rule and outputs
    assert out["ranks"] == [k] and sv.get_rank() == [k]
    assert np.array_equal(eig_only[0], eigs)
    print(f"n={n} r={r} k={k}: |eigs-np|={amax(eigs - w_np):.3e} (bar {ebar:.3e}) lost={lost:.3e}")
    assert eigs.shape == (r,) and amax(eigs - w_np) <= ebar
    assert abs(lost - float(np.maximum(w_np[k:], 0.0).sum())) <= ebar
    # 1. the product
    ref = X @ q[:, :k]
    Y = get(sv, R, n, k)
    print(f"  product: {amax(Y - ref):.3e} (bar {1e-12 * amax(ref):.3e})")
    assert amax(Y - ref) <= 1e-12 * amax(ref)
    assert np.array_equal(sv.get_factor(U), sv.get_factor(R)) and np.array_equal(sv.get_factor(V), sv.get_factor(R))
    x0, x1 = (X * X).sum(axis=1), (Y * Y).sum(axis=1)
    assert amax(x0 - x1) <= lost + 1e-12 * amax(x0)
    # 8. the other buffers are zero
    for which in (D, G, S0, Y0, S1, Y1):
        assert not sv.get_factor(which).any(), which
    # 2. padding: dirty columns in [k, ld') would show in A(Y Y^T) and in the Gram
    cvs = sv.constr_rr()[0]
    print(f"  A(YY^T): {amax(cvs - x1):.3e} (bar {1e-12 * amax(x1):.3e})")
    assert amax(cvs - x1) <= 1e-12 * amax(x1)
    g1 = sv.gram()
    print(f"  gram offdiag {amax(g1 - np.diag(np.diag(g1))):.3e} diag {amax(np.diag(g1) - eigs[:k]):.3e} (bar {gbar:.3e})")
    assert amax(g1 - np.diag(np.diag(g1))) <= gbar
    assert amax(np.diag(g1) - eigs[:k]) <= gbar
    # 5. idempotence: the sign rule makes the second rotation +I up to rounding
    again = sv.compress(ranks=[k], rel_tol=TOL)
    Y2 = get(sv, R, n, k)
    print(f"  second compress moves R by {amax(Y2 - Y):.3e} (bar {(64 * r * UU + 2e-12) * amax(Y):.3e})")
    assert again["ranks"] == [k]
    assert amax(again["eigs"][0] - eigs[:k]) <= gbar
    assert amax(Y2 - Y) <= (64 * r * UU + 2e-12) * amax(Y)
    # 3. slack, explicit ranks
    start(sv, X)
    assert sv.compress(rel_tol=TOL, slack=2)["ranks"] == [min(r, k + 2)]
    start(sv, X)
    kx = k + 1 if k < r else max(1, k - 1)
    ex = sv.compress(ranks=[kx], rel_tol=TOL, return_q=True)
    assert ex["ranks"] == [kx] and sv.get_rank() == [kx]
    refx = X @ ex["q"][0][:, :kx]
    assert amax(get(sv, R, n, kx) - refx) <= 1e-12 * amax(refx)
    # 4. k = r: a rotation alone leaves A(X) as it was
    start(sv, X)
    before = sv.constr_rr()[0]
    assert sv.compress(ranks=[r], rel_tol=TOL)["ranks"] == [r]
    after = sv.constr_rr()[0]
    print(f"  k = r: A(X) moves by {amax(after - before):.3e} (bar {1e-12 * amax(before):.3e})")
    assert amax(after - before) <= 1e-12 * amax(before)
    # 1. which = U: the source is (U + V) / 2 with U != V
    E = np.random.default_rng(7).standard_normal((n, r)) * 1e-3
    sv.set_rank([r])
    put(sv, U, X + E)
    put(sv, V, X - E)
    S = 0.5 * ((X + E) + (X - E))
    ou = sv.compress(rel_tol=TOL, which=U, return_q=True)
    ku = ou["ranks"][0]
    refu = S @ ou["q"][0][:, :ku]
    print(f"  which=U: rank {ku}, product {amax(get(sv, R, n, ku) - refu):.3e}")
    assert ku == k
    assert amax(get(sv, R, n, ku) - refu) <= 1e-12 * amax(refu)
    assert np.array_equal(sv.get_factor(U), sv.get_factor(R)) and np.array_equal(sv.get_factor(V), sv.get_factor(R))
    sv.close()


@pytest.mark.parametrize("n,r,k", [(70, 19, 7), (300, 64, 13)])
def test_compress_is_reproducible(solver_mod, inst_mod, n, r, k):
    """6. Two fresh contexts given the same input return the same bits."""
    X = factor(n, r, k, seed=5)
    got = []
    for _ in range(2):
        sv = context(solver_mod, inst_mod, n)
        start(sv, X)
        out = sv.compress(rel_tol=TOL, return_q=True)
        got.append((sv.get_factor(R), out["eigs"][0], out["q"][0], out["ranks"]))
        sv.close()
    assert got[0][3] == got[1][3] == [k]
    for a, b in zip(got[0][:3], got[1][:3]):
        assert np.array_equal(a, b)


def test_compress_several_cones(solver_mod):
    """7. theta25x3 at ranks [5, 11, 33] -> explicit [2, 11, 7]: each cone is its own product."""
    sv = solver_mod.Solver(instance("theta25x3"))
    dims, old, new = sv.dims, [5, 11, 33], [2, 11, 7]
    assert dims == [25, 25, 25]
    rng = np.random.default_rng(11)
    Xs = [rng.standard_normal((n, r)) for n, r in zip(dims, old)]
    sv.set_rank(old)
    sv.set_factor(R, np.concatenate([x.ravel(order="F") for x in Xs]))
    lam = rng.standard_normal(sv.m)
    sv.set_vec(LAMBDA, lam)
    out = sv.compress(ranks=new, return_q=True)
    assert out["ranks"] == new and sv.get_rank() == new
    flat, off = sv.get_factor(R), 0
    for X, n, r, k, q, e in zip(Xs, dims, old, new, out["q"], out["eigs"]):
        Y = flat[off:off + n * k].reshape(k, n).T
        off += n * k
        ref = X @ q[:, :k]
        assert q.shape == (r, r) and e.shape == (r,)
        assert amax(Y - ref) <= 1e-12 * amax(ref)
        assert amax(e - np.linalg.eigvalsh(X.T @ X)[::-1]) <= (64 * r * UU + 1e-12) * e[0]
    assert off == flat.size
    assert np.array_equal(sv.get_vec(LAMBDA), lam)
    sv.close()


def test_compress_keeps_the_lp_block(solver_mod):
    """7. mc_lp60: the LP cone's rows and LAMBDA are the same bits before and after."""
    sv = solver_mod.Solver(instance("mc_lp60"))
    n, nlp = sv.dims
    r, k = 9, 4
    rng = np.random.default_rng(13)
    X = factor(n, r, k, seed=17)
    lp = rng.uniform(0.1, 2.0, nlp)
    sv.set_rank([r, 1])
    sv.set_factor(R, np.concatenate([X.ravel(order="F"), lp]))
    lam = rng.standard_normal(sv.m)
    sv.set_vec(LAMBDA, lam)
    eigs, counts = sv.spectrum(R, TOL)
    assert counts[0] == k and eigs[1].shape == (1,) and abs(eigs[1][0] - float(lp @ lp)) <= 1e-12 * float(lp @ lp)
    out = sv.compress(rel_tol=TOL, return_q=True)
    assert out["ranks"] == [k, 1] and sv.get_rank() == [k, 1]
    flat = sv.get_factor(R)
    assert flat[n * k:].tobytes() == lp.tobytes()
    assert sv.get_vec(LAMBDA).tobytes() == lam.tobytes()
    ref = X @ out["q"][0][:, :k]
    assert amax(flat[:n * k].reshape(k, n).T - ref) <= 1e-12 * amax(ref)
    sv.close()


def test_compress_then_warm_solve(solver_mod):
    """8. mc_torus12x10: solve, compress the phase-2 point, warm re-solve."""
    sv = solver_mod.Solver(instance("mc_torus12x10"))
    a = sv.solve()
    lam = sv.get_vec(LAMBDA)
    out = sv.compress(rel_tol=TOL, which=U)
    assert sv.get_rank() == out["ranks"] and out["ranks"][0] <= a["final_rank"]
    assert sv.get_vec(LAMBDA).tobytes() == lam.tobytes()
    b = sv.solve_warm()
    tol = 10 * (a["gap"] + b["gap"])
    print(f"cold pobj {a['pobj']!r} gap {a['gap']:.3e} rank {a['final_rank']}; compressed to {out['ranks']} lost "
          f"{out['lost']}; warm pobj {b['pobj']!r} gap {b['gap']:.3e} pinf {b['pinf']:.3e} rank {b['final_rank']}")
    sv.close()
    assert b["pinf"] <= 1e-4
    assert abs(b["pobj"] - a["pobj"]) <= tol * (1 + abs(a["pobj"]))


def _traj_solve(solver_mod, name, shrink):
    sv = solver_mod.Solver(instance(name))
    if shrink is not None:
        sv.set_rank_shrink(shrink)
    res = sv.solve()
    t1, t2 = sv.trajectory(1), sv.trajectory(2)
    sv.close()
    return res, t1, t2


@pytest.mark.parametrize("name,want", [("mc_torus12x10", 7), ("mc_rand200", 8)])
def test_rank_shrink_hook(solver_mod, name, want):
    """9. With the hook on the ADMM phase runs at the last phase-1 oracle rank; off, nothing differs."""
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "solves.json")))
    entry = next(e for e in gold if e["instance"] == name)
    assert entry["json"]["trajectory"]["phase_1"]["oracle_rank"][-1] == want   # the reference's own run
    plain, p1, p2 = _traj_solve(solver_mod, name, None)
    off, o1, o2 = _traj_solve(solver_mod, name, 0)
    hook, h1, h2 = _traj_solve(solver_mod, name, TOL)
    print(f"{name}: plain rank {plain['final_rank']} admm {plain['admm_iter']} pobj {plain['pobj']!r} gap {plain['gap']:.3e}; "
          f"hook rank {hook['final_rank']} admm {hook['admm_iter']} pobj {hook['pobj']!r} gap {hook['gap']:.3e} "
          f"pinf {hook['pinf']:.3e}; phase-2 ranks {h2[0]}")
    # off: field for field what a context that never called it returns
    assert (p1, p2) == (o1, o2)
    for key in plain:
        if not key.endswith("time"):
            assert plain[key] == off[key], key
    assert h1 == p1 and h1[1][-1] == want
    assert len(h2[0]) >= 1 and all(c == want for c in h2[0])
    assert hook["final_rank"] == want
    tol = 10 * (plain["gap"] + hook["gap"])
    assert hook["pinf"] <= 1e-4
    assert abs(hook["pobj"] - plain["pobj"]) <= tol * (1 + abs(plain["pobj"]))


def test_compress_with_registered_cuts(solver_mod, inst_mod):
    """10. A cut-carrying context: the cut list is untouched, the slacks move by what was dropped."""
    import tri_util as tu
    n, r, k = 33, 19, 7
    sv = solver_mod.Solver(coo=inst_mod.coo_arrays(rand_problem(inst_mod, n)))
    start(sv, factor(n, r, k, seed=23))
    i, j, kk = tu.triples(n)
    rng = np.random.default_rng(29)
    pick = rng.choice(i.size, size=20, replace=False)
    cuts = np.stack([i[pick], j[pick], kk[pick], rng.integers(0, 4, size=20)], axis=1).astype(np.int32)
    assert sv.append_cuts(cuts, carry=True) == 20 and sv.get_rank() == [r, 1]
    have, (slack0, lam0) = sv.cuts(), sv.cuts_state()
    lp0 = sv.get_factor(R)[n * r:]
    out = sv.compress(rel_tol=TOL)
    assert out["ranks"] == [k, 1] and sv.get_rank() == [k, 1]
    assert np.array_equal(sv.cuts(), have)
    slack1, lam1 = sv.cuts_state()
    print(f"slacks move by {amax(slack1 - slack0):.3e}, lost {out['lost'][0]:.3e}")
    assert amax(slack1 - slack0) <= 3 * out["lost"][0] / 1.0 + 1e-12   # min b = 1
    assert lam1.tobytes() == lam0.tobytes()
    assert sv.get_factor(R)[n * k:].tobytes() == lp0.tobytes()
    sv.close()


def _code(solver_mod, call):
    with pytest.raises(solver_mod.CompressError) as ei:
        call()
    assert ei.value.message
    return ei.value.code


def test_refusals_change_nothing(solver_mod, inst_mod):
    """11. Every refusal with its code; the context is as before."""
    code = lambda call: _code(solver_mod, call)
    path = instance("mc_torus12x10")
    sv = solver_mod.Solver(path)
    assert code(lambda: sv.compress()) == -6 and code(lambda: sv.spectrum()) == -6   # no ranks
    n, r = sv.dims[0], 6
    X = factor(n, r, 3, seed=31)
    start(sv, X)
    flat = sv.get_factor(R)
    for which in (D, G, V, S0, 17, -1):
        assert code(lambda: sv.compress(which=which)) == -11
        assert code(lambda: sv.spectrum(which=which)) == -11
    assert code(lambda: sv.compress(ranks=[-1])) == -2
    assert code(lambda: sv.compress(ranks=[r + 1])) == -2
    for bad in (-1e-3, 1.0, 2.0, float("nan")):
        assert code(lambda: sv.compress(rel_tol=bad)) == -2
        assert code(lambda: sv.spectrum(rel_tol=bad)) == -2
    assert code(lambda: sv.compress(slack=-1)) == -2
    assert code(lambda: sv.set_rank_shrink(1.0)) == -2 and code(lambda: sv.set_rank_shrink(1e-6, slack=-1)) == -2
    assert sv.get_rank() == [r] and sv.get_factor(R).tobytes() == flat.tobytes()
    assert sv.compress(ranks=[0], rel_tol=TOL)["ranks"] == [3]   # 0: the rule
    sv.close()
    lp = solver_mod.Solver(instance("mc_lp60"))
    lp.set_rank([4, 1])
    for bad in (2, -1):
        assert code(lambda: lp.compress(ranks=[2, bad])) == -2
    assert lp.get_rank() == [4, 1]
    assert lp.compress(ranks=[2, 0])["ranks"] == [2, 1] and lp.compress(ranks=[2, 1])["ranks"] == [2, 1]
    lp.close()
    # a loopback-sharded context
    grp = solver_mod.LoopbackGroup(2)
    codes, errs = [None, None], []

    def work(rk):
        try:
            s2 = solver_mod.Solver(path)
            s2.shard_loopback(grp, rk)
            codes[rk] = (code(lambda: s2.compress()), code(lambda: s2.spectrum()))
            s2.close()
        except BaseException as e:   # reported below
            errs.append(f"rank {rk}: {e!r}")

    ts = [threading.Thread(target=work, args=(rk,), daemon=True) for rk in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not any(t.is_alive() for t in ts), "sharded refusal did not return"
    grp.close()
    assert not errs, errs
    assert codes == [(-3, -3), (-3, -3)]


def test_cut_loop_with_compression(solver_mod, inst_mod):
    """cut_loop(compress_tol=...) records the rank at the end of every round (AUG_RANK may grow a
    compressed start again: rank_max is untouched); None keeps today's records.  Measured: ranks
    10, 8, 12 over the three rounds."""
    problem = inst_mod.maxcut_torus_problem(12, 10, 120)
    out = []
    for tol in (None, TOL):
        sv = solver_mod.Solver(coo=inst_mod.coo_arrays(problem))
        out.append(sv.cut_loop(2, 64, compress_tol=tol))
        sv.close()
    plain, comp = out
    print("plain", [(q["n_cuts"], q["pobj"]) for q in plain], "compressed", [(q["n_cuts"], q["pobj"], q["rank"]) for q in comp])
    assert all("rank" not in q for q in plain) and all(q["rank"] >= 1 for q in comp)
    assert len(comp) == len(plain) >= 2
    assert comp[0]["pobj"] == plain[0]["pobj"]   # round 0 is the plain solve either way
    assert [q["n_cuts"] for q in comp] == [q["n_cuts"] for q in plain]
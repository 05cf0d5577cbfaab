"""Rank-one dense constraint matrices as a factor on the FP64 matrix cores: a
cone that factors its coefficients A = sigma a a^T keeps V = [a_1 .. a_p] in place of p full
matrices; k_r1_vtx forms V^T X (and V^T Z in the same pass), k_r1_vals the terms' values,
k_r1_apply the adjoint V diag(w sigma) (V^T X), and every host-driven operator adds those terms.
The reference evaluates the same matrices through its dense branches, so its fixtures
(scripts/make_golden_rank1.py) are the oracle, next to numpy on the expanded matrices:

* kernels_r1_64 / kernels_r1_70x37: one call of each operator (bars of test_gpu_densea.py);
* steps_r1_64 / r1_70x37 / r1_200: K in {1,2,3,5,8} trips of the inner loop to 1e-9, factored,
  on the stack (LRS_RANK1_A=0, LRS_DENSE_A=1) and on the slots (both 0);
* admm_sweep_r1_70x37: one ADMM sweep + dual update;
* solves_rank1.json: the whole solve of r1_64;
* lrs_load_coo_rank1: the same instance passed as terms, its refusals, and a capacity case with
  more terms than rows (p = 403 > n = 192) that no stack is built for.
"""
import importlib
import json
import os
import threading

import numpy as np
import pytest

from golden_util import GOLDEN, rel_err, split_inputs
from rank1_util import EXPECT_RANK1, args_of, env, r1_path

pytestmark = pytest.mark.gpu
TOL = 1e-10
STEP_TOL = 1e-9
# (LRS_RANK1_A, LRS_DENSE_A): factored (the other dense coefficients on the stack / in the slots),
# the stack alone, the slots alone
FACTOR, FACTOR_SLOTS, STACK, SLOTS = ("1", "1"), ("1", "0"), ("0", "1"), ("0", "0")


@pytest.fixture(scope="module")
def solver_mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.solver")


@pytest.fixture(scope="module")
def inst_mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.instances")


@pytest.fixture(scope="module")
def gen_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("rank1")


def _load(solver_mod, path, mode, coo=None, **extra):
    with env(LRS_RANK1_A=mode[0], LRS_DENSE_A=mode[1], **extra):
        return solver_mod.Solver(path, coo=coo)


def _dense_problem(problem, terms=()):
    """C (per block) and {(constraint 0-based, block 0-based): full symmetric matrix} of an
    in-memory problem, the rank-one terms added as sigma a a^T."""
    m, dims, b, entries = problem
    Cs = [np.zeros((d, d)) for d in dims]
    A = {}
    for con, blk, ii, jj, vv in entries:
        con = np.asarray(con)
        blk = np.broadcast_to(np.asarray(blk), con.shape)
        for c, bk, i, j, v in zip(con.tolist(), blk.tolist(), np.asarray(ii).tolist(), np.asarray(jj).tolist(),
                                  np.asarray(vv, dtype=float).tolist()):
            if abs(v) < 1e-12:
                continue
            M = Cs[bk - 1] if c == 0 else A.setdefault((c - 1, bk - 1), np.zeros((dims[bk - 1], dims[bk - 1])))
            v = -v if c == 0 else v
            M[i - 1, j - 1] += v
            if i != j:
                M[j - 1, i - 1] += v
    for con, blk, sigma, a in terms:
        n = dims[blk - 1]
        A[(con - 1, blk - 1)] = A.get((con - 1, blk - 1), np.zeros((n, n))) + sigma * np.outer(a, a)
    return m, dims, np.asarray(b, dtype=float), Cs, A


def _numpy_ops(dense, rank, R, D, lam, cvs_in, rho):
    """q1, q2, A(R R^T) and the gradient 2 (C + sum_i M1_i A_i) R, M1 = -lam - rho b + rho cvs
    (lorads_alm.c:45-49), from the full matrices.  Factors are the reference's: per cone n x rank,
    column-major."""
    m, dims, b, Cs, A = dense
    off = np.concatenate([[0], np.cumsum([d * rank for d in dims])])
    Rk = [R[off[k]:off[k + 1]].reshape(rank, dims[k]).T for k in range(len(dims))]
    Dk = [D[off[k]:off[k + 1]].reshape(rank, dims[k]).T for k in range(len(dims))]
    q1, q2, cvs = np.zeros(m), np.zeros(m), np.zeros(m)
    for (i, k), M in A.items():
        MD = M @ Dk[k]
        q1[i] += 2.0 * np.sum(Rk[k] * MD)
        q2[i] += np.sum(Dk[k] * MD)
        cvs[i] += np.sum(Rk[k] * (M @ Rk[k]))
    M1 = -lam - rho * b + rho * cvs_in
    S = [c.copy() for c in Cs]
    for (i, k), M in A.items():
        S[k] += M1[i] * M
    G = np.concatenate([(2.0 * S[k] @ Rk[k]).T.ravel() for k in range(len(dims))])
    return q1, q2, cvs, G


# ---- 1. the path taken and its bytes
def test_paths_and_bytes(solver_mod, gen_dir):
    sv = _load(solver_mod, r1_path("r1_200", gen_dir), ("1", None))
    assert sv.dense_a_info(0)[0] == 20 and sv.dense_a_info(0)[2] == 0       # n_dense counts them, no stack
    assert sv.rank1_info(0) == (20, True, 8 * 200 * 32)                     # ldp = 32: 20 terms in two MFMA tiles
    sv.close()
    path = r1_path("r1_64", gen_dir)
    sv = _load(solver_mod, path, FACTOR)
    assert sv.dense_a_info(0) == (6, True, 8 * 64 * 64)                     # one stack matrix
    assert sv.rank1_info(0) == (5, True, 8 * 64 * 16)                       # five terms
    sv.close()
    sv = _load(solver_mod, path, FACTOR_SLOTS)
    assert sv.dense_a_info(0) == (6, False, 0) and sv.rank1_info(0) == (5, True, 8 * 64 * 16)
    sv.close()
    sv = _load(solver_mod, path, STACK)
    assert sv.dense_a_info(0) == (6, True, 6 * 8 * 64 * 64) and sv.rank1_info(0) == (0, False, 0)
    sv.set_rank([4])
    with pytest.raises(RuntimeError, match="no rank-one factor"):
        sv.time_rank1(0, 1)
    sv.close()
    sv = _load(solver_mod, path, (None, None))   # detected, the cone below the automatic threshold
    assert sv.rank1_info(0) == (5, False, 0) and sv.dense_a_info(0) == (6, False, 0)
    sv.close()


def test_time_rank1_reports_bytes(solver_mod, gen_dir):
    sv = _load(solver_mod, r1_path("r1_200", gen_dir), ("1", None))
    sv.set_rank([11])
    sv.set_factor(solver_mod.R, np.random.default_rng(0).standard_normal(200 * 11))
    ms, nbytes = sv.time_rank1(0, 3)
    sv.close()
    assert ms > 0
    assert nbytes == 8 * 200 * (32 + 16)   # V's 32 padded columns and R's rows at the pitch 16 of rank 11


# ---- 2. one call of each operator: the reference's fixture and numpy on the expanded matrices
@pytest.mark.parametrize("mode", [FACTOR, FACTOR_SLOTS])
@pytest.mark.parametrize("name", ["r1_64", "r1_70x37"])
def test_operators_match_reference_and_numpy(solver_mod, inst_mod, gen_dir, name, mode):
    z = np.load(os.path.join(GOLDEN, f"kernels_{name}.npz"))
    g = {k: z[k] for k in z.files}
    s = split_inputs(g)
    problem, _ = inst_mod.rank_one_constraints_problem(**args_of(name))
    nq1, nq2, ncvs, nG = _numpy_ops(_dense_problem(problem), s["rank"], s["R"], s["D"], s["lam"], s["cvs"], s["rho"])
    sv = _load(solver_mod, r1_path(name, gen_dir), mode)
    assert sv.rank1_info(0)[1]
    sv.set_rank([s["rank"]] * len(s["dims"]))
    S = solver_mod
    sv.set_factor(S.R, s["R"])
    sv.set_factor(S.D, s["D"])
    q1, p1, q2, p2 = sv.q12()
    e = {"q1": rel_err(q1, g["q1"]), "q2": rel_err(q2, g["q2"])}
    en = {"q1": rel_err(q1, nq1), "q2": rel_err(q2, nq2)}
    cvs, pinf, pobj = sv.constr_rr()
    e["cvs"] = rel_err(cvs, g["cvs_rr"])
    en["cvs"] = rel_err(cvs, ncvs)
    auv, _ = sv.auv(S.R, S.D)
    en["auv"] = rel_err(2.0 * auv, nq1)
    sv.set_vec(S.LAMBDA, s["lam"])
    sv.set_vec(S.CVS, s["cvs"])
    G, lag = sv.grad(s["rho"])
    e["grad"] = rel_err(G, g["grad"])
    en["grad"] = rel_err(G, nG)
    sv.q12()
    tau, rn = sv.line_search(s["rho"])
    sv.set_factor(S.U, s["U"]); sv.set_factor(S.V, s["V"])
    sv.set_vec(S.LAMBDA, s["lam"])
    u, rhs, it = sv.admm_half(s["rho_admm"], s["cg_tol"])
    e["rhs"] = rel_err(rhs, g["rhs_cg"])
    e["u_cg"] = rel_err(u, g["u_cg"])
    print(name, mode, e, "numpy", en, "p1", p1, g["p1"], "p2", p2, g["p2"], "pinf", pinf, g["pinf_rr"], "lag", lag,
          g["lag"], "tau", tau, g["tau"], "cg", it, g["cg_iters"])
    sv.close()
    for key in ("q1", "q2", "cvs", "grad", "rhs"):
        assert e[key] < TOL, (key, e[key])
    for key, v in en.items():
        assert v < TOL, ("numpy", key, v)
    assert abs(p1 - g["p1"]) <= TOL * max(1, abs(g["p1"])) and abs(p2 - g["p2"]) <= TOL * max(1, abs(g["p2"]))
    assert abs(pinf - g["pinf_rr"]) <= TOL * max(1, abs(g["pinf_rr"]))
    assert abs(pobj - g["pobj_rr"]) <= TOL * max(1, abs(g["pobj_rr"]))
    assert abs(lag - g["lag"]) <= TOL * g["lag"]
    assert rn == int(g["rootnum"])
    assert abs(tau - g["tau"]) <= 1e-9 * max(1, abs(g["tau"]))
    assert e["u_cg"] < 1e-6
    assert abs(it - g["cg_iters"]) <= max(2, 0.1 * g["cg_iters"])


def test_adjoint_matches_numpy(solver_mod, inst_mod, gen_dir):
    """lrs_op_adjoint: scale (C + sum_i y_i A_i) R on the factor path against the full matrices."""
    name = "r1_70x37"
    z = np.load(os.path.join(GOLDEN, f"kernels_{name}.npz"))
    s = split_inputs({k: z[k] for k in z.files})
    problem, _ = inst_mod.rank_one_constraints_problem(**args_of(name))
    m, dims, b, Cs, A = _dense_problem(problem)
    y = np.random.default_rng(3).standard_normal(m)
    rank = s["rank"]
    off = np.concatenate([[0], np.cumsum([d * rank for d in dims])])
    Sm = [c.copy() for c in Cs]
    for (i, k), M in A.items():
        Sm[k] += y[i] * M
    want = np.concatenate([(0.5 * Sm[k] @ s["R"][off[k]:off[k + 1]].reshape(rank, dims[k]).T).T.ravel()
                           for k in range(len(dims))])
    sv = _load(solver_mod, r1_path(name, gen_dir), FACTOR)
    sv.set_rank([rank] * len(dims))
    sv.set_factor(solver_mod.R, s["R"])
    got = sv.adjoint(y, solver_mod.R, 0.5)
    sv.close()
    assert rel_err(got, want) < TOL


# ---- 3. K trips of the inner loop
def _steps_check(sv, z, ks=None):
    for K in ks or [int(k) for k in z["ks"]]:
        trips = z[f"K{K}_trips"]
        assert trips.shape[0] == K
        d = sv.alm_steps(K, reoptLevel=0)
        assert d["inner"] == K, (K, d["inner"])
        tau, rn, lag, pinf = trips[K - 1]
        errs = {key: rel_err(d[key], z[f"K{K}_{key}"]) for key in ("R", "G", "cvs", "s", "y")}
        lam = z[f"K{K}_lam"]
        if np.linalg.norm(lam) > 0:
            errs["lam"] = rel_err(d["lam"], lam)
        beta = float(z[f"K{K}_beta"][0])
        print(K, "tau", d["tau"], tau, "lag", d["lag"], lag, "pinf", d["pinf"], pinf, "beta", d["beta"], beta, errs)
        assert abs(d["tau"] - tau) <= STEP_TOL * abs(tau), (K, d["tau"], tau)
        assert abs(d["lag"] - lag) <= STEP_TOL * abs(lag), (K, d["lag"], lag)
        assert abs(d["pinf"] - pinf) <= STEP_TOL * max(abs(pinf), 1e-300), (K, d["pinf"], pinf)
        assert abs(d["beta"] - beta) <= STEP_TOL * abs(beta), (K, d["beta"], beta)
        for key, e in errs.items():
            assert e < STEP_TOL, (K, key, e)


@pytest.mark.parametrize("mode", [("1", None), STACK, SLOTS], ids=["factor", "stack", "slots"])
@pytest.mark.parametrize("name", ["r1_64", "r1_70x37", "r1_200"])
def test_steps_match_reference(solver_mod, gen_dir, name, mode):
    """Ranks 9 (r1_64), 9 and 7 (r1_70x37), 11 (r1_200): none a multiple of 16.  r1_64: slots,
    one full matrix and five terms in one cone; r1_70x37: n = 70, a term with entries in the second
    cone; r1_200: 20 terms (two MFMA tiles of terms, the second ragged), no stack, four row chunks
    of 64, 64, 64 and 8 rows."""
    z = np.load(os.path.join(GOLDEN, f"steps_{name}.npz"))
    sv = _load(solver_mod, r1_path(name, gen_dir), mode)
    assert sv.rank1_info(0)[1] == (mode[0] == "1")
    _steps_check(sv, z)
    sv.close()


def test_steps_cross_ragged_row_chunks(solver_mod, gen_dir):
    """LRS_R1_CHUNK=48 (white box): k_r1_vtx takes r1_200's rows in four chunks of 48 and one of
    8, so its partials cross four chunk boundaries with a ragged tail."""
    z = np.load(os.path.join(GOLDEN, "steps_r1_200.npz"))
    with env(LRS_R1_CHUNK="48"):
        sv = _load(solver_mod, r1_path("r1_200", gen_dir), ("1", None))
        _steps_check(sv, z, ks=[3, 8])
        sv.close()


def test_single_workgroup_paths_decline(solver_mod, gen_dir):
    """LRS_SMALL=1 / LRS_SMALL_CG=1 ask for the single-workgroup loops, which see the slots only: a
    cone with a factor keeps the operator-composed loop (the trips still match) and the stage
    timers refuse."""
    z = np.load(os.path.join(GOLDEN, "steps_r1_64.npz"))
    with env(LRS_SMALL="1", LRS_SMALL_CG="1"):
        sv = _load(solver_mod, r1_path("r1_64", gen_dir), FACTOR_SLOTS)
        _steps_check(sv, z, ks=[3])
        assert sv.kernel_path() != 4
        with pytest.raises(RuntimeError, match="operator-composed"):
            sv.time_stages(1)
        sv.close()


# ---- 4. the ADMM sweep
def test_admm_sweep_matches_reference(solver_mod, gen_dir):
    name = "r1_70x37"
    g = np.load(os.path.join(GOLDEN, f"admm_sweep_{name}.npz"))
    z = np.load(os.path.join(GOLDEN, f"kernels_{name}.npz"))
    s = split_inputs({k: z[k] for k in z.files})
    dims, rank = s["dims"], s["rank"]
    sv = _load(solver_mod, r1_path(name, gen_dir), FACTOR)
    S = solver_mod
    sv.set_rank([rank] * len(dims))
    sv.set_factor(S.U, s["U"]); sv.set_factor(S.V, s["V"])
    sv.set_vec(S.LAMBDA, s["lam"])
    sv.admm_constr()
    its = []
    for cone in range(len(dims)):
        for side in (0, 1):
            _, _, it = sv.admm_half(s["rho_admm"], float(g["cg_tol"]), cone=cone, side=side, init=False)
            its.append(it)
    sv.dual_update(s["rho_admm"])
    U, V, lam = sv.get_factor(S.U), sv.get_factor(S.V), sv.get_vec(S.LAMBDA)
    sv.close()
    e = {"U": rel_err(U, g["U"]), "V": rel_err(V, g["V"]), "lam": rel_err(lam, g["lam"])}
    print(e, its, g["cg_last"], g["cg_total"])
    for key, v in e.items():
        assert v < 1e-6, (key, v)
    for c in range(len(dims)):
        ref = float(g["cg_last"][c])
        bar = 0.5 if ref > dims[c] * rank else 0.25
        assert abs(its[2 * c + 1] - ref) <= max(2, bar * ref), (c, its, g["cg_last"])
    assert abs(sum(its) - float(g["cg_total"])) <= max(4, 0.15 * float(g["cg_total"])), (its, g["cg_total"])


# ---- 5. the whole solve
def _solves():
    with open(os.path.join(GOLDEN, "solves_rank1.json")) as f:
        return {g["instance"]: g for g in json.load(f)}


def _check_solve(pobj, gap, pinf, g):
    j = g["json"]["metrics"]
    bar = 10 * max(gap, j["primal_dual_gap"])
    err = abs(pobj - j["primal_obj"]) / (1 + abs(j["primal_obj"]) + abs(j["dual_obj"]))
    print(g["instance"], "pobj", pobj, j["primal_obj"], "err", err, "bar", bar, "pinf", pinf)
    assert pinf <= 1e-4
    assert err <= bar, (pobj, j["primal_obj"], err, bar)


def test_solve_matches_reference(solver_mod, gen_dir):
    g = _solves()["r1_64"]
    sv = _load(solver_mod, r1_path("r1_64", gen_dir), FACTOR)
    res = sv.solve(reoptLevel=0)
    sv.close()
    _check_solve(res["pobj"], res["gap"], res["pinf"], g)
    assert res["final_rank"] == g["json"]["trajectory"]["phase_2"]["curr_rank"][-1]


def test_cli_solve_matches_reference(solver_mod, gen_dir, tmp_path, monkeypatch):
    """No new flag: the .dat-s file takes the path by detection."""
    monkeypatch.setenv("LRS_RANK1_A", "1")
    g = _solves()["r1_64"]
    out = tmp_path / "o.json"
    ok, t, pobj = solver_mod.run_lorads(r1_path("r1_64", gen_dir), out, {"reoptLevel": "0"})
    assert ok and t > 0
    js = json.load(open(out))
    mt = js["metrics"]
    _check_solve(mt["primal_obj"], mt["primal_dual_gap"], mt["constr_violation_l1"], g)
    assert js["trajectory"]["phase_2"]["curr_rank"][-1] == g["json"]["trajectory"]["phase_2"]["curr_rank"][-1]


# ---- 6. dual infeasibility
@pytest.mark.parametrize("mode", [FACTOR, FACTOR_SLOTS], ids=["stack+factor", "factor"])
def test_dual_infeasibility_matches_dense_eigensolve(solver_mod, inst_mod, gen_dir, mode):
    """lambda_min(C - sum_i lambda_i A_i) at r1_64's final multipliers against numpy's dense
    eigensolve of the same S (bar of test_gpu_dinf.py: 1e-2 relative, dsaupd's tolerance); the
    Lanczos product takes the terms through the factor kernels at r = 1."""
    sv = _load(solver_mod, r1_path("r1_64", gen_dir), mode)
    sv.solve(reoptLevel=0)
    lam = sv.get_vec(solver_mod.LAMBDA)
    l1, lmin = sv.dual_infeasibility()
    sv.close()
    problem, _ = inst_mod.rank_one_constraints_problem(**args_of("r1_64"))
    m, dims, b, Cs, A = _dense_problem(problem)
    Sm = Cs[0].copy()
    for (i, k), M in A.items():
        Sm -= lam[i] * M
    ref = float(np.linalg.eigvalsh(Sm)[0])
    cn1 = sum(float(np.abs(c).sum()) for c in Cs)
    eps23 = float(np.finfo(float).eps) ** (2.0 / 3.0)
    bar = 1e-2 * max(abs(ref), eps23) + 1e-3 * 1e-5 * (1 + cn1) + 1e-12   # test_gpu_dinf.py's bar()
    print("lambda_min", lmin[0], ref, "bar", bar, "l1", l1)
    assert ref <= lmin[0] + 1e-12 * max(1.0, abs(ref))       # a Ritz value bounds lambda_min from above
    assert abs(lmin[0] - ref) <= bar, (lmin[0], ref)
    assert abs(l1 - abs(min(lmin[0], 0.0)) / (1 + cn1)) <= 1e-12 + 1e-9 * l1


# ---- 7. reproducibility
def test_five_trips_bitwise_reproducible(solver_mod, gen_dir):
    path = r1_path("r1_70x37", gen_dir)
    out = []
    for _ in range(2):
        sv = _load(solver_mod, path, FACTOR)
        out.append(sv.alm_steps(5, reoptLevel=0))
        sv.close()
    a, b = out
    assert a["tau"] == b["tau"] and a["lag"] == b["lag"] and a["pinf"] == b["pinf"]
    for key in ("R", "G", "cvs", "s", "y"):
        assert np.array_equal(a[key], b[key]), key


# ---- 8. sharded contexts refuse
def test_sharded_context_refuses_factor(solver_mod, gen_dir):
    path = r1_path("r1_64", gen_dir)
    group = solver_mod.LoopbackGroup(2)
    svs = [_load(solver_mod, path, FACTOR_SLOTS) for _ in range(2)]
    errs = [None, None]

    def shard(rank):   # collective over the group's threads (both meet in its barrier)
        try:
            svs[rank].shard_loopback(group, rank)
        except RuntimeError as e:
            errs[rank] = str(e)

    th = [threading.Thread(target=shard, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(60)
        assert not t.is_alive()
    for e in errs:
        assert e is not None and "rank-one factor" in e, errs
    for sv in svs:
        sv.close()
    group.close()
    sv = _load(solver_mod, path, FACTOR_SLOTS)   # the process goes on
    assert sv.alm_steps(1, reoptLevel=0)["inner"] == 1
    sv.close()


# ---- 9. lrs_load_coo_rank1
def test_coo_terms_match_file(solver_mod, inst_mod, gen_dir):
    """r1_64 with its five coefficients passed as terms (never expanded) against the file load:
    the same ranks, the same rank1_info, five trips within 1e-9."""
    a = _load(solver_mod, r1_path("r1_64", gen_dir), FACTOR)
    problem, terms = inst_mod.rank_one_constraints_problem(**args_of("r1_64"), expand=False)
    coo = dict(inst_mod.coo_arrays(problem), terms=terms)
    b = _load(solver_mod, None, ("0", "1"), coo=coo)   # factored whatever LRS_RANK1_A says
    assert b.rank1_info(0) == a.rank1_info(0) == (5, True, 8 * 64 * 16)
    assert b.dense_a_info(0) == a.dense_a_info(0)
    da, db = a.alm_steps(5, reoptLevel=0), b.alm_steps(5, reoptLevel=0)
    ra, rb = a.get_rank(), b.get_rank()
    a.close(); b.close()
    assert ra == rb
    assert abs(da["tau"] - db["tau"]) <= STEP_TOL * abs(da["tau"])
    for key in ("R", "G", "cvs"):
        assert rel_err(db[key], da[key]) < STEP_TOL, key


def test_coo_terms_refusals(solver_mod, inst_mod):
    problem, terms = inst_mod.rank_one_constraints_problem([20, 12], [6, 4], 3, 2, 0, None, None, 0.0, None, False, 1,
                                                           expand=False)
    base = inst_mod.coo_arrays(problem)
    a = terms[0][3]
    lp = inst_mod.coo_arrays((problem[0], [20, 12, -3], problem[2], problem[3]))
    for bad, coo, what in [((0, 1, 1.0, a), base, "constraint 0"), ((11, 3, 1.0, np.ones(3)), lp, "LP block"),
                           ((1, 1, 1.0, a), base, "explicit entries")]:
        with pytest.raises(RuntimeError, match=what):
            solver_mod.Solver(None, coo=dict(coo, terms=[bad]))


def test_coo_sparse_term_lands_in_slots(solver_mod, inst_mod):
    """A term whose expansion stays within 10 % of the lower triangle is expanded into entries:
    no factor, and the constraint values are numpy's."""
    n = 40
    problem, _ = inst_mod.rank_one_constraints_problem([n], [8], 3, 0, 0, None, None, 0.0, None, False, 2)
    m, dims, b, entries = problem
    a = np.zeros(n)
    a[[3, 7, 20, 31]] = [1.5, -2.0, 0.5, 1.0]   # 10 entries of 820
    dense = np.random.default_rng(4).standard_normal(n)
    coo = dict(inst_mod.coo_arrays((m + 2, dims, np.concatenate([b, [a @ a, -(dense @ dense)]]), entries)),
               terms=[(m + 1, 1, 1.0, a), (m + 2, 1, -1.0, dense)])
    sv = _load(solver_mod, None, (None, None), coo=coo)
    assert sv.rank1_info(0) == (1, True, 8 * n * 16)   # the dense one alone
    assert sv.dense_a_info(0)[0] == 1
    rank = 5
    sv.set_rank([rank])
    R = np.random.default_rng(6).standard_normal(n * rank)
    sv.set_factor(solver_mod.R, R)
    cvs, _, _ = sv.constr_rr()
    sv.close()
    Rm = R.reshape(rank, n).T
    assert abs(cvs[m] - np.sum((a @ Rm) ** 2)) <= TOL * np.sum((a @ Rm) ** 2)
    assert abs(cvs[m + 1] + np.sum((dense @ Rm) ** 2)) <= TOL * np.sum((dense @ Rm) ** 2)


def test_coo_capacity_more_terms_than_rows(solver_mod, inst_mod):
    """n = 192, 403 terms (p > n, p no multiple of 16), 50 sparse constraints: loads without a
    stack (403 full matrices would be 119 MB; the factor is 0.6 MB), the operators agree with
    numpy on the expanded matrices, three trips run."""
    n, p, ms, rank = 192, 403, 50, 11
    problem, terms = inst_mod.rank_one_constraints_problem([n], [ms], 4, p, 0, 7, 11, 0.33, None, False, 192,
                                                           expand=False)
    coo = dict(inst_mod.coo_arrays(problem), terms=terms)
    sv = _load(solver_mod, None, (None, None), coo=coo)
    assert sv.dense_a_info(0) == (p, False, 0)
    assert sv.rank1_info(0) == (p, True, 8 * n * 416)
    rng = np.random.default_rng(8)
    m = problem[0]
    R, D = rng.standard_normal(n * rank), rng.standard_normal(n * rank)
    lam, cvs_in, rho = rng.standard_normal(m), rng.standard_normal(m), 1.7
    nq1, nq2, ncvs, nG = _numpy_ops(_dense_problem(problem, terms), rank, R, D, lam, cvs_in, rho)
    S = solver_mod
    sv.set_rank([rank])
    sv.set_factor(S.R, R); sv.set_factor(S.D, D)
    q1, _, q2, _ = sv.q12()
    cvs, _, _ = sv.constr_rr()
    sv.set_vec(S.LAMBDA, lam); sv.set_vec(S.CVS, cvs_in)
    G, _ = sv.grad(rho)
    e = {"q1": rel_err(q1, nq1), "q2": rel_err(q2, nq2), "cvs": rel_err(cvs, ncvs), "grad": rel_err(G, nG)}
    print(e)
    d = sv.alm_steps(3, reoptLevel=0)
    sv.close()
    for key, v in e.items():
        assert v < TOL, (key, v)
    assert d["inner"] == 3 and np.all(np.isfinite(d["R"])) and np.isfinite(d["lag"])

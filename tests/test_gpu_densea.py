"""Dense constraint matrices on the FP64 matrix cores: a cone on the dense-A
path (LRS_DENSE_A=1) keeps its SDP_COEFF_DENSE coefficients out of the slot pattern as a stack
of full matrices; k_dcon_ax forms T_i = A_i X with the dots <X, T_i>, <Z, T_i>, k_dcon_comb the
adjoint's combination, and every host-driven operator adds those terms.  The reference's own
dense branches (denseAUV, dataMatDenseMultiRkMatInnerProRkMat, dataMatDenseAddDenseSDPCoeff,
dsymm; data/lorads_sdp_data.c) are the oracle, through the fixtures of
scripts/make_golden_densea.py:

* kernels_da64 / kernels_da70x40: one call of each operator (bars of test_gpu_parity.py);
* steps_da64 / da70x40 / da200: K in {1,2,3,5,8} trips of the inner loop to 1e-9, on the dense
  path and, for the first two, on the slot path (LRS_DENSE_A=0) as well;
* admm_sweep_da70x40: one ADMM sweep + dual update (bars of test_capi.py);
* solves_densea.json: whole solves (pinf, final ranks, objectives within 10 x the larger gap).
"""
import importlib
import json
import os

import numpy as np
import pytest

from densea_util import EXPECT_DENSE, args_of, da_path, dense_a
from golden_util import GOLDEN, read_sdpa_dense, rel_err, split_inputs

pytestmark = pytest.mark.gpu
TOL = 1e-10
STEP_TOL = 1e-9


@pytest.fixture(scope="module")
def solver_mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.solver")


@pytest.fixture(scope="module")
def gen_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("densea")


def _load(solver_mod, path, mode, **kw):
    with dense_a(mode):
        return solver_mod.Solver(path, **kw)


# ---- 1. the path taken
@pytest.mark.parametrize("name", ["da64", "da70x40", "da200"])
def test_dense_a_info(solver_mod, gen_dir, name):
    path = da_path(name, gen_dir)
    for mode in ("1", "0"):
        sv = _load(solver_mod, path, mode)
        for cone, want in enumerate(EXPECT_DENSE[name]):
            n, on, nbytes = sv.dense_a_info(cone)
            assert n == len(want), (mode, cone, n)
            assert on == (mode == "1" and n > 0), (mode, cone, on)
            assert nbytes == (8 * n * sv.dims[cone] ** 2 if on else 0)
        if mode == "0":
            sv.set_rank([4] * len(sv.dims))
            with pytest.raises(RuntimeError, match="dense constraint-matrix path"):
                sv.time_dense_a(0, 1)
        sv.close()


# ---- 2. one call of each operator
@pytest.mark.parametrize("mode", ["1", "0"])
@pytest.mark.parametrize("name", ["da64", "da70x40"])
def test_operators_match_reference(solver_mod, gen_dir, name, mode):
    z = np.load(os.path.join(GOLDEN, f"kernels_{name}.npz"))
    g = {k: z[k] for k in z.files}
    s = split_inputs(g)
    sv = _load(solver_mod, da_path(name, gen_dir), mode)
    sv.set_rank([s["rank"]] * len(s["dims"]))
    S = solver_mod
    sv.set_factor(S.R, s["R"])
    sv.set_factor(S.D, s["D"])
    q1, p1, q2, p2 = sv.q12()
    e = {"q1": rel_err(q1, g["q1"]), "q2": rel_err(q2, g["q2"])}
    cvs, pinf, pobj = sv.constr_rr()
    e["cvs"] = rel_err(cvs, g["cvs_rr"])
    sv.set_vec(S.LAMBDA, s["lam"])
    sv.set_vec(S.CVS, s["cvs"])
    G, lag = sv.grad(s["rho"])
    e["grad"] = rel_err(G, g["grad"])
    sv.q12()
    tau, rn = sv.line_search(s["rho"])
    sv.set_factor(S.U, s["U"]); sv.set_factor(S.V, s["V"])
    sv.set_vec(S.LAMBDA, s["lam"])
    u, rhs, it = sv.admm_half(s["rho_admm"], s["cg_tol"])
    e["rhs"] = rel_err(rhs, g["rhs_cg"])
    e["u_cg"] = rel_err(u, g["u_cg"])
    print(name, mode, e, "p1", p1, g["p1"], "p2", p2, g["p2"], "pinf", pinf, g["pinf_rr"], "lag", lag, g["lag"],
          "tau", tau, g["tau"], "cg", it, g["cg_iters"])
    sv.close()
    for key in ("q1", "q2", "cvs", "grad", "rhs"):
        assert e[key] < TOL, (key, e[key])
    assert abs(p1 - g["p1"]) <= TOL * max(1, abs(g["p1"])) and abs(p2 - g["p2"]) <= TOL * max(1, abs(g["p2"]))
    assert abs(pinf - g["pinf_rr"]) <= TOL * max(1, abs(g["pinf_rr"]))
    assert abs(pobj - g["pobj_rr"]) <= TOL * max(1, abs(g["pobj_rr"]))
    assert abs(lag - g["lag"]) <= TOL * g["lag"]
    assert rn == int(g["rootnum"])
    assert abs(tau - g["tau"]) <= 1e-9 * max(1, abs(g["tau"]))
    assert e["u_cg"] < 1e-6
    assert abs(it - g["cg_iters"]) <= max(2, 0.1 * g["cg_iters"])


# ---- 3 / 4. K trips of the inner loop
def _steps_check(solver_mod, sv, z):
    for K in [int(k) for k in z["ks"]]:
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


@pytest.mark.parametrize("name,mode", [("da64", "1"), ("da70x40", "1"), ("da200", "1"), ("da64", "0"),
                                       ("da70x40", "0")])
def test_steps_match_reference(solver_mod, gen_dir, name, mode):
    """da64: r = 9 in a padded row, n = 64; da70x40: n = 70 (no multiple of 16), two cones, a
    constraint dense in one and sparse in the other; da200: several tiles, two full matrices."""
    z = np.load(os.path.join(GOLDEN, f"steps_{name}.npz"))
    sv = _load(solver_mod, da_path(name, gen_dir), mode)
    _steps_check(solver_mod, sv, z)
    sv.close()


def test_steps_with_dense_objective(solver_mod, gen_dir, monkeypatch):
    """A dense objective (LRS_DENSE_C=1) and dense constraints in one cone."""
    monkeypatch.setenv("LRS_DENSE_C", "1")
    z = np.load(os.path.join(GOLDEN, "steps_da64.npz"))
    sv = _load(solver_mod, da_path("da64", gen_dir), "1")
    _steps_check(solver_mod, sv, z)
    sv.close()


# ---- 5. the ADMM sweep
def test_admm_sweep_matches_reference(solver_mod, gen_dir):
    name = "da70x40"
    g = np.load(os.path.join(GOLDEN, f"admm_sweep_{name}.npz"))
    z = np.load(os.path.join(GOLDEN, f"kernels_{name}.npz"))
    s = split_inputs({k: z[k] for k in z.files})
    dims, rank = s["dims"], s["rank"]
    sv = _load(solver_mod, da_path(name, gen_dir), "1")
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


# ---- 6. whole solves
def _solves():
    with open(os.path.join(GOLDEN, "solves_densea.json")) as f:
        return {g["instance"]: g for g in json.load(f)}


def _check_solve(pobj, gap, pinf, g):
    j = g["json"]["metrics"]
    bar = 10 * max(gap, j["primal_dual_gap"])
    err = abs(pobj - j["primal_obj"]) / (1 + abs(j["primal_obj"]) + abs(j["dual_obj"]))
    print(g["instance"], "pobj", pobj, j["primal_obj"], "err", err, "bar", bar, "pinf", pinf)
    assert pinf <= 1e-4
    assert err <= bar, (pobj, j["primal_obj"], err, bar)


@pytest.mark.parametrize("name", ["da64", "da70x40"])
def test_solve_matches_reference(solver_mod, gen_dir, name):
    g = _solves()[name]
    sv = _load(solver_mod, da_path(name, gen_dir), "1")
    res = sv.solve(reoptLevel=0)
    sv.close()
    _check_solve(res["pobj"], res["gap"], res["pinf"], g)
    assert res["final_rank"] == g["json"]["trajectory"]["phase_2"]["curr_rank"][-1]


@pytest.mark.parametrize("name", ["da64", "da70x40"])
def test_cli_solve_matches_reference(solver_mod, gen_dir, tmp_path, name, monkeypatch):
    monkeypatch.setenv("LRS_DENSE_A", "1")
    g = _solves()[name]
    out = tmp_path / "o.json"
    ok, t, pobj = solver_mod.run_lorads(da_path(name, gen_dir), out, {"reoptLevel": "0"})
    assert ok and t > 0
    js = json.load(open(out))
    mt = js["metrics"]
    _check_solve(mt["primal_obj"], mt["primal_dual_gap"], mt["constr_violation_l1"], g)
    assert js["trajectory"]["phase_2"]["curr_rank"][-1] == g["json"]["trajectory"]["phase_2"]["curr_rank"][-1]


# ---- 7. dual infeasibility
def test_dual_infeasibility_matches_dense_eigensolve(solver_mod, gen_dir):
    """lambda_min(C - sum_i lambda_i A_i) at da64's final multipliers against numpy's dense
    eigensolve of the same S (bar of test_gpu_dinf.py: 1e-2 relative, dsaupd's tolerance)."""
    path = da_path("da64", gen_dir)
    sv = _load(solver_mod, path, "1")
    sv.solve(reoptLevel=0)
    lam = sv.get_vec(solver_mod.LAMBDA)
    l1, lmin = sv.dual_infeasibility()
    sv.close()
    m, dims, b, Cs, A = read_sdpa_dense(path)
    Sm = Cs[0].copy()
    for (i, blk), ents in A.items():
        acc = {}
        for r, c, v in ents:   # duplicates sum, as the presolve merges them
            acc[(r, c)] = acc.get((r, c), 0.0) + v
        for (r, c), v in acc.items():
            Sm[r, c] -= lam[i] * v
            if r != c:
                Sm[c, r] -= lam[i] * v
    ref = float(np.linalg.eigvalsh(Sm)[0])
    cn1 = sum(float(np.abs(c).sum()) for c in Cs)
    eps23 = float(np.finfo(float).eps) ** (2.0 / 3.0)
    bar = 1e-2 * max(abs(ref), eps23) + 1e-3 * 1e-5 * (1 + cn1) + 1e-12   # test_gpu_dinf.py's bar()
    print("lambda_min", lmin[0], ref, "bar", bar, "l1", l1)
    assert ref <= lmin[0] + 1e-12 * max(1.0, abs(ref))       # a Ritz value bounds lambda_min from above
    assert abs(lmin[0] - ref) <= bar, (lmin[0], ref)
    assert abs(l1 - abs(min(lmin[0], 0.0)) / (1 + cn1)) <= 1e-12 + 1e-9 * l1


# ---- 8. reproducibility
def test_five_trips_bitwise_reproducible(solver_mod, gen_dir):
    path = da_path("da70x40", gen_dir)
    out = []
    for _ in range(2):
        sv = _load(solver_mod, path, "1")
        out.append(sv.alm_steps(5, reoptLevel=0))
        sv.close()
    a, b = out
    assert a["tau"] == b["tau"] and a["lag"] == b["lag"] and a["pinf"] == b["pinf"]
    for key in ("R", "G", "cvs", "s", "y"):
        assert np.array_equal(a[key], b[key]), key


# ---- 9. sharded contexts refuse
def test_sharded_context_refuses_dense_path(solver_mod, gen_dir):
    import threading
    path = da_path("da64", gen_dir)
    group = solver_mod.LoopbackGroup(2)
    svs = [_load(solver_mod, path, "1") for _ in range(2)]
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
        assert e is not None and "dense constraint-matrix path" in e, errs
    for sv in svs:
        sv.close()
    group.close()
    # the process goes on: the same instance solves its first trips
    sv = _load(solver_mod, path, "1")
    assert sv.alm_steps(1, reoptLevel=0)["inner"] == 1
    sv.close()


# ---- 10. in-memory load
def test_coo_load_matches_file(solver_mod, gen_dir):
    inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")
    a = _load(solver_mod, da_path("da64", gen_dir), "1")
    b = _load(solver_mod, None, "1", coo=inst.coo_arrays(inst.dense_constraints_problem(**args_of("da64"))))
    assert b.dense_a_info(0)[:2] == (4, True)
    da, db = a.alm_steps(3, reoptLevel=0), b.alm_steps(3, reoptLevel=0)
    a.close(); b.close()
    assert da["tau"] == db["tau"]
    for key in ("R", "G", "cvs"):
        assert np.array_equal(da[key], db[key]), key

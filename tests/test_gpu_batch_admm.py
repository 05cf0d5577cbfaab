"""The ADMM meeting of a batched solve (lrs_solve_batch): members inside the ADMM
phase whose iteration is the one-workgroup form (k_small_cg a side, k_small_eval) file it and
park; one round runs all parked members' side-0 half-steps, side-1 half-steps and evaluations in
shared launches (k_small_cg_tab, k_small_eval_tab), a block a cone.  A block runs the same body
on the same arguments as the member's own launch, so every comparison against the solo solve
here is exact (bit for bit)."""
import importlib
import os

import numpy as np
import pytest

from golden_util import GOLDEN, instance

pytestmark = pytest.mark.gpu
# one cone and three cones, constant and slot objectives, and a 13 x 10 torus: its 130 rows take
# three rows a 16-lane group where the others (<= 128 rows) take two, so the set spans two kernel
# variants whatever the ranks are
SET = ["mc_torus12x10", "torus6x5", "theta40", "theta25x3", "torus13x10"]
KEYS = ("alm_inner", "admm_iter", "cg_iter", "status", "final_rank")
COUNTS = ("alm_inner", "alm_outer", "retcode", "final_rank")   # test_gpu_batch.py's, for the multi-launch paths


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.solver")


@pytest.fixture(scope="module")
def inst():
    return importlib.import_module("ltr-lowrank-sdp_amd.instances")


@pytest.fixture(scope="module")
def paths(inst, tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_admm_inst")
    p = {n: os.path.join(GOLDEN, "instances", f"{n}.dat-s")
         for n in ("mc_torus12x10", "mc_rand200", "theta40", "theta25x3", "rsparse60", "mc_lp60")}
    p["torus6x5"] = inst.maxcut_torus(str(d / "torus6x5.dat-s"), 6, 5, 11)
    p["torus13x10"] = inst.maxcut_torus(str(d / "torus13x10.dat-s"), 13, 10, 12)
    return p


def snapshot(mod, sv, res):
    """What a whole solve left behind: the result, both trajectories, the factors and vectors."""
    out = {"res": res, "traj1": sv.trajectory(1), "traj2": sv.trajectory(2), "rank": sv.get_rank(),
           "dims": list(sv.dims)}
    for name, f in (("R", mod.R), ("U", mod.U), ("V", mod.V)):
        out[name] = sv.get_factor(f)
    out["lam"] = sv.get_vec(mod.LAMBDA)
    out["cvs"] = sv.get_vec(mod.CVS)
    return out


def assert_bitwise(a, b, what):
    for k in KEYS:
        assert a["res"][k] == b["res"][k], (what, k, a["res"][k], b["res"][k])
    assert a["traj2"] == b["traj2"], what
    assert a["traj1"] == b["traj1"] and a["rank"] == b["rank"], what
    for k in ("R", "U", "V", "lam", "cvs"):
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in ("pobj", "dobj"):
        assert np.float64(a["res"][k]).tobytes() == np.float64(b["res"][k]).tobytes(), (what, k)


def solo(mod, path, **kw):
    sv = mod.Solver(path)
    res = sv.solve(**kw)
    out = snapshot(mod, sv, res)
    out["form"] = sv.admm_form()
    sv.close()
    return out


@pytest.fixture(scope="module")
def solos(mod, paths):
    """The set's whole solves at default parameters, each alone through lrs_solve (computed once,
    never changed)."""
    return {n: solo(mod, paths[n]) for n in SET}


def variant(n, r):
    """k_small_cg's instantiation for a cone of n rows at rank r: (elements a lane, rows a group)."""
    el, rows = -(-r // 16), -(-n // 64)
    rpg = 2 if rows <= 2 else 3 if rows <= 3 else 4 if rows <= 4 else 6 if rows <= 6 else 8
    return el, rpg


def test_whole_solves_bit_for_bit_and_the_rounds_ran(mod, paths, solos):
    for n in ("mc_torus12x10", "theta25x3"):   # the solo path repeats itself bit for bit
        assert_bitwise(solos[n], solo(mod, paths[n]), "solo repeat " + n)
    svs = [mod.Solver(paths[n]) for n in SET]
    b = mod.Batch()
    res = b.solve(svs)
    st, widths = b.admm_stats(), b.admm_round_widths()
    print("ADMM stats", st, "round widths", widths, "ALM stats", b.stats())
    variants = set()
    for n, sv, r in zip(SET, svs, res):
        got = snapshot(mod, sv, r)
        assert_bitwise(solos[n], got, n)
        assert solos[n]["res"]["admm_iter"] > 0, n
        assert sv.admm_form()[1], n
        variants.add(variant(max(got["dims"]), max(got["rank"])))
    assert st["launches"] >= 1 and st["widest"] >= 2 and st["alone"] == 0
    assert st["served"] >= len(SET)
    # at least two (EL, RPG) variants launched in one round: from the members' sizes and ranks,
    # and as the launcher counted them
    assert len(variants) >= 2, variants
    assert st["variants"] >= 2, st
    for sv in svs:
        sv.close()
    b.close()


def test_three_cones_in_the_table(mod, paths, solos):
    b = mod.Batch()
    sv = mod.Solver(paths["theta25x3"])
    res = b.solve([sv])
    st, widths = b.admm_stats(), b.admm_round_widths()
    print("theta25x3 alone:", st, widths)
    assert_bitwise(solos["theta25x3"], snapshot(mod, sv, res[0]), "theta25x3 alone")
    rounds = sum(widths.values())
    # every round: one launch a side with a block a cone, and the evaluation
    assert st["blocks"] == 3 and st["variants"] == 1 and st["widest"] == 1 and set(widths) == {1}
    assert st["launches"] == 3 * rounds and st["served"] == rounds and st["alone"] == 0
    assert rounds >= res[0]["admm_iter"] > 0
    other = mod.Solver(paths["theta40"])
    res = b.solve([sv, other])
    st = b.admm_stats()
    print("theta25x3 beside theta40:", st, b.admm_round_widths())
    assert_bitwise(solos["theta25x3"], snapshot(mod, sv, res[0]), "theta25x3 beside theta40")
    assert_bitwise(solos["theta40"], snapshot(mod, other, res[1]), "theta40 beside theta25x3")
    assert st["widest"] == 2 and st["alone"] == 0 and st["blocks"] >= 3
    sv.close()
    other.close()
    b.close()


def test_members_outside_the_quorum(mod, paths):
    """Members whose ADMM iteration is not the one-workgroup form (an LP block; whichever of
    rsparse60 and mc_rand200 the device says does not take it) run that phase on their own stream
    beside two members that meet.  The bars of test_gpu_batch.py's mixed batch: counts, trajectory
    and ranks for the multi-launch paths, bit for bit on the single-workgroup ones."""
    kw = dict(reoptLevel=0)
    cand = {n: solo(mod, paths[n], **kw) for n in ("mc_lp60", "rsparse60", "mc_rand200")}
    for n, s in cand.items():
        print(n, "cones on k_small_cg:", s["form"][0], "of", len(s["dims"]), "round form:", s["form"][1])
    outsiders = [n for n, s in cand.items() if not s["form"][1]]
    assert "mc_lp60" in outsiders
    # two members whose ADMM phases overlap: theta40 enters first and runs the longer phase
    inside = ["theta40", "theta25x3"]
    refs = {n: solo(mod, paths[n], **kw) for n in inside}
    assert all(refs[n]["form"][1] and refs[n]["res"]["admm_iter"] > 0 for n in inside)
    mem = outsiders + inside
    svs = [mod.Solver(paths[n]) for n in mem]
    b = mod.Batch()
    res = b.solve(svs, kw)
    st = b.admm_stats()
    print("mixed ADMM batch", mem, st, b.admm_round_widths())
    for n, sv, r in zip(mem, svs, res):
        got = snapshot(mod, sv, r)
        if n in inside:
            assert_bitwise(refs[n], got, n)
        else:
            a = cand[n]
            for k in COUNTS:
                assert a["res"][k] == r[k], (n, k, a["res"][k], r[k])
            assert a["traj1"] == got["traj1"] and a["rank"] == got["rank"], n
    assert st["alone"] >= 1 and st["widest"] == 2
    assert st["alone"] >= sum(cand[n]["res"]["admm_iter"] > 0 for n in outsiders)
    for sv in svs:
        sv.close()
    b.close()


def test_uneven_lengths(mod, inst):
    """14 of test_gpu_batch.py's tori (its generator's, 5 x 4 to 12 x 10, in its order), whole
    solves.  A torus whose solo solve ends with no ADMM iteration at all (phase 1 already meets the
    tolerances: admm_optimize returns at its entry) never calls the ADMM meeting, so it cannot
    count towards a round's width: the members are the first 14 that do iterate."""
    rng = np.random.default_rng(2024)
    shapes = [(5, 4), (12, 10)] + [(int(rng.integers(5, 13)), int(rng.integers(4, 11))) for _ in range(38)]
    coos, refs, kept = [], [], []
    for i, (r, c) in enumerate(shapes):
        coo = inst.coo_arrays(inst.maxcut_torus_problem(r, c, 100 + i))
        sv = mod.Solver(coo=coo)
        a = sv.solve()
        sv.close()
        if a["admm_iter"] > 0:
            coos.append(coo)
            refs.append(a)
            kept.append(shapes[i])
        if len(coos) == 14:
            break
    assert len(coos) == 14 and (5, 4) in kept and (12, 10) in kept, kept
    svs = [mod.Solver(coo=coo) for coo in coos]
    b = mod.Batch()
    res = b.solve(svs)
    st, widths = b.admm_stats(), b.admm_round_widths()
    print("14 tori:", kept, st, widths, "admm_iter", [a["admm_iter"] for a in refs], "ALM rounds", b.round_widths())
    for i, (a, r) in enumerate(zip(refs, res)):
        assert a["admm_iter"] == r["admm_iter"] and a["cg_iter"] == r["cg_iter"], (i, kept[i])
        assert np.float64(a["pobj"]).tobytes() == np.float64(r["pobj"]).tobytes(), (i, kept[i])
    assert len({a["admm_iter"] for a in refs}) > 1   # the lengths do differ
    assert st["alone"] == 0
    assert st["widest"] == len(svs), (st, widths)
    for sv in svs:
        sv.close()
    b.close()


def test_switch_and_isolation(mod, paths, solos, monkeypatch):
    names = ["mc_torus12x10", "theta40", "theta25x3", "torus6x5"]
    svs = [mod.Solver(paths[n]) for n in names]
    b = mod.Batch()
    # LRS_BATCH_ADMM=0: every member's ADMM phase on its own stream, the same bits
    monkeypatch.setenv("LRS_BATCH_ADMM", "0")
    res = b.solve(svs)
    st = b.admm_stats()
    print("LRS_BATCH_ADMM=0:", st)
    assert st["launches"] == 0 and st["served"] == 0 and st["widest"] == 0 and st["alone"] >= len(names)
    for n, sv, r in zip(names, svs, res):
        assert_bitwise(solos[n], snapshot(mod, sv, r), n + " (switch off)")
    monkeypatch.delenv("LRS_BATCH_ADMM")
    # one member whose parameters fail, one whose maxADMMIter differs: the others solve bitwise
    short = solo(mod, paths["theta25x3"], maxADMMIter=40)
    print("theta25x3 admm_iter", solos["theta25x3"]["res"]["admm_iter"], "at maxADMMIter=40", short["res"]["admm_iter"])
    assert short["res"]["admm_iter"] > 0
    prm = [{}, {"lbfgsListLength": 0}, {"maxADMMIter": 40}, {}]
    with pytest.raises(mod.BatchError) as ei:
        b.solve(svs, prm)
    assert ei.value.rc[1] != 0 and [ei.value.rc[i] for i in (0, 2, 3)] == [0, 0, 0]
    assert "lbfgsListLength" in ei.value.errors[1]
    for i in (0, 2, 3):
        ref = short if i == 2 else solos[names[i]]
        assert ei.value.errors[i] == ""
        assert_bitwise(ref, snapshot(mod, svs[i], ei.value.results[i]), names[i] + " (beside a failure)")
    st = b.admm_stats()
    assert st["launches"] >= 1 and st["widest"] >= 2 and st["alone"] == 0
    # the same object, the same contexts, a second call: everyone solves
    res = b.solve(svs)
    for n, sv, r in zip(names, svs, res):
        assert_bitwise(solos[n], snapshot(mod, sv, r), n + " (afterwards)")
    assert b.admm_stats()["widest"] >= 2
    for sv in svs:
        sv.close()
    b.close()


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _load_sweep_inputs(mod, name):
    k = np.load(os.path.join(GOLDEN, f"kernels_{name}.npz"))
    vec, m, rank = k["inputs"], int(k["m"]), int(k["rank"])
    dims = [int(d) for d in k["dims"]]
    NR = sum(d * rank for d in dims)
    g = np.load(os.path.join(GOLDEN, f"admm_sweep_{name}.npz"))
    sv = mod.Solver(instance(name))
    sv.set_rank([rank] * len(dims))
    sv.set_factor(mod.U, vec[7 * NR:8 * NR])
    sv.set_factor(mod.V, vec[8 * NR:9 * NR])
    sv.set_vec(mod.LAMBDA, vec[9 * NR:9 * NR + m])
    sv.admm_constr()
    return sv, len(dims), float(vec[9 * NR + 2 * m:][3]), float(g["cg_tol"]), g


def test_reference_parity_through_the_round(mod, monkeypatch):
    """One sweep a member from the reference's own inputs (admm_sweep_theta40 / theta25x3.npz),
    both members in ONE round of the table kernels (Batch.admm_round, a thin wrapper over the
    launcher), to the bars of tests/test_gpu_small_cg.py: the half-steps' right-hand sides against
    the multi-launch device CG's at 1e-10, the CG solutions U and V against the reference's at
    1e-6.  (The round's evaluation then replaces CVS by A(R R^T), which the reference's sweep does
    not, so the dual update is not part of this comparison.)  Side 1's right-hand side is the one
    a cone's buffer still holds after the round; it is formed from side 0's solution."""
    names = ["theta40", "theta25x3"]
    ctx = [_load_sweep_inputs(mod, n) for n in names]
    b = mod.Batch()
    b.admm_round([c[0] for c in ctx], [c[2] for c in ctx], [c[3] for c in ctx])
    st = b.admm_stats()
    assert st["blocks"] >= 3   # theta25x3's three cones in one launch
    for n, (sv, ncone, rho, tol, g) in zip(names, ctx):
        U, V = sv.get_factor(mod.U), sv.get_factor(mod.V)
        rhs = [sv.admm_rhs(c) for c in range(ncone)]
        sv.close()
        # the multi-launch device CG on the same inputs, cone by cone (the reference's order)
        monkeypatch.setenv("LRS_SMALL_CG", "0")
        ml, _, _, _, _ = _load_sweep_inputs(mod, n)
        ml_rhs = []
        for c in range(ncone):
            ml.admm_half(rho, tol, cone=c, side=0, init=False)
            ml_rhs.append(ml.admm_half(rho, tol, cone=c, side=1, init=False)[1])
        ml.close()
        monkeypatch.delenv("LRS_SMALL_CG")
        # and the member's own single-workgroup launches, cone by cone: the same bits
        own, _, _, _, _ = _load_sweep_inputs(mod, n)
        for c in range(ncone):
            for side in (0, 1):
                own.admm_half(rho, tol, cone=c, side=side, init=False)
        assert np.array_equal(own.get_factor(mod.U), U) and np.array_equal(own.get_factor(mod.V), V), n
        for c in range(ncone):
            assert np.array_equal(own.admm_rhs(c), rhs[c]), (n, c)
        own.close()
        for c in range(ncone):
            print(n, "cone", c, "rhs", rel(rhs[c], ml_rhs[c]))
            assert rel(rhs[c], ml_rhs[c]) < 1e-10, (n, c)
        print(n, "U", rel(U, g["U"]), "V", rel(V, g["V"]))
        assert rel(U, g["U"]) < 1e-6 and rel(V, g["V"]) < 1e-6, n
    b.close()

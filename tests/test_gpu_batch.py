"""Batched solves (lrs_solve_batch): many small instances whose single-workgroup
inner loops share launches, one workgroup each.  A block of a combined launch runs the same loop
on the same arguments as the instance's own launch, so every comparison against the solo solve
here is exact (bit for bit) wherever the solo path itself is deterministic."""
import importlib
import os
import threading

import numpy as np
import pytest

from golden_util import GOLDEN, rel_err

pytestmark = pytest.mark.gpu
SET = ["mc_torus12x10", "mc_rand200", "theta40", "theta25x3", "torus6x5"]
COUNTS = ("alm_inner", "alm_outer", "retcode", "final_rank")
TOL = 1e-9   # the bar of test_gpu_steps.py


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.solver")


@pytest.fixture(scope="module")
def inst():
    return importlib.import_module("ltr-lowrank-sdp_amd.instances")


@pytest.fixture(scope="module")
def paths(inst, tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_inst")
    p = {n: os.path.join(GOLDEN, "instances", f"{n}.dat-s")
         for n in ("mc_torus12x10", "mc_rand200", "theta40", "theta25x3", "rsparse60", "mc_lp60")}
    p["torus6x5"] = inst.maxcut_torus(str(d / "torus6x5.dat-s"), 6, 5, 11)
    # three cones of 150 rows: R and D of all three exceed one CU's LDS -> one workgroup per cone
    p["theta150x3"] = inst.theta_multiblock(str(d / "theta150x3.dat-s"), 150, 600, 3, 5)
    return p


def snapshot(mod, sv, res, factors=(0,)):
    """What a solve left behind: counts, phase-1 trajectory, ranks, kernel path, factors, vectors."""
    out = {"res": res, "traj1": sv.trajectory(1), "rank": sv.get_rank(), "path": sv.kernel_path()}
    for f in factors:
        out[f"F{f}"] = sv.get_factor(f)
    out["lam"] = sv.get_vec(mod.LAMBDA)
    out["cvs"] = sv.get_vec(mod.CVS)
    return out


def assert_same(a, b, what, counts=COUNTS, bitwise=True):
    for k in counts:
        assert a["res"][k] == b["res"][k], (what, k, a["res"][k], b["res"][k])
    assert a["traj1"] == b["traj1"], what
    assert a["rank"] == b["rank"], what
    if bitwise:
        for k in a:
            if k[0] == "F" or k in ("lam", "cvs"):
                assert np.array_equal(a[k], b[k]), (what, k)


def solo(mod, path, factors=(0,), **kw):
    sv = mod.Solver(path)
    res = sv.solve(**kw)
    out = snapshot(mod, sv, res, factors)
    sv.close()
    return out


@pytest.fixture(scope="module")
def solo_phase1(mod, paths):
    """The set's phase-1 solves, each alone through lrs_solve (computed once, never changed)."""
    return {n: solo(mod, paths[n], skipADMM=1) for n in SET}


def test_batch_is_bitwise_the_solo_solves(mod, paths, solo_phase1):
    svs = [mod.Solver(paths[n]) for n in SET]
    b = mod.Batch()
    res = b.solve(svs, {"skipADMM": 1})
    st = b.stats()
    groups = set()
    for n, sv, r in zip(SET, svs, res):
        got = snapshot(mod, sv, r)
        assert_same(solo_phase1[n], got, n)
        assert got["path"] == 4 and solo_phase1[n]["path"] == 4, n
        groups.add(tuple(sv.get_rank()))
    # at least two kernel instantiations: the set's factor rows differ in width (the single-workgroup
    # loop's row widths: the smallest of these that holds the rank)
    widths = {min(w for w in (8, 16, 24, 32, 48, 64) if w >= max(g)) for g in groups}
    assert len(widths) >= 2, groups
    print("batch stats", st, "round widths", b.round_widths())
    assert st["launches"] >= 1 and st["widest"] >= 2 and st["alone"] == 0
    assert st["served"] >= len(SET)
    for sv in svs:
        sv.close()
    b.close()


def test_whole_solves_through_the_batch(mod, paths):
    U, V, R = mod.U, mod.V, mod.R
    first = solo(mod, paths["mc_torus12x10"], factors=(R, U, V))
    again = solo(mod, paths["mc_torus12x10"], factors=(R, U, V))
    exact = all(np.array_equal(first[k], again[k]) for k in ("F0", f"F{U}", f"F{V}", "lam")) and \
        all(first["res"][k] == again["res"][k] for k in COUNTS + ("admm_iter", "cg_iter", "status"))
    print("solo whole solve repeats bit for bit:", exact)
    refs = {n: (first if n == "mc_torus12x10" else solo(mod, paths[n], factors=(R, U, V))) for n in SET}
    svs = [mod.Solver(paths[n]) for n in SET]
    b = mod.Batch()
    res = b.solve(svs)
    for n, sv, r in zip(SET, svs, res):
        got = snapshot(mod, sv, r, factors=(R, U, V))
        a = refs[n]
        if exact:
            assert_same(a, got, n, counts=COUNTS + ("admm_iter", "cg_iter", "status"))
        elif n.startswith("mc_") or n.startswith("torus"):
            # the bars of test_single_workgroup_solve_matches_default
            assert abs(a["res"]["alm_inner"] - r["alm_inner"]) <= 2
            for k in ("alm_pobj", "pobj"):
                assert abs(a["res"][k] - r[k]) <= 1e-6 * abs(a["res"][k]), (n, k)
        else:
            tol = 10 * (a["res"]["gap"] + r["gap"]) + 1e-6
            for k in ("pobj", "dobj"):
                assert abs(a["res"][k] - r[k]) <= tol * (1 + abs(a["res"][k])), (n, k)
            assert r["pinf"] <= 1e-4
    assert b.stats()["alone"] == 0 and b.stats()["widest"] >= 2
    for sv in svs:
        sv.close()
    b.close()


def test_reference_parity_through_the_batch(mod, paths):
    """Trip K of each member of a batch against the reference's own trips (steps_*.npz), 1e-9."""
    names = ["mc_rand200", "theta40", "mc_torus12x10"]
    zs = {n: np.load(os.path.join(GOLDEN, f"steps_{n}.npz")) for n in names}
    ks = {n: [int(k) for k in zs[n]["ks"] if zs[n][f"K{int(k)}_trips"].shape[0] >= int(k)] for n in names}
    svs = {n: mod.Solver(paths[n]) for n in names}
    b = mod.Batch()
    for j in range(max(len(v) for v in ks.values())):
        mem = [n for n in names if j < len(ks[n])]
        prm = []
        for n in mem:
            kw = dict(reoptLevel=0, maxALMIter=1000000000, skipADMM=1, timeSecLimit=1e30, almInnerBudget=ks[n][j])
            if int(zs[n]["rank_flag"]) > 0:
                kw["fixedRank"] = int(zs[n]["rank_flag"])
            prm.append(kw)
        res = b.solve([svs[n] for n in mem], prm)
        for n, r in zip(mem, res):
            K, z, sv = ks[n][j], zs[n], svs[n]
            assert r["alm_inner"] == K, (n, K, r["alm_inner"])
            d = sv.alm_last_step()
            tau, _rn, lag, pinf = z[f"K{K}_trips"][K - 1]
            assert abs(d["tau"] - tau) <= TOL * abs(tau), (n, K)
            assert abs(d["lag"] - lag) <= TOL * abs(lag), (n, K)
            assert abs(d["pinf"] - pinf) <= TOL * max(abs(pinf), 1e-300), (n, K)
            assert abs(d["beta"] - z[f"K{K}_beta"][0]) <= TOL * abs(z[f"K{K}_beta"][0]), (n, K)
            ours = {"R": sv.get_factor(mod.R), "G": sv.get_factor(mod.G), "cvs": sv.get_vec(mod.CVS),
                    "s": sv.get_factor(d["pair"][0]), "y": sv.get_factor(d["pair"][1])}
            for key, v in ours.items():
                assert rel_err(v, z[f"K{K}_{key}"]) < TOL, (n, K, key)
            assert sv.kernel_path() == 4, n
    assert b.stats()["alone"] == 0
    for sv in svs.values():
        sv.close()
    b.close()


def test_mixed_batch(mod, paths):
    """Members off the single-workgroup path run on their own streams inside the same call."""
    mem = [("rsparse60", {}), ("mc_lp60", {}), ("mc_rand200", {"lbfgsListLength": 3}),
           ("theta150x3", {"almInnerBudget": 40}), ("theta40", {}), ("mc_torus12x10", {})]
    prm = [dict(kw, skipADMM=1) for _n, kw in mem]
    refs = [solo(mod, paths[n], **kw) for (n, _), kw in zip(mem, prm)]
    assert refs[3]["path"] == 4 and refs[4]["path"] == 4 and refs[5]["path"] == 4
    assert refs[0]["path"] != 4 and refs[1]["path"] != 4
    b = mod.Batch()
    # the one-workgroup-per-cone member alone in a batch: all its inner-loop calls launch alone
    sv = mod.Solver(paths["theta150x3"])
    b.solve([sv], prm[3])
    calls = b.stats()["alone"]
    assert calls >= 1 and b.stats()["launches"] == 0 and b.stats()["served"] == 0
    assert sv.xwg_fallbacks() == 0
    sv.close()
    svs = [mod.Solver(paths[n]) for n, _ in mem]
    res = b.solve(svs, prm)
    st = b.stats()
    print("mixed batch stats", st, b.round_widths())
    for i, ((n, _), s, r) in enumerate(zip(mem, svs, res)):
        got = snapshot(mod, s, r)
        # bit for bit on the single-workgroup paths (one workgroup, and one per cone with its
        # ordered exchange); counts for the multi-launch and the host-driven L-BFGS paths
        assert_same(refs[i], got, n, bitwise=i >= 3)
        assert got["path"] == refs[i]["path"], n
    assert svs[3].xwg_fallbacks() == 0
    assert st["alone"] == calls
    assert st["launches"] >= 1 and st["widest"] == 2
    assert st["served"] >= 2
    for s in svs:
        s.close()
    b.close()


def test_uneven_lengths_and_width(mod, inst):
    """40 tori from 5 x 4 to 12 x 10: the first round runs all 40, later ones whoever is left."""
    rng = np.random.default_rng(2024)
    shapes = [(5, 4), (12, 10)] + [(int(rng.integers(5, 13)), int(rng.integers(4, 11))) for _ in range(38)]
    coos = [inst.coo_arrays(inst.maxcut_torus_problem(r, c, 100 + i)) for i, (r, c) in enumerate(shapes)]
    refs = []
    for coo in coos:
        sv = mod.Solver(coo=coo)
        refs.append(sv.solve(skipADMM=1))
        sv.close()
    svs = [mod.Solver(coo=coo) for coo in coos]
    b = mod.Batch()
    res = b.solve(svs, {"skipADMM": 1})
    for i, (a, r) in enumerate(zip(refs, res)):
        assert a["alm_inner"] == r["alm_inner"], (i, shapes[i])
        assert np.float64(a["alm_pobj"]).tobytes() == np.float64(r["alm_pobj"]).tobytes(), (i, shapes[i])
    st, widths = b.stats(), b.round_widths()
    print("40 tori:", st, widths)
    assert st["widest"] == 40 and widths.get(40, 0) >= 1 and st["alone"] == 0
    assert len({a["alm_inner"] for a in refs}) > 1   # the lengths do differ
    for sv in svs:
        sv.close()
    b.close()


def test_failure_isolation(mod, paths, solo_phase1):
    names = ["mc_torus12x10", "theta40", "mc_rand200", "torus6x5"]
    svs = [mod.Solver(paths[n]) for n in names]
    prm = [{"skipADMM": 1} for _ in names]
    prm[1] = {"skipADMM": 1, "lbfgsListLength": 0}
    b = mod.Batch()
    with pytest.raises(mod.BatchError) as ei:
        b.solve(svs, prm)
    assert ei.value.rc[1] != 0 and [ei.value.rc[i] for i in (0, 2, 3)] == [0, 0, 0]
    assert "lbfgsListLength" in ei.value.errors[1] and "instance 1" in str(ei.value)
    for i in (0, 2, 3):
        assert ei.value.errors[i] == ""
        assert_same(solo_phase1[names[i]], snapshot(mod, svs[i], ei.value.results[i]), names[i])
    # the same object, the same contexts, a second call: everyone solves
    res = b.solve(svs, {"skipADMM": 1})
    for n, sv, r in zip(names, svs, res):
        assert_same(solo_phase1[n], snapshot(mod, sv, r), n)
    for sv in svs:
        sv.close()
    b.close()


def test_degenerate_batches(mod, paths, solo_phase1):
    b = mod.Batch()
    sv = mod.Solver(paths["theta40"])
    res = b.solve([sv], {"skipADMM": 1})
    assert_same(solo_phase1["theta40"], snapshot(mod, sv, res[0]), "n = 1")
    assert b.stats()["widest"] == 1 and b.stats()["alone"] == 0
    other = mod.Solver(paths["torus6x5"])
    with pytest.raises(mod.BatchError, match="same context"):
        b.solve([sv, other, sv], {"skipADMM": 1})
    with pytest.raises(mod.BatchError, match=f"1 to {mod.BATCH_MAX}"):
        b.solve([sv] * (mod.BATCH_MAX + 1), {"skipADMM": 1})
    # a sharded context (loopback world 2; lrs_shard_loopback is collective over two threads)
    grp = mod.LoopbackGroup(2)
    sh, errs = [None, None], []

    def work(r):
        try:
            sh[r] = mod.Solver(paths["mc_rand200"])
            sh[r].shard_loopback(grp, r)
        except Exception as e:   # reported below
            errs.append(repr(e))

    ts = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not errs and not any(t.is_alive() for t in ts), errs
    with pytest.raises(mod.BatchError, match="sharded"):
        b.solve([other, sh[0]], {"skipADMM": 1})
    # nothing ran in the refused calls, and the batch object still works
    res = b.solve([sv, other], {"skipADMM": 1})
    assert_same(solo_phase1["theta40"], snapshot(mod, sv, res[0]), "after refusals")
    assert_same(solo_phase1["torus6x5"], snapshot(mod, other, res[1]), "after refusals")
    for s in (sv, other, sh[0], sh[1]):
        s.close()
    grp.close()
    b.close()

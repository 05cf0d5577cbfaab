"""The latency kernels' argument lists (k_lat_a / k_lat_b): the leading arguments are preloaded
into scalar registers at wave launch -- the previous stage's partials, the control words'
pointers, the row header's pointers, n and one packed word (row waves, row blocks, the partial
block counts) -- and the batch-end mirror of k_lat_b runs behind the head's loads.  Nothing in
the arithmetic changes, so the checks are on the launches whose argument decoding can go wrong at
the edges: every PLAIN x TSUM instantiation at the smallest, the largest and the chosen number of
row waves, rows past the prefetch windows, global constraints (a second partial pointer and
count in k_lat_b's head), and a batch boundary through the mirror."""
import importlib

import numpy as np
import pytest

from golden_util import instance

pytestmark = pytest.mark.gpu
SETTINGS = [(True, True), (True, False), (False, True), (False, False)]   # (LRS_LAT_PLAIN, LRS_LAT_TSUM)
WAVES = [1, 7, None]                                                      # LRS_LAT_ROWWAVES (None: unset)


@pytest.fixture(scope="module")
def solver_mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.solver")


def _env(monkeypatch, plain, tsum, waves):
    monkeypatch.setenv("LRS_SMALL", "0")   # path 0 = the latency kernels (not the single-workgroup loop)
    monkeypatch.setenv("LRS_LAT_PLAIN", "1" if plain else "0")
    monkeypatch.setenv("LRS_LAT_TSUM", "1" if tsum else "0")
    if waves is None:
        monkeypatch.delenv("LRS_LAT_ROWWAVES", raising=False)
    else:
        monkeypatch.setenv("LRS_LAT_ROWWAVES", str(waves))


def _state(sm, sv):
    out = {k: sv.get_factor(getattr(sm, k)) for k in ("R", "G", "S0", "Y0", "S1", "Y1")}
    out.update({k: sv.get_vec(getattr(sm, k)) for k in ("LAMBDA", "CVS")})
    return out


def _open(sm, src, kernel_path):
    sv = sm.Solver(coo=src) if isinstance(src, dict) else sm.Solver(src)
    if kernel_path is not None:
        sv.set_kernel_path(kernel_path)
    return sv


def _four_way(sm, src, monkeypatch, ks, waves=None, kernel_path=None, is_plain=True):
    """State after K inner iterations under each PLAIN x TSUM setting: the latency kernels ran,
    the instantiation asked for ran, and the four states are bitwise equal."""
    ref = None
    for plain, tsum in SETTINGS:
        _env(monkeypatch, plain, tsum, waves)
        sv = _open(sm, src, kernel_path)
        got = {}
        for K in ks:
            d = sv.alm_steps(K, reoptLevel=0)
            assert d["inner"] == K, (K, d["inner"])
            assert sv.kernel_path() == 0, (plain, tsum, waves, K, sv.kernel_path())
            assert bool(sv.lat_plain_used()) == (plain and is_plain), (plain, tsum, waves, K)
            assert bool(sv.lat_tsum_used()) == tsum, (plain, tsum, waves, K)
            got[K] = _state(sm, sv)
            assert all(np.isfinite(v).all() for v in got[K].values()), (plain, tsum, waves, K)
        sv.close()
        if ref is None:
            ref = got
            continue
        for K in ks:
            for key in ref[K]:
                assert np.array_equal(ref[K][key], got[K][key]), (
                    plain, tsum, waves, K, key, float(np.max(np.abs(ref[K][key] - got[K][key]))))


def _solve(sm, src, kernel_path):
    sv = _open(sm, src, kernel_path)
    r = sv.solve(reoptLevel=0)
    out = (r, sv.kernel_path())
    sv.close()
    return out


@pytest.fixture(scope="module")
def torus_general(solver_mod):
    """mc_torus12x10 solved by the general row kernels (kernel path 1): the reference, once."""
    mp = pytest.MonkeyPatch()
    mp.setenv("LRS_SMALL", "0")
    try:
        r, p = _solve(solver_mod, instance("mc_torus12x10"), 1)
    finally:
        mp.undo()
    assert p == 1
    return r


@pytest.mark.parametrize("waves", WAVES)
def test_torus_four_way_bitwise(solver_mod, waves, monkeypatch):
    """mc_torus12x10 (the headline's shape in small) at one row wave a block (15 blocks), seven (3
    blocks, the last one partly past n) and the count the launch chooses."""
    _four_way(solver_mod, instance("mc_torus12x10"), monkeypatch, (1, 2, 3, 9), waves=waves)


@pytest.mark.parametrize("waves", WAVES)
def test_torus_solves_like_general(solver_mod, torus_general, waves, monkeypatch):
    """The whole solve under every setting against kernel path 1, test_latency_kernels_match_general's
    bounds: inner iterations +-2, the ALM objective 1e-8 relative, the final objective 1e-6."""
    b = torus_general
    for plain, tsum in SETTINGS:
        _env(monkeypatch, plain, tsum, waves)
        a, pa = _solve(solver_mod, instance("mc_torus12x10"), 0)
        assert pa == 0, (plain, tsum, waves, pa)
        print(f"waves {waves} plain {plain} tsum {tsum}: inner {a['alm_inner']} / {b['alm_inner']}, "
              f"alm_pobj rel {abs(a['alm_pobj'] - b['alm_pobj']) / abs(b['alm_pobj']):.3e}, "
              f"pobj rel {abs(a['pobj'] - b['pobj']) / max(1.0, abs(b['pobj'])):.3e}")
        assert abs(a["alm_inner"] - b["alm_inner"]) <= 2, (plain, tsum, waves, a["alm_inner"], b["alm_inner"])
        assert abs(a["alm_pobj"] - b["alm_pobj"]) <= 1e-8 * abs(b["alm_pobj"]), (plain, tsum, waves)
        assert abs(a["pobj"] - b["pobj"]) <= 1e-6 * max(1.0, abs(b["pobj"])), (plain, tsum, waves, a["pobj"], b["pobj"])


def test_tail_loops_four_way_bitwise(solver_mod, monkeypatch):
    """test_gpu_lat_plain's random 200-vertex / 460-edge graph: rows past both prefetch windows, so
    the loops behind the barrier (which load the adjacency and operand bases again) run."""
    inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")
    n = 200
    ei, ej = inst._random_edges(np.random.default_rng(5), n, 460)
    lo, hi = np.minimum(ei, ej), np.maximum(ei, ej)
    assert np.bincount(np.concatenate([lo, hi]), minlength=n).max() > 4 and np.bincount(hi, minlength=n).max() > 2
    w = np.random.default_rng(6).choice([-1.0, 1.0], size=ei.size)
    coo = inst.coo_arrays(inst._maxcut_problem(n, ei, ej, w))
    _four_way(solver_mod, coo, monkeypatch, (1, 3, 9))


def test_global_constraints_four_way_bitwise(solver_mod, monkeypatch):
    """rsparse60 on set_kernel_path(5) (one lane group a row, so the latency kernels run): every
    constraint is a global one -- nblkB > 0, stage G's partial pointer and count in k_lat_b's
    head, the global constraints' loop behind k_lat_a's barrier.  Not a PLAIN cone: the general
    instantiation runs under either LRS_LAT_PLAIN setting."""
    _four_way(solver_mod, instance("rsparse60"), monkeypatch, (1, 3), kernel_path=5, is_plain=False)


def test_global_constraints_solve_like_general(solver_mod, monkeypatch):
    """rsparse60, the whole solve on path 5 under every setting against kernel path 1, the bound of
    test_latency_kernels_match_general for instances that are not MaxCut: the objectives within
    10 (gap_a + gap_b) + 1e-6."""
    monkeypatch.setenv("LRS_SMALL", "0")
    b, pb = _solve(solver_mod, instance("rsparse60"), 1)
    assert pb == 1
    for plain, tsum in SETTINGS:
        _env(monkeypatch, plain, tsum, None)
        a, pa = _solve(solver_mod, instance("rsparse60"), 5)
        assert pa == 0, (plain, tsum, pa)
        tol = 10 * (a["gap"] + b["gap"]) + 1e-6
        print(f"plain {plain} tsum {tsum}: pobj {a['pobj']!r} / {b['pobj']!r}, tol {tol:.3e}")
        assert abs(a["pobj"] - b["pobj"]) <= tol * max(1.0, abs(b["pobj"])), (plain, tsum, a["pobj"], b["pobj"])


def test_batch_boundary_through_mirror(solver_mod, monkeypatch):
    """Eager launches (no graph replay): the last k_lat_b of a batch mirrors the control block and
    the batch's sequence number into pinned host memory and the host spins on it, so a mirror
    that is skipped, or taken behind the early return of an idle iteration, fails the run.  The
    bench's fixed budget of 300 iterations, twice, over many batch boundaries."""
    monkeypatch.setenv("LRS_SMALL", "0")
    monkeypatch.setenv("LRS_GRAPHS", "0")
    monkeypatch.delenv("LRS_LAT_ROWWAVES", raising=False)
    sv = solver_mod.Solver(instance("mc_torus12x10"))
    r = sv.determine_rank()[0]
    outs = [sv.alm_throughput(0, 300, fixedRank=r, reoptLevel=0)["done"] for _ in range(2)]
    assert sv.kernel_path() == 0
    assert outs == [300, 300], outs
    sv.close()

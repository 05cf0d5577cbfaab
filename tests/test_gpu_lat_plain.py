"""The latency kernels' PLAIN instantiations (k_lat_a / k_lat_b on cones whose slots carry at
most one constraint entry and one local constraint: no slot lists, parameters from LDS, the
stores of a row issued in one run behind its arithmetic) against the general instantiation
(LRS_LAT_PLAIN=0): the same arithmetic in the same order, so every state array is bitwise equal
after K inner iterations; instances that need the lists or dense-row slices never take them."""
import importlib
import os

import numpy as np
import pytest

from golden_util import ROOT, instance

pytestmark = pytest.mark.gpu
KS = (1, 2, 3, 9)


@pytest.fixture(scope="module")
def solver_mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.solver")


def _state(sm, sv):
    out = {k: sv.get_factor(getattr(sm, k)) for k in ("R", "G", "S0", "Y0", "S1", "Y1")}
    out.update({k: sv.get_vec(getattr(sm, k)) for k in ("LAMBDA", "CVS")})
    return out


def _run(sm, path, plain, monkeypatch, ks=KS):
    """State after K inner iterations of a fixed-budget run (a fresh solve per K), the kernel
    path and whether the PLAIN instantiation ran."""
    monkeypatch.setenv("LRS_SMALL", "0")   # path 0 = the latency kernels (not the single-workgroup loop)
    monkeypatch.setenv("LRS_LAT_PLAIN", "1" if plain else "0")
    sv = sm.Solver(coo=path) if isinstance(path, dict) else sm.Solver(path)
    out = {}
    for K in ks:
        d = sv.alm_steps(K, reoptLevel=0)
        assert d["inner"] == K, (K, d["inner"])
        out[K] = (_state(sm, sv), sv.kernel_path(), sv.lat_plain_used())
    sv.close()
    return out


def _equal(a, b, want_path0):
    for K in KS:
        (sa, pa, ua), (sb, pb, ub) = a[K], b[K]
        assert pa == pb, (K, pa, pb)
        if want_path0:
            assert pa == 0, (K, pa)
        assert ua == (pa == 0) and not ub, (K, pa, ua, ub)
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), (K, key, float(np.max(np.abs(sa[key] - sb[key]))))


@pytest.mark.parametrize("name", ["mc_torus12x10", "mc_rand200"])
def test_plain_bitwise_equals_general(solver_mod, name, monkeypatch):
    """Default rank, K = 1, 2, 3, 9.  mc_torus12x10 runs the latency kernels (path 0): all of stage
    B's entries within the prefetch window, stage A's wrap-around rows (up to four lower
    neighbours, two prefetched) through its tail loop.  mc_rand200 (1 500 edges, 16 entries a row)
    gets lane-group teams from the stage plan and so the general row kernels under either switch
    setting, today as before: its rows do not reach the latency kernels, the case only pins that
    the switch changes nothing there; test_plain_tail_loop_bitwise below has the long rows."""
    a = _run(solver_mod, instance(name), True, monkeypatch)
    b = _run(solver_mod, instance(name), False, monkeypatch)
    _equal(a, b, name == "mc_torus12x10")


def test_plain_tail_loop_bitwise(solver_mod, monkeypatch):
    """A random MaxCut graph sparse enough for the latency kernels (200 vertices, 460 edges: 5.6
    entries a row, no teams) with rows past both prefetch windows (more than four neighbours;
    more than two lower ones), so the PLAIN path's tail loops run in both stages."""
    inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")
    n = 200
    ei, ej = inst._random_edges(np.random.default_rng(5), n, 460)
    lo, hi = np.minimum(ei, ej), np.maximum(ei, ej)
    assert np.bincount(np.concatenate([lo, hi]), minlength=n).max() > 4 and np.bincount(hi, minlength=n).max() > 2
    w = np.random.default_rng(6).choice([-1.0, 1.0], size=ei.size)
    coo = inst.coo_arrays(inst._maxcut_problem(n, ei, ej, w))
    a = _run(solver_mod, coo, True, monkeypatch)
    b = _run(solver_mod, coo, False, monkeypatch)
    _equal(a, b, True)


def test_multi_constraint_slots_take_general(solver_mod, monkeypatch):
    """rsparse60 has slots with several constraint entries (slot1.y == -2): PLAIN never runs on
    it, whichever path the iteration takes, and it solves as test_latency_kernels_match_general
    expects (path 0 against the general row kernels)."""
    monkeypatch.setenv("LRS_SMALL", "0")
    monkeypatch.setenv("LRS_LAT_PLAIN", "1")
    out = []
    for path in (0, 1):
        sv = solver_mod.Solver(instance("rsparse60"))
        sv.set_kernel_path(path)
        sv.alm_steps(3, reoptLevel=0)
        assert not sv.lat_plain_used()
        r = sv.solve(reoptLevel=0)
        assert not sv.lat_plain_used()
        out.append((r, sv.kernel_path()))
        sv.close()
    (a, _), (b, pb) = out
    assert pb == 1
    tol = 10 * (a["gap"] + b["gap"]) + 1e-6
    assert abs(a["pobj"] - b["pobj"]) <= tol * max(1.0, abs(b["pobj"])), (a["pobj"], b["pobj"])


def test_dense_row_slices_unchanged(solver_mod, monkeypatch):
    """checker_1.5 (a hub instance: dense-row slice blocks and k_lat_f): PLAIN is off, so the two
    switch settings run the same kernels and give the same bits."""
    path = os.path.join(ROOT, "data", "bundled", "checker_1.5.dat-s")
    a = _run(solver_mod, path, True, monkeypatch, ks=(3,))
    b = _run(solver_mod, path, False, monkeypatch, ks=(3,))
    (sa, pa, ua), (sb, pb, ub) = a[3], b[3]
    assert pa == 0 and pb == 0, "latency kernels not taken on a hub instance"
    assert not ua and not ub
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key

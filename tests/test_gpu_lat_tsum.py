"""The latency kernels' transposed wave sums (wave_tsum: a reduce-scatter butterfly over wave_sum's
own pair tree -- pairs, quads, eights and sixteens inside a row of 16 lanes, then
(row0 + row1) + (row2 + row3)) against one wave_sum a value (LRS_LAT_TSUM=0).  IEEE addition is
commutative, so pairing the same subtrees gives the same bits: the helper is compared bit for bit
on inputs whose sums depend on the order, and the solver's state arrays bit for bit after K inner
iterations on every kind of latency launch (PLAIN and general, tail loops, dense-row slice blocks
with k_lat_f, global constraints)."""
import importlib
import os

import numpy as np
import pytest

from golden_util import ROOT, instance

pytestmark = pytest.mark.gpu
KS = (1, 2, 3, 9)
NVS = (5, 7, 8, 10)
NBLK = (1, 2, 63, 64, 65, 250, 256)
NW = (2, 3, 6, 8)


@pytest.fixture(scope="module")
def solver_mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.solver")


@pytest.fixture(scope="module")
def probe(solver_mod):
    sv = solver_mod.Solver(instance("mc_torus12x10"))
    yield sv
    sv.close()


def _inputs(nv, cols, seed):
    """Three [nv][cols] inputs whose sums depend on the order of the additions: values over ~30
    decades with mixed signs; -0.0 and denormals (a column of -0.0 only sums to -0.0, which a
    stray +0.0 would turn into +0.0); huge values facing their negations in the partner lane (the
    small rest survives only if the pair is added first)."""
    rng = np.random.default_rng(seed)
    spread = rng.choice([-1.0, 1.0], size=(nv, cols)) * 10.0 ** rng.uniform(-15.0, 15.0, size=(nv, cols))
    tiny = rng.choice([-0.0, 0.0, 5e-324, -5e-324, 2.5e-310, -1.5e-308], size=(nv, cols))
    tiny[0, :] = -0.0
    cancel = rng.standard_normal((nv, cols))
    for v in range(nv):
        for q in range(0, cols - 1, 2 << (v % 3)):   # (columns q, q + 1: a lane pair, every 2, 4 or 8 columns)
            big = 10.0 ** rng.uniform(20.0, 300.0)
            cancel[v, q] = big
            cancel[v, q + 1] = -big
    return {"spread": spread, "tiny": tiny, "cancel": cancel}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("nv", NVS)
def test_prologue_form_bitwise(probe, nv):
    """sum_partials against its wave_tsum form over nblk producer blocks (one block, one past a
    wave's 64 lanes, the q = 3 remainder, the cap)."""
    for nblk in NBLK:
        for name, x in _inputs(nv, nblk, 100 * nv + nblk).items():
            ref, new = probe.wave_tsum_probe(0, x)
            assert np.array_equal(_bits(new), _bits(ref)), (nv, nblk, name, ref, new)
            assert np.array_equal(new, ref), (nv, nblk, name)
            if name == "tiny":
                assert np.signbit(ref[0]) == np.signbit(new[0])


@pytest.mark.parametrize("nv", NVS)
def test_tail_form_bitwise(probe, nv):
    """write_partials_nw_to against its wave_tsum form over blocks of nw waves."""
    for nw in NW:
        for name, x in _inputs(nv, 64 * nw, 1000 * nv + nw).items():
            ref, new = probe.wave_tsum_probe(1, x)
            assert np.array_equal(_bits(new), _bits(ref)), (nv, nw, name, ref, new)
            assert np.array_equal(new, ref), (nv, nw, name)


def test_probe_sums_are_sums(probe):
    """The reference side of the probe is the sum it claims to be (exact on small integers), so
    the comparisons above are not of two empty outputs."""
    x = np.arange(10 * 65, dtype=np.float64).reshape(10, 65) % 17 - 8
    ref, new = probe.wave_tsum_probe(0, x)
    assert np.array_equal(ref, x.sum(axis=1)) and np.array_equal(new, ref)
    x = np.arange(8 * 192, dtype=np.float64).reshape(8, 192) % 13 - 6
    ref, new = probe.wave_tsum_probe(1, x)
    assert np.array_equal(ref, x.sum(axis=1)) and np.array_equal(new, ref)


def _state(sm, sv):
    out = {k: sv.get_factor(getattr(sm, k)) for k in ("R", "G", "S0", "Y0", "S1", "Y1")}
    out.update({k: sv.get_vec(getattr(sm, k)) for k in ("LAMBDA", "CVS")})
    return out


def _run(sm, path, tsum, monkeypatch, ks=KS, plain=True, kernel_path=None):
    """State after K inner iterations of a fixed-budget run (a fresh solve per K), the kernel
    path, whether the PLAIN instantiation ran and whether the transposed sums ran."""
    monkeypatch.setenv("LRS_SMALL", "0")   # path 0 = the latency kernels (not the single-workgroup loop)
    monkeypatch.setenv("LRS_LAT_PLAIN", "1" if plain else "0")
    monkeypatch.setenv("LRS_LAT_TSUM", "1" if tsum else "0")
    sv = sm.Solver(coo=path) if isinstance(path, dict) else sm.Solver(path)
    if kernel_path is not None:
        sv.set_kernel_path(kernel_path)
    out = {}
    for K in ks:
        d = sv.alm_steps(K, reoptLevel=0)
        assert d["inner"] == K, (K, d["inner"])
        out[K] = (_state(sm, sv), sv.kernel_path(), sv.lat_plain_used(), sv.lat_tsum_used())
    sv.close()
    return out


def _equal(a, b, ks, want_plain):
    for K in ks:
        (sa, pa, ua, ta), (sb, pb, ub, tb) = a[K], b[K]
        assert pa == 0 and pb == 0, (K, pa, pb)
        assert ua == want_plain and ub == want_plain, (K, ua, ub)
        assert ta and not tb, (K, ta, tb)
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), (K, key, float(np.max(np.abs(sa[key] - sb[key]))))


@pytest.mark.parametrize("plain", [True, False])
def test_torus_bitwise(solver_mod, plain, monkeypatch):
    """mc_torus12x10, the headline's shape in small: the PLAIN and the general instantiation."""
    a = _run(solver_mod, instance("mc_torus12x10"), True, monkeypatch, plain=plain)
    b = _run(solver_mod, instance("mc_torus12x10"), False, monkeypatch, plain=plain)
    _equal(a, b, KS, plain)


def test_tail_loops_bitwise(solver_mod, monkeypatch):
    """test_gpu_lat_plain's random 200-vertex / 460-edge graph: rows past both prefetch windows."""
    inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")
    n = 200
    ei, ej = inst._random_edges(np.random.default_rng(5), n, 460)
    w = np.random.default_rng(6).choice([-1.0, 1.0], size=ei.size)
    coo = inst.coo_arrays(inst._maxcut_problem(n, ei, ej, w))
    a = _run(solver_mod, coo, True, monkeypatch)
    b = _run(solver_mod, coo, False, monkeypatch)
    _equal(a, b, KS, True)


def test_dense_row_slices_bitwise(solver_mod, monkeypatch):
    """checker_1.5 (a hub instance): dense-row slice blocks and k_lat_f's partials."""
    path = os.path.join(ROOT, "data", "bundled", "checker_1.5.dat-s")
    a = _run(solver_mod, path, True, monkeypatch, ks=(3,))
    b = _run(solver_mod, path, False, monkeypatch, ks=(3,))
    _equal(a, b, (3,), False)


def test_global_constraints_bitwise(solver_mod, monkeypatch):
    """rsparse60 at K = 3 on the latency kernels (kernel_path() == 0): every constraint is a global
    one, so the global constraints' loop gives the control wave a non-zero tail accumulator, and
    the line search's control wave sums A's and G's partials.  Its rows (60 rows, 300 constraints
    of four entries) get lane-group teams from the automatic plan, which excludes the latency
    kernels (kernel_path() was 1 under set_kernel_path(0)); set_kernel_path(5) plans one lane
    group a row, with which they run."""
    a = _run(solver_mod, instance("rsparse60"), True, monkeypatch, ks=(3,), kernel_path=5)
    b = _run(solver_mod, instance("rsparse60"), False, monkeypatch, ks=(3,), kernel_path=5)
    _equal(a, b, (3,), False)
    assert all(np.isfinite(v).all() for v in a[3][0].values())


def test_path5_solves_like_general(solver_mod, monkeypatch):
    """set_kernel_path(5) on rsparse60 -- the latency kernels on rows that would get teams --
    solves like the general row kernels (test_gpu_parity's bar for this instance: the objectives
    within ten times the two gaps)."""
    monkeypatch.setenv("LRS_SMALL", "0")
    out = []
    for path in (5, 1):
        sv = solver_mod.Solver(instance("rsparse60"))
        sv.set_kernel_path(path)
        r = sv.solve(reoptLevel=0)
        out.append((r, sv.kernel_path()))
        sv.close()
    (a, pa), (b, pb) = out
    assert pa == 0 and pb == 1, (pa, pb)
    tol = 10 * (a["gap"] + b["gap"]) + 1e-6
    assert abs(a["pobj"] - b["pobj"]) <= tol * max(1.0, abs(b["pobj"])), (a["pobj"], b["pobj"])


def test_global_constraints_latency_bitwise(solver_mod, monkeypatch):
    """A random sparse SDP of low degree (600 rows, 900 constraints of two entries each: no teams,
    most constraints span two slots) on the latency kernels' general instantiation: the global
    constraints' loop runs in every wave, so the control wave's tail accumulator is not zero, and
    the line search's control wave sums A's seven and G's five partial vectors in one pass."""
    inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")
    coo = inst.coo_arrays(inst.random_sparse_problem(600, 900, 2, 12))
    a = _run(solver_mod, coo, True, monkeypatch, ks=(1, 3))
    b = _run(solver_mod, coo, False, monkeypatch, ks=(1, 3))
    _equal(a, b, (1, 3), False)

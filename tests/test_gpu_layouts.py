"""Every factor layout and kernel path against the CPU oracle (MI355X).

Factor arrays are row-major n x ld on the device, ld = G E >= r, and the hot kernels are templates
over (G, E): 17 layouts of each (csrc/lrs_kernels.hip LRS_LAYOUT_SWITCH).  The fixtures written by
the reference sit at a handful of ranks; here oracle/lrsdp_oracle.c, which takes the rank as a
parameter and is pinned to the reference by tests/test_oracle_golden.py (at ranks 48, 97, 192, 256
and 290 among others), is the live reference for a sweep over rank x kernel path:

  three ranks a layout class (lower edge, an interior rank with r mod E != 0 and r mod 4 != 0,
  the upper edge r = ld), ranks 1, 2, 3, and r = ld - 1 for the padding check;
  kernel paths 0, 1, 2, 3, 5 (lrs_set_kernel_path) and 4 (k_small_alm<LD>, all six LD);
  the six layouts only LRS_LAYOUT reaches; two cones of different layouts in one problem.

Bars.  Inner iterations (K = 3 trips from the reference's initial point): R, G, A(RR^T) and lambda
to 1e-9 norm-wise, the bar of tests/test_gpu_steps.py for up to 8 trips.  Operators: 1e-10, tau
to 1e-9 with the same root count, the L-BFGS direction to 1e-9, the CG iterate to 1e-6 where the
oracle's CG converges inside its cap: the bars of tests/test_gpu_parity.py.  ADMM sweeps: 1e-6, the
bar of tests/test_gpu_small_cg.py.  The oracle's own rounding sensitivity (two builds of it,
scripts/layout_admit.py) is at most 3.5e-12 on the admitted iteration cases and 1.2e-14 on the
admitted sweeps; the admitted lists are frozen in tests/layout_util.py.  No bar comes from the device's output.
The padding columns [r, ld) of all nine factor arrays are read back after every run of the trips
(lrs_factor_padding) and must be exactly zero.

Each case prints one LAYOUT_SWEEP line a (path) with the worst relative errors before it asserts."""
import importlib
import json
import os

import numpy as np
import pytest

import layout_util as lu
from golden_util import rel_err

pytestmark = pytest.mark.gpu
STEP_TOL = 1e-9
TOL = 1e-10
K = 3
MULTI_PATHS = (0, 1, 2, 3, 5)


@pytest.fixture(scope="module")
def solver_mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.solver")


@pytest.fixture(scope="module")
def olib(oracle_lib):
    return lu.bind_oracle(oracle_lib)


@pytest.fixture(scope="module")
def gen_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("layout_instances")


class Checks:
    """Collects failed comparisons so that a case prints all its figures before it fails."""

    def __init__(self):
        self.bad = []

    def le(self, what, val, bar):
        if not val <= bar:
            self.bad.append(f"{what}: {val:.3e} > {bar:.1e}")

    def eq(self, what, a, b):
        if a != b:
            self.bad.append(f"{what}: {a!r} != {b!r}")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def report(**kw):
    print("LAYOUT_SWEEP " + json.dumps(kw))


# Which kernels an ALM iteration runs (lrs_get_kernel_path) by instance and forced path, from
# csrc/lrs_kernels.hip enqueue_alm_stages / lat_plan / plan_a / plan_b / team_size:
#   paths 1, 2, 3: the general row kernels, always (1);
#   path 5: the latency kernels k_lat_a / k_lat_b (0): one lane group a row, every group resident;
#   path 0: the latency kernels where no stage gives a row a team of lane groups (lat_plan: pa.T ==
#     1 and pb.T == 1).  team_size doubles a team while 2 T U <= pattern entries a row (U = 2 on the
#     lower entries in stage A, 4 on all entries in stage B) and 2 T G <= kRowBlock = 512, so at every
#     G <= 64 a cone with >= 4 lower entries a row gets one.  The tori have 3 lower entries a row
#     and 5 in all: no team, the latency kernels run.  mc_rand300w has 9.3 lower entries a row,
#     rsparse60 15.2, theta40 20.5 (C = -J fills the pattern), theta25x3 13: teams, so path 0 runs the
#     general row kernels there at every layout, and the latency kernels are reached through path 5.
#   path 4: k_small_alm (4) where small_alm_args takes the problem: one layout for all cones,
#     ld in {8, 16, 24, 32, 48, 64}, R and D within kSmallMaxDynLds.  Above ld 64 (32 x 3 and wider)
#     there is no k_small_alm<LD>: the pair (layout, path 4) cannot occur and is not run.
#   paths 3 (k_wide_*): plan_a / plan_b take the long-row kernels at E <= 2 only; at E >= 3 path 3
#     runs the bandwidth-regime kernels of path 2 (the iteration is still compared, as path 2's).
LAT_ON_AUTO = {"mc_torus12x10": True, "torus24x22": True, "mc_2blk": True, "mc_rand300w": False, "rsparse60": False,
               "theta40": False, "theta25x3": False}


def expected_path(name, kpath):
    if kpath in (1, 2, 3):
        return 1
    if kpath == 5:
        return 0
    if kpath == 0:
        return 0 if LAT_ON_AUTO[name] else 1
    return 4


def cone_blocks(v, name, ranks):
    out, p = [], 0
    for n, r in zip(lu.dims_of(name), ranks):
        out.append(v[p:p + n * r].reshape(r, n).T)
        p += n * r
    assert p == v.size
    return out


ALL_FACTORS = range(9)   # R, D, G, U, V, S0, Y0, S1, Y1 (solver.py)


def padding_check(sv, solver_mod, name, d, ck, tag, auut):
    """Columns [r, ld) of the device's factor arrays after the trips.

    lrs_factor_padding reads the arrays back as they are stored and returns max |x| over exactly
    those columns, so any non-zero (or NaN) a kernel left there makes it positive: every factor must
    give 0.0.  With `auut` (MaxCut, at a class's lower edge and at r = ld - 1) A(RR^T) from the
    constraint entries is also compared with the row norms of the unpadded R that lrs_factor_get
    returns: k_auv_diag and k_auv_con (auv_entry) sum all E doubles of all G lanes of a row, so
    a padding entry p adds p^2 to the row's value."""
    worst = 0.0
    for which in ALL_FACTORS:
        p = sv.factor_padding(which)
        ck.eq(f"{tag} padding of factor {which}", p, 0.0)
        worst = max(worst, p)
    out = {"pad": worst}
    if auut:
        rows = np.concatenate([(x * x).sum(axis=1) for x in cone_blocks(d["R"], name, sv.get_rank())])
        for key, env in (("pad_diag", None), ("pad_con", "1")):
            if env:
                os.environ["LRS_NO_AUV_DIAG"] = env
            try:
                sv.time_auut(1)
            finally:
                os.environ.pop("LRS_NO_AUV_DIAG", None)
            e = float(np.abs(sv.get_vec(solver_mod.Q1) - rows).max() / np.abs(rows).max())
            ck.le(f"{tag} {key}", e, 1e-12)
            out[key] = e
    return out


def steps_on_paths(sv, solver_mod, name, r, paths, ref, ck, layouts=None, pad=False, extra=None, expect=None):
    """K trips on every path in `paths` against the oracle's; the kernels that ran (expect: {path:
    kernels} where the path is declined); the padding of every factor, always."""
    want = lu.cone_ranks(name, r)
    for kpath in paths:
        sv.set_kernel_path(kpath)
        d = sv.alm_steps(K, fixedRank=r, reoptLevel=0)
        tag = f"{name} r {r} path {kpath}"
        ck.eq(f"{tag} trips", d["inner"], K)
        ck.eq(f"{tag} ranks", sv.get_rank(), want)
        lay = [sv.layout(k) for k in range(len(want))]
        ck.eq(f"{tag} layouts", lay, layouts or [lu.table_layout(q) for q in want])
        used = sv.kernel_path()
        ck.eq(f"{tag} kernels", used, (expect or {}).get(kpath, expected_path(name, kpath)))
        errs = {key: rel_err(d[key], ref[key]) for key in ("R", "G", "cvs")}
        if np.linalg.norm(ref["lam"]) > 0:
            errs["lam"] = rel_err(d["lam"], ref["lam"])
        else:
            ck.eq(f"{tag} lambda zero", bool(np.any(d["lam"])), False)
        rec = dict(kind="steps", inst=name, r=r, path=kpath, used=used, layout=lay, **errs)
        rec.update(padding_check(sv, solver_mod, name, d, ck, tag, auut=pad and name in lu.MAXCUT))
        if extra:
            rec.update(extra)
        report(**rec)
        for key, e in errs.items():
            ck.le(f"{tag} {key}", e, STEP_TOL)


def oracle_ref(olib, path, name, r):
    nr = sum(n * q for n, q in zip(lu.dims_of(name), lu.cone_ranks(name, r)))
    return lu.oracle_alm_steps(olib, path, r, K, lu.read_m(path), nr)


def pad_rank(r):
    """A(RR^T) against the unpadded row norms runs at a class's lower edge and at r = ld - 1."""
    return r in lu.LOWER_EDGES or r == lu.table_layout(r)[2] - 1


# ---- a. the table ---------------------------------------------------------------------------------
def test_layout_table(solver_mod, monkeypatch):
    """lrs_get_layout at every rank 1 .. 512 equals the table of tests/layout_util.py, ld >= r; with
    LRS_LAYOUT=GxE the forced layout wherever it holds the rank, else the table's."""
    monkeypatch.delenv("LRS_LAYOUT", raising=False)
    sv = solver_mod.Solver(lu.instance_path("mc_torus12x10"))
    with pytest.raises(RuntimeError, match="ranks not set"):
        sv.layout()
    seen = set()
    for r in range(1, 513):
        sv.set_rank([r])
        g, e, ld = sv.layout()
        assert (g, e, ld) == lu.table_layout(r) and ld == g * e and ld >= r, (r, g, e, ld)
        seen.add((g, e))
    assert len(seen) == len(lu.CLASSES)
    with pytest.raises(RuntimeError, match="cone"):
        sv.layout(1)
    with pytest.raises(RuntimeError, match="cone"):
        sv.layout(-1)
    with pytest.raises(RuntimeError, match="rank 513"):
        sv.set_rank([513])
    for g in (8, 16, 32, 64):
        for e in (1, 2, 3, 4):
            monkeypatch.setenv("LRS_LAYOUT", f"{g}x{e}")
            for r in sorted({1, max(1, g * e - 1), g * e, g * e + 1, 512}):
                sv.set_rank([r])
                assert sv.layout() == ((g, e, g * e) if g * e >= r else lu.table_layout(r)), (g, e, r)
    monkeypatch.setenv("LRS_LAYOUT", "24x2")   # not a layout: ignored
    sv.set_rank([40])
    assert sv.layout() == lu.table_layout(40)
    sv.close()


# ---- b. inner iterations, default layouts -----------------------------------------------------------
STEP_CASES = [(n, r) for n in ("mc_rand300w", "torus24x22", "rsparse60", "theta40", "theta25x3", "mc_torus12x10")
              for r in lu.STEP_RANKS[n]]


@pytest.mark.parametrize("name,r", STEP_CASES)
def test_inner_iterations_match_oracle(solver_mod, olib, gen_dir, monkeypatch, name, r):
    monkeypatch.setenv("LRS_SMALL", "0")   # path 0 = the multi-launch kernels (path 4: asked for below)
    monkeypatch.delenv("LRS_LAYOUT", raising=False)
    path = lu.instance_path(name, gen_dir)
    ref = oracle_ref(olib, path, name, r)
    sv = solver_mod.Solver(path)
    ck = Checks()
    paths = MULTI_PATHS
    if name == "mc_torus12x10" and lu.table_layout(r)[2] in lu.SMALL_LDS:
        paths = MULTI_PATHS + (4,)
    steps_on_paths(sv, solver_mod, name, r, paths, ref, ck, pad=pad_rank(r))
    sv.close()
    ck.done()


@pytest.mark.parametrize("r", [q for q in lu.STEP_RANKS["theta25x3"] if lu.table_layout(q)[2] in (8, 16, 24)])
def test_small_loop_multi_cone_matches_oracle(solver_mod, olib, monkeypatch, r):
    """Path 4 on theta25x3 at ld 8, 16 and 24: one workgroup for all cones and one a cone
    (LRS_SMALL_MC), C = -J as slots and as the constant objective's column sums (LRS_CONST_C)."""
    monkeypatch.delenv("LRS_LAYOUT", raising=False)
    name = "theta25x3"
    path = lu.instance_path(name)
    ref = oracle_ref(olib, path, name, r)
    ck = Checks()
    for const in ("0", "1"):
        monkeypatch.setenv("LRS_CONST_C", const)
        sv = solver_mod.Solver(path)
        for mc in ("0", "1"):
            monkeypatch.setenv("LRS_SMALL_MC", mc)
            steps_on_paths(sv, solver_mod, name, r, (4,), ref, ck, extra=dict(const=const, mc=mc))
        sv.close()
    ck.done()


# ---- c. operators, default layouts -------------------------------------------------------------------
def operators_against_oracle(sv, S, olib, path, name, r, ck, monkeypatch, extra=None):
    """The six steps of test_device_kernels_match_reference and time_auut on seeded inputs."""
    m, dims = lu.read_m(path), lu.dims_of(name)
    vec, NR = lu.op_inputs(name, r, m)
    s = lu.split_vec(vec, m, NR)
    g = lu.oracle_kernels(olib, path, r, vec, m, dims)
    assert g["tau"] != 0.0 and g["rootnum"] >= 1   # frozen so (tests/layout_util.py op_choice)
    tag = f"{name} r {r}"
    sv.set_rank([r] * len(dims))
    e = {}
    # (1) ALMCalq12p12
    sv.set_factor(S.R, s["R"])
    sv.set_factor(S.D, s["D"])
    q1, p1, q2, p2 = sv.q12()
    e["q1"], e["q2"] = rel_err(q1, g["q1"]), rel_err(q2, g["q2"])
    e["p1"] = abs(p1 - g["p1"]) / max(1, abs(g["p1"]))
    e["p2"] = abs(p2 - g["p2"]) / max(1, abs(g["p2"]))
    # (2) primalInfeasibility + CalObjRR, and A(RR^T) straight from the constraint entries
    cvs, pinf, pobj = sv.constr_rr()
    e["cvs_rr"] = rel_err(cvs, g["cvs_rr"])
    e["pinf_rr"] = abs(pinf - g["pinf_rr"]) / max(1, abs(g["pinf_rr"]))
    e["pobj_rr"] = abs(pobj - g["pobj_rr"]) / max(1, abs(g["pobj_rr"]))
    monkeypatch.delenv("LRS_NO_AUV_DIAG", raising=False)
    sv.time_auut(1)
    e["auut"] = rel_err(sv.get_vec(S.Q1), g["cvs_rr"])
    monkeypatch.setenv("LRS_NO_AUV_DIAG", "1")
    sv.time_auut(1)
    e["auut_con"] = rel_err(sv.get_vec(S.Q1), g["cvs_rr"])
    monkeypatch.delenv("LRS_NO_AUV_DIAG")
    # (3) ALMCalGrad
    sv.set_vec(S.LAMBDA, s["lam"])
    sv.set_vec(S.CVS, s["cvs"])
    G, lag = sv.grad(s["rho"])
    e["grad"] = rel_err(G, g["grad"])
    e["lag"] = abs(lag - g["lag"]) / abs(g["lag"])
    # (4) ALMLineSearch on (R, D) with q0 = b - cvs
    sv.q12()
    tau, rn = sv.line_search(s["rho"])
    ck.eq(f"{tag} roots", rn, int(g["rootnum"]))
    e_tau = abs(tau - g["tau"]) / max(1, abs(g["tau"]))
    # (5) L-BFGS two-loop (NodeNum 2 and 1) + UseGrad
    sv.set_factor(S.G, s["G"])
    sv.set_factor(S.S0, s["s1"]); sv.set_factor(S.Y0, s["y1"])
    sv.set_factor(S.S1, s["s2"]); sv.set_factor(S.Y1, s["y2"])
    e_l2 = rel_err(sv.lbfgs(2, s["beta1"], s["beta2"]), g["d_lbfgs2"])
    e_l1 = rel_err(sv.lbfgs(1, s["beta1"], s["beta2"]), g["d_lbfgs1"])
    # (6) ADMM half step (CG)
    sv.set_factor(S.U, s["U"]); sv.set_factor(S.V, s["V"])
    sv.set_vec(S.LAMBDA, s["lam"])
    u, rhs, it = sv.admm_half(s["rho_admm"], s["cg_tol"])
    e["rhs_cg"] = rel_err(rhs, g["rhs_cg"])
    e_u, ref_it = rel_err(u, g["u_cg"]), int(g["cg_iters"])
    rec = dict(kind="ops", inst=name, r=r, layout=[sv.layout(k) for k in range(len(dims))], tau=e_tau, lbfgs2=e_l2,
               lbfgs1=e_l1, u_cg=e_u, cg=it, cg_ref=ref_it, **e)
    if extra:
        rec.update(extra)
    report(**rec)
    for key, v in e.items():
        ck.le(f"{tag} {key}", v, TOL)
    ck.le(f"{tag} tau", e_tau, 1e-9)
    ck.le(f"{tag} lbfgs2", e_l2, 1e-9)
    ck.le(f"{tag} lbfgs1", e_l1, 1e-9)
    if name in lu.MAXCUT:
        ck.le(f"{tag} u_cg", e_u, 1e-6)
        ck.le(f"{tag} cg count {it} vs {ref_it}", abs(it - ref_it), 0.1 * ref_it)
    elif ref_it < lu.CG_COUNT_CAP:
        ck.le(f"{tag} u_cg", e_u, 1e-6)


OP_CASES = [(n, r) for n in ("mc_rand300w", "torus24x22", "mc_torus12x10", "rsparse60", "theta40", "theta25x3")
            for r in lu.OP_RANKS[n]]


@pytest.mark.parametrize("name,r", OP_CASES)
def test_operators_match_oracle(solver_mod, olib, gen_dir, monkeypatch, name, r):
    monkeypatch.delenv("LRS_LAYOUT", raising=False)
    path = lu.instance_path(name, gen_dir)
    sv = solver_mod.Solver(path)
    ck = Checks()
    operators_against_oracle(sv, solver_mod, olib, path, name, r, ck, monkeypatch)
    ck.eq(f"{name} r {r} layout", sv.layout(), lu.table_layout(r))
    sv.close()
    ck.done()


@pytest.mark.parametrize("name,r", lu.SWEEP_CASES)
def test_admm_sweep_matches_oracle(solver_mod, olib, monkeypatch, name, r):
    """LORADSUpdateSDPVar over every cone + LORADSUpdateDualVar through the operators at cg_tol 1e-9
    against the oracle's sweep: U, V and lambda to 1e-6; on MaxCut the total CG count within 15 %
    (elsewhere the oracle's own count moves by more than that between two builds of it)."""
    monkeypatch.delenv("LRS_LAYOUT", raising=False)
    S = solver_mod
    path = lu.instance_path(name)
    m, dims = lu.read_m(path), lu.dims_of(name)
    vec, NR = lu.op_inputs(name, r, m)
    vec[9 * NR + 2 * m + 4] = 1e-9
    s = lu.split_vec(vec, m, NR)
    g = lu.oracle_admm_sweep(olib, path, r, vec, m, dims)
    sv = S.Solver(path)
    sv.set_rank([r] * len(dims))
    sv.set_factor(S.U, s["U"])
    sv.set_factor(S.V, s["V"])
    sv.set_vec(S.LAMBDA, s["lam"])
    sv.admm_constr()
    its = []
    for c in range(len(dims)):
        for side in (0, 1):
            its.append(sv.admm_half(s["rho_admm"], s["cg_tol"], cone=c, side=side, init=False)[2])
    sv.dual_update(s["rho_admm"])
    e = {"U": rel_err(sv.get_factor(S.U), g["U"]), "V": rel_err(sv.get_factor(S.V), g["V"]),
         "lam": rel_err(sv.get_vec(S.LAMBDA), g["lam"])}
    report(kind="sweep", inst=name, r=r, layout=[sv.layout(k) for k in range(len(dims))], cg=int(sum(its)),
           cg_ref=int(g["cg_total"]), **e)
    sv.close()
    for key, v in e.items():
        assert v < 1e-6, (key, v)
    if name in lu.MAXCUT:
        assert abs(sum(its) - g["cg_total"]) <= max(4, 0.15 * g["cg_total"]), (its, g["cg_total"])


# ---- d. the layouts only LRS_LAYOUT reaches ------------------------------------------------------------
@pytest.mark.parametrize("g,e,pad", [(g, e, pad) for g, e in lu.FORCED for pad in (0, 1)])
def test_forced_layouts_match_oracle(solver_mod, olib, monkeypatch, g, e, pad):
    """8 x 4, 16 x 1, 16 x 4, 32 x 1, 32 x 4 and 64 x 1 at r = G E and r = G E - 1 on mc_rand300w:
    the inner iterations on paths 0, 1, 2, 3 and 5 and the operators, the getter confirming the layout."""
    monkeypatch.setenv("LRS_SMALL", "0")
    monkeypatch.setenv("LRS_LAYOUT", f"{g}x{e}")
    name, r = "mc_rand300w", g * e - pad
    path = lu.instance_path(name)
    ref = oracle_ref(olib, path, name, r)
    sv = solver_mod.Solver(path)
    ck = Checks()
    steps_on_paths(sv, solver_mod, name, r, MULTI_PATHS, ref, ck, layouts=[(g, e, g * e)], pad=bool(pad),
                   extra=dict(forced=f"{g}x{e}"))
    operators_against_oracle(sv, solver_mod, olib, path, name, r, ck, monkeypatch, extra=dict(forced=f"{g}x{e}"))
    ck.eq("layout after set_rank", sv.layout(), (g, e, g * e))
    sv.close()
    ck.done()


# ---- e. cones of different layouts in one problem ---------------------------------------------------------
@pytest.mark.parametrize("r,lay", [(64, [(32, 2, 64), (16, 3, 48)]), (100, [(64, 2, 128), (16, 3, 48)])])
def test_mixed_layouts_match_oracle(solver_mod, olib, gen_dir, monkeypatch, r, lay):
    """Two MaxCut blocks (n = 120 and 36) at --fixedRank 64 / 100: cone ranks 64 / 100 and 36, so
    the cones' layouts differ (no merged launch; k_small_alm needs one layout for all cones, so path
    4 must decline and run the iteration as path 0 does)."""
    monkeypatch.setenv("LRS_SMALL", "0")
    monkeypatch.delenv("LRS_LAYOUT", raising=False)
    name = "mc_2blk"
    path = lu.instance_path(name, gen_dir)
    ref = oracle_ref(olib, path, name, r)
    assert ref["R"].size == 120 * min(r, 120) + 36 * 36
    sv = solver_mod.Solver(path)
    assert sv.dims == [120, 36]
    ck = Checks()
    steps_on_paths(sv, solver_mod, name, r, (0, 1, 2), ref, ck, layouts=lay)
    assert lay[0] != lay[1]
    # path 4: refused by small_alm_args (c.ld != ld), the iteration falls back to the automatic path
    steps_on_paths(sv, solver_mod, name, r, (4,), ref, ck, layouts=lay, expect={4: expected_path(name, 0)})
    sv.close()
    ck.done()

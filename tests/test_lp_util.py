"""The NumPy restatement of the LP block's column sweep (tests/lp_util.py) against the reference's
own run (tests/golden/admm_sweep_lp_mc_lp60.npz, scripts/make_golden_lp.py), and the helpers' own
properties.  CPU only.

Bar of the restatement: 16 eps relative to max(1, max |ref|) per array.  The sweep is closed-form
arithmetic in one fixed order, so the float64 restatement repeats the reference's roundings except
where the fixture's inputs differ in their last bits: the constraint sums the sweep starts from are
formed here from the fixture's output SDP rows and input LP values (the reference holds them as
running sums through the two CG half-steps).  Measured: u 3.8e-16, v 3.1e-16, sums 3.0e-16."""
import os

import numpy as np

import lp_util as lu
from golden_util import GOLDEN, instance


def mc_lp60():
    g = np.load(os.path.join(GOLDEN, "admm_sweep_lp_mc_lp60.npz"))
    problem = lu.read_problem(instance("mc_lp60"))
    return g, problem, lu.lp_columns(problem)


def test_lp_columns_of_mc_lp60():
    """63 columns: 60 slacks with one entry, the split free variable's two columns, and column 62
    in 20 of 61 constraints (>= m/4): exactly one dropped column, its 20 entries gone, its norm kept."""
    _, problem, cols = mc_lp60()
    assert (cols.m, cols.n) == (61, 63)
    assert cols.dense == [62] and cols.dropped == 20
    assert cols.con[62].size == 0 and abs(cols.nrm2[62] - 20 * 0.01 ** 2) <= 8 * lu.EPS * 20 * 0.01 ** 2
    assert cols.entries == 62 and cols.slots == list(range(63))
    assert [x.tolist() for x in cols.con[:3]] == [[0], [1], [2]]
    assert cols.con[60].tolist() == [60] and cols.a[61].tolist() == [-1.0]
    assert cols.c[:60].tolist() == [0.1] * 60 and cols.c[60:].tolist() == [0.5, 0.5, 1.0]


def test_restatement_reproduces_the_reference_sweep():
    g, problem, cols = mc_lp60()
    rank, dims = int(g["rank"]), [int(d) for d in g["dims"]]
    nsdp = dims[0] * rank
    # the sums the LP loop starts from: the SDP cone after its two half-steps, the LP block before
    Uin = np.concatenate([g["U"][:nsdp], g["U0"][nsdp:]])
    Vin = np.concatenate([g["V"][:nsdp], g["V0"][nsdp:]])
    cvs0 = lu.constr_values(problem, cols, Uin, Vin, rank)
    u, v, cvs = lu.lp_sweep(cols, problem[2], g["lam0"], float(g["rho"]), g["U0"][nsdp:], g["V0"][nsdp:], cvs0)
    errs = {"u": lu.rel_max(u, g["U"][nsdp:]), "v": lu.rel_max(v, g["V"][nsdp:]), "cvs": lu.rel_max(cvs, g["cvs"])}
    print("restatement against the reference (relative to max(1, max |ref|)):", errs)
    for key, e in errs.items():
        assert e <= 16 * lu.EPS, (key, e)
    # and the dual update that follows: lambda += rho (b - A(X))
    lam = g["lam0"] + float(g["rho"]) * (problem[2] - cvs)
    assert lu.rel_max(lam, g["lam"]) <= 16 * lu.EPS


def test_longdouble_restatement_is_the_same_sweep():
    """The two types walk the same chain: their difference on mc_lp60 is rounding (below 64 eps),
    and longdouble is really wider here (the floor is not zero)."""
    g, problem, cols = mc_lp60()
    nsdp = int(g["dims"][0]) * int(g["rank"])
    assert np.finfo(np.longdouble).eps < lu.EPS
    floor, hi = lu.sweep_floor(cols, problem[2], g["lam0"], float(g["rho"]), g["U0"][nsdp:], g["V0"][nsdp:], g["cvs"])
    assert 0.0 < floor <= 64 * lu.EPS, floor
    assert hi[0].dtype == np.longdouble


def test_lp_problem_round_trip_and_column_typing():
    """lp_problem's columns come back from lp_columns: duplicates summed, entries in constraint
    order, a column without data, a cost-only column, and the m/4 rule at its edge (m = 8: two
    entries are exactly a quarter)."""
    cols_in = [(0.5, [(3, 1.0), (1, 2.0), (3, 0.25)]), (None, []), (2.0, []), (None, [(0, -1.0)]),
               (None, [(2, 1.0), (5, -2.0)]), (1.0, [(7, 3.0), (7, -1.0)])]
    problem = lu.lp_problem(4, 8, cols_in, seed=1)
    assert problem[0] == 8 and problem[1] == [4, -6]
    cols = lu.lp_columns(problem)
    assert cols.c.tolist() == [0.5, 0.0, 2.0, 0.0, 0.0, 1.0]
    assert cols.con[0].tolist() == [] and cols.nrm2[0] == np.sqrt(2.0 ** 2 + 1.25 ** 2) ** 2   # 2 of 8: dense
    assert cols.con[4].tolist() == [] and cols.dense == [0, 4] and cols.dropped == 4
    assert cols.con[3].tolist() == [0] and cols.a[3].tolist() == [-1.0]
    assert cols.con[5].tolist() == [7] and cols.a[5].tolist() == [2.0] and cols.nrm2[5] == 4.0
    assert cols.slots == [0, 2, 3, 5] and cols.entries == 2
    # a column without data: u <- v_old, v <- that value (to the rounding of rho y / rho)
    rng = np.random.default_rng(2)
    u0, v0 = rng.standard_normal(6), rng.standard_normal(6)
    u, v, cvs = lu.lp_sweep(cols, problem[2], rng.standard_normal(8), 0.37, u0, v0, rng.standard_normal(8))
    assert abs(u[1] - v0[1]) <= 2 * lu.EPS * abs(v0[1]) and abs(v[1] - v0[1]) <= 4 * lu.EPS * abs(v0[1])
    u2, v2, _ = lu.lp_sweep(cols, problem[2], rng.standard_normal(8), 4.0, u0, v0, rng.standard_normal(8))
    assert u2[1] == v0[1] and v2[1] == v0[1]                       # exactly, at a power of two

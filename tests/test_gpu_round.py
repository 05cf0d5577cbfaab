"""Sign rounding of a factor on the device (include/lrsdp.h lrs_round_signs)
against the NumPy restatement of tests/round_util.py, which reads the instance file only.

Bars.  The sign words must equal the restatement's bit for bit: before any comparison the test
checks on the CPU that every |<R_i, g_t>| / (|R_i| |g_t|) exceeds 1e-9 (seven orders above the
1e-16-relative difference two FP64 summation orders of a dot can have), so no sign is a matter of
rounding, and no row or trial is left out.  On the golden MaxCut instances the weights are
half-integers and b = 1, so every value is an exact FP64 sum whatever its order: values must be
equal.  With b in {1, 4, 9} the products C_ij sqrt(b_i b_j) are exact too, but the bar the issue
sets there is 1e-12 relative.  The descent is deterministic given the signs, so its final words,
values and sweep count must equal the sequential restatement's."""
import importlib
import threading

import numpy as np
import pytest

import round_util as ru
from golden_util import instance

pytestmark = pytest.mark.gpu

R_ID = 0   # LRS_R


@pytest.fixture(scope="module")
def solver_mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.solver")


@pytest.fixture(scope="module")
def inst_mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.instances")


@pytest.fixture(scope="module")
def nonunit(tmp_path_factory, inst_mod):
    """A 70-vertex random graph with weights +-1 and b_i in {1, 4, 9}."""
    rng = np.random.default_rng(11)
    n = 70
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.size) < 0.08
    ei, ej = iu[keep], ju[keep]
    w = rng.choice([-1.0, 1.0], size=ei.size)
    deg = np.zeros(n)
    np.add.at(deg, ei, w)
    np.add.at(deg, ej, w)
    d = np.arange(1, n + 1)
    nz = deg != 0
    ents = [(np.zeros(ei.size, int), 1, ei + 1, ej + 1, -0.5 * w), (np.zeros(int(nz.sum()), int), 1, d[nz], d[nz], 0.5 * deg[nz]),
            (d, 1, d, d, np.ones(n))]
    b = rng.choice([1.0, 4.0, 9.0], size=n)
    return inst_mod.write_sdpa(str(tmp_path_factory.mktemp("round") / "mc_b149.dat-s"), n, [n], b, ents)


_cd_cache = {}


def cone_data(path, cone=0):
    """The file's view of a cone, read once and shared (never modified by a test)."""
    key = (path, cone)
    if key not in _cd_cache:
        _cd_cache[key] = ru.cone_data(path, cone)
    return _cd_cache[key]


def factor_and_dirs(n, r, T, seed):
    """Seeded factor and hyperplanes whose every sign clears the 1e-9 margin (checked here, on
    the CPU, for all n x T pairs)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, r))
    g = rng.standard_normal((r, T))
    mg = ru.margin(X, g)
    assert mg > 1e-9, mg
    return X, g


def put_factor(sv, X_list):
    """Factors (n_k x r_k each) into LRS_R, column-major per cone."""
    sv.set_rank([X.shape[1] for X in X_list])
    sv.set_factor(R_ID, np.concatenate([X.ravel(order="F") for X in X_list]))


def check_best(out, vals):
    bt = int(np.argmin(vals))   # the first smallest
    assert out["best_trial"] == bt
    assert out["best_value"] == vals[bt]


BITS_CASES = [("mc_torus12x10", 1), ("mc_torus12x10", 3), ("mc_torus12x10", 19), ("mc_torus12x10", 64),
              ("mc_rand300w", 19), ("mc_rand300w", 290)]


@pytest.mark.parametrize("T", [64, 192])
@pytest.mark.parametrize("name,r", BITS_CASES)
def test_bits_and_values_match_restatement(solver_mod, name, r, T):
    path = instance(name)
    cd = cone_data(path)
    X, g = factor_and_dirs(cd["n"], r, T, seed=1000 + r + T)
    sv = solver_mod.Solver(path)
    put_factor(sv, [X])
    out = sv.round_signs(T, dirs=g, local_search=False)
    sv.close()
    S = ru.signs(X, g)
    assert np.array_equal(out["bits"], ru.signs_to_bits(S))
    vals = ru.values(cd, S)
    assert np.array_equal(out["values"], vals), np.abs(out["values"] - vals).max()
    check_best(out, out["values"])
    assert np.array_equal(out["x"], S[:, out["best_trial"]].astype(np.int8))
    assert out["sweeps"] == 0


def test_nonunit_b_matches_restatement(solver_mod, nonunit):
    cd = cone_data(nonunit)
    assert set(np.unique(cd["b"])) == {1.0, 4.0, 9.0}
    T = 192
    X, g = factor_and_dirs(cd["n"], 19, T, seed=77)
    sv = solver_mod.Solver(nonunit)
    put_factor(sv, [X])
    out = sv.round_signs(T, dirs=g, local_search=False)
    sv.close()
    S = ru.signs(X, g)
    assert np.array_equal(out["bits"], ru.signs_to_bits(S))
    vals = ru.values(cd, S)
    err = np.abs(out["values"] - vals) / np.maximum(1.0, np.abs(vals))
    print("non-unit b: largest relative value error", err.max())
    assert err.max() <= 1e-12, err.max()
    check_best(out, out["values"])
    assert np.array_equal(out["x"], S[:, out["best_trial"]].astype(np.int8))


@pytest.mark.parametrize("name", ["mc_torus12x10", "mc_rand300w", "nonunit"])
def test_descent_matches_sequential_restatement(solver_mod, nonunit, name):
    path = nonunit if name == "nonunit" else instance(name)
    cd = cone_data(path)
    T = 128
    X, g = factor_and_dirs(cd["n"], 19, T, seed=500 + cd["n"])
    sv = solver_mod.Solver(path)
    put_factor(sv, [X])
    before = sv.round_signs(T, dirs=g, local_search=False)
    out = sv.round_signs(T, dirs=g, local_search=True)
    one = sv.round_signs(T, dirs=g, local_search=True, max_sweeps=1)
    sv.close()
    S0 = ru.signs(X, g)
    assert np.array_equal(before["bits"], ru.signs_to_bits(S0))
    S, used = ru.descent(cd, S0, 50)
    assert used.max() < 50                      # every trial reached its local optimum
    assert np.array_equal(out["bits"], ru.signs_to_bits(S))
    vals = ru.values(cd, S)
    if name == "nonunit":
        assert (np.abs(out["values"] - vals) <= 1e-12 * np.maximum(1.0, np.abs(vals))).all()
    else:
        assert np.array_equal(out["values"], vals)
    assert out["sweeps"] == int(used.max())
    assert (out["values"] <= before["values"]).all()
    assert (out["values"] < before["values"]).any()      # the descent did something
    # no single flip of any final assignment lowers its value
    assert (ru.one_flip_gains(cd, ru.bits_to_signs(out["bits"], T)) >= 0).all()
    check_best(out, out["values"])
    assert np.array_equal(out["x"], S[:, out["best_trial"]].astype(np.int8))
    # max_sweeps = 1: one sweep, the same words as the restatement's first sweep
    S1, used1 = ru.descent(cd, S0, 1)
    assert one["sweeps"] == 1 and used1.max() == 1
    assert np.array_equal(one["bits"], ru.signs_to_bits(S1))


def test_two_cones_round_independently(solver_mod, inst_mod, tmp_path):
    """Two tori of different sizes in one file, constraints numbered consecutively: each cone is
    rounded by its own call, and cone 1's result is the single-cone instance's."""
    m0, d0, b0, e0 = inst_mod.maxcut_torus_problem(6, 5, 3)
    m1, d1, b1, e1 = inst_mod.maxcut_torus_problem(7, 6, 4)
    n0, n1 = d0[0], d1[0]
    ents = [e0[0], e0[1], (e1[0][0], 2, e1[0][2], e1[0][3], e1[0][4]), (e1[1][0] + n0, 2, e1[1][2], e1[1][3], e1[1][4])]
    both = inst_mod.write_sdpa(str(tmp_path / "two.dat-s"), n0 + n1, [n0, n1], np.concatenate([b0, b1]), ents)
    alone = inst_mod.write_sdpa(str(tmp_path / "one.dat-s"), m1, d1, b1, e1)
    T = 64
    X0, g0 = factor_and_dirs(n0, 5, T, seed=21)
    X1, g1 = factor_and_dirs(n1, 7, T, seed=22)
    sv = solver_mod.Solver(both)
    put_factor(sv, [X0, X1])
    o0 = sv.round_signs(T, dirs=g0, cone=0)
    o1 = sv.round_signs(T, dirs=g1, cone=1)
    sv.close()
    sa = solver_mod.Solver(alone)
    put_factor(sa, [X1])
    oa = sa.round_signs(T, dirs=g1)
    sa.close()
    for k in ("values", "bits", "x"):
        assert np.array_equal(o1[k], oa[k]), k
    assert (o1["best_trial"], o1["best_value"], o1["sweeps"]) == (oa["best_trial"], oa["best_value"], oa["sweeps"])
    for cone, (o, X, g) in enumerate([(o0, X0, g0), (o1, X1, g1)]):
        cd = cone_data(both, cone)
        S, used = ru.descent(cd, ru.signs(X, g), 50)
        assert np.array_equal(o["bits"], ru.signs_to_bits(S))
        assert np.array_equal(o["values"], ru.values(cd, S))
        assert o["sweeps"] == int(used.max())


def test_seeded_equals_explicit_and_repeats(solver_mod):
    path = instance("mc_torus12x10")
    n, r, T = 120, 19, 128
    g = solver_mod.round_dirs(7, r, T)
    X = np.random.default_rng(5).standard_normal((n, r))
    assert ru.margin(X, g) > 1e-9
    sv = solver_mod.Solver(path)
    put_factor(sv, [X])
    a = sv.round_signs(T, seed=7)
    b = sv.round_signs(T, dirs=g)
    c = sv.round_signs(T, seed=7)
    sv.close()
    assert np.array_equal(a["bits"], ru.signs_to_bits(ru.descent(cone_data(path), ru.signs(X, g), 50)[0]))
    for k in ("bits", "values", "x"):
        assert np.array_equal(a[k], b[k]), k
        assert a[k].tobytes() == c[k].tobytes(), k
    assert (a["best_trial"], a["best_value"], a["sweeps"]) == (c["best_trial"], c["best_value"], c["sweeps"])


def test_sandwich_on_a_solved_instance(solver_mod, inst_mod, tmp_path):
    """pobj (a lower bound up to the solve's tolerance) <= the integer optimum <= the best rounded
    value, on a 4 x 5 torus whose optimum over the 2^19 assignments NumPy enumerates."""
    path = inst_mod.maxcut_torus(str(tmp_path / "torus4x5.dat-s"), 4, 5, 9)
    cd = cone_data(path)
    n = cd["n"]
    assert n == 20
    codes = np.arange(1 << (n - 1), dtype=np.int64)
    S = np.ones((n, codes.size), dtype=np.int8)            # s_0 = +1: the value is even in s
    for i in range(1, n):
        S[i] = 1 - 2 * ((codes >> (i - 1)) & 1)
    opt = np.zeros(codes.size)
    for i, j, v in zip(cd["ci"], cd["cj"], cd["cv"]):
        opt += (v if i == j else 2.0 * v) * (S[i] * S[j])
    optimum = float(opt.min())
    sv = solver_mod.Solver(path)
    res = sv.solve()
    out = sv.round_signs(256, seed=1, local_search=True)
    sv.close()
    pobj = res["pobj"]
    print(f"sandwich: pobj {pobj!r} optimum {optimum!r} rounded {out['best_value']!r}")
    assert pobj - 1e-4 * (1 + abs(pobj)) <= optimum <= out["best_value"]
    x = out["x"].astype(np.float64)
    assert set(np.unique(x)) <= {-1.0, 1.0}
    assert out["best_value"] == ru.values(cd, x[:, None])[0]
    assert out["best_value"] == out["values"].min()


def _refused(call):
    with pytest.raises(Exception) as ei:
        call()
    e = ei.value
    assert type(e).__name__ == "RoundError", repr(e)
    assert e.code < 0 and e.message, (e.code, e.message)
    return e.code


def test_refusals_leave_the_context_usable(solver_mod):
    path = instance("mc_torus12x10")
    T = 64
    X, g = factor_and_dirs(120, 3, T, seed=31)
    sv = solver_mod.Solver(path)
    assert _refused(lambda: sv.round_signs(T, seed=1)) == -6          # ranks unset
    put_factor(sv, [X])
    ref = sv.round_signs(T, dirs=g)

    def still_works():
        again = sv.round_signs(T, dirs=g)
        assert np.array_equal(again["bits"], ref["bits"]) and np.array_equal(again["values"], ref["values"])

    assert _refused(lambda: sv.round_signs(100, seed=1)) == -2
    still_works()
    assert _refused(lambda: sv.round_signs(8192, seed=1)) == -2
    still_works()
    assert _refused(lambda: sv.round_signs(T, seed=1, cone=1)) == -4
    still_works()
    th = solver_mod.Solver(instance("theta40"))                        # not diagonally constrained
    th.set_rank(th.determine_rank())
    assert _refused(lambda: th.round_signs(T, seed=1)) in (-7, -9)
    th.close()
    still_works()
    lp = solver_mod.Solver(instance("mc_lp60"))                        # the LP block's cone
    lp.set_rank(lp.determine_rank())
    assert lp.K == 2
    assert _refused(lambda: lp.round_signs(T, seed=1, cone=1)) == -5
    assert _refused(lambda: lp.round_signs(T, seed=1, cone=0)) == -7  # X_ii + s_i = 1 touches the LP block
    lp.close()
    still_works()
    # a loopback-sharded context
    grp = solver_mod.LoopbackGroup(2)
    codes, errs = [None, None], []

    def work(rk):
        try:
            s2 = solver_mod.Solver(path)
            s2.shard_loopback(grp, rk)
            codes[rk] = _refused(lambda: s2.round_signs(T, seed=1))
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
    assert codes == [-3, -3]
    still_works()
    sv.close()

"""The NumPy restatements of tests/cut_util.py on cases worked by hand, and weak
duality of the restated bound against enumeration.  No GPU."""
import importlib

import numpy as np
import pytest

import cut_util as cu
import round_util as ru
import tri_util as tu


@pytest.fixture(scope="module")
def inst_mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.instances")


def k4(inst_mod):
    """The complete graph on 4 vertices, unit weights: C = -F0 has -3/2 on the diagonal and +1/2
    off it, so <C, x x^T> = -2 (edges cut) and the optimum is -8."""
    iu, ju = np.triu_indices(4, 1)
    return inst_mod._maxcut_problem(4, iu, ju, np.ones(iu.size))


def test_slack_on_the_hand_written_case():
    """Rows (1,-1,0), (0,1,-1), (-1,0,1), (1,-1,0), b = 1: x01 = x02 = x12 = x13 = x23 = -1, x03 = 2
    (the case of tests/test_tri_cuts.py).  slack = 1 + sigma . x = -violation."""
    X = np.array([[1.0, -1.0, 0.0], [0.0, 1.0, -1.0], [-1.0, 0.0, 1.0], [1.0, -1.0, 0.0]])
    cuts = [[0, 1, 2, 0],    # 1 + (-1 - 1 - 1)
            [0, 1, 3, 1],    # 1 + (-1 - 2 + 1)
            [0, 2, 3, 3],    # 1 + (+1 - 2 - 1)
            [1, 2, 3, 2]]    # 1 + (+1 - 1 + 1)
    assert cu.slack(X, np.ones(4), cuts).tolist() == [-2.0, -1.0, -1.0, 2.0]
    rc, rv, _, _ = tu.separate(X, np.ones(4), 8)
    assert (cu.slack(X, np.ones(4), rc) == -rv).all()
    # b scaled: x_ij = <X_i, X_j> / sqrt(b_i b_j)
    b = np.array([1.0, 4.0, 4.0, 16.0])
    assert cu.slack(X, b, [[0, 1, 2, 0], [0, 1, 3, 1]]).tolist() == [1 + (-0.5 - 0.5 - 0.25), 1 + (-0.5 - 0.5 + 0.125)]


def test_dense_s_and_bound_on_the_hand_written_case(inst_mod):
    """K4 plus the cut (0, 1, 2, type 0), lambda = (-2, -2, -2, -2, mu).  S = C - sum lambda_i A_i has
    1/2 on the diagonal, (1 - mu) / 2 on the pairs of the triangle {0, 1, 2} and 1/2 on the pairs
    with vertex 3.
    mu = +1: S = [[I, 1], [1^T, 1]] / 2, eigenvalues 1/2, 1/2 and (1 +- sqrt 3) / 2, so
    bound = (-8 - 1) + 4 (1 - sqrt 3) / 2 + 0 = -7 - 2 sqrt 3.
    mu = -1: S = [[2 J - I, 1], [1^T, 1]] / 2, eigenvalues -1/2, -1/2 and (3 +- sqrt 7) / 2, so
    bound = (-8 + 1) + 4 (-1/2) + 4 (-1) = -13."""
    prob = inst_mod.add_triangle_cuts(k4(inst_mod), [[0, 1, 2, 0]])
    assert prob[0] == 5 and prob[1] == [4, -1]
    lam = np.array([-2.0, -2.0, -2.0, -2.0, 1.0])
    S = cu.dense_S(prob, lam)
    assert np.array_equal(S, 0.5 * np.array([[1, 0, 0, 1], [0, 1, 0, 1], [0, 0, 1, 1], [1, 1, 1, 1.0]]))
    val, lmin = cu.bound(prob, lam)
    assert abs(lmin - (1 - np.sqrt(3)) / 2) < 1e-14 and abs(val - (-7 - 2 * np.sqrt(3))) < 1e-13
    assert cu.lp_dual_slack(prob, lam).tolist() == [1.0]
    lam[4] = -1.0
    S = cu.dense_S(prob, lam)
    assert np.array_equal(S, 0.5 * np.array([[1, 2, 2, 1], [2, 1, 2, 1], [2, 2, 1, 1], [1, 1, 1, 1.0]]))
    val, lmin = cu.bound(prob, lam)
    assert abs(lmin + 0.5) < 1e-14 and abs(val + 13.0) < 1e-13
    assert cu.lp_dual_slack(prob, lam).tolist() == [-1.0]
    # the plain problem: S = C + 2 I = J / 2 >= 0 (eigenvalues 0, 0, 0, 2), bound = b^T lambda = -8,
    # the optimum
    val, lmin = cu.bound(k4(inst_mod), lam[:4])
    assert abs(lmin) < 1e-14 and abs(val + 8.0) < 1e-13


def cycle5(inst_mod):
    ei = np.arange(5)
    return inst_mod._maxcut_problem(5, ei, (ei + 1) % 5, np.ones(5))


@pytest.mark.parametrize("name", ["cycle5", "torus4x5"])
def test_restated_bound_is_below_the_optimum(inst_mod, tmp_path, name):
    """Weak duality, which holds by mathematics for every lambda: on the plain problem and with
    seeded sets of triangle inequalities, at a handful of arbitrary multipliers."""
    prob = cycle5(inst_mod) if name == "cycle5" else inst_mod.maxcut_torus_problem(4, 5, 3)
    n = prob[1][0]
    opt = tu.brute_force_min(ru.cone_data(inst_mod.write_sdpa(str(tmp_path / "p.dat-s"), *prob)))
    if name == "cycle5":
        assert opt == -8.0
    rng = np.random.default_rng(11)
    i, j, k = tu.triples(n)
    tight = []
    for T in (0, 1, 7, 40):
        p = prob
        if T:
            pick = rng.choice(i.size, size=min(T, i.size), replace=False)
            p = inst_mod.add_triangle_cuts(prob, np.stack([i[pick], j[pick], k[pick], rng.integers(0, 4, pick.size)], 1))
        for scale in (0.0, 0.3, 1.0, 5.0):
            lam = scale * rng.standard_normal(p[0])
            lam[:n] -= 1.0
            val, _ = cu.bound(p, lam, m0=n)
            assert val <= opt + 1e-9 * (1 + abs(opt)), (T, scale, val, opt)
            tight.append(opt - val)
    assert min(tight) < 30.0      # the bound is not vacuous at every sample

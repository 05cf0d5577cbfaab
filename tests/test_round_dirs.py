"""lrs_round_dirs, the host-side generator of the sign rounding's hyperplane normals (include/
lrsdp.h): splitmix64 of (seed, trial, column), then Box-Muller.  No GPU."""
import importlib

import numpy as np
import pytest

from round_util import round_dirs_py


@pytest.fixture(scope="module")
def solver_mod():
    return importlib.import_module("ltr-lowrank-sdp_amd.solver")


def test_round_dirs_is_deterministic_and_seeded(solver_mod):
    a = solver_mod.round_dirs(7, 19, 128)
    b = solver_mod.round_dirs(7, 19, 128)
    c = solver_mod.round_dirs(8, 19, 128)
    assert a.shape == (19, 128)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)
    assert np.abs(a - c).max() > 0.1
    # a trial's direction depends on (seed, trial, column) alone: fewer trials are a prefix
    assert np.array_equal(solver_mod.round_dirs(7, 19, 64), a[:, :64])


@pytest.mark.parametrize("seed,r,trials", [(0, 1, 64), (7, 19, 64), (2 ** 63 + 12345, 5, 128)])
def test_round_dirs_matches_the_documented_generator(solver_mod, seed, r, trials):
    got = solver_mod.round_dirs(seed, r, trials)
    ref = round_dirs_py(seed, r, trials)
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() <= 1e-14, np.abs(got - ref).max()


def test_round_dirs_moments(solver_mod):
    g = solver_mod.round_dirs(3, 64, 512)
    assert g.size == 64 * 512
    assert abs(g.mean()) <= 0.05, g.mean()
    assert abs(g.var() - 1.0) <= 0.05, g.var()


def test_round_dirs_refuses_bad_arguments(solver_mod):
    with pytest.raises(RuntimeError):
        solver_mod.round_dirs(1, 0, 64)

"""Rank-one dense constraint-matrix instances for the tests (scripts/make_golden_rank1.py):
regenerated from the generator arguments in tests/golden/rank1_instances.json, checked against
the stored sha256, written once per session."""
import hashlib
import importlib
import json
import os

from golden_util import GOLDEN

GEN_KEYS = ("dims", "m_sparse", "k", "n_terms", "n_full", "neg", "hole", "hole_frac", "cross", "boundary", "seed",
            "scale")
# per cone: 0-based constraints the reference's rule types dense / the rank-one ones among them
# with their signs.  The constraints follow sum(m_sparse) sparse ones: n_full full random
# coefficients, then the terms (r1_70x37's last term, the boundary one, comes out sparse).
EXPECT_DENSE = {"r1_64": [[40, 41, 42, 43, 44, 45]], "r1_70x37": [[50, 51, 52, 53], []],
                "r1_200": [list(range(300, 320))]}
EXPECT_RANK1 = {"r1_64": [[41, 42, 43, 44, 45]], "r1_70x37": [[50, 51, 52, 53], []],
                "r1_200": [list(range(300, 320))]}
EXPECT_SIGMA = {"r1_64": [[1.0, -1.0, 1.0, 1.0, 1.0]], "r1_70x37": [[-1.0, 1.0, 1.0, 1.0], []],
                "r1_200": [[1.0, 1.0, 1.0, -1.0] + [1.0] * 16]}


def meta():
    with open(os.path.join(GOLDEN, "rank1_instances.json")) as f:
        return json.load(f)


def args_of(name):
    g = meta()[name]
    return {k: g[k] for k in GEN_KEYS}


def r1_path(name, directory):
    """The instance `name` as a .dat-s file under `directory` (generated once, sha256 checked)."""
    inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")
    path = os.path.join(str(directory), f"{name}.dat-s")
    if not os.path.exists(path):
        inst.rank_one_constraints(path, **args_of(name))
    sha = hashlib.sha256(open(path, "rb").read()).hexdigest()
    assert sha == meta()[name]["sha256"], f"generator drifted: {name}"
    return path


class env:
    """Environment settings for the problems loaded inside the block (LRS_RANK1_A, LRS_DENSE_A and
    LRS_R1_CHUNK are read at load / launch time); None unsets."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

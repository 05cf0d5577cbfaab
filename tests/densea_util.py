"""Dense constraint-matrix instances for the tests (scripts/make_golden_densea.py): regenerated
from the generator arguments in tests/golden/densea_instances.json, checked against the stored
sha256, written once per session."""
import hashlib
import importlib
import json
import os

from golden_util import GOLDEN

# 0-based constraints the reference's rule (more than 10 % of the lower triangle, strictly) types
# dense, per cone: the fills constraints follow the sum(m_sparse) sparse ones; da70x40's last one
# sits at exactly floor(0.1 T) entries (sparse), and its constraint 51 has five entries in cone 1
EXPECT_DENSE = {"da64": [[40, 41, 42, 43]], "da70x40": [[50, 51, 52], []], "da200": [[300, 301, 302, 303, 304]]}


def meta():
    with open(os.path.join(GOLDEN, "densea_instances.json")) as f:
        return json.load(f)


def args_of(name):
    g = meta()[name]
    return {k: g[k] for k in ("dims", "m_sparse", "k", "fills", "cross", "seed")}


def da_path(name, directory):
    """The instance `name` as a .dat-s file under `directory` (generated once, sha256 checked)."""
    inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")
    path = os.path.join(str(directory), f"{name}.dat-s")
    if not os.path.exists(path):
        inst.dense_constraints(path, **args_of(name))
    sha = hashlib.sha256(open(path, "rb").read()).hexdigest()
    assert sha == meta()[name]["sha256"], f"generator drifted: {name}"
    return path


class dense_a:
    """LRS_DENSE_A for the problems loaded inside the block (read at load time)."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.old = os.environ.get("LRS_DENSE_A")
        os.environ["LRS_DENSE_A"] = self.v

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("LRS_DENSE_A", None)
        else:
            os.environ["LRS_DENSE_A"] = self.old

"""bench.py's plain run and its --full / --dump-outputs options.

CPU: the dump writer on a stand-in solver (float64 files, the size cap's seeded sample is the
same from call to call).  GPU: a plain run on a small torus times exactly --steps inner
iterations, carries the contract keys and none of the --full legs, and dumps the state that
W + K trips of the same solve give in one go (bit for bit, as
test_gpu_steps.py::test_budget_hook_resumes_same_solve pins for the factor)."""
import importlib
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
NAMES = ("R", "G", "lambda", "cvs", "s", "y", "last_step")
FULL_ONLY = ("roofline", "wall_clock_to_eps", "cpu_baseline", "north_star", "configs_wall_clock_to_eps",
             "roofline_at_scale", "config_c5", "config_c5b", "sharded")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Lib:
    @staticmethod
    def lrs_alm_last_step(ctx, out, newest):
        for k in range(4):
            out[k] = 0.5 + k
        newest._obj.value = 1
        return 0


class _Solver:
    """The calls dump_outputs makes, answered from fixed arrays."""
    lib, ctx = _Lib(), None

    def __init__(self, nr, m):
        self.nr, self.m = nr, m

    def _check(self, rc, what):
        assert rc == 0, what

    def get_factor(self, which):
        return np.arange(self.nr, dtype=np.float64) + 1000.0 * which

    def get_vec(self, which):
        return np.arange(self.m, dtype=np.float64) - 7.0 * which


def test_dump_outputs_files_and_seeded_sample(tmp_path, monkeypatch):
    b = _bench()
    solver = importlib.import_module("ltr-lowrank-sdp_amd.solver")
    sv = _Solver(5000, 300)
    b.dump_outputs(sv, str(tmp_path / "a"))
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in NAMES}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{n}.npy" for n in NAMES)
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["R"], sv.get_factor(solver.R)) and np.array_equal(got["cvs"], sv.get_vec(solver.CVS))
    assert np.array_equal(got["s"], sv.get_factor(solver.S1))      # newest pair = 1
    assert got["last_step"].tolist() == [0.5, 1.5, 2.5, 3.5]
    # over the cap: a sample of the entries, in place order, the same in every call, within the cap
    monkeypatch.setattr(b, "DUMP_CAP_BYTES", 7 * (4096 + 8 * 1000))
    b.dump_outputs(sv, str(tmp_path / "b"))
    b.dump_outputs(sv, str(tmp_path / "c"))
    total = 0
    for n in NAMES:
        x, y = np.load(tmp_path / "b" / f"{n}.npy"), np.load(tmp_path / "c" / f"{n}.npy")
        assert np.array_equal(x, y)
        total += os.path.getsize(tmp_path / "b" / f"{n}.npy")
        if n in ("lambda", "cvs", "last_step"):
            assert np.array_equal(x, got[n])                      # under the cap: whole
        else:
            assert x.size == 1000 and np.all(np.diff(x) > 0) and np.all(np.isin(x, got[n]))
    assert total <= b.DUMP_CAP_BYTES


def test_instance_cache_leaves_an_unwritable_tree(tmp_path, monkeypatch):
    """Where .bench_instances cannot be made in the tree, the instances go to a per-user
    directory under the system's temporary directory, and are generated there."""
    b = _bench()
    (tmp_path / "w").mkdir()
    monkeypatch.setattr(b, "ROOT", str(tmp_path / "w"))
    assert b.instance_cache() == str(tmp_path / "w" / ".bench_instances")
    blocker = tmp_path / "tree"
    blocker.write_text("a file where the tree would be: nothing can be created below it")
    monkeypatch.setattr(b, "ROOT", str(blocker))
    monkeypatch.setenv("TMPDIR", str(tmp_path))
    import tempfile
    monkeypatch.setattr(tempfile, "tempdir", None)
    cache = b.instance_cache()
    assert os.path.dirname(cache) == str(tmp_path) and os.path.isdir(cache)
    assert b.instance_cache() == cache
    path = b.instance_for(0, 6, 7, cache)
    assert os.path.dirname(path) == cache and os.path.getsize(path) > 0


def test_full_and_dump_options_parse_in_dry_run(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--dry-run", "--full", "--dump-outputs",
                        str(tmp_path / "d")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["dry_run"]


@pytest.mark.gpu
def test_plain_run_steps_keys_and_dump(tmp_path):
    W, K = 7, 23
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--rows", "12", "--cols", "10", "--steps", str(K),
                        "--warmup", str(W), "--dump-outputs", str(tmp_path / "d")], capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == K and d["warmup"] == W and d["n_gpus"] == 1 and d["dtype"] == "f64"
    assert d["unit"] == "ALM inner iterations/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) <= 1e-6 * 1e3
    assert not [k for k in FULL_ONLY if k in d], d.keys()
    # the dump against W + K trips of the same seeded instance in one go
    solver = importlib.import_module("ltr-lowrank-sdp_amd.solver")
    inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")
    path = str(tmp_path / "t.dat-s")
    inst.maxcut_torus(path, 12, 10, seed=67)
    sv = solver.Solver(path)
    ref = sv.alm_steps(W + K, fixedRank=d["config"]["rank"], reoptLevel=0, phase1Tol=1e-300)
    sv.close()
    assert ref["inner"] == W + K
    for name, key in (("R", "R"), ("G", "G"), ("lambda", "lam"), ("cvs", "cvs"), ("s", "s"), ("y", "y")):
        got = np.load(tmp_path / "d" / f"{name}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, ref[key]), name
    last = np.load(tmp_path / "d" / "last_step.npy")
    assert last.tolist() == [ref["tau"], ref["lag"], ref["pinf"], ref["beta"]]

#!/usr/bin/env python3
"""Dense constraint matrices: the dense-A path against the slot path.

Instance (seeded, instances.dense_constraints_problem): one block of n rows, m sparse
constraints of 6 entries, `--full` constraints filling the whole lower triangle and `--part` at
30 %, fixed rank r.  Reports, on one GPU:

* ALM inner iterations per second after warm-up over at least 0.5 s of work, under
  LRS_DENSE_A=1 and LRS_DENSE_A=0 alternating, three repeats each (the =0 leg is the behaviour
  without the dense path);
* lrs_time_dense_a (one k_dcon_ax launch over the stack) against the stack's bytes over 8 TB/s
  and against 2 k_d n^2 r flop over the measured FP64 matrix-core rate;
* with --reference: the reference's rate on the same instance written as a file
  (oracle/_ref/lorads_ref_harness alm_rate, one core; CPU only, no GPU needed with --no-gpu).

Run:  python scripts/densea_probe.py [--n 2000] [--out profiles/densea_probe_n2000]
"""
import argparse
import importlib
import json
import math
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HARNESS = os.path.join(ROOT, "oracle", "_ref", "lorads_ref_harness")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--m", type=int, default=2000)
    ap.add_argument("--full", type=int, default=8)
    ap.add_argument("--part", type=int, default=8)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--ref-seconds", type=float, default=20.0)
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")
    t0 = time.time()
    prob = inst.dense_constraints_problem([a.n], [a.m], 6, [1.0] * a.full + [0.3] * a.part, None, a.n)
    out = {"n": a.n, "m": prob[0], "k_d": a.full + a.part, "rank": a.rank, "gen_seconds": time.time() - t0}
    if not a.no_gpu:
        solver = importlib.import_module("ltr-lowrank-sdp_amd.solver")
        coo = inst.coo_arrays(prob)
        kw = dict(fixedRank=a.rank, reoptLevel=0)
        svs = {}
        for mode in ("1", "0"):
            os.environ["LRS_DENSE_A"] = mode
            t0 = time.time()
            svs[mode] = solver.Solver(coo=coo)
            out[f"load_seconds_A{mode}"] = time.time() - t0
        os.environ.pop("LRS_DENSE_A")
        nd, on, nbytes = svs["1"].dense_a_info(0)
        out.update(n_dense=nd, on_dense_path=on, stack_bytes=nbytes, slots_A1=svs["1"].nslots, slots_A0=svs["0"].nslots)
        steps = {}
        for mode in ("1", "0"):   # calibration: enough steps for min-seconds of timed work
            r = svs[mode].alm_timed(5, 10, **kw)
            steps[mode] = max(10, int(math.ceil(1.2 * a.min_seconds * r["done"] / r["seconds"])))
        legs = {"1": [], "0": []}
        for _ in range(a.repeats):
            for mode in ("1", "0"):
                r = svs[mode].alm_timed(5, steps[mode], **kw)
                legs[mode].append({"iters": r["done"], "seconds": r["seconds"], "iters_per_s": r["done"] / r["seconds"]})
        out["legs"] = legs
        for mode in ("1", "0"):
            v = [x["iters_per_s"] for x in legs[mode]]
            out[f"iters_per_s_A{mode}"] = {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}
        ms = svs["1"].time_dense_a(0, 20)
        peak = svs["1"].mfma_f64_peak()
        flop = 2.0 * nd * a.n * a.n * a.rank
        out["dcon_ax"] = {"ms": ms, "stack_bytes": nbytes, "hbm_bound_ms": nbytes / 8e12 * 1e3,
                          "achieved_TBps": nbytes / (ms * 1e-3) / 1e12, "flop": flop, "mfma_f64_peak_TF": peak,
                          "mfma_bound_ms": flop / (peak * 1e12) * 1e3, "achieved_TF": flop / (ms * 1e-3) / 1e12}
        out["dcon_ax"]["bound"] = "HBM" if out["dcon_ax"]["hbm_bound_ms"] >= out["dcon_ax"]["mfma_bound_ms"] else "MFMA"
        for sv in svs.values():
            sv.close()
    if a.reference:
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "densea.dat-s")
            inst.write_sdpa(path, *prob)
            t0 = time.time()
            r = subprocess.run([HARNESS, "alm_rate", path, str(a.rank), "1000000", str(a.ref_seconds)], capture_output=True, text=True,
                               env=dict(os.environ, OPENBLAS_NUM_THREADS="1"))
            rate = [ln for ln in r.stdout.splitlines() if ln.startswith("REF_RATE")]
            out["reference"] = {"wall_seconds": time.time() - t0, "budget_seconds": a.ref_seconds,
                                "ref_rate": rate[-1] if rate else r.stdout[-300:]}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + ".json.log", "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

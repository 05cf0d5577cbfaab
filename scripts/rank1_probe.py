#!/usr/bin/env python3
"""Rank-one dense constraint matrices: the factor against the stack and the slots.

Instance (seeded, instances.rank_one_constraints_problem): densea_probe.py's family with the 16
dense coefficients made rank one -- one block of n rows, m sparse constraints of 6 entries, 16
constraints sigma a a^T (one with sigma = -1, one with a third of a zero), fixed rank r.
Reports, on one GPU:

* ALM inner iterations per second after warm-up over at least 0.5 s of work, three legs
  alternating, three repeats each: the factor (LRS_RANK1_A=1), the stack (LRS_RANK1_A=0,
  LRS_DENSE_A=1) and the slots (LRS_RANK1_A=0, LRS_DENSE_A=0) -- the last two are the behaviour
  without the factor;
* lrs_time_rank1 (one V^T R launch, finish included) against its bytes over 8 TB/s;
* with --capacity P: one leg with P terms passed through lrs_load_coo_rank1 (never expanded; no
  stack or slot leg exists to compare with);
* with --reference: the reference's rate on the same instance written as a file
  (oracle/_ref/lorads_ref_harness alm_rate, one core; CPU only, no GPU needed with --no-gpu).

Run:  python scripts/rank1_probe.py [--n 2000] [--out profiles/rank1_probe_n2000]
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
LEGS = {"factor": ("1", None), "stack": ("0", "1"), "slots": ("0", "0")}


def setenv(r1, da):
    for k, v in (("LRS_RANK1_A", r1), ("LRS_DENSE_A", da)):
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def rate_legs(svs, kw, repeats, min_seconds):
    steps = {}
    for leg, sv in svs.items():   # calibration: enough steps for min_seconds of timed work
        r = sv.alm_timed(5, 10, **kw)
        steps[leg] = max(10, int(math.ceil(1.2 * min_seconds * r["done"] / r["seconds"])))
    legs = {leg: [] for leg in svs}
    for _ in range(repeats):
        for leg, sv in svs.items():
            r = sv.alm_timed(5, steps[leg], **kw)
            legs[leg].append({"iters": r["done"], "seconds": r["seconds"], "iters_per_s": r["done"] / r["seconds"]})
    out = {"legs": legs}
    for leg in svs:
        v = [x["iters_per_s"] for x in legs[leg]]
        out[f"iters_per_s_{leg}"] = {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--m", type=int, default=2000)
    ap.add_argument("--terms", type=int, default=16)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--capacity", type=int, default=0)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--ref-seconds", type=float, default=20.0)
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")
    gen = lambda p, expand: inst.rank_one_constraints_problem([a.n], [a.m], 6, p, 0, 1, 2, 0.33, None, False, a.n,
                                                              expand=expand)
    out = {"n": a.n, "terms": a.terms, "rank": a.rank}
    kw = dict(fixedRank=a.rank, reoptLevel=0)
    if a.capacity:
        solver = importlib.import_module("ltr-lowrank-sdp_amd.solver")
        t0 = time.time()
        prob, terms = gen(a.capacity, False)
        setenv(None, None)
        sv = solver.Solver(coo=dict(inst.coo_arrays(prob), terms=terms))
        out.update(m=prob[0], terms=a.capacity, load_seconds=time.time() - t0)
        nd, on_d, stack = sv.dense_a_info(0)
        n1, on, fbytes = sv.rank1_info(0)
        out.update(n_dense=nd, stack_bytes=stack, n_rank1=n1, on_factor_path=on, factor_bytes=fbytes,
                   stack_would_be_bytes=8 * a.capacity * a.n * a.n)
        out.update(rate_legs({"capacity": sv}, kw, a.repeats, a.min_seconds))
        ms, nbytes = sv.time_rank1(0, 20)
        out["r1_vtx"] = {"ms": ms, "bytes": nbytes, "hbm_bound_ms": nbytes / 8e12 * 1e3,
                         "achieved_TBps": nbytes / (ms * 1e-3) / 1e12}
        sv.close()
    else:
        t0 = time.time()
        prob, _ = gen(a.terms, True)
        out.update(m=prob[0], gen_seconds=time.time() - t0)
        if not a.no_gpu:
            solver = importlib.import_module("ltr-lowrank-sdp_amd.solver")
            coo = inst.coo_arrays(prob)
            svs = {}
            for leg, (r1, da) in LEGS.items():
                setenv(r1, da)
                t0 = time.time()
                svs[leg] = solver.Solver(coo=coo)
                out[f"load_seconds_{leg}"] = time.time() - t0
            setenv(None, None)
            n1, on, fbytes = svs["factor"].rank1_info(0)
            out.update(n_rank1=n1, on_factor_path=on, factor_bytes=fbytes, stack_bytes=svs["stack"].dense_a_info(0)[2],
                       slots={leg: sv.nslots for leg, sv in svs.items()})
            auto = solver.Solver(coo=coo)   # unset: what the automatic rule picks for this instance
            out["auto"] = {"on_factor_path": auto.rank1_info(0)[1], "on_dense_path": auto.dense_a_info(0)[1]}
            auto.close()
            out.update(rate_legs(svs, kw, a.repeats, a.min_seconds))
            ms, nbytes = svs["factor"].time_rank1(0, 20)
            out["r1_vtx"] = {"ms": ms, "bytes": nbytes, "hbm_bound_ms": nbytes / 8e12 * 1e3,
                             "achieved_TBps": nbytes / (ms * 1e-3) / 1e12}
            for sv in svs.values():
                sv.close()
        if a.reference:
            with tempfile.TemporaryDirectory() as td:
                path = os.path.join(td, "rank1.dat-s")
                inst.write_sdpa(path, *prob)
                t0 = time.time()
                r = subprocess.run([HARNESS, "alm_rate", path, str(a.rank), "1000000", str(a.ref_seconds)],
                                   capture_output=True, text=True, env=dict(os.environ, OPENBLAS_NUM_THREADS="1"))
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

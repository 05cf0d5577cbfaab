"""Batched solves against the two ways the library already had of solving many small instances
(profiles/batch_probe.md).  B instances, timed three ways on one build:

  (a) sequential   one thread, lrs_solve on each context in turn
  (b) threads      B host threads, each lrs_solve on its own context (own stream)
  (c) batch        one lrs_solve_batch

Two sets: B copies of the 12 x 10 torus with different seeds; a mixed set of generated tori
(5 x 4 .. 12 x 10) and theta instances (n 20 .. 50).  Two legs: phase 1 only (skipADMM=1) and whole
solves.  The contexts are created and every way is run once before the timing; each timed figure
is a host clock around calls that end in a stream synchronise.  `--repeats` interleaved repeats
(a, b, c, a, b, c, ...); median and range of each, the batch's counters and its rounds by width.

`--legs whole` (or `phase1`) keeps one leg; `--flag disableOracle=1` (repeatable) adds a solver
parameter to every leg, e.g. to take the rank oracle's Gram out of the ADMM iterations.  Where the
library has the ADMM meeting, its counters (lrs_batch_admm_stats) and rounds by width are reported
beside the ALM meeting's; the script also runs on a build without them, for an A/B.

    python scripts/batch_probe.py [--B 32] [--repeats 5] [--legs both] [--flag k=v] [--json out.json] [--md out.md]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
solver = importlib.import_module("ltr-lowrank-sdp_amd.solver")
inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")


def theta_problem(n, n_edges, seed):
    rng = np.random.default_rng(seed)
    ei, ej = inst._random_edges(rng, n, n_edges)
    b = np.zeros(1 + n_edges)
    b[0] = 1.0
    return 1 + n_edges, [n], b, inst._theta_entries(n, ei, ej, 1, 1)


def make_sets(B):
    rng = np.random.default_rng(7)
    same = [inst.maxcut_torus_problem(12, 10, 1000 + i) for i in range(B)]
    mixed = []
    for i in range(B):
        if i % 2 == 0:
            mixed.append(inst.maxcut_torus_problem(int(rng.integers(5, 13)), int(rng.integers(4, 11)), 2000 + i))
        else:
            n = int(rng.integers(20, 51))
            mixed.append(theta_problem(n, 3 * n, 3000 + i))
    return {"torus12x10 x B": same, "mixed tori + theta": mixed}


def run_set(name, problems, kw, repeats):
    lib = solver.load_library()
    svs = [solver.Solver(coo=inst.coo_arrays(p)) for p in problems]
    B = len(svs)
    prm = solver.default_params(**kw)
    res = (solver.Result * B)()
    rc = (C.c_int * B)()
    ctxs = (C.c_void_p * B)(*[sv.ctx for sv in svs])
    batch = solver.Batch()

    def way_a():
        t0 = time.perf_counter()
        for i, sv in enumerate(svs):
            assert lib.lrs_solve(sv.ctx, C.byref(prm), C.byref(res[i])) == 0
        return time.perf_counter() - t0

    def way_b():
        def work(i):
            rc[i] = lib.lrs_solve(svs[i].ctx, C.byref(prm), C.byref(res[i]))
        ts = [threading.Thread(target=work, args=(i,)) for i in range(B)]
        t0 = time.perf_counter()
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        dt = time.perf_counter() - t0
        assert not any(rc), list(rc)
        return dt

    def way_c():
        t0 = time.perf_counter()
        r = lib.lrs_solve_batch(batch.h, ctxs, B, C.byref(prm), 1, res, rc)
        dt = time.perf_counter() - t0
        assert r == 0, lib.lrs_last_error()
        return dt

    ways = {"a sequential": way_a, "b threads": way_b, "c batch": way_c}
    inner = {}
    for k, f in ways.items():   # warm-up, and the three ways compute the same
        f()
        inner[k] = [int(res[i].alm_inner) for i in range(B)]
    assert inner["a sequential"] == inner["b threads"] == inner["c batch"], "the ways differ in their iteration counts"
    times = {k: [] for k in ways}
    for _ in range(repeats):
        for k, f in ways.items():
            times[k].append(f())
    out = {"set": name, "B": B, "flags": kw, "alm_inner_total": sum(inner["c batch"]),
           "alm_inner_max": max(inner["c batch"]), "batch_stats": batch.stats(),
           "round_widths": batch.round_widths(),
           "admm_stats": batch.admm_stats() if hasattr(batch, "admm_stats") else None,
           "admm_round_widths": batch.admm_round_widths() if hasattr(batch, "admm_round_widths") else None,
           "admm_iter_total": sum(int(res[i].admm_iter) for i in range(B)),
           "seconds": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}
                       for k, v in times.items()}}
    for sv in svs:
        sv.close()
    batch.close()
    return out


def to_markdown(results):
    lines = ["| set | leg | (a) sequential ms | (b) threads ms | (c) batch ms | a / c | b / c |", "|---|---|---|---|---|---|---|"]
    for r in results:
        s = r["seconds"]
        cell = lambda k: f"{s[k]['median'] * 1e3:.2f} ({s[k]['min'] * 1e3:.2f} .. {s[k]['max'] * 1e3:.2f})"
        leg = "phase 1 (skipADMM=1)" if r["flags"].get("skipADMM") else "whole solve"
        extra = {k: v for k, v in r["flags"].items() if k != "skipADMM"}
        leg += f" {extra}" if extra else ""
        lines.append(f"| {r['set']} (B = {r['B']}) | {leg} | {cell('a sequential')} | {cell('b threads')} | "
                     f"{cell('c batch')} | {s['a sequential']['median'] / s['c batch']['median']:.2f} | "
                     f"{s['b threads']['median'] / s['c batch']['median']:.2f} |")
    lines.append("")
    for r in results:
        leg = "phase 1" if r["flags"].get("skipADMM") else "whole solve"
        lines.append(f"* {r['set']}, {leg}: inner iterations {r['alm_inner_total']} in all, longest member "
                     f"{r['alm_inner_max']}; lrs_batch_stats {r['batch_stats']}; rounds by width {r['round_widths']}")
        if r.get("admm_stats") is not None:
            lines.append(f"  * ADMM iterations {r['admm_iter_total']} in all; lrs_batch_admm_stats {r['admm_stats']}; "
                         f"ADMM rounds by width {r['admm_round_widths']}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", choices=("both", "phase1", "whole"), default="both")
    ap.add_argument("--flag", action="append", default=[], help="k=v: a solver parameter for every leg")
    ap.add_argument("--json")
    ap.add_argument("--md")
    a = ap.parse_args()
    results = []
    for name, problems in make_sets(a.B).items():
        for kw in ({"skipADMM": 1}, {}):
            if a.legs != "both" and (a.legs == "phase1") != bool(kw):
                continue
            for f in a.flag:
                k, v = f.split("=", 1)
                kw[k] = float(v) if "." in v or "e" in v.lower() else int(v)
            results.append(run_set(name, problems, kw, a.repeats))
            print(json.dumps(results[-1]), flush=True)
    md = to_markdown(results)
    print(md)
    if a.json:
        json.dump(results, open(a.json, "w"), indent=1)
    if a.md:
        open(a.md, "w").write(md + "\n")


if __name__ == "__main__":
    main()

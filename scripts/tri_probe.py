"""Triangle-inequality separation after a default solve (profiles/tri_probe.md) on
the bundled G11 (n = 800) and the G67-like 100 x 100 torus of instances.CONFIGS (n = 10^4).  Per
instance:

  * the solve's time and pobj;
  * ms per Solver.separate_triangles(K) call on LRS_R: a host clock around a call that ends in a
    stream synchronise (the call's last step copies the records back), one untimed call first, then
    `--reps` calls, median (min .. max);
  * the same for a call with min_violation = 10, above every possible violation of a unit-diagonal
    matrix: the Gram kernel and exactly one scan, in which no inequality qualifies, so 4 C(n, 3)
    over its time is the scan's rate without the selection's atomics; the full call's time over it
    says how many scans the selection took and what the qualifying inequalities cost;
  * at n <= --numpy-max-n, the same K cuts by a blockwise NumPy restatement on the host (one i at a
    time, all j < k at once, the running best K kept), timed once, and whether its cuts and count
    equal the device's (reported, not asserted: on a solved instance violations lie within
    rounding of 0 and of each other).

    python scripts/tri_probe.py [--cuts 1024] [--reps 5] [--instances G11,G67] [--md out.md] [--json out.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
solver = importlib.import_module("ltr-lowrank-sdp_amd.solver")
inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")


def timed(fn, reps):
    fn()
    ts = []
    out = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return out, ts


def numpy_separate(X, K, minv=0.0):
    """The K most violated inequalities of unit-diagonal x = X X^T, one row i at a time."""
    n = X.shape[0]
    x = X @ X.T
    best_v = np.empty(0)
    best_i = np.empty(0, dtype=np.int64)
    count = 0
    for i in range(n - 2):
        j, k = np.triu_indices(n - i - 1, 1)
        j += i + 1
        k += i + 1
        a, b, c = x[i, j], x[i, k], x[j, k]
        ab, amb = a + b, a - b
        v = np.stack([-1.0 - (ab + c), -1.0 - (amb - c), -1.0 - (-amb - c), -1.0 - (c - ab)], axis=1).ravel()
        q = np.flatnonzero(v > minv)
        count += q.size
        idx = ((i * n + j[q // 4]) * n + k[q // 4]) * 4 + q % 4
        best_v = np.concatenate([best_v, v[q]])
        best_i = np.concatenate([best_i, idx])
        if best_v.size > 4 * K:
            keep = np.lexsort((best_i, -best_v))[:K]
            best_v, best_i = best_v[keep], best_i[keep]
    keep = np.lexsort((best_i, -best_v))[:K]
    best_v, best_i = best_v[keep], best_i[keep]
    t = best_i // 4
    cuts = np.stack([t // (n * n), t // n % n, t % n, best_i % 4], axis=1).astype(np.int32)
    return cuts, best_v, count


def probe(name, directory, K, reps, numpy_max_n, log):
    path = os.path.join(ROOT, "data", "bundled", f"{name}.dat-s")
    if not os.path.exists(path):
        path = inst.config_instance(name, directory)
    sv = solver.Solver(path)
    res = sv.solve()
    n, r = sv.dims[0], sv.get_rank()[0]
    total = 4 * (n * (n - 1) * (n - 2) // 6)
    pobj = res["pobj"] if abs(res["pobj"]) < 1e29 else res["alm_pobj"]
    row = dict(instance=name, n=n, rank=r, cuts=K, inequalities=total, pobj=pobj, solve_ms=1e3 * res["solve_time"])
    log(row)
    _, t_one = timed(lambda: sv.separate_triangles(K, min_violation=10.0), reps)
    row.update(one_scan_ms=t_one, scan_rate=total / (1e-3 * statistics.median(t_one)))
    log(row)
    out, t_full = timed(lambda: sv.separate_triangles(K), reps)
    row.update(call_ms=t_full, n_cuts=int(out[0].shape[0]), n_violated=int(out[2]), max_violation=float(out[3]),
               kth_violation=float(out[1][-1]) if out[1].size else 0.0,
               scans_equivalent=statistics.median(t_full) / statistics.median(t_one))
    log(row)
    if n <= numpy_max_n:
        X = sv.get_factor(solver.R).reshape(r, n).T
        t0 = time.perf_counter()
        cuts, viol, count = numpy_separate(X, K)
        row.update(numpy_ms=1e3 * (time.perf_counter() - t0), numpy_cuts_equal=bool(np.array_equal(cuts, out[0])),
                   numpy_n_violated=int(count),
                   numpy_max_abs_diff=float(np.abs(viol - out[1]).max()) if viol.shape == out[1].shape else None)
        log(row)
    sv.close()
    return row


def fmt(ts):
    return f"{statistics.median(ts):.2f} ({min(ts):.2f} .. {max(ts):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cuts", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--instances", default="G11,G67")
    ap.add_argument("--numpy-max-n", type=int, default=800)
    ap.add_argument("--md")
    ap.add_argument("--json")
    a = ap.parse_args()
    rows = []

    def log(row):
        print(json.dumps(row), flush=True)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(rows + [row], f, indent=1)

    with tempfile.TemporaryDirectory() as d:
        for name in a.instances.split(","):
            rows.append(probe(name, d, a.cuts, a.reps, a.numpy_max_n, log))
    lines = [f"| instance | n | rank | inequalities | solve ms | call ms, K = {a.cuts} | Gram + one scan ms | scan, inequalities / s |"
             " call / one scan | violated | largest | K-th | NumPy ms | NumPy cuts equal |", "|" + "---|" * 14]
    for q in rows:
        npms = f"{q['numpy_ms']:.0f}" if "numpy_ms" in q else "not run"
        npeq = f"{q['numpy_cuts_equal']} (count {q['numpy_n_violated']})" if "numpy_ms" in q else ""
        lines.append(f"| {q['instance']} | {q['n']} | {q['rank']} | {q['inequalities']:.3e} | {q['solve_ms']:.1f} | "
                     f"{fmt(q['call_ms'])} | {fmt(q['one_scan_ms'])} | {q['scan_rate']:.3e} | {q['scans_equivalent']:.2f} | "
                     f"{q['n_violated']} | {q['max_violation']:.4f} | {q['kth_violation']:.4f} | {npms} | {npeq} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.md:
        with open(a.md, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

"""Rank reduction on the device, measured (profiles/compress_probe.md).  One run
each on one MI355X; nothing is asserted.

  (a) lrs_factor_compress wall time on a factor with a prescribed spectrum (kept eigenvalues
      geometric 1 .. 1e-3, dropped 1e-9 .. 1e-12) at n = 2e4, r = 64 -> 13; n = 2e4, r = 290 -> 64;
      the 2000 x 2000 torus (n = 4e6), r = 16 -> 8; the k_rot launches alone between two HIP events
      (lrs_compress_timing) and their fraction of 8 TB/s at 8 n (r + k) bytes; against the only
      route without it: get_factor + NumPy eigh + set_rank + set_factor through solver.py (R only).
  (b) whole solves with and without the in-solve hook (set_rank_shrink(1e-6)): theta25x3, theta40,
      the bundled theta102, G11, and the G81-like torus at fixedRank 64.
  (c) cut_loop on G11, 3 rounds x 1024 cuts, with and without compress_tol = 1e-6.

Host clock around calls that end in a stream synchronise.

    python scripts/compress_probe.py [--parts a,b,c] [--skip-torus] [--time-limit 60] [--md out.md]
"""
import argparse
import importlib
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
solver = importlib.import_module("ltr-lowrank-sdp_amd.solver")
inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")

R = 0
PEAK = 8e12   # bytes / s


def spectrum(r, k):
    kept = np.geomspace(1.0, 1e-3, k) if k > 1 else np.ones(1)
    return np.concatenate([kept, np.geomspace(1e-9, 1e-12, r - k)])


def factor(n, r, k, seed):
    rng = np.random.default_rng(seed)
    u0 = np.linalg.qr(rng.standard_normal((n, r)))[0]
    v0 = np.linalg.qr(rng.standard_normal((r, r)))[0]
    return (u0 * np.sqrt(spectrum(r, k))) @ v0.T


def part_a(lines, skip_torus):
    lines += ["## (a) lrs_factor_compress against the host route\n",
              "| n | r -> k | compress ms (wall) | k_rot ms (events) | k_rot bytes | fraction of 8 TB/s | host route ms | "
              "of it get / eigh + product / set_rank + set_factor |", "|---|---|---|---|---|---|---|---|"]
    cases = [("rand", 20000, 64, 13), ("rand", 20000, 290, 64)] + ([] if skip_torus else [("torus", 4000000, 16, 8)])
    for kind, n, r, k in cases:
        if kind == "rand":
            rng = np.random.default_rng(1)
            ei = rng.integers(0, n, 3 * n)
            ej = (ei + 1 + rng.integers(0, n - 1, 3 * n)) % n
            key = np.unique(np.minimum(ei, ej) * n + np.maximum(ei, ej))   # no edge twice
            problem = inst._maxcut_problem(n, key // n, key % n, np.ones(key.size))
        else:
            problem = inst.maxcut_torus_problem(2000, 2000, 2000)
        sv = solver.Solver(coo=inst.coo_arrays(problem))
        del problem
        X = factor(n, r, k, seed=r)
        flat = np.ascontiguousarray(X).ravel(order="F")
        sv.set_rank([r])
        sv.set_factor(R, flat)
        sv.compress(ranks=[r])          # first use: module load, allocator warm-up
        sv.set_rank([r])
        sv.set_factor(R, flat)
        sv.sync()
        t0 = time.perf_counter()
        out = sv.compress(rel_tol=1e-6)
        wall = 1e3 * (time.perf_counter() - t0)
        ms, nbytes = sv.compress_timing()
        assert out["ranks"] == [k], out["ranks"]
        # the host route
        sv.set_rank([r])
        sv.set_factor(R, flat)
        sv.sync()
        t0 = time.perf_counter()
        H = sv.get_factor(R).reshape(r, n).T
        t1 = time.perf_counter()
        w, Q = np.linalg.eigh(H.T @ H)
        Y = H @ Q[:, ::-1][:, :k]
        t2 = time.perf_counter()
        sv.set_rank([k])
        sv.set_factor(R, np.ascontiguousarray(Y).ravel(order="F"))
        sv.sync()
        t3 = time.perf_counter()
        sv.close()
        lines.append(f"| {n} | {r} -> {k} | {wall:.2f} | {ms:.3f} | {nbytes:.3e} | {nbytes / (ms * 1e-3) / PEAK:.3f} | "
                     f"{1e3 * (t3 - t0):.1f} | {1e3 * (t1 - t0):.1f} / {1e3 * (t2 - t1):.1f} / {1e3 * (t3 - t2):.1f} |")
        print(lines[-1], flush=True)
    lines.append("")


def locate(name, directory):
    for base in (os.path.join(ROOT, "tests", "golden", "instances"), os.path.join(ROOT, "data", "bundled")):
        path = os.path.join(base, f"{name}.dat-s")
        if os.path.exists(path):
            return path
    return inst.config_instance(name, directory)


def part_b(lines, limit, directory):
    lines += ["## (b) whole solves with and without set_rank_shrink(1e-6)\n",
              "| instance | hook | s | ADMM iterations | pobj | dobj | gap | pinf | final rank | status |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    for name, kw in (("theta25x3", {}), ("theta40", {}), ("theta102", {}), ("G11", {}), ("G81", dict(fixedRank=64))):
        path = locate(name, directory)
        for hook in (False, True):
            sv = solver.Solver(path)
            if hook:
                sv.set_rank_shrink(1e-6)
            t0 = time.perf_counter()
            res = sv.solve(timeSecLimit=limit, **kw)
            dt = time.perf_counter() - t0
            ranks = sv.get_rank()
            sv.close()
            if res["pobj"] > 1e29:   # the ALM phase met phase2Tol: no ADMM phase, no ADMM objectives
                res["pobj"], res["dobj"] = res["alm_pobj"], res["alm_dobj"]
            lines.append(f"| {name} | {'on' if hook else 'off'} | {dt:.3f} | {res['admm_iter']} | {res['pobj']:.8e} | "
                         f"{res['dobj']:.8e} | {res['gap']:.2e} | {res['pinf']:.2e} | {res['final_rank']} {ranks} | "
                         f"{res['status']} |")
            print(lines[-1], flush=True)
    lines.append("")


def part_c(lines, limit):
    lines += ["## (c) cut_loop on G11, 3 rounds x 1024 cuts\n",
              "| compress_tol | round | cuts | s | ALM inner | ADMM | pobj | certified bound | rank |",
              "|---|---|---|---|---|---|---|---|---|"]
    path = os.path.join(ROOT, "data", "bundled", "G11.dat-s")
    for tol in (None, 1e-6):
        sv = solver.Solver(path)
        recs = sv.cut_loop(3, 1024, compress_tol=tol, timeSecLimit=limit)
        sv.close()
        for q, rec in enumerate(recs):
            if rec["pobj"] > 1e29:
                rec["pobj"] = float("nan")   # no ADMM phase in that round: read the certified bound
            lines.append(f"| {tol} | {q} | {rec['n_cuts']} | {rec['time_sec']:.3f} | {rec['alm_inner']} | {rec['admm_iter']} | "
                         f"{rec['pobj']:.6f} | {rec['certified_bound']:.4f}{'' if rec['bound_converged'] else ' (nc)'} | "
                         f"{rec.get('rank', '')} |")
            print(lines[-1], flush=True)
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--skip-torus", action="store_true")
    ap.add_argument("--time-limit", type=float, default=60.0)
    ap.add_argument("--md")
    a = ap.parse_args()
    lines = ["# Rank reduction: rotate factors to principal axes on the device\n"]

    def flush():
        if a.md:   # written after every part: a long run keeps what it has
            with open(a.md, "w") as f:
                f.write("\n".join(lines) + "\n")

    with tempfile.TemporaryDirectory() as d:
        for part in a.parts.split(","):
            if part == "a":
                part_a(lines, a.skip_torus)
            elif part == "b":
                part_b(lines, a.time_limit, d)
            elif part == "c":
                part_c(lines, a.time_limit)
            flush()
    print("\n".join(lines))


if __name__ == "__main__":
    main()

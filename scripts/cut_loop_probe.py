"""Cutting-plane rounds in one context, warm against cold (DESIGN.md §4.14,
profiles/cut_loop_probe.md) on the bundled G11 (n = 800), the 12 x 10 torus of the golden
instances and the G67-like 100 x 100 torus of instances.CONFIGS (n = 10^4): `--rounds` rounds of
K = `--cuts` (64 on the torus).  Per round:

  * warm: the context of the previous round takes the new cuts in place (Solver.append_cuts with
    carry; its time is reported on its own) and re-solves with Solver.solve_warm;
  * cold: a fresh context of the plain problem takes the same cut list without carry and solves
    from the random start with Solver.solve;
  * for both: ALM inner iterations, ADMM iterations, wall time of the solve, pobj, the certified
    bound and whether its eigen-solve converged.

Every solve gets `--time-limit` seconds (timeSecLimit); one that hits it is marked.  Host clock
around calls that end in a stream synchronise.  Nothing is asserted: whether warm rounds are
faster is what the table is for.

    python scripts/cut_loop_probe.py [--cuts 1024] [--rounds 3] [--instances G11,torus,G67]
                                     [--time-limit 60] [--md out.md] [--json out.json]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
solver = importlib.import_module("ltr-lowrank-sdp_amd.solver")
inst = importlib.import_module("ltr-lowrank-sdp_amd.instances")


def locate(name, directory):
    if name == "torus":
        return os.path.join(ROOT, "tests", "golden", "instances", "mc_torus12x10.dat-s")
    path = os.path.join(ROOT, "data", "bundled", f"{name}.dat-s")
    return path if os.path.exists(path) else inst.config_instance(name, directory)


def solved(sv, warm, limit):
    t0 = time.perf_counter()
    res = sv.solve_warm(timeSecLimit=limit) if warm else sv.solve(timeSecLimit=limit)
    dt = time.perf_counter() - t0
    bound, _, conv = sv.certified_bound()
    # a solve whose ALM phase already meets phase2Tol skips the ADMM phase and reports no ADMM objective
    pobj = res["pobj"] if res["pobj"] < 1e29 else res["alm_pobj"]
    return dict(alm_inner=res["alm_inner"], admm_iter=res["admm_iter"], sec=dt, pobj=pobj, bound=bound,
                converged=conv, status=res["status"])


def probe(name, path, K, rounds, limit, minv):
    sv = solver.Solver(path)
    n = sv.dims[0]
    out = dict(instance=name, n=n, K=K, rounds=[])
    first = solved(sv, False, limit)
    out["rounds"].append(dict(n_cuts=0, n_added=0, carry_ms=0.0, warm=first, cold=first))
    for _ in range(rounds):
        have = sv.cuts()
        slack = sv.cuts_state()[0]
        want = min(K + int((slack < -minv).sum()), 65536)
        cand, _, nv, mv = sv.separate_triangles(want, minv)
        known = {tuple(q) for q in have.tolist()}
        new = np.asarray([q for q in cand.tolist() if tuple(q) not in known][:K], dtype=np.int32).reshape(-1, 4)
        if new.shape[0] == 0:
            break
        t0 = time.perf_counter()
        na = sv.append_cuts(new, carry=True)
        carry_ms = 1e3 * (time.perf_counter() - t0)
        warm = solved(sv, True, limit)
        cold_sv = solver.Solver(path)
        cold_sv.append_cuts(sv.cuts(), carry=False)
        cold = solved(cold_sv, False, limit)
        cold_sv.close()
        out["rounds"].append(dict(n_cuts=int(sv.cuts().shape[0]), n_added=na, n_violated=nv, max_violation=mv,
                                  carry_ms=carry_ms, warm=warm, cold=cold))
        print(f"{name}: {out['rounds'][-1]}", flush=True)
    sv.close()
    return out


def table(results):
    head = ("| instance | n | round | cuts | append + carry ms | inner warm / cold | ADMM warm / cold | s warm / cold | "
            "pobj warm | pobj cold | bound warm | bound cold |\n|---|---|---|---|---|---|---|---|---|---|---|---|\n")
    rows = []
    for r in results:
        for q, rd in enumerate(r["rounds"]):
            w, c = rd["warm"], rd["cold"]
            mark = lambda d: ("" if d["converged"] else " (nc)") + (" (tl)" if d["status"] == 4 else "")
            rows.append(f"| {r['instance']} | {r['n']} | {q} | {rd['n_cuts']} | {rd['carry_ms']:.2f} | "
                        f"{w['alm_inner']} / {c['alm_inner']} | {w['admm_iter']} / {c['admm_iter']} | "
                        f"{w['sec']:.3f} / {c['sec']:.3f} | {w['pobj']:.6f} | {c['pobj']:.6f} | "
                        f"{w['bound']:.4f}{mark(w)} | {c['bound']:.4f}{mark(c)} |")
    return head + "\n".join(rows) + "\n\n(nc): the bound's eigen-solve did not converge; (tl): the solve hit the time limit.\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cuts", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--instances", default="G11,torus,G67")
    ap.add_argument("--time-limit", type=float, default=60.0)
    ap.add_argument("--min-violation", type=float, default=1e-6)
    ap.add_argument("--md")
    ap.add_argument("--json")
    a = ap.parse_args()
    results = []
    with tempfile.TemporaryDirectory() as d:
        for name in a.instances.split(","):
            K = 64 if name == "torus" else a.cuts
            results.append(probe(name, locate(name, d), K, a.rounds, a.time_limit, a.min_violation))
            text = table(results)
            if a.md:      # written after every instance: a long run keeps what it has
                with open(a.md, "w") as f:
                    f.write(text)
            if a.json:
                with open(a.json, "w") as f:
                    json.dump(results, f, indent=1)
    print(text)


if __name__ == "__main__":
    main()

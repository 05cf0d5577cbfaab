#!/usr/bin/env python3
"""Admission check of the layout sweep's cases (tests/layout_util.py, tests/test_gpu_layouts.py).

The sweep's reference is the CPU oracle itself, so a case may only run where the oracle's own
rounding is far below the test's bar.  This script builds oracle/lrsdp_oracle.c twice (-O2, and
-O3 -march=native -ffast-math -ffp-contract=fast: other summation orders, contractions and
reciprocals) and prints, for the candidate lists of tests/layout_util.py:

* inner iterations (K = 3): the largest relative difference between the builds over R, G, A(RR^T)
  and lambda; admitted at <= 1e-11 (the tests' bar is 1e-9);
* operators: the (seed, sign) rule of the inputs -- seed 1000 + r; D negated when the oracle's tau
  is 0; the next seed when it still is -- the two builds' difference of every output and the CG
  counts;
* ADMM sweeps: the builds' difference on U, V, lambda (admitted at <= 1e-8; the bar is 1e-6) and
  the CG counts.

The lists it prints are frozen by hand in tests/layout_util.py.  CPU only.
Run:  python scripts/layout_admit.py [steps|ops|sweeps]"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import layout_util as lu  # noqa: E402
from golden_util import rel_err  # noqa: E402

BUILDS = {"O2": ["-O2"], "fast": ["-O3", "-march=native", "-ffast-math", "-ffp-contract=fast"]}
ADMIT = 1e-11


def build(td):
    libs = {}
    for name, flags in BUILDS.items():
        so = os.path.join(td, f"oracle_{name}.so")
        subprocess.run(["gcc", *flags, "-std=gnu11", "-fPIC", "-shared", "-o", so,
                        os.path.join(ROOT, "oracle", "lrsdp_oracle.c"), "-lm"], check=True)
        libs[name] = lu.bind_oracle(C.CDLL(so))
    return libs


def forced_ranks():
    return sorted({g * e - d for g, e in lu.FORCED for d in (0, 1)})


def steps(libs, td):
    cases = [(n, r) for n, rs in lu.STEP_RANKS.items() for r in rs]
    cases += [("mc_rand300w", r) for r in (33, 34, 227, 229, 230)]   # the refused ones and their neighbours
    cases += [("mc_rand300w", r) for r in forced_ranks() if ("mc_rand300w", r) not in cases]
    cases += [("mc_2blk", 64), ("mc_2blk", 100)]
    worst = 0.0
    for name, r in cases:
        path = lu.instance_path(name, td)
        m = lu.read_m(path)
        nr = sum(n * k for n, k in zip(lu.dims_of(name), lu.cone_ranks(name, r)))
        a = lu.oracle_alm_steps(libs["O2"], path, r, 3, m, nr)
        b = lu.oracle_alm_steps(libs["fast"], path, r, 3, m, nr)
        d = max(rel_err(a[k], b[k]) for k in ("R", "G", "cvs") + (("lam",) if np.linalg.norm(b["lam"]) else ()))
        worst = max(worst, d if d <= ADMIT else 0.0)
        print(f"steps {name:14s} r {r:3d}  builds differ {d:.2e}  {'admit' if d <= ADMIT else 'REFUSE'}")
    print(f"steps: worst admitted {worst:.2e}")


def ops(libs, td):
    negated, seeds = {}, {}
    cases = [(n, r) for n, rs in lu.OP_RANKS.items() for r in rs]
    cases += [("mc_rand300w", r) for r in forced_ranks() if ("mc_rand300w", r) not in cases]
    for name, r in cases:
        path = lu.instance_path(name, td)
        m, dims = lu.read_m(path), lu.dims_of(name)
        seed, sign, o = 1000 + r, 1, None
        while True:
            vec, _ = lu.signed_inputs(m, dims, r, seed, sign)
            o = lu.oracle_kernels(libs["O2"], path, r, vec, m, dims)
            if o["tau"] != 0.0:
                break
            if sign == 1:
                sign = -1
            else:
                seed, sign = seed + 1, 1
        f = lu.oracle_kernels(libs["fast"], path, r, vec, m, dims)
        if sign < 0:
            negated.setdefault(name, []).append(r)
        if seed != 1000 + r:
            seeds[(name, r)] = seed
        d = {k: rel_err(o[k], f[k]) for k in ("q1", "q2", "cvs_rr", "grad", "d_lbfgs2", "d_lbfgs1", "rhs_cg", "u_cg")}
        print(f"ops {name:14s} r {r:3d} seed {seed} sign {sign:+d} tau {o['tau']:.6e} / {f['tau']:.6e} roots "
              f"{int(o['rootnum'])}/{int(f['rootnum'])} cg {int(o['cg_iters'])}/{int(f['cg_iters'])} "
              f"u {d['u_cg']:.1e} rest {max(v for k, v in d.items() if k != 'u_cg'):.1e}")
    print("OP_NEGATED =", negated)
    print("OP_SEED =", seeds)


def sweeps(libs, td):
    refused = [("theta25x3", r) for r in (3, 5, 8, 9, 13, 16, 17, 19, 24, 25)]   # for the record
    for name, r in list(lu.SWEEP_CASES) + refused:
        path = lu.instance_path(name, td)
        m, dims = lu.read_m(path), lu.dims_of(name)
        vec, NR = lu.op_inputs(name, r, m)
        vec[9 * NR + 2 * m + 4] = 1e-9
        a = lu.oracle_admm_sweep(libs["O2"], path, r, vec, m, dims)
        b = lu.oracle_admm_sweep(libs["fast"], path, r, vec, m, dims)
        d = max(rel_err(a[k], b[k]) for k in ("U", "V", "lam"))
        verdict = "admit" if d <= lu.SWEEP_ADMIT else "REFUSE"
        print(f"sweep {name:12s} r {r:3d} builds differ {d:.2e} {verdict} cg total {int(a['cg_total'])}/{int(b['cg_total'])} "
              f"last {a['cg_last'].astype(int).tolist()}/{b['cg_last'].astype(int).tolist()}")


def main():
    what = set(sys.argv[1:]) or {"steps", "ops", "sweeps"}
    with tempfile.TemporaryDirectory() as td:
        libs = build(td)
        if "steps" in what:
            steps(libs, td)
        if "ops" in what:
            ops(libs, td)
        if "sweeps" in what:
            sweeps(libs, td)


if __name__ == "__main__":
    main()

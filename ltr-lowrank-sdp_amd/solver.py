"""Host-side mirror of the reference's solver interface over the C-ABI
(include/lrsdp.h).

* :func:`run_lorads` mirrors benchmark.py's ``run_lorads`` (benchmark.py:219-285):
  same argv contract, runs the MI355X drop-in binary, returns
  ``(success, solve_time_sec, primal_obj)`` from the JSON metrics.
* :class:`Solver` exposes the per-operator entry points (the reference's
  ``lorads_func`` / cone / coefficient vtable slots, lorads_solver.c:1014-1053)
  for tests and benchmarking.

The product path is the HIP library; there is no CPU fallback: importing this
module on a machine without the built ``liblrsdp.so`` raises.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "_build" / "liblrsdp.so"
BIN_PATH = _HERE / "_build" / "LoRADS_v_2_0_1-alpha"

R, D, G, U, V, S0, Y0, S1, Y1 = range(9)
LAMBDA, CVS, Q1, Q2, B = range(5)


class Params(C.Structure):
    _fields_ = [
        ("initRho", C.c_double), ("rhoMax", C.c_double), ("rhoCellingALM", C.c_double),
        ("rhoCellingADMM", C.c_double), ("maxALMIter", C.c_int), ("maxADMMIter", C.c_int),
        ("timesLogRank", C.c_double), ("fixedRank", C.c_int), ("initRank", C.c_int), ("rhoFreq", C.c_int),
        ("rhoFactor", C.c_double), ("ALMRhoFactor", C.c_double), ("rankUpdateFactor", C.c_double),
        ("phase1Tol", C.c_double), ("phase2Tol", C.c_double), ("timeSecLimit", C.c_double),
        ("heuristicFactor", C.c_double), ("lbfgsListLength", C.c_int), ("endTauTol", C.c_double),
        ("endALMSubTol", C.c_double), ("l2Rescaling", C.c_int), ("reoptLevel", C.c_int),
        ("dyrankLevel", C.c_int), ("highAccMode", C.c_int), ("oracleRankNaive", C.c_int),
        ("disableOracle", C.c_int), ("nearStallFactor", C.c_double), ("rankSchedule", C.POINTER(C.c_int)),
        ("rankScheduleLen", C.c_int), ("verbose", C.c_int), ("almInnerBudget", C.c_long), ("skipADMM", C.c_int),
    ]


class Result(C.Structure):
    _fields_ = [
        ("alm_inner", C.c_long), ("alm_outer", C.c_long), ("admm_iter", C.c_long), ("cg_iter", C.c_long),
        ("alm_pobj", C.c_double), ("alm_dobj", C.c_double), ("alm_pinf", C.c_double), ("alm_gap", C.c_double),
        ("alm_rho", C.c_double), ("pobj", C.c_double), ("dobj", C.c_double), ("pinf", C.c_double),
        ("pinf_inf", C.c_double), ("gap", C.c_double), ("rho", C.c_double), ("solve_time", C.c_double),
        ("alm_time", C.c_double), ("admm_time", C.c_double), ("read_time", C.c_double), ("status", C.c_int),
        ("retcode", C.c_int), ("final_rank", C.c_int), ("oracle_rank", C.c_int), ("traj1_len", C.c_int),
        ("traj2_len", C.c_int), ("rho_max", C.c_double), ("dinf", C.c_double), ("dinf_inf", C.c_double),
        ("dinf_2", C.c_double), ("dinf_converged", C.c_int), ("dinf_iters", C.c_int), ("dinf_steps", C.c_long),
        ("dinf_time", C.c_double), ("obj_scale", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None
_HOOK = C.CFUNCTYPE(C.c_long, C.c_void_p, C.c_long)


def load_library(path=None):
    """Load liblrsdp.so (raises if it was not built: no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise RuntimeError(f"HIP library not built: {p} (run __graft_entry__.build())")
    lib = C.CDLL(str(p))
    dp = C.POINTER(C.c_double)
    ip = C.POINTER(C.c_int)
    vp = C.c_void_p
    sig = {
        "lrs_params_default": (None, [C.POINTER(Params)]),
        "lrs_last_error": (C.c_char_p, []),
        "lrs_version": (C.c_char_p, []),
        "lrs_ctx_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "lrs_ctx_destroy": (None, [vp]),
        "lrs_load_sdpa": (C.c_int, [vp, C.c_char_p, dp]),
        "lrs_problem_info": (C.c_int, [vp, ip, ip, ip, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
        "lrs_determine_rank": (C.c_int, [vp, C.POINTER(Params), ip]),
        "lrs_set_rank": (C.c_int, [vp, ip]),
        "lrs_get_rank": (C.c_int, [vp, ip]),
        "lrs_factor_set": (C.c_int, [vp, C.c_int, dp]),
        "lrs_factor_get": (C.c_int, [vp, C.c_int, dp]),
        "lrs_vec_set": (C.c_int, [vp, C.c_int, dp]),
        "lrs_vec_get": (C.c_int, [vp, C.c_int, dp]),
        "lrs_op_q12": (C.c_int, [vp, dp, dp, dp, dp]),
        "lrs_op_constr_rr": (C.c_int, [vp, dp, dp, dp]),
        "lrs_op_grad": (C.c_int, [vp, C.c_double, dp]),
        "lrs_op_line_search": (C.c_int, [vp, C.c_double, dp, ip]),
        "lrs_op_lbfgs": (C.c_int, [vp, C.c_int, C.c_double, C.c_double]),
        "lrs_op_admm_constr": (C.c_int, [vp]),
        "lrs_op_admm_half": (C.c_int, [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, ip, dp]),
        "lrs_op_dual_update": (C.c_int, [vp, C.c_double]),
        "lrs_op_gram": (C.c_int, [vp, C.c_int, C.c_int, dp]),
        "lrs_op_alm_update": (C.c_int, [vp, C.c_double, C.c_double, dp, dp]),
        "lrs_op_adjoint": (C.c_int, [vp, dp, C.c_int, dp, C.c_double, C.c_int]),
        "lrs_op_auv": (C.c_int, [vp, C.c_int, C.c_int, dp, dp]),
        "lrs_op_dimacs": (C.c_int, [vp, C.c_int, dp]),
        "lrs_abi_version": (C.c_int, []),
        "lrs_solve": (C.c_int, [vp, C.POINTER(Params), C.POINTER(Result)]),
        "lrs_trajectory": (C.c_int, [vp, C.c_int, ip, ip, C.c_int]),
        "lrs_write_json": (C.c_int, [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(Result),
                                     C.POINTER(Params)]),
        "lrs_alm_throughput": (C.c_int, [vp, C.POINTER(Params), C.c_long, C.c_long, dp, C.POINTER(C.c_long),
                                         dp, dp]),
        "lrs_set_log_path": (C.c_int, [vp, C.c_char_p]),
        "lrs_set_budget_hook": (C.c_int, [vp, _HOOK, vp]),
        "lrs_sync": (C.c_int, [vp]),
        "lrs_alm_last_step": (C.c_int, [vp, dp, ip]),
        "lrs_time_auut": (C.c_int, [vp, C.c_int, dp]),
        "lrs_profile_stages": (C.c_int, [vp, C.POINTER(Params), C.c_long, dp, C.POINTER(C.c_long)]),
        "lrs_time_stages": (C.c_int, [vp, C.c_int, dp]),
        "lrs_set_kernel_path": (C.c_int, [vp, C.c_int]),
        "lrs_op_dual_infeasibility": (C.c_int, [vp, dp, dp]),
        "lrs_get_kernel_path": (C.c_int, [vp, ip]),
        "lrs_lat_plain_used": (C.c_int, [vp, ip]),
        "lrs_lat_tsum_used": (C.c_int, [vp, ip]),
        "lrs_get_layout": (C.c_int, [vp, C.c_int, ip, ip, ip]),
        "lrs_lp_sweep_info": (C.c_int, [vp, ip, ip, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]),
        "lrs_factor_padding": (C.c_int, [vp, C.c_int, dp]),
        "lrs_wave_tsum_probe": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, dp, dp, dp]),
        "lrs_stage_bytes": (C.c_int, [vp, dp]),
        "lrs_tile_info": (C.c_int, [vp, ip, ip]),
        "lrs_tile_used": (C.c_int, [vp, ip]),
        "lrs_auut_bytes": (C.c_int, [vp, dp]),
        "lrs_time_gram": (C.c_int, [vp, C.c_int, C.c_int, dp, dp]),
        "lrs_mfma_f64_peak": (C.c_int, [vp, dp]),
        "lrs_mfma_f64_probe": (C.c_int, [vp, C.c_int, C.c_int, dp, dp, dp]),
        "lrs_time_dense": (C.c_int, [vp, C.c_int, C.c_int, dp]),
        "lrs_dense_a_info": (C.c_int, [vp, C.c_int, ip, ip, C.POINTER(C.c_long)]),
        "lrs_time_dense_a": (C.c_int, [vp, C.c_int, C.c_int, dp]),
        "lrs_dense_a_plan": (C.c_int, [C.c_char_p, C.c_int, ip, ip, ip, C.c_int]),
        "lrs_rank1_info": (C.c_int, [vp, C.c_int, ip, ip, C.POINTER(C.c_long)]),
        "lrs_rank1_plan": (C.c_int, [C.c_char_p, C.c_int, ip, ip, ip, dp, C.c_int]),
        "lrs_time_rank1": (C.c_int, [vp, C.c_int, C.c_int, dp, dp]),
        "lrs_load_coo": (C.c_int, [vp, C.c_int, C.c_int, ip, dp, C.c_long, ip, ip, ip, ip, dp]),
        "lrs_load_coo_rank1": (C.c_int, [vp, C.c_int, C.c_int, ip, dp, C.c_long, ip, ip, ip, ip, dp, C.c_int, ip, ip,
                                         dp, dp]),
        "lrs_debug_phase_times": (C.c_int, [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
        "lrs_comm_unique_id": (C.c_int, [C.c_char_p]),
        "lrs_shard_rccl": (C.c_int, [vp, C.c_int, C.c_int, C.c_char_p]),
        "lrs_loopback_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "lrs_loopback_destroy": (None, [vp]),
        "lrs_shard_loopback": (C.c_int, [vp, vp, C.c_int]),
        "lrs_shard_info": (C.c_int, [vp, ip, ip, ip, ip, ip]),
        "lrs_shard_comm_ranks": (C.c_int, [vp, ip]),
        "lrs_shard_comm_record": (C.c_int, [vp, C.c_int]),
        "lrs_xwg_fallbacks": (C.c_int, [vp, ip]),
        "lrs_shard_comm_log": (C.c_int, [vp, C.POINTER(C.c_long), C.c_long, C.POINTER(C.c_long)]),
        "lrs_batch_create": (C.c_int, [C.POINTER(vp)]),
        "lrs_batch_destroy": (None, [vp]),
        "lrs_solve_batch": (C.c_int, [vp, C.POINTER(vp), C.c_int, C.POINTER(Params), C.c_int, C.POINTER(Result), ip]),
        "lrs_batch_error": (C.c_char_p, [vp, C.c_int]),
        "lrs_batch_stats": (C.c_int, [vp, C.POINTER(C.c_long), ip, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
        "lrs_batch_round_widths": (C.c_int, [vp, C.POINTER(C.c_long), C.c_int, C.POINTER(C.c_long)]),
        "lrs_batch_admm_stats": (C.c_int, [vp, C.POINTER(C.c_long), ip, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
        "lrs_batch_admm_round_widths": (C.c_int, [vp, C.POINTER(C.c_long), C.c_int, C.POINTER(C.c_long)]),
        "lrs_batch_admm_shape": (C.c_int, [vp, ip, ip]),
        "lrs_op_admm_round": (C.c_int, [vp, C.POINTER(vp), C.c_int, dp, dp, C.c_int]),
        "lrs_op_admm_rhs": (C.c_int, [vp, C.c_int, dp]),
        "lrs_admm_form": (C.c_int, [vp, ip, ip]),
        "lrs_round_dirs": (C.c_int, [C.c_ulonglong, C.c_int, C.c_int, dp]),
        "lrs_round_signs": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, dp, C.c_ulonglong, C.c_int, C.c_int, dp,
                                      C.POINTER(C.c_ulonglong), ip, dp, C.POINTER(C.c_byte), ip]),
        "lrs_separate_triangles": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double, ip, dp, ip,
                                             C.POINTER(C.c_longlong), dp]),
        "lrs_solve_warm": (C.c_int, [vp, C.POINTER(Params), C.POINTER(Result)]),
        "lrs_cuts_append": (C.c_int, [vp, ip, C.c_int, C.c_int, ip]),
        "lrs_cuts_drop": (C.c_int, [vp, C.POINTER(C.c_ubyte), C.c_int, ip]),
        "lrs_cuts_get": (C.c_int, [vp, ip, C.c_int, ip]),
        "lrs_cuts_state": (C.c_int, [vp, C.c_int, dp, dp]),
        "lrs_certified_bound": (C.c_int, [vp, dp, dp, ip]),
        "lrs_sym_eig": (C.c_int, [C.c_int, dp, dp, dp]),
        "lrs_factor_spectrum": (C.c_int, [vp, C.c_int, C.c_double, dp, ip]),
        "lrs_factor_compress": (C.c_int, [vp, C.c_int, ip, C.c_double, C.c_int, ip, dp, dp, dp]),
        "lrs_set_rank_shrink": (C.c_int, [vp, C.c_double, C.c_int]),
        "lrs_compress_timing": (C.c_int, [vp, dp, dp]),
        "lrs_shard_plan": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_long), ip, ip, ip, ip, ip, ip, ip]),
    }
    for name, (res, args) in sig.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if os.environ.get("LRS_LIB"):   # an older build compared side by side (scripts/*_probe.py)
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def default_params(**kw):
    lib = load_library()
    p = Params()
    lib.lrs_params_default(C.byref(p))
    sched = kw.pop("rankSchedule", None)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    if sched:
        arr = (C.c_int * len(sched))(*sched)
        p.rankSchedule = arr
        p.rankScheduleLen = len(sched)
        p._sched_keepalive = arr
    return p


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def comm_unique_id():
    """RCCL unique id (128 bytes) for lrs_shard_rccl; made on rank 0 and broadcast."""
    lib = load_library()
    buf = C.create_string_buffer(128)
    if lib.lrs_comm_unique_id(buf) != 0:
        raise RuntimeError(f"comm_unique_id: {lib.lrs_last_error().decode()}")
    return buf.raw


class RoundError(RuntimeError):
    """A refused Solver.round_signs: `code` is lrs_round_signs' negative return value."""

    def __init__(self, code, msg):
        super().__init__(f"round_signs ({code}): {msg}")
        self.code = code
        self.message = msg


class TriangleError(RuntimeError):
    """A refused Solver.separate_triangles: `code` is lrs_separate_triangles' negative return value."""

    def __init__(self, code, msg):
        super().__init__(f"separate_triangles ({code}): {msg}")
        self.code = code
        self.message = msg


class CutError(RuntimeError):
    """A refused Solver.solve_warm / append_cuts / drop_cuts / cuts_state / certified_bound: `code`
    is the library's negative return value."""

    def __init__(self, what, code, msg):
        super().__init__(f"{what} ({code}): {msg}")
        self.code = code
        self.message = msg


class CompressError(RuntimeError):
    """A refused Solver.spectrum / compress / set_rank_shrink or sym_eig: `code` is the library's
    negative return value."""

    def __init__(self, what, code, msg):
        super().__init__(f"{what} ({code}): {msg}")
        self.code = code
        self.message = msg


def sym_eig(a, vectors=True):
    """Eigenvalues (descending) and eigenvectors of a symmetric matrix on the host (lrs_sym_eig:
    Householder tridiagonalisation, implicit QL): (w, q) with q[:, j] the unit eigenvector of w[j],
    its component of largest magnitude positive; vectors=False returns w alone."""
    lib = load_library()
    a = np.ascontiguousarray(a, dtype=np.float64)
    r = a.shape[0] if a.ndim == 2 and a.shape[0] == a.shape[1] else 0
    w = np.empty(max(1, r))
    q = np.empty((max(1, r), max(1, r))) if vectors else None
    rc = lib.lrs_sym_eig(r, _dptr(a), _dptr(w), _dptr(q) if vectors else None)
    if rc != 0:
        raise CompressError("sym_eig", rc, lib.lrs_last_error().decode())
    return (w, np.ascontiguousarray(q.T)) if vectors else w   # q is column-major in the library


def round_dirs(seed, r, trials):
    """The seeded hyperplane normals of Solver.round_signs as an (r, trials) array (host only:
    lrs_round_dirs, splitmix64 of (seed, trial, column) then Box-Muller)."""
    lib = load_library()
    out = np.empty((int(trials), int(r)))
    if lib.lrs_round_dirs(int(seed), int(r), int(trials), _dptr(out)) != 0:
        raise RuntimeError(f"round_dirs: {lib.lrs_last_error().decode()}")
    return np.ascontiguousarray(out.T)


class LoopbackGroup:
    """One-process loopback transport of a sharded solve (tests): `world` Solvers on one
    GPU, each driven by its own thread, call Solver.shard_loopback(group, rank)."""

    def __init__(self, world):
        self.lib = load_library()
        self.h = C.c_void_p()
        if self.lib.lrs_loopback_create(world, C.byref(self.h)) != 0:
            raise RuntimeError(f"loopback_create: {self.lib.lrs_last_error().decode()}")
        self.world = world

    def close(self):
        if self.h:
            self.lib.lrs_loopback_destroy(self.h)
            self.h = C.c_void_p()


class Solver:
    """One device context with a loaded SDPA problem."""

    def __init__(self, path=None, device=0, coo=None):
        """path: SDPA .dat-s file; or coo: dict from instances.coo_arrays (lrs_load_coo)."""
        self.lib = load_library()
        self.ctx = C.c_void_p()
        self._check(self.lib.lrs_ctx_create(device, C.byref(self.ctx)), "ctx_create")
        t = C.c_double()
        if coo is not None:
            import time as _time
            t0 = _time.perf_counter()
            a = {k: coo[k] for k in ("dims", "b", "con", "blk", "row", "col", "val")}
            ip_ = lambda x: x.ctypes.data_as(C.POINTER(C.c_int))
            dp_ = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
            terms = coo.get("terms")
            if terms:
                # rank-one terms (con, blk, sigma, a), 1-based con / blk: sigma a a^T (lrs_load_coo_rank1)
                tcon = np.ascontiguousarray([tm[0] for tm in terms], dtype=np.int32)
                tblk = np.ascontiguousarray([tm[1] for tm in terms], dtype=np.int32)
                tsig = np.ascontiguousarray([tm[2] for tm in terms], dtype=np.float64)
                for tm in terms:
                    if not 1 <= int(tm[1]) <= len(a["dims"]) or len(tm[3]) != abs(int(a["dims"][int(tm[1]) - 1])):
                        raise ValueError("rank-one term: block out of range or vector length differs from the block's")
                tvec = np.ascontiguousarray(np.concatenate([np.asarray(tm[3], dtype=np.float64) for tm in terms]))
                self._check(self.lib.lrs_load_coo_rank1(self.ctx, int(coo["m"]), len(a["dims"]), ip_(a["dims"]),
                                                        dp_(a["b"]), len(a["con"]), ip_(a["con"]), ip_(a["blk"]),
                                                        ip_(a["row"]), ip_(a["col"]), dp_(a["val"]), len(terms),
                                                        ip_(tcon), ip_(tblk), dp_(tsig), dp_(tvec)), "load_coo_rank1")
            else:
                self._check(self.lib.lrs_load_coo(self.ctx, int(coo["m"]), len(a["dims"]), ip_(a["dims"]), dp_(a["b"]),
                                                  len(a["con"]), ip_(a["con"]), ip_(a["blk"]), ip_(a["row"]),
                                                  ip_(a["col"]), dp_(a["val"])), "load_coo")
            t.value = _time.perf_counter() - t0
        else:
            self._check(self.lib.lrs_load_sdpa(self.ctx, str(path).encode(), C.byref(t)), "load_sdpa")
        self.read_time = t.value
        m, k = C.c_int(), C.c_int()
        self._check(self.lib.lrs_problem_info(self.ctx, C.byref(m), C.byref(k), None, None, None), "info")
        self.m, self.K = m.value, k.value
        dims = (C.c_int * self.K)()
        ns, nz = C.c_long(), C.c_long()
        self._check(self.lib.lrs_problem_info(self.ctx, None, None, dims, C.byref(ns), C.byref(nz)), "info")
        self.dims = list(dims)
        self.nslots, self.nnz = ns.value, nz.value
        self.ranks = None

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {self.lib.lrs_last_error().decode()}")

    def close(self):
        if self.ctx:
            self.lib.lrs_ctx_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- sharded solve (include/lrsdp.h lrs_shard_*): call after loading, before solving
    def shard_rccl(self, world, rank, uid):
        self._check(self.lib.lrs_shard_rccl(self.ctx, world, rank, uid), "shard_rccl")
        self._after_shard()

    def shard_loopback(self, group, rank):
        self._check(self.lib.lrs_shard_loopback(self.ctx, group.h, rank), "shard_loopback")
        self._after_shard()

    def _after_shard(self):
        """The shard's local sizes (every cone: owned + halo rows; the local constraints)."""
        m, k = C.c_int(), C.c_int()
        self._check(self.lib.lrs_problem_info(self.ctx, C.byref(m), C.byref(k), None, None, None), "info")
        dims = (C.c_int * max(1, k.value))()
        self._check(self.lib.lrs_problem_info(self.ctx, C.byref(m), C.byref(k), dims, None, None), "info")
        self.m, self.dims = m.value, list(dims)[:k.value]

    def shard_info(self):
        """(world, rank, first global row, owned rows, halo rows)."""
        v = [C.c_int() for _ in range(5)]
        self._check(self.lib.lrs_shard_info(self.ctx, *[C.byref(x) for x in v]), "shard_info")
        return tuple(x.value for x in v)

    def xwg_fallbacks(self):
        """Inner-loop calls rerun on the multi-launch iteration after a one-workgroup-per-cone
        exchange timed out (include/lrsdp.h lrs_xwg_fallbacks)."""
        n = C.c_int()
        self._check(self.lib.lrs_xwg_fallbacks(self.ctx, C.byref(n)), "xwg_fallbacks")
        return n.value

    def comm_record(self, on=True):
        """Start (clearing the log) or stop recording the transport's operations."""
        self._check(self.lib.lrs_shard_comm_record(self.ctx, 1 if on else 0), "comm_record")

    def comm_log(self):
        """The recorded operations: an (n, 5) int64 array {kind, peer, cone, count, offset}
        (include/lrsdp.h lrs_shard_comm_log)."""
        n = C.c_long()
        self._check(self.lib.lrs_shard_comm_log(self.ctx, None, 0, C.byref(n)), "comm_log")
        out = np.zeros(5 * max(1, n.value), dtype=np.int64)
        self._check(self.lib.lrs_shard_comm_log(self.ctx, out.ctypes.data_as(C.POINTER(C.c_long)), n.value,
                                                C.byref(n)), "comm_log")
        return out[:5 * n.value].reshape(-1, 5)

    def comm_ranks(self):
        """Ranks the shard transport counts itself (RCCL ncclCommCount; 1 unsharded)."""
        n = C.c_int()
        self._check(self.lib.lrs_shard_comm_ranks(self.ctx, C.byref(n)), "shard_comm_ranks")
        return n.value

    # ---- ranks / state
    def determine_rank(self, **kw):
        out = (C.c_int * self.K)()
        self._check(self.lib.lrs_determine_rank(self.ctx, C.byref(default_params(**kw)), out), "determine_rank")
        return list(out)

    def set_rank(self, ranks):
        ranks = list(ranks)
        self._check(self.lib.lrs_set_rank(self.ctx, (C.c_int * self.K)(*ranks)), "set_rank")
        self.ranks = ranks

    def nr(self):
        # the context's current ranks (a solve may have grown them since set_rank): every host
        # buffer handed to the library is sized from them
        self.ranks = self.get_rank()
        return sum(n * r for n, r in zip(self.dims, self.ranks))

    def set_factor(self, which, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.size == self.nr()
        self._check(self.lib.lrs_factor_set(self.ctx, which, _dptr(x)), "factor_set")

    def get_factor(self, which):
        x = np.empty(self.nr())
        self._check(self.lib.lrs_factor_get(self.ctx, which, _dptr(x)), "factor_get")
        return x

    def set_vec(self, which, v):
        v = np.ascontiguousarray(v, dtype=np.float64)
        assert v.size == self.m
        self._check(self.lib.lrs_vec_set(self.ctx, which, _dptr(v)), "vec_set")

    def get_vec(self, which):
        v = np.empty(self.m)
        self._check(self.lib.lrs_vec_get(self.ctx, which, _dptr(v)), "vec_get")
        return v

    # ---- operators
    def q12(self):
        q1, q2 = np.empty(self.m), np.empty(self.m)
        p1, p2 = C.c_double(), C.c_double()
        self._check(self.lib.lrs_op_q12(self.ctx, _dptr(q1), C.byref(p1), _dptr(q2), C.byref(p2)), "q12")
        return q1, p1.value, q2, p2.value

    def constr_rr(self):
        cvs = np.empty(self.m)
        pinf, pobj = C.c_double(), C.c_double()
        self._check(self.lib.lrs_op_constr_rr(self.ctx, _dptr(cvs), C.byref(pinf), C.byref(pobj)), "constr_rr")
        return cvs, pinf.value, pobj.value

    def grad(self, rho):
        lag = C.c_double()
        self._check(self.lib.lrs_op_grad(self.ctx, rho, C.byref(lag)), "grad")
        return self.get_factor(G), lag.value

    def line_search(self, rho):
        tau, rn = C.c_double(), C.c_int()
        self._check(self.lib.lrs_op_line_search(self.ctx, rho, C.byref(tau), C.byref(rn)), "line_search")
        return tau.value, rn.value

    def lbfgs(self, node_num, beta_new, beta_old):
        self._check(self.lib.lrs_op_lbfgs(self.ctx, node_num, beta_new, beta_old), "lbfgs")
        return self.get_factor(D)

    def admm_constr(self):
        """LORADSInitConstrValAll + Sum on (U, V): the state the ADMM half-steps read."""
        self._check(self.lib.lrs_op_admm_constr(self.ctx), "admm_constr")

    def admm_half(self, rho, cg_tol, cg_maxit=800, cone=0, side=0, init=True):
        """One half-step of LORADSUpdateSDPVar for `cone` (side 0: U with V fixed, 1: V with U
        fixed) and the cone's constraint refresh; init=True first recomputes the constraint
        values from (U, V).  Returns (the updated factor, all cones; the cone's RHS; CG its)."""
        if init:
            self.admm_constr()
        it = C.c_int()
        rhs = np.empty(self.dims[cone] * self.get_rank()[cone])
        self._check(self.lib.lrs_op_admm_half(self.ctx, cone, side, rho, cg_tol, cg_maxit, C.byref(it), _dptr(rhs)),
                    "admm_half")
        return self.get_factor(V if side else U), rhs, it.value

    def admm_form(self):
        """(cones whose ADMM half-step is the single-workgroup kernel, whether the whole iteration
        is the one-workgroup form a batch's ADMM meeting combines), at the current ranks."""
        ncg, form = C.c_int(), C.c_int()
        self._check(self.lib.lrs_admm_form(self.ctx, C.byref(ncg), C.byref(form)), "admm_form")
        return ncg.value, bool(form.value)

    def admm_rhs(self, cone=0):
        """The right-hand side that the last half-step of `cone` left (as admm_half's)."""
        rhs = np.empty(self.dims[cone] * self.get_rank()[cone])
        self._check(self.lib.lrs_op_admm_rhs(self.ctx, cone, _dptr(rhs)), "admm_rhs")
        return rhs

    def dual_update(self, rho):
        """LORADSUpdateDualVar: lambda += rho (b - A(X))."""
        self._check(self.lib.lrs_op_dual_update(self.ctx, rho), "dual_update")

    def alm_update(self, rho, tau):
        """setAsNegGrad + ALMupdateVar + constrValSum update + ALMCalGrad + setlbfgsHisTwo
        (lorads_alm.c:1340-1355): returns (||G||^2, beta of the new pair)."""
        lag, beta = C.c_double(), C.c_double()
        self._check(self.lib.lrs_op_alm_update(self.ctx, rho, tau, C.byref(lag), C.byref(beta)), "alm_update")
        return lag.value, beta.value

    def adjoint(self, y, which=R, scale=1.0, with_c=True):
        """scale (with_c C + sum_i y_i A_i) X_which (sdpDataWSum + mul_rk)."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        assert y.size == self.m
        out = np.empty(self.nr())
        self._check(self.lib.lrs_op_adjoint(self.ctx, _dptr(y), which, _dptr(out), scale, 1 if with_c else 0),
                    "adjoint")
        return out

    def auv(self, u=R, v=R):
        """(A(sym(X_u X_v^T)), <C, sym(X_u X_v^T)>) -- coneAUV + objAUV; the state is unchanged."""
        out, cobj = np.empty(self.m), C.c_double()
        self._check(self.lib.lrs_op_auv(self.ctx, u, v, _dptr(out), C.byref(cobj)), "auv")
        return out, cobj.value

    def dimacs(self, admm=False):
        """updateDimacsALM / ADMM with the objectives: {pobj, dobj, pinf, pinf_inf, gap}."""
        o = np.empty(5)
        self._check(self.lib.lrs_op_dimacs(self.ctx, 1 if admm else 0, _dptr(o)), "dimacs")
        return dict(zip(("pobj", "dobj", "pinf", "pinf_inf", "gap"), o.tolist()))

    def gram(self, cone=0, which=R):
        r = self.get_rank()[cone]
        g = np.empty(r * r)
        self._check(self.lib.lrs_op_gram(self.ctx, cone, which, _dptr(g)), "gram")
        return g.reshape(r, r)

    # ---- sign rounding (include/lrsdp.h lrs_round_signs)
    def round_signs(self, trials, seed=0, dirs=None, local_search=True, max_sweeps=50, cone=0, which=R):
        """Round factor `which` of a diagonally constrained cone to `trials` +-1 assignments on
        the device.  dirs: (r, trials) array of hyperplane normals, or None for round_dirs(seed,
        r, trials).  Returns values (trials,), bits (trials // 64, n) uint64 (bit t of bits[w, i]
        set: row i of trial 64 w + t is +1), best_trial, best_value, x (n,) int8 of +-1, sweeps.
        A refusal raises RoundError with the library's negative code."""
        trials = int(trials)
        n = self.dims[cone] if 0 <= cone < len(self.dims) else 1
        nw = max(1, trials // 64)
        d = None
        if dirs is not None:
            r = self.get_rank()[cone]
            d = np.ascontiguousarray(np.asarray(dirs, dtype=np.float64).T)   # column-major r x trials
            if d.shape != (trials, r):
                raise ValueError(f"dirs: expected shape ({r}, {trials})")
        values = np.empty(max(1, trials))
        bits = np.zeros((nw, max(1, n)), dtype=np.uint64)
        x = np.zeros(max(1, n), dtype=np.int8)
        bt, sw, bv = C.c_int(), C.c_int(), C.c_double()
        rc = self.lib.lrs_round_signs(self.ctx, cone, which, trials, _dptr(d) if d is not None else None,
                                      int(seed), 1 if local_search else 0, int(max_sweeps), _dptr(values),
                                      bits.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(bt), C.byref(bv),
                                      x.ctypes.data_as(C.POINTER(C.c_byte)), C.byref(sw))
        if rc != 0:
            raise RoundError(rc, self.lib.lrs_last_error().decode())
        return {"values": values[:trials], "bits": bits, "best_trial": bt.value, "best_value": bv.value, "x": x[:n],
                "sweeps": sw.value}

    # ---- triangle-inequality separation (include/lrsdp.h lrs_separate_triangles)
    def separate_triangles(self, max_cuts, min_violation=0.0, cone=0, which=R):
        """The `max_cuts` most violated triangle inequalities of factor `which` of a diagonally
        constrained cone, found on the device: (cuts (n_cuts, 4) int32 rows {i, j, k, type},
        0-based with i < j < k; violation (n_cuts,), descending, ties by (i, j, k, type);
        n_violated, the exact number with violation > min_violation; max_violation).
        instances.add_triangle_cuts turns the cuts into constraints.  A refusal raises
        TriangleError with the library's negative code."""
        max_cuts = int(max_cuts)
        cap = max(1, min(max_cuts, 65536))
        cuts = np.zeros((cap, 4), dtype=np.int32)
        viol = np.zeros(cap)
        nc, nv, mv = C.c_int(), C.c_longlong(), C.c_double()
        rc = self.lib.lrs_separate_triangles(self.ctx, cone, which, max_cuts, float(min_violation),
                                             cuts.ctypes.data_as(C.POINTER(C.c_int)), _dptr(viol), C.byref(nc),
                                             C.byref(nv), C.byref(mv))
        if rc != 0:
            raise TriangleError(rc, self.lib.lrs_last_error().decode())
        return cuts[:nc.value].copy(), viol[:nc.value].copy(), nv.value, mv.value

    # ---- solves
    def solve(self, **kw):
        p = default_params(**kw)
        res = Result()
        self._check(self.lib.lrs_solve(self.ctx, C.byref(p), C.byref(res)), "solve")
        return res.as_dict()

    # ---- cutting-plane rounds in one context (include/lrsdp.h lrs_solve_warm .. lrs_certified_bound,
    # DESIGN.md §4.14)
    def _cut_check(self, rc, what):
        if rc != 0:
            raise CutError(what, rc, self.lib.lrs_last_error().decode())

    def _refresh_info(self):
        """m, K and dims after the cut list changed the problem."""
        m, k = C.c_int(), C.c_int()
        self._check(self.lib.lrs_problem_info(self.ctx, C.byref(m), C.byref(k), None, None, None), "info")
        dims = (C.c_int * max(1, k.value))()
        ns, nz = C.c_long(), C.c_long()
        self._check(self.lib.lrs_problem_info(self.ctx, None, None, dims, C.byref(ns), C.byref(nz)), "info")
        self.m, self.K, self.dims = m.value, k.value, list(dims)[:k.value]
        self.nslots, self.nnz = ns.value, nz.value
        self.ranks = None

    def solve_warm(self, **kw):
        """lrs_solve's flow started from the context's current R and LAMBDA at its current ranks
        (everything else as a cold start).  A refusal raises CutError."""
        p = default_params(**kw)
        res = Result()
        self._cut_check(self.lib.lrs_solve_warm(self.ctx, C.byref(p), C.byref(res)), "solve_warm")
        return res.as_dict()

    def append_cuts(self, cuts, carry=True):
        """Register triangle inequalities (rows {i, j, k, type} as separate_triangles returns them)
        as constraints with LP slacks, in place; cuts already present are skipped.  carry: keep
        the ranks, the SDP rows of R and LAMBDA, new multipliers 0, LP rows sqrt(max(slack, 0)).
        Returns the number added."""
        a = np.ascontiguousarray(np.asarray(cuts, dtype=np.int32).reshape(-1, 4))
        na = C.c_int()
        self._cut_check(self.lib.lrs_cuts_append(self.ctx, a.ctypes.data_as(C.POINTER(C.c_int)), a.shape[0],
                                                 1 if carry else 0, C.byref(na)), "append_cuts")
        self._refresh_info()
        return na.value

    def drop_cuts(self, mask, carry=True):
        """Remove the cuts whose entry of `mask` (one per registered cut) is true; order kept.
        Returns the number dropped."""
        k = np.ascontiguousarray(np.asarray(mask).astype(bool).astype(np.uint8).ravel())
        nc = C.c_int()
        self._check(self.lib.lrs_cuts_get(self.ctx, None, 0, C.byref(nc)), "cuts_get")
        if nc.value and k.size != nc.value:
            raise ValueError(f"drop_cuts: mask of {k.size} for {nc.value} cuts")
        nd = C.c_int()
        self._cut_check(self.lib.lrs_cuts_drop(self.ctx, k.ctypes.data_as(C.POINTER(C.c_ubyte)), 1 if carry else 0,
                                               C.byref(nd)), "drop_cuts")
        self._refresh_info()
        return nd.value

    def cuts(self):
        """The registered cuts, (n_cuts, 4) int32 in append order."""
        nc = C.c_int()
        self._check(self.lib.lrs_cuts_get(self.ctx, None, 0, C.byref(nc)), "cuts_get")
        out = np.zeros((max(1, nc.value), 4), dtype=np.int32)
        self._check(self.lib.lrs_cuts_get(self.ctx, out.ctypes.data_as(C.POINTER(C.c_int)), nc.value, C.byref(nc)),
                    "cuts_get")
        return out[:nc.value].copy()

    def cuts_state(self, which=R):
        """(slack, lambda) of every registered cut at factor `which`: slack = 1 + sigma . x in the
        separation's arithmetic (bitwise minus its violation), lambda the cut's multiplier."""
        nc = C.c_int()
        self._check(self.lib.lrs_cuts_get(self.ctx, None, 0, C.byref(nc)), "cuts_get")
        slack, lam = np.zeros(max(1, nc.value)), np.zeros(max(1, nc.value))
        self._cut_check(self.lib.lrs_cuts_state(self.ctx, which, _dptr(slack), _dptr(lam)), "cuts_state")
        return slack[:nc.value].copy(), lam[:nc.value].copy()

    def certified_bound(self):
        """(bound, lambda_min, converged): the weak-duality bound of the current multipliers in the
        instance file's units; certified only when converged (else lambda_min is a Ritz value, an
        upper bound of the smallest eigenvalue)."""
        b, lm, cv = C.c_double(), C.c_double(), C.c_int()
        self._cut_check(self.lib.lrs_certified_bound(self.ctx, C.byref(b), C.byref(lm), C.byref(cv)),
                        "certified_bound")
        return b.value, lm.value, bool(cv.value)

    # ---- rank reduction (include/lrsdp.h lrs_factor_spectrum .. lrs_set_rank_shrink)
    def _compress_check(self, rc, what):
        if rc != 0:
            raise CompressError(what, rc, self.lib.lrs_last_error().decode())

    def spectrum(self, which=R, rel_tol=1e-6):
        """(eigs, counts): per cone the eigenvalues of the Gram of factor `which` (R, or U for the
        phase-2 point (U + V) / 2), descending, and how many exceed rel_tol times the largest.
        Changes nothing.  A refusal raises CompressError."""
        ranks = self.get_rank() if self.ctx else []
        tot = max(1, sum(ranks)) if len(ranks) == self.K else 1
        e = np.zeros(tot)
        cnt = (C.c_int * max(1, self.K))()
        self._compress_check(self.lib.lrs_factor_spectrum(self.ctx, which, float(rel_tol), _dptr(e), cnt), "spectrum")
        offs = np.concatenate([[0], np.cumsum(ranks)]).astype(int)
        return [e[offs[k]:offs[k + 1]].copy() for k in range(self.K)], list(cnt)[:self.K]

    def compress(self, ranks=None, rel_tol=1e-6, slack=0, which=R, return_q=False):
        """Rotate factor `which` (R, or U for (U + V) / 2) to the principal axes of its Gram on the
        device and keep the leading columns: per SDP cone ranks[k] when given and > 0, else min(r,
        max(1, count(rel_tol) + slack)).  Afterwards R = U = V = the compressed point at the new
        ranks, LAMBDA kept, everything else as after set_rank.  Returns {"ranks", "eigs" (a list per
        cone, at the old ranks), "lost" (trace dropped per cone)} and, with return_q, "q" (per cone
        the r x r eigenvector matrix, new R = old R @ q[:, :k]).  A refusal raises CompressError."""
        old = self.get_rank() if self.ctx else []
        ok = len(old) == self.K and all(r > 0 for r in old)
        tot = max(1, sum(old)) if ok else 1
        tq = max(1, sum(r * r for r in old)) if ok else 1
        e, lost = np.zeros(tot), np.zeros(max(1, self.K))
        qb = np.zeros(tq) if return_q else None
        out = (C.c_int * max(1, self.K))()
        nr = None
        if ranks is not None:
            ranks = [int(v) for v in ranks]
            if len(ranks) != self.K:
                raise ValueError(f"compress: {len(ranks)} ranks for {self.K} cones")
            nr = (C.c_int * max(1, self.K))(*ranks)
        rc = self.lib.lrs_factor_compress(self.ctx, which, nr, float(rel_tol), int(slack), out, _dptr(e), _dptr(lost),
                                          _dptr(qb) if return_q else None)
        self._compress_check(rc, "compress")
        self._refresh_info()
        offs = np.concatenate([[0], np.cumsum(old)]).astype(int)
        res = {"ranks": list(out)[:self.K], "eigs": [e[offs[k]:offs[k + 1]].copy() for k in range(self.K)],
               "lost": lost[:self.K].tolist()}
        if return_q:
            qo = np.concatenate([[0], np.cumsum([r * r for r in old])]).astype(int)
            res["q"] = [np.ascontiguousarray(qb[qo[k]:qo[k + 1]].reshape(old[k], old[k]).T) for k in range(self.K)]
        return res

    def set_rank_shrink(self, rel_tol, slack=0):
        """solve() / solve_warm() compress the ALM point once before the ADMM phase when the rule
        min(r, max(1, count(rel_tol) + slack)) lowers some cone's rank; rel_tol <= 0 turns it off
        (the default).  Batched solves ignore it."""
        self._compress_check(self.lib.lrs_set_rank_shrink(self.ctx, float(rel_tol), int(slack)), "set_rank_shrink")

    def compress_timing(self):
        """(ms, bytes) of the last compress()'s rotation kernel launches: HIP events, algorithmic bytes."""
        ms, by = C.c_double(), C.c_double()
        self._check(self.lib.lrs_compress_timing(self.ctx, C.byref(ms), C.byref(by)), "compress_timing")
        return ms.value, by.value

    def cut_loop(self, rounds, max_cuts, min_violation=1e-6, drop_slack=None, round_trials=0, compress_tol=None,
                 compress_slack=0, **solve_kw):
        """Cutting-plane rounds in this context: round 0 is the plain solve(); each later round
        separates max_cuts + E inequalities at R (E: registered cuts violated by more than
        min_violation), takes the max_cuts most violated that are not registered yet, stops when
        none is new, optionally drops cuts with slack > drop_slack and lambda >= 0, appends with
        carry and calls solve_warm().  Returns one dict a round: n_cuts, n_added, n_dropped,
        n_violated, max_violation, pobj, dobj, certified_bound, bound_converged, alm_inner,
        admm_iter, time_sec, and best_value when round_trials > 0.  compress_tol (None: off):
        compress(rel_tol=compress_tol, slack=compress_slack) on R before each solve_warm(), so a
        warm round runs at the rank its start needs; each round's dict then carries `rank`, the SDP
        cone's rank at the end of the round."""
        import time as _time
        out = []

        def record(res, t0, n_added, n_dropped, n_violated, max_violation):
            bound, _, conv = self.certified_bound()
            rec = {"n_cuts": int(self.cuts().shape[0]), "n_added": int(n_added), "n_dropped": int(n_dropped),
                   "n_violated": int(n_violated), "max_violation": float(max_violation), "pobj": res["pobj"],
                   "dobj": res["dobj"], "certified_bound": bound, "bound_converged": conv,
                   "alm_inner": res["alm_inner"], "admm_iter": res["admm_iter"]}
            if round_trials > 0:
                rec["best_value"] = self.round_signs(int(round_trials))["best_value"]
            if compress_tol is not None:
                rec["rank"] = int(self.get_rank()[0])
            rec["time_sec"] = _time.perf_counter() - t0
            out.append(rec)

        t0 = _time.perf_counter()
        res = self.solve(**solve_kw)
        _, _, nv, mv = self.separate_triangles(1, min_violation)
        record(res, t0, 0, 0, nv, mv)
        for _ in range(int(rounds)):
            t0 = _time.perf_counter()
            have = self.cuts()
            slack, lam = self.cuts_state()
            extra = int((slack < -min_violation).sum())
            want = min(int(max_cuts) + extra, 65536)
            cand, _, nv, mv = self.separate_triangles(want, min_violation)
            known = {tuple(int(v) for v in q) for q in have}
            new = [q for q in cand if tuple(int(v) for v in q) not in known][:int(max_cuts)]
            if not new:
                break
            nd = 0
            if drop_slack is not None and have.shape[0]:
                nd = self.drop_cuts((slack > drop_slack) & (lam >= 0.0), carry=True)
            na = self.append_cuts(np.asarray(new, dtype=np.int32), carry=True)
            if compress_tol is not None:
                self.compress(rel_tol=compress_tol, slack=compress_slack)
            res = self.solve_warm(**solve_kw)
            record(res, t0, na, nd, nv, mv)
        return out

    def trajectory(self, phase):
        n = self.lib.lrs_trajectory(self.ctx, phase, None, None, 0)
        cur, orc = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))()
        self.lib.lrs_trajectory(self.ctx, phase, cur, orc, n)
        return list(cur)[:n], list(orc)[:n]

    def alm_throughput(self, warmup, steps, auut=False, **kw):
        p = default_params(**kw)
        sec, kms, ims = C.c_double(), C.c_double(), C.c_double()
        done = C.c_long()
        self._check(self.lib.lrs_alm_throughput(self.ctx, C.byref(p), warmup, steps, C.byref(sec), C.byref(done),
                                                C.byref(kms) if auut else None, C.byref(ims)), "alm_throughput")
        return {"seconds": sec.value, "done": done.value, "auut_ms": kms.value if auut else None,
                "iter_ms": ims.value}

    def alm_timed(self, warmup, steps, on_start=None, on_stop=None, **kw):
        """ONE phase-1 solve: `warmup` inner iterations, then exactly `steps` more of the same
        solve (lrs_set_budget_hook), with no solver setup between them.  on_start() runs when
        the warmup iterations are done and the stream is idle, on_stop() after the timed ones
        (the caller's barrier + clock); returns {"done": timed iterations, "seconds": host
        time between the two callbacks (the callbacks' own work excluded), "inner": total}."""
        import time as _time
        kw = dict(kw)
        p = default_params(**kw)
        p.phase1Tol = 1e-300
        p.maxALMIter = 1000000000
        p.skipADMM = 1
        p.timeSecLimit = 1e30
        p.almInnerBudget = max(1, int(warmup))
        st = {"t0": None, "t1": None, "i0": 0, "i1": 0}

        def hook(_user, inner):
            if st["t0"] is None:
                if on_start:
                    on_start()
                st["i0"] = inner
                st["t0"] = _time.perf_counter()
                return inner + int(steps)
            st["t1"] = _time.perf_counter()
            st["i1"] = inner
            if on_stop:
                on_stop()
            return 0

        cb = _HOOK(hook)
        self._check(self.lib.lrs_set_budget_hook(self.ctx, cb, None), "set_budget_hook")
        try:
            res = Result()
            self._check(self.lib.lrs_solve(self.ctx, C.byref(p), C.byref(res)), "solve")
        finally:
            self.lib.lrs_set_budget_hook(self.ctx, _HOOK(), None)
        if st["t0"] is None or st["t1"] is None:
            raise RuntimeError("alm_timed: the phase-1 budget was not reached")
        return {"done": st["i1"] - st["i0"], "seconds": st["t1"] - st["t0"], "inner": res.alm_inner}

    def alm_steps(self, K, **kw):
        """Exactly K ALM inner iterations of a fresh phase-1 solve (budget stop), then
        (tau, ||G||^2, pinf, beta) of trip K, the newest pair's index and the state."""
        kw = dict(kw)
        p = default_params(**kw)
        p.maxALMIter = 1000000000
        p.skipADMM = 1
        p.timeSecLimit = 1e30
        p.almInnerBudget = int(K)
        res = Result()
        self._check(self.lib.lrs_solve(self.ctx, C.byref(p), C.byref(res)), "solve")
        out = (C.c_double * 4)()
        nw = C.c_int()
        self._check(self.lib.lrs_alm_last_step(self.ctx, out, C.byref(nw)), "alm_last_step")
        self.ranks = self.get_rank()
        pair = (S0, Y0) if nw.value == 0 else (S1, Y1)
        return {"inner": res.alm_inner, "tau": out[0], "lag": out[1], "pinf": out[2], "beta": out[3],
                "R": self.get_factor(R), "G": self.get_factor(G), "cvs": self.get_vec(CVS),
                "lam": self.get_vec(LAMBDA), "s": self.get_factor(pair[0]), "y": self.get_factor(pair[1])}

    def alm_last_step(self):
        """(tau, ||G||^2, pinf, beta) of the last completed ALM inner trip of the last solve
        and the newest L-BFGS pair's (s, y) selectors (lrs_alm_last_step)."""
        out = (C.c_double * 4)()
        nw = C.c_int()
        self._check(self.lib.lrs_alm_last_step(self.ctx, out, C.byref(nw)), "alm_last_step")
        return {"tau": out[0], "lag": out[1], "pinf": out[2], "beta": out[3],
                "pair": (S0, Y0) if nw.value == 0 else (S1, Y1)}

    def get_rank(self):
        out = (C.c_int * self.K)()
        self._check(self.lib.lrs_get_rank(self.ctx, out), "get_rank")
        return list(out)

    def sync(self):
        self._check(self.lib.lrs_sync(self.ctx), "sync")

    def profile_stages(self, steps, **kw):
        """Average ms per launch of the four split-iteration stages (HIP events)."""
        p = default_params(**kw)
        ms = (C.c_double * 4)()
        done = C.c_long()
        self._check(self.lib.lrs_profile_stages(self.ctx, C.byref(p), steps, ms, C.byref(done)), "profile_stages")
        return list(ms), done.value

    def auut_bytes(self):
        """Algorithmic bytes of one A(UU^T) (constraint-entry kernel) launch."""
        v = C.c_double()
        self._check(self.lib.lrs_auut_bytes(self.ctx, C.byref(v)), "auut_bytes")
        return v.value

    def tile_info(self):
        """(constraint entries in 2-D tiles, lower pattern in 2-D tiles) for some cone."""
        a, b = C.c_int(), C.c_int()
        self._check(self.lib.lrs_tile_info(self.ctx, C.byref(a), C.byref(b)), "tile_info")
        return a.value, b.value

    def tile_used(self):
        """True when the last ALM iteration ran its stages over the 2-D tiles."""
        v = C.c_int()
        self._check(self.lib.lrs_tile_used(self.ctx, C.byref(v)), "tile_used")
        return bool(v.value)

    def stage_bytes(self):
        """Algorithmic bytes per launch of the stages [A, G, B] at the current ranks."""
        v = (C.c_double * 3)()
        self._check(self.lib.lrs_stage_bytes(self.ctx, v), "stage_bytes")
        return list(v)

    def set_kernel_path(self, path):
        """0 = automatic (latency-regime kernels where they apply), 1 = general row kernels, 5 =
        automatic without lane-group teams (the latency kernels on cones with denser rows too)."""
        self._check(self.lib.lrs_set_kernel_path(self.ctx, int(path)), "set_kernel_path")

    def dual_infeasibility(self):
        """(l1 dual infeasibility, [lambda_min(S_k)] per cone) of the current multipliers."""
        l1 = C.c_double()
        lm = np.zeros(max(1, len(self.dims)))
        self._check(self.lib.lrs_op_dual_infeasibility(self.ctx, C.byref(l1), _dptr(lm)), "dual_infeasibility")
        return l1.value, lm[:len(self.dims)]

    def kernel_path(self):
        """Path of the last enqueued ALM iteration: 0 latency-regime kernels, 1 general, -1 none."""
        v = C.c_int(-1)
        self._check(self.lib.lrs_get_kernel_path(self.ctx, C.byref(v)), "get_kernel_path")
        return v.value

    def lat_plain_used(self):
        """True when the last enqueued ALM iteration ran the latency kernels' PLAIN instantiation."""
        v = C.c_int(0)
        self._check(self.lib.lrs_lat_plain_used(self.ctx, C.byref(v)), "lat_plain_used")
        return bool(v.value)

    def lat_tsum_used(self):
        """True when the last enqueued ALM iteration ran the latency kernels with their wave sums as
        transposed butterflies (LRS_LAT_TSUM=0: one wave sum a value)."""
        v = C.c_int(0)
        self._check(self.lib.lrs_lat_tsum_used(self.ctx, C.byref(v)), "lat_tsum_used")
        return bool(v.value)

    def layout(self, cone=0):
        """(G, E, ld) of `cone`'s factor rows at the current ranks: G lanes a row, E doubles a lane,
        ld = G E >= rank the row pitch on the device (lrs_get_layout)."""
        g, e, ld = C.c_int(), C.c_int(), C.c_int()
        self._check(self.lib.lrs_get_layout(self.ctx, int(cone), C.byref(g), C.byref(e), C.byref(ld)), "get_layout")
        return g.value, e.value, ld.value

    def lp_sweep_info(self):
        """The LP block's ADMM column sweep as the next launch runs it (lrs_lp_sweep_info): lp_cone
        (-1 without an LP block), staged (1 operands in LDS, 0 the global-memory walk, under the
        current LRS_LP_LDS_MAX), lds_bytes the staged variant needs, entries on the device, and
        dense_dropped (entries of columns in >= m/4 constraints, which the column typing drops)."""
        k, st = C.c_int(), C.c_int()
        lds, ne, dd = C.c_long(), C.c_long(), C.c_long()
        self._check(self.lib.lrs_lp_sweep_info(self.ctx, C.byref(k), C.byref(st), C.byref(lds), C.byref(ne),
                                               C.byref(dd)), "lp_sweep_info")
        return SimpleNamespace(lp_cone=k.value, staged=st.value, lds_bytes=lds.value, entries=ne.value,
                               dense_dropped=dd.value)

    def factor_padding(self, which=R):
        """The largest |x| in the padding columns [rank, ld) of factor `which` as stored on the device
        (lrs_factor_padding); 0 unless a kernel wrote past the rank."""
        v = C.c_double()
        self._check(self.lib.lrs_factor_padding(self.ctx, int(which), C.byref(v)), "factor_padding")
        return v.value

    def wave_tsum_probe(self, form, x):
        """The latency kernels' wave sums of x in both forms, (ref, new), each [nv]
        (lrs_wave_tsum_probe).  form 0: x[nv][nblk], the control wave's sum over nblk producer
        blocks' partials.  form 1: x[nv][64 nw], the block tail over nw waves' accumulators."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        nv, cols = x.shape
        n = cols if form == 0 else cols // 64
        if form != 0 and cols != 64 * n:
            raise ValueError("form 1 takes 64 accumulators a wave")
        ref, out = np.empty(nv), np.empty(nv)
        self._check(self.lib.lrs_wave_tsum_probe(self.ctx, int(form), nv, n, _dptr(x), _dptr(ref), _dptr(out)),
                    "wave_tsum_probe")
        return ref, out

    def time_stages(self, reps=200):
        """Per-launch ms of the split-iteration stages [A, G, B] (back-to-back relaunches)."""
        ms = (C.c_double * 3)()
        self._check(self.lib.lrs_time_stages(self.ctx, reps, ms), "time_stages")
        return list(ms)

    def debug_phase_times(self):
        """In-kernel timestamps (diagnostics library only): ([4][16] block-0 phase ticks,
        [4][1024][2] per-block entry/exit ticks) or None from the product library."""
        out = (C.c_ulonglong * 64)()
        blk = (C.c_ulonglong * (4 * 1024 * 2))()
        rc = self.lib.lrs_debug_phase_times(self.ctx, out, blk)
        if rc < 0:
            raise RuntimeError(self.lib.lrs_last_error().decode())
        if rc != 64:
            return None
        ph = [list(out[16 * k:16 * k + 16]) for k in range(4)]
        b = [[(blk[(k * 1024 + i) * 2], blk[(k * 1024 + i) * 2 + 1]) for i in range(1024)] for k in range(4)]
        return ph, b

    def time_gram(self, cone=0, reps=20):
        """(ms per Gram incl. reduction, ms of the MFMA kernel alone) on R of `cone`."""
        ms, kms = C.c_double(), C.c_double()
        self._check(self.lib.lrs_time_gram(self.ctx, cone, reps, C.byref(ms), C.byref(kms)), "time_gram")
        return ms.value, kms.value

    def time_dense(self, cone=0, reps=10):
        """ms per dense-objective product C R of `cone` on the matrix cores (lrs_time_dense)."""
        t = C.c_double()
        self._check(self.lib.lrs_time_dense(self.ctx, cone, reps, C.byref(t)), "time_dense")
        return t.value

    def dense_a_info(self, cone=0):
        """(dense constraint coefficients of `cone`, on the dense-A path, bytes of its stack)
        (lrs_dense_a_info)."""
        n, on, nb = C.c_int(), C.c_int(), C.c_long()
        self._check(self.lib.lrs_dense_a_info(self.ctx, cone, C.byref(n), C.byref(on), C.byref(nb)), "dense_a_info")
        return n.value, bool(on.value), nb.value

    def time_dense_a(self, cone=0, reps=10):
        """ms per k_dcon_ax launch over the stack of `cone` on R (lrs_time_dense_a)."""
        t = C.c_double()
        self._check(self.lib.lrs_time_dense_a(self.ctx, cone, reps, C.byref(t)), "time_dense_a")
        return t.value

    def rank1_info(self, cone=0):
        """(rank-one dense coefficients of `cone`, whether it keeps a factor, the factor's bytes)
        (lrs_rank1_info)."""
        n, on, nb = C.c_int(), C.c_int(), C.c_long()
        self._check(self.lib.lrs_rank1_info(self.ctx, cone, C.byref(n), C.byref(on), C.byref(nb)), "rank1_info")
        return n.value, bool(on.value), nb.value

    def time_rank1(self, cone=0, reps=10):
        """(ms per V^T R launch of `cone`'s rank-one factor, finish included; that launch's
        algorithmic bytes) (lrs_time_rank1)."""
        t, b = C.c_double(), C.c_double()
        self._check(self.lib.lrs_time_rank1(self.ctx, cone, reps, C.byref(t), C.byref(b)), "time_rank1")
        return t.value, b.value

    def mfma_f64_peak(self):
        """Measured FP64 matrix-core TFLOP/s of this device (lrs_mfma_f64_peak)."""
        t = C.c_double()
        self._check(self.lib.lrs_mfma_f64_peak(self.ctx, C.byref(t)), "mfma_f64_peak")
        return t.value

    def mfma_f64_probe(self, waves_per_simd=4, chains=8):
        """(TFLOP/s, shader MHz under the load, cycles per MFMA per SIMD) of the FP64 matrix-core
        probe at the given occupancy (lrs_mfma_f64_probe)."""
        t, f, cy = C.c_double(), C.c_double(), C.c_double()
        self._check(self.lib.lrs_mfma_f64_probe(self.ctx, int(waves_per_simd), int(chains), C.byref(t), C.byref(f),
                                                C.byref(cy)), "mfma_f64_probe")
        return t.value, f.value, cy.value

    def time_auut(self, reps=100):
        ms = C.c_double()
        self._check(self.lib.lrs_time_auut(self.ctx, reps, C.byref(ms)), "time_auut")
        return ms.value


def dense_a_plan(path, cone=0):
    """Host-only classification of the dense constraint coefficients of `cone` (lrs_dense_a_plan;
    no device needed): (0-based constraint indices, whether the cone takes the dense-A path)."""
    lib = load_library()
    n, on = C.c_int(), C.c_int()
    if lib.lrs_dense_a_plan(str(path).encode(), cone, C.byref(n), C.byref(on), None, 0) != 0:
        raise RuntimeError(lib.lrs_last_error().decode())
    cons = np.zeros(max(1, n.value), dtype=np.int32)
    if lib.lrs_dense_a_plan(str(path).encode(), cone, C.byref(n), C.byref(on),
                            cons.ctypes.data_as(C.POINTER(C.c_int)), n.value) != 0:
        raise RuntimeError(lib.lrs_last_error().decode())
    return cons[:n.value].tolist(), bool(on.value)


def rank1_plan(path, cone=0):
    """Host-only detection of the rank-one dense coefficients of `cone` (lrs_rank1_plan; no device
    needed): (0-based constraint indices, their signs sigma, whether the cone keeps a factor)."""
    lib = load_library()
    n, on = C.c_int(), C.c_int()
    if lib.lrs_rank1_plan(str(path).encode(), cone, C.byref(n), C.byref(on), None, None, 0) != 0:
        raise RuntimeError(lib.lrs_last_error().decode())
    cons = np.zeros(max(1, n.value), dtype=np.int32)
    sig = np.zeros(max(1, n.value), dtype=np.float64)
    if lib.lrs_rank1_plan(str(path).encode(), cone, C.byref(n), C.byref(on), cons.ctypes.data_as(C.POINTER(C.c_int)),
                          sig.ctypes.data_as(C.POINTER(C.c_double)), n.value) != 0:
        raise RuntimeError(lib.lrs_last_error().decode())
    return cons[:n.value].tolist(), sig[:n.value].tolist(), bool(on.value)


def shard_plan(path, world, rank):
    """Host-only row partition of a sharded solve (lrs_shard_plan; no device needed)."""
    lib = load_library()
    cnt = (C.c_long * 8)()
    nul = C.POINTER(C.c_int)()
    rc = lib.lrs_shard_plan(str(path).encode(), world, rank, cnt, nul, nul, nul, nul, nul, nul, nul)
    if rc != 0:
        raise RuntimeError(lib.lrs_last_error().decode())
    n, r0, nown, nl, ns, nsh, ml, w = list(cnt)
    arr = {k: np.zeros(max(1, v), dtype=np.int32) for k, v in
           (("bounds", world + 1), ("local_gid", nl), ("send_ptr", world + 1), ("send_gid", ns),
            ("shared_gid", nsh), ("con_gid", ml), ("primary", ml))}
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    rc = lib.lrs_shard_plan(str(path).encode(), world, rank, cnt, ip(arr["bounds"]), ip(arr["local_gid"]),
                            ip(arr["send_ptr"]), ip(arr["send_gid"]), ip(arr["shared_gid"]), ip(arr["con_gid"]),
                            ip(arr["primary"]))
    if rc != 0:
        raise RuntimeError(lib.lrs_last_error().decode())
    out = {k: v[:n_] for (k, v), n_ in zip(arr.items(), (world + 1, nl, world + 1, ns, nsh, ml, ml))}
    out.update(n=n, row0=r0, nown=nown)
    return out


BATCH_MAX = 256   # LRS_BATCH_MAX of include/lrsdp.h


class BatchError(RuntimeError):
    """lrs_solve_batch returned -1: .rc and .errors per instance, .results of those that solved."""

    def __init__(self, msg, rc, errors, results):
        super().__init__(msg)
        self.rc, self.errors, self.results = rc, errors, results


class Batch:
    """A batched solve of many Solvers at once (include/lrsdp.h lrs_solve_batch): the instances on
    the single-workgroup inner loop share launches, one workgroup each."""

    def __init__(self):
        self.lib = load_library()
        self.h = C.c_void_p()
        if self.lib.lrs_batch_create(C.byref(self.h)) != 0:
            raise RuntimeError(f"batch_create: {self.lib.lrs_last_error().decode()}")

    def close(self):
        if self.h:
            self.lib.lrs_batch_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, solvers, params=None, raise_on_failure=True):
        """params: None (defaults), one dict for all, or a list of one dict per solver.  Returns
        the list of result dicts; when an instance failed, raises BatchError (or, with
        raise_on_failure=False, returns None in its place; see .rc / .errors)."""
        n = len(solvers)
        if params is None or isinstance(params, dict):
            plist = [default_params(**(params or {}))]
        else:
            if len(params) != n:
                raise ValueError("one parameter dict per solver")
            plist = [default_params(**(q or {})) for q in params]
        parr = (Params * len(plist))(*plist)
        ctxs = (C.c_void_p * max(n, 1))(*[sv.ctx for sv in solvers])
        res = (Result * max(n, 1))()
        rc = (C.c_int * max(n, 1))()
        for q in range(max(n, 1)):
            rc[q] = -2   # not run (a refused call starts nothing)
        ret = self.lib.lrs_solve_batch(self.h, ctxs, n, parr, len(plist), res, rc)
        self.rc = list(rc)[:n]
        self.errors = [self.lib.lrs_batch_error(self.h, q).decode() if self.rc[q] not in (0, -2) else ""
                       for q in range(n)]
        out = [res[q].as_dict() if self.rc[q] == 0 else None for q in range(n)]
        del plist   # (kept alive until here: rank schedules)
        if ret != 0 and raise_on_failure:
            raise BatchError(self.lib.lrs_last_error().decode(), self.rc, self.errors, out)
        return out

    def stats(self):
        la, se, al = C.c_long(), C.c_long(), C.c_long()
        wi = C.c_int()
        if self.lib.lrs_batch_stats(self.h, C.byref(la), C.byref(wi), C.byref(se), C.byref(al)) != 0:
            raise RuntimeError(self.lib.lrs_last_error().decode())
        return {"launches": la.value, "widest": wi.value, "served": se.value, "alone": al.value}

    def round_widths(self):
        """{width: rounds} of the last solve."""
        h = (C.c_long * (BATCH_MAX + 1))()
        if self.lib.lrs_batch_round_widths(self.h, h, BATCH_MAX + 1, None) != 0:
            raise RuntimeError(self.lib.lrs_last_error().decode())
        return {w: h[w] for w in range(BATCH_MAX + 1) if h[w]}

    def admm_stats(self):
        """The ADMM meeting's counters of the last solve: combined launches, the widest round in
        members, iterations served by rounds, iterations members ran alone; plus the most kernel
        variants in one round and the most blocks in one half-step launch."""
        la, se, al = C.c_long(), C.c_long(), C.c_long()
        wi, va, bl = C.c_int(), C.c_int(), C.c_int()
        if self.lib.lrs_batch_admm_stats(self.h, C.byref(la), C.byref(wi), C.byref(se), C.byref(al)) != 0:
            raise RuntimeError(self.lib.lrs_last_error().decode())
        if self.lib.lrs_batch_admm_shape(self.h, C.byref(va), C.byref(bl)) != 0:
            raise RuntimeError(self.lib.lrs_last_error().decode())
        return {"launches": la.value, "widest": wi.value, "served": se.value, "alone": al.value,
                "variants": va.value, "blocks": bl.value}

    def admm_round(self, solvers, rho, cg_tol, cg_maxit=800):
        """One ADMM iteration's shared launches for `solvers` (each after admm_constr): both sides'
        half-steps of every cone, then the evaluation (lrs_op_admm_round).  rho, cg_tol: one a solver."""
        n = len(solvers)
        ctxs = (C.c_void_p * n)(*[sv.ctx for sv in solvers])
        r = (C.c_double * n)(*[float(x) for x in rho])
        t = (C.c_double * n)(*[float(x) for x in cg_tol])
        if self.lib.lrs_op_admm_round(self.h, ctxs, n, r, t, cg_maxit) != 0:
            raise RuntimeError(f"admm_round: {self.lib.lrs_last_error().decode()}")

    def admm_round_widths(self):
        """{members: rounds} of the last solve's ADMM meeting."""
        h = (C.c_long * (BATCH_MAX + 1))()
        if self.lib.lrs_batch_admm_round_widths(self.h, h, BATCH_MAX + 1, None) != 0:
            raise RuntimeError(self.lib.lrs_last_error().decode())
        return {w: h[w] for w in range(BATCH_MAX + 1) if h[w]}


_batch = None


def _default_batch():
    global _batch
    if _batch is None:
        _batch = Batch()
    return _batch


def solve_batch(solvers, params=None, **kw):
    """Solve every Solver of the list at once (Batch.solve on the module's own batch object)."""
    return _default_batch().solve(solvers, params, **kw)


def batch_stats():
    """Counters of the last solve_batch (launches, widest, served, alone)."""
    return _default_batch().stats()


def run_lorads_batch(jobs, params, near_stall_factor=0.7, timeout=3600, device=0):
    """run_lorads for many instances in ONE process of the MI355X binary (--batch): jobs is a
    list of (instance_path, json_output_path) or (instance_path, json_output_path, fixed_rank,
    rank_schedule_path); params as for run_lorads, shared.  Returns run_lorads' triple per job."""
    if not BIN_PATH.exists():
        raise RuntimeError(f"binary not built: {BIN_PATH}")
    jobs = [tuple(j) + (None,) * (4 - len(j)) for j in jobs]
    lines = []
    for inst, js, fixed_rank, sched in jobs:
        if fixed_rank is not None and sched is not None:
            raise ValueError("fixed_rank and rank_schedule_path are mutually exclusive")
        Path(js).parent.mkdir(parents=True, exist_ok=True)
        Path(js).unlink(missing_ok=True)   # an earlier run's file is no result of this one
        line =[str(inst), str(js)]
        if sched is not None:
            line += ["--rankSchedule", str(sched), "--nearStallFactor", str(near_stall_factor)]
        elif fixed_rank is not None:
            line += ["--fixedRank", str(fixed_rank)]
        if any(any(ch.isspace() for ch in tok) for tok in line):
            raise ValueError("a batch manifest separates fields by blanks: no blanks in paths")
        lines.append(" ".join(line))
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".batch", delete=False) as f:
        f.write("\n".join(lines) + "\n")
        manifest = f.name
    cmd = [str(BIN_PATH), "--batch", manifest]
    for k, v in params.items():
        cmd += [f"--{k}", str(v)]
    cmd += ["--disableOracle", "--device", str(device)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            print(f"  [error] lorads --batch: {r.stderr[:400]}")
    except subprocess.TimeoutExpired:
        print("  [error] lorads --batch timed out")
    finally:
        os.unlink(manifest)
    out = []
    for inst, js, _fr, _sc in jobs:
        try:
            with open(js) as f:
                m = json.load(f)
            m = m.get("final_metrics", m.get("metrics", {}))
            out.append((True, m.get("solve_time_sec"), m.get("primal_obj", m.get("primal_objective"))))
        except Exception:
            out.append((False, None, None))
    return out


def run_lorads(instance_path, json_output_path, params, fixed_rank=None, rank_schedule_path=None,
               near_stall_factor=0.7, timeout=3600, device=0, round_trials=None):
    """Same contract as benchmark.py:219-285, on the MI355X binary.  round_trials (a multiple of
    64): passed through as --roundTrials, the JSON then carries a "rounding" object."""
    if not BIN_PATH.exists():
        raise RuntimeError(f"binary not built: {BIN_PATH}")
    json_output_path = Path(json_output_path)
    json_output_path.parent.mkdir(parents=True, exist_ok=True)
    cmd = [str(BIN_PATH), str(instance_path)]
    for k, v in params.items():
        cmd += [f"--{k}", str(v)]
    cmd += ["--jsonfile", str(json_output_path), "--disableOracle", "--device", str(device)]
    if fixed_rank is not None and rank_schedule_path is not None:
        raise ValueError("fixed_rank and rank_schedule_path are mutually exclusive")
    if rank_schedule_path is not None:
        cmd += ["--rankSchedule", str(rank_schedule_path), "--nearStallFactor", str(near_stall_factor)]
    elif fixed_rank is not None:
        cmd += ["--fixedRank", str(fixed_rank)]
    if round_trials:
        cmd += ["--roundTrials", str(int(round_trials))]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            print(f"  [error] lorads failed: {r.stderr[:200]}")
            return False, None, None
        if not json_output_path.exists():
            return False, None, None
        with open(json_output_path) as f:
            out = json.load(f)
        # same key fallbacks as benchmark.py:270-274
        m = out.get("final_metrics", out.get("metrics", {}))
        return True, m.get("solve_time_sec"), m.get("primal_obj", m.get("primal_objective"))
    except subprocess.TimeoutExpired:
        print("  [error] lorads timed out")
        return False, None, None
    except Exception as e:   # benchmark.py:283-285
        print(f"  [error] unexpected error: {e}")
        return False, None, None

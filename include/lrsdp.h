/*
 * lrsdp.h -- C-ABI of the MI355X-native low-rank SDP inner solver (liblrsdp.so).
 *
 * This is the in-process boundary that replaces the reference's operator
 * vtables on the hot path:
 *   - algorithm slots  lorads_func        (lorads/src/src_semi/data/def_lorads_solver.h:169-187,
 *                                          bound in data/lorads_solver.c:1014-1053)
 *   - cone slots       lorads_sdp_cone    (data/def_lorads_sdp_conic.h:100-124,
 *                                          bound in data/lorads_sdp_conic.c:974-1029)
 *   - coefficient slots sdp_coeff         (data/def_lorads_sdp_data.h:66-85)
 *   - CG callback      Mvec               (linalg/def_lorads_cgs.h:71-72, linalg/lorads_cgs.c:107)
 * The process boundary (the LoRADS CLI that benchmark.py calls,
 * benchmark.py:240-262 / src_semi/main.c:256) is the `LoRADS_v_2_0_1-alpha`
 * binary built on top of this library.
 *
 * Conventions: every function returns 0 on success and a negative code on
 * failure (message via lrs_last_error()); no function calls exit().  A NULL
 * context, a context with no problem loaded (or, for the operators, no ranks
 * set) and a NULL required pointer are failures of that kind, never a crash.  All
 * arrays crossing the boundary are host memory, column-major n x r per cone
 * (the reference layout, lorads_alg_common.c:62-68), cones concatenated in
 * cone order.  Device memory is owned by the context.
 */
#ifndef LRSDP_H
#define LRSDP_H
/* ABI revision, also in lrs_version()'s string.  2: lrs_op_admm_half takes (cone, side) and
 * refreshes the cone's constraint values itself (was: the whole sweep's first half-step);
 * lrs_op_alm_update, lrs_op_adjoint, lrs_op_auv and lrs_op_dimacs added.
 * 3: lrs_solve_warm, lrs_cuts_append / _drop / _get / _state and lrs_certified_bound added.
 * 4: lrs_sym_eig, lrs_factor_spectrum, lrs_factor_compress, lrs_set_rank_shrink and
 * lrs_compress_timing added (lrs_params and lrs_result unchanged).
 * Read-only diagnostic getters (lrs_get_kernel_path, lrs_lat_plain_used, lrs_lat_tsum_used,
 * lrs_get_layout, lrs_factor_padding, ...) are additive and leave the revision as it is: it moves
 * when a signature or a struct changes or a family of operations is added. */
#define LRSDP_ABI_VERSION 4
#ifdef __cplusplus
extern "C" {
#endif

typedef struct lrs_ctx lrs_ctx;
typedef struct lrs_loopback lrs_loopback;

/* LoRADS flags (main.c:56-86 defaults, main.c:125-154 names) + the three flags
 * benchmark.py passes that the reference never implemented. */
typedef struct {
    double initRho, rhoMax, rhoCellingALM, rhoCellingADMM;
    int maxALMIter, maxADMMIter;
    double timesLogRank;
    int fixedRank, initRank, rhoFreq;
    double rhoFactor, ALMRhoFactor, rankUpdateFactor, phase1Tol, phase2Tol, timeSecLimit, heuristicFactor;
    int lbfgsListLength;
    double endTauTol, endALMSubTol;
    int l2Rescaling, reoptLevel, dyrankLevel, highAccMode, oracleRankNaive;
    /* additions (INTEGRATION.md "rank-schedule hook") */
    int disableOracle;
    double nearStallFactor;
    const int *rankSchedule;
    int rankScheduleLen;
    int verbose;          /* print the LoRADS-format iteration log to stdout */
    long almInnerBudget;  /* >0: stop phase 1 after this many inner iterations (benchmarking) */
    int skipADMM;         /* 1: phase 1 only */
} lrs_params;

typedef struct {
    long alm_inner, alm_outer, admm_iter, cg_iter;
    double alm_pobj, alm_dobj, alm_pinf, alm_gap, alm_rho;
    double pobj, dobj, pinf, pinf_inf, gap, rho;   /* admm_state after main.c:519-525 */
    double solve_time, alm_time, admm_time, read_time;
    int status;          /* lorads_status: 0 unknown, 1 primal-dual optimal, 2 primal optimal, 3 maxiter, 4 time limit */
    int retcode;         /* RET_CODE_* of phase 1 */
    int final_rank, oracle_rank;
    int traj1_len, traj2_len;
    double rho_max;      /* params.rhoMax after LORADS_ALMtoADMM (written to the JSON) */
    double dinf, dinf_inf, dinf_2;   /* dual infeasibility l_1 / l_inf / l_2 (main.c:515-521); -1 if not evaluated */
    int dinf_converged;  /* 1: every cone's eigen-solve met its test (ARPACK's tol 1e-2 relative Ritz estimate,
                            or an absolute one that pins the l_1 value to 1e-3 phase2Tol); 0: the 600 update
                            iterations ran out (dinf is then a lower bound and status 1 is withheld); -1: not
                            evaluated */
    int dinf_iters;      /* thick-restart update iterations (dsaupd's iparam(3) count) over cones and calls */
    long dinf_steps;     /* Lanczos steps (matrix-vector products) over cones and calls */
    double dinf_time;    /* seconds in the dual-infeasibility eigen-solves (inside solve_time, as main.c:515-521) */
    double obj_scale;    /* scaleObjHis at the end (the reopt rounds' objScale_dualvar factors; 1 without reopt) */
} lrs_result;

/* factor / vector selectors */
enum { LRS_R = 0, LRS_D = 1, LRS_G = 2, LRS_U = 3, LRS_V = 4, LRS_S0 = 5, LRS_Y0 = 6, LRS_S1 = 7, LRS_Y1 = 8 };
enum { LRS_LAMBDA = 0, LRS_CVS = 1, LRS_Q1 = 2, LRS_Q2 = 3, LRS_B = 4 };

void lrs_params_default(lrs_params *p);
const char *lrs_last_error(void);
const char *lrs_version(void);
int lrs_abi_version(void);   /* LRSDP_ABI_VERSION of the library */

int lrs_ctx_create(int device, lrs_ctx **out);
void lrs_ctx_destroy(lrs_ctx *ctx);

/* SDPA .dat-s reader + presolve + upload (replaces LReadSDPA io/lorads_file_io.c:59,
 * LORADSPreprocess data/lorads_solver.c:278, AConePresolveData data/lorads_sdp_conic.c:1185).
 * read_seconds may be NULL. */
int lrs_load_sdpa(lrs_ctx *ctx, const char *path, double *read_seconds);
int lrs_problem_info(lrs_ctx *ctx, int *m, int *ncones, int *dims, long *nslots, long *nnz_constraints);

/* ranks: LORADSDetermineRank (data/lorads_solver.c:406) given flags; or explicit. */
int lrs_determine_rank(lrs_ctx *ctx, const lrs_params *p, int *ranks_out);
int lrs_set_rank(lrs_ctx *ctx, const int *ranks);
int lrs_get_rank(lrs_ctx *ctx, int *ranks);

int lrs_factor_set(lrs_ctx *ctx, int which, const double *colmajor);
int lrs_factor_get(lrs_ctx *ctx, int which, double *colmajor);
int lrs_vec_set(lrs_ctx *ctx, int which, const double *v);
int lrs_vec_get(lrs_ctx *ctx, int which, double *v);

/* ---- operators (one device pass each; scalars returned through pointers) ---- */
/* ALMCalq12p12 (lorads_alm.c:714): q1 = 2A(sym RD^T), p1 = 2<C,sym RD^T>, q2 = A(DD^T), p2 = <C,DD^T> */
int lrs_op_q12(lrs_ctx *ctx, double *q1, double *p1, double *q2, double *p2);
/* primalInfeasibility (lorads_alg_common.c:386) on R: CVS <- A(RR^T); pinf; and <C,RR^T> */
int lrs_op_constr_rr(lrs_ctx *ctx, double *cvs, double *pinf, double *pobj);
/* ALMCalGrad (lorads_alm.c:74) from LAMBDA, CVS at rho: G <- 2(C + A^*(M1))R */
int lrs_op_grad(lrs_ctx *ctx, double rho, double *lag_norm_sq);
/* ALMLineSearch (lorads_alm.c:266) on the state left by lrs_op_q12 with q0 = b - CVS */
int lrs_op_line_search(lrs_ctx *ctx, double rho, double *tau, int *root_num);
/* LBFGSDirection + LBFGSDirectionUseGrad (lorads_alm.c:468-505, :607-627) from G and
 * the ring (S0,Y0 = newest pair with beta_new; S1,Y1 = older pair with beta_old),
 * node_num in {0,1,2}; result in D. */
int lrs_op_lbfgs(lrs_ctx *ctx, int node_num, double beta_new, double beta_old);
/* LORADSInitConstrValAll + LORADSInitConstrValSum (lorads_alg_common.c:104-229) on (U, V):
 * the per-cone A_k(sym UV^T) and their sum CVS that the ADMM half-steps read and update. */
int lrs_op_admm_constr(lrs_ctx *ctx);
/* One ADMM half-step of LORADSUpdateSDPVar (lorads_alg_common.c:298-326) for cone `cone`:
 * LORADSUpdateSDPVarOne (lorads_admm.c:564-616) solving side 0 = U with V fixed or side 1 =
 * V with U fixed (RHS -(S Y - rho Y)/rho with S = C + A*(rho (CVS - A_k(UV^T) - b) - LAMBDA),
 * CG at cg_tol / cg_maxit, warm-started from the current factor), then the cone's
 * constraint-value refresh (CVS -= A_k, A_k <- A_k(sym UV^T), CVS += A_k).  Calling it for
 * (0, 0), (0, 1), (1, 0), (1, 1), ... after lrs_op_admm_constr is the reference's sweep.
 * cg_iters (may be NULL): this solve's CG iterations; rhs (may be NULL): the cone's
 * right-hand side, column-major n_k x r_k. */
int lrs_op_admm_half(lrs_ctx *ctx, int cone, int side, double rho, double cg_tol, int cg_maxit, int *cg_iters,
                     double *rhs);
/* LP blocks (LORADSSetLpCone, data/lorads_lp_conic.c:347; the *LP slots of lorads_func bound in
 * LORADSInitFuncSet, data/lorads_solver.c:1014-1053): a problem whose last SDPA block has negative
 * size -k carries its k LP columns (x_j = r_j^2) as one more cone, the LAST one, of k rows at rank 1
 * (lrs_get_rank reports 1 for it; lrs_set_rank refuses another rank).  Factors therefore hold the
 * LP values after the SDP cones' (the reference's rLp / uLp / vLp), and every operator above acts on
 * it as on an SDP cone with a diagonal pattern -- which is the LP algebra.  Two exceptions follow
 * the reference: lrs_op_admm_half(ctx, lp_cone, 0, ...) runs the LP block's whole ADMM update, the
 * closed-form column sweep of LORADSUpdateSDPLPVar (u_j then v_j per column, lorads_admm.c:759-792;
 * side 1 is refused, cg_iters = 0, rhs untouched), and lrs_op_dual_infeasibility's LP term is
 * sum_j |min(c_j - sum_i lambda_i a_ij, 0)| (lam_min[lp_cone] = the smallest such value).  The
 * oracle rank, AUG_RANK and the reported ranks cover the SDP cones only.  Sharded contexts refuse
 * LP blocks. */
/* LORADSUpdateDualVar (lorads_alg_common.c:511-524): LAMBDA += rho (b - CVS). */
int lrs_op_dual_update(lrs_ctx *ctx, double rho);
/* The second half of one ALM inner trip after the line search (lorads_alm.c:1340-1355):
 * setAsNegGrad (:780-801), ALMupdateVar R += tau D (:804-833), CVS += tau q1 + tau^2 q2 with the
 * q1, q2 of the last lrs_op_q12 (:1349-1352), ALMCalGrad at rho (:74-87: G <- 2(C + A^*(M1))R,
 * lag_norm_sq = ||G||^2) and setlbfgsHisTwo (:842-863: s = tau D, y = G_new - G_old, beta =
 * 1/<y,s>).  The new pair lands in (LRS_S0, LRS_Y0) and the previous newest moves to (LRS_S1,
 * LRS_Y1), the roles lrs_op_lbfgs reads, so a caller steps the reference's loop with
 * lrs_op_lbfgs -> lrs_op_q12 -> lrs_op_line_search -> lrs_op_alm_update -> lrs_op_dimacs
 * (updateDimacsALM).  lag_norm_sq, beta may be NULL.  Unsharded contexts. */
int lrs_op_alm_update(lrs_ctx *ctx, double rho, double tau, double *lag_norm_sq, double *beta);
/* sdpDataWSum + mul_rk (data/def_lorads_sdp_data.h:66-85) over every cone: out = scale (with_C C +
 * sum_i y[i] A_i) X, X the factor `which` (LRS_R, LRS_U, ...), y[m] host, out column-major like
 * lrs_factor_get.  Unsharded contexts. */
int lrs_op_adjoint(lrs_ctx *ctx, const double *y, int which, double *out, double scale, int with_C);
/*   lrs_op_adjoint works in the solver's scratch: the constraint weights (the M1 buffer), the slot
 *   values S, and the X / CG-Q work factors are overwritten.  No operator reads those across
 *   calls -- lrs_op_grad, lrs_op_admm_half and the fused loops form M1 and S afresh -- so the
 *   iterate (R, U, V, D, G, the L-BFGS pairs), LAMBDA and CVS are unchanged by it. */
/* coneAUV + objAUV (data/def_lorads_sdp_conic.h:106-111) summed over the cones: out_m[i] =
 * <A_i, sym(X_u X_v^T)> (u == v: X_u X_u^T), cobj = <C, sym(X_u X_v^T)> before the division by
 * the reopt objective scale.  Leaves the solver state (CVS) unchanged.  out_m, cobj may be NULL.
 * Unsharded contexts. */
int lrs_op_auv(lrs_ctx *ctx, int u, int v, double *out_m, double *cobj);
/* LORADSUpdateDimacsErrorALM (admm = 0, on R) / LORADSUpdateDimacsErrorADMM (admm = 1: R = (U +
 * V)/2 first) (lorads_alg/lorads_alg_common.c:424-428, :454-462) with the objectives they read
 * (LORADSCalObjRR_ALM lorads_alm.c:1488, LORADSCalObjUV_ADMM, LORADSCalDualObj
 * lorads_alg_common.c:531): CVS <- A(R R^T); out5 = {pObj, dObj, l_1 primal infeasibility, l_inf
 * primal infeasibility, |pObj - dObj| / (1 + |pObj| + |dObj|)}. */
int lrs_op_dimacs(lrs_ctx *ctx, int admm, double *out5);
/* Gram R^T R of cone k (r x r, row-major) */
int lrs_op_gram(lrs_ctx *ctx, int cone, int which, double *gram);
/* Dual infeasibility of the current multipliers (calculate_dual_infeasibility_solver,
 * data/lorads_solver.c:1396-1426): l1 = sum_k |min(lambda_min(S_k), 0)| / scaleObjHis /
 * (||C||_1 + 1) with S = C - sum_i lambda_i A_i; lam_min[k] per cone (may be NULL).  The
 * reference's ARPACK dsaupd "SA" (ncv 40, tol 1e-2, data/lorads_sdp_conic.c:1636-1699) is
 * replaced by a device thick-restart Lanczos with dsaupd's semantics: a basis of 40 vectors,
 * 20 Ritz vectors kept per restart, two-pass classical Gram-Schmidt, convergence when the
 * Ritz residual is <= tol * max(eps^(2/3), |theta|), at most 600 restarts. */
int lrs_op_dual_infeasibility(lrs_ctx *ctx, double *l1, double *lam_min);

/* ---- whole solves ---- */
/* main.c:380-610 flow: ALM phase, ADMM phase, reoptLevel 1/2 rounds (all on the device), dual
 * infeasibility (skipped after a time-limit exit, as main.c:505-510 jumps to END_SOLVING). */
int lrs_solve(lrs_ctx *ctx, const lrs_params *p, lrs_result *res);
/* ---- Batched solves: many small instances at once.  No reference counterpart
 * (the reference's dataset loop runs one process per instance, dataset/run_lorads.sh:85-114).
 * Every instance whose ALM inner loop is the single-workgroup launch (one
 * workgroup) stops launching on its own: the members currently in that phase meet, and one
 * launch per kernel instantiation runs all of them, one block each -- each block computes bit for
 * bit what the instance's own launch computes.  Every other instance (LP blocks, dense or rank-one
 * coefficients, lbfgsListLength != 2, multi-launch kernel paths, one workgroup per cone) runs that
 * phase unchanged on the context's own stream.
 * The ADMM phase has a second, independent meeting: a member inside that phase (the first pass or a
 * reoptimisation's) whose iteration is wholly the one-workgroup form -- every cone on the
 * single-workgroup half-step with one kernel variant, no constraint across cones, the one-launch
 * evaluation; no LP block, no dense or rank-one constraint matrices -- files its iteration and
 * parks; one round runs the parked members' side-0 half-steps, their side-1 half-steps and their
 * evaluations in shared launches, a block a cone, each bit for bit the member's own launch.  A
 * member in one phase never waits for members in the other.  The dual update, the rank oracle's
 * Gram, the first evaluation of a phase, every member that does not qualify and the dual
 * infeasibility stay on the context's own stream.  LRS_BATCH_ADMM=0 in the environment (read at
 * each lrs_solve_batch) keeps every member's ADMM phase on its own stream.
 * lrs_solve_batch: n contexts (distinct, same device, unsharded, each with a problem loaded;
 * n <= LRS_BATCH_MAX), params[n] or one shared set (nparams = 1 or n), res[n], rc[n]: each
 * instance's own return code and, on failure, its message through lrs_batch_error(b, i).  Returns
 * 0 when every instance returned 0, else -1 (lrs_last_error() names the first); one failing
 * instance does not stop the others, and the batch object stays usable.  A refused call (a
 * duplicate, sharded, unloaded or null context, another device, n out of range) starts nothing.
 * Each instance runs on a host thread of the call's own.  params' verbose is off inside a batch
 * (one stdout); lrs_set_log_path still receives each instance's log.  lrs_result's times are wall
 * clock inside the batch: they include the time an instance spent parked waiting for the others
 * of its round.  Afterwards every context is as after lrs_solve (lrs_trajectory, lrs_write_json,
 * lrs_factor_get, ...).
 * lrs_batch_stats, of the last lrs_solve_batch (each may be NULL): combined launches; the widest
 * round (blocks launched together, over the round's concurrent launches); members' inner-loop
 * calls served by combined launches; single-workgroup inner-loop calls that launched alone (the
 * one-workgroup-per-cone members').
 * lrs_batch_round_widths: out[w] (w < cap) = rounds of the last call that ran w blocks; *rounds
 * their number (each may be NULL).  Both count the ALM meeting only.
 * lrs_batch_admm_stats, the ADMM meeting's of the last lrs_solve_batch (each may be NULL): combined
 * ADMM launches; the widest round in members; ADMM iterations served by rounds; ADMM iterations
 * that members ran on their own stream.  lrs_batch_admm_round_widths: as lrs_batch_round_widths,
 * w in members.  lrs_batch_admm_shape: the most kernel variants of the half-step launched in one
 * round, and the most blocks (cones) in one half-step launch. */
#define LRS_BATCH_MAX 256
typedef struct lrs_batch lrs_batch;
int lrs_batch_create(lrs_batch **out);
void lrs_batch_destroy(lrs_batch *b);
int lrs_solve_batch(lrs_batch *b, lrs_ctx **ctxs, int n, const lrs_params *params, int nparams,
                    lrs_result *res, int *rc);
const char *lrs_batch_error(lrs_batch *b, int i);
int lrs_batch_stats(lrs_batch *b, long *launches, int *widest, long *served, long *alone);
int lrs_batch_round_widths(lrs_batch *b, long *out, int cap, long *rounds);
int lrs_batch_admm_stats(lrs_batch *b, long *launches, int *widest, long *served, long *alone);
int lrs_batch_admm_round_widths(lrs_batch *b, long *out, int cap, long *rounds);
int lrs_batch_admm_shape(lrs_batch *b, int *variants, int *blocks);
/* Operator-level access to one ADMM round (tests, as lrs_op_admm_half is to one half-step): for n
 * contexts with solver state, each after lrs_op_admm_constr and each qualifying for the ADMM
 * meeting (else refused), the shared launches of one iteration -- side 0 of every cone, side 1 of
 * every cone, the evaluation (R = (U + V) / 2, CVS = A(R R^T)) -- at rho[i], cg_tol[i], cg_maxit.
 * No dual update.  lrs_op_admm_rhs: the right-hand side the last half-step of `cone` left
 * (column-major n_k x r_k, as lrs_op_admm_half's rhs). */
int lrs_op_admm_round(lrs_batch *b, lrs_ctx **ctxs, int n, const double *rho, const double *cg_tol, int cg_maxit);
int lrs_op_admm_rhs(lrs_ctx *ctx, int cone, double *rhs);
/* How the context's ADMM iteration runs at its current ranks (each may be NULL): the cones whose
 * half-step is the single-workgroup kernel, and whether the whole iteration is the
 * one-workgroup form that the ADMM meeting of a batch combines. */
int lrs_admm_form(lrs_ctx *ctx, int *small_cg_cones, int *round_form);
/* ---- Sign rounding of a factor for diagonally constrained cones.  No reference
 * counterpart (the reference stops at the factor).  For a cone whose constraints are X_ii = b_i for
 * every i and nothing else (MaxCut's relaxation: n consecutive constraints, constraint o + i the
 * single entry (i, i), none of them touching another cone), every b_i > 0, the objective in the
 * slot pattern, and a factor X (n x r, `which` one of LRS_R .. LRS_V) it draws `trials` hyperplanes
 * g_t in R^r (a multiple of 64, 64 .. 4096), sets s_i^t = +1 if <X_i, g_t> >= 0 else -1, x_i^t =
 * sqrt(b_i) s_i^t, and evaluates value_t = <C, x^t x^t^T> = sum_i C_ii b_i + 2 sum_{j<i} C_ij
 * sqrt(b_i b_j) s_i^t s_j^t in the units of the instance file (C = -F0: the units of
 * lrs_result.pobj and the JSON's primal_obj, whatever a reopt round scaled on the device): the
 * objective of a feasible rank-one point, an upper bound on the optimum over such points next to
 * the relaxation's lower bound pobj.  All of it on the device and the context's stream: a
 * projection kernel, a value kernel with a fixed-order finish (no float atomics: bitwise
 * reproducible) and, with local_search != 0, a one-flip descent per trial in between: rows
 * i = 0 .. n - 1 swept in order (Gauss-Seidel), f = sum_{j != i} C_ij sqrt(b_i b_j) s_j in
 * adjacency (column) order, s_i flipped iff that lowers the value (-4 s_i f < 0, strictly), sweeps
 * repeated until one flips nothing in that trial or max_sweeps (<= 0: 50) have run.
 * dirs: r x trials column-major (trial t's direction at dirs + r t), or NULL: lrs_round_dirs(seed,
 * r, trials, .) is generated on the host and uploaded (no device generator).  Outputs, each may be
 * NULL: values[trials]; bits[trials / 64][n], bit t of bits[w][i] set iff s_i^(64 w + t) = +1;
 * best_trial, the smallest value's trial, the lowest index on ties; best_value; best_x[n] that
 * trial's signs (+1 / -1); sweeps, the sweeps the descent ran (the most over the trials; the last
 * one, which flips nothing, counts; 0 without local_search).
 * Refusals, each a negative code with its message in lrs_last_error() and nothing started: -2
 * trials not a multiple of 64 or out of range, -3 a sharded context, -4 no such cone, -5 the LP
 * block, -6 ranks not set, -7 a cone that is not diagonally constrained in the sense above, -8 a
 * b_i <= 0, -9 a dense or constant objective, -10 dense or rank-one constraint matrices, -11 a
 * selector other than LRS_R .. LRS_V (-1: the header's general failures).
 * lrs_round_dirs (host only, no context): the seeded directions, out[c + r t] for column c of
 * trial t: with mix(x) = splitmix64's output function of x + 0x9E3779B97F4A7C15 (z = that sum; z =
 * (z ^ z >> 30) 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) 0x94D049BB133111EB; z ^ z >> 31; mod 2^64),
 * h = mix(mix(seed) ^ (t 2^32 + c)), a = mix(h), b = mix(a), u1 = ((a >> 11) + 1) 2^-53, u2 =
 * (b >> 11) 2^-53, and the entry is sqrt(-2 ln u1) cos(6.283185307179586 u2) (Box-Muller).  A
 * seeded lrs_round_signs equals the call with these directions passed explicitly. */
int lrs_round_dirs(unsigned long long seed, int r, int trials, double *out);
int lrs_round_signs(lrs_ctx *ctx, int cone, int which, int trials, const double *dirs, unsigned long long seed,
                    int local_search, int max_sweeps, double *values, unsigned long long *bits, int *best_trial,
                    double *best_value, signed char *best_x, int *sweeps);
/* ---- Triangle-inequality separation for diagonally constrained cones.  No
 * reference counterpart.  For a cone that is diagonally constrained in lrs_round_signs' sense
 * (X_ii = b_i / a_i for every i and nothing else, none of it touching another cone, every b_i / a_i
 * > 0) and a factor X (n x r, `which` one of LRS_R .. LRS_V), x_ij = <X_i, X_j> / sqrt(b_i b_j)
 * over the columns c < r, and for every i < j < k the four inequalities of the metric polytope
 *   type 0: + x_ij + x_ik + x_jk >= -1      type 2: - x_ij + x_ik - x_jk >= -1
 *   type 1: + x_ij - x_ik - x_jk >= -1      type 3: - x_ij - x_ik + x_jk >= -1
 * have the violation v = -1 - ((s_ij x_ij + s_ik x_ik) + s_jk x_jk), summed in that order with the
 * type's signs.  Of the inequalities with v > min_violation (>= 0) the call returns the max_cuts
 * largest (1 .. LRS_TRI_MAX_K) under the strict total order v descending, then (i, j, k, type)
 * ascending lexicographically, sorted in that order: cuts[t] = {i, j, k, type} (0-based) and
 * violation[t], t < *n_cuts = min(max_cuts, *n_violated); *n_violated the exact number with v >
 * min_violation; *max_violation the largest v (0 when none qualifies).  Every output may be NULL.
 * The objective is not read (a dense or constant C is fine).  All of it runs on the device and the
 * context's stream: the matrix x (kept as tri_pad(n)^2 doubles in a per-context workspace, hence n
 * <= LRS_TRI_MAX_N), then scans of the 4 C(n, 3) inequalities: one that counts, as many as the
 * radix select over the key (v, index) needs to bound the cut, one that collects.  Integer atomics
 * only: every output is the same bits on every run.  A row of X need not have norm sqrt(b_i):
 * x_ij is what the formula says.
 * Refusals, each a negative code with its message in lrs_last_error() and nothing started: -2
 * max_cuts outside 1 .. LRS_TRI_MAX_K, -3 a sharded context, -4 no such cone, -5 the LP block, -6
 * ranks not set, -7 a cone that is not diagonally constrained, -8 a b_i <= 0, -10 dense or rank-one
 * constraint matrices, -11 a selector other than LRS_R .. LRS_V, -12 min_violation negative or NaN,
 * -13 n < 3, -14 n > LRS_TRI_MAX_N (-1: the header's general failures). */
#define LRS_TRI_MAX_K 65536
#define LRS_TRI_MAX_N 32768
int lrs_separate_triangles(lrs_ctx *ctx, int cone, int which, int max_cuts, double min_violation,
                           int *cuts /* [max_cuts][4]: i, j, k (0-based, i<j<k), type 0..3 */,
                           double *violation /* [max_cuts] */, int *n_cuts,
                           long long *n_violated, double *max_violation);
/* ---- Cutting-plane rounds in one context.  No reference counterpart.
 * lrs_solve_warm: lrs_solve's flow (ALM phase, ALM-to-ADMM, ADMM, reopt rounds, dual infeasibility,
 * trajectories, JSON state) with the ALM phase started from the context's current R (what
 * lrs_factor_get(LRS_R) returns) and LAMBDA (lrs_vec_get(LRS_LAMBDA)) at its current ranks.
 * Everything else is a cold start's: D, G, the L-BFGS pairs, the control block, U, V and the CG
 * work are reset, rho comes from the parameters, rank_max is lrs_determine_rank's for the current
 * m, and the current ranks are kept, clipped to it (a clipped cone keeps its leading columns);
 * AUG_RANK may grow them.  The start is evaluated first, and one that already meets the phase-1
 * test leaves the ALM phase at once, with alm_inner = 0.  If the previous solve's reopt rounds left
 * obj_scale != 1, LAMBDA is first divided by it: the multipliers are brought back to the unscaled
 * objective's units, as the objective itself is.  Refusals: -3 a sharded context, -6 ranks not set
 * (no workspace), -1 lbfgsListLength < 1 and the header's general failures.
 * Registered triangle cuts.  A context whose problem is one SDP cone diagonally constrained in
 * lrs_round_signs' sense by constraints 1 .. n (m = n), with no LP block of its own, keeps a list
 * of triangle inequalities {i, j, k, type} (lrs_separate_triangles' form).  The first append
 * remembers m0 = m.  Cut t of the list, in append order, is constraint m0 + t (0-based) with
 * right-hand side -1, the three SDP entries sigma / (2 sqrt(d_p d_q)) (d_i = b_i / a_i) on its pairs
 * and -1 on column t of one LP block, the last cone: sigma . x - s_t = -1, s_t >= 0 -- the problem
 * lrs_load_coo builds from instances.add_triangle_cuts' output.  The problem is rebuilt through
 * the presolve and uploaded afresh; everything keyed on the old one is dropped.
 * lrs_cuts_append: cuts[n][4]; a cut already in the list (or twice in the call) is skipped and
 * *n_added (may be NULL) counts the new ones; with none new nothing changes.  A malformed cut (not
 * 0 <= i < j < k < n, type 0 .. 3) or more than LRS_CUT_MAX_TOTAL cuts in all refuses the whole
 * call with -2.  lrs_cuts_drop: drop[n_cuts] != 0 marks the cuts to remove; the list is compacted,
 * order kept; *n_dropped (may be NULL); with none marked nothing changes.
 * carry != 0 needs solver state (ranks set) and keeps it: the same ranks, the SDP cone's rows of R
 * and LAMBDA[0, m0 + kept) the same bits, a new cut's multiplier 0 and its LP row sqrt(max(slack_t,
 * 0)) at those rows (a kept cut's LP row: recomputed likewise by an append, kept by a drop), so the
 * next lrs_solve_warm starts with zero residual on every cut the point satisfies.  Every other
 * buffer is zero, and a reopt scale of the previous solve is undone first (LAMBDA divided by
 * obj_scale).  carry == 0 leaves the ranks unset, as after a load.
 * lrs_cuts_get: *n_cuts (may be NULL) the list's length, cuts[min(cap, n_cuts)][4] (may be NULL).
 * lrs_cuts_state: for factor `which` (LRS_R .. LRS_V) slack[t] = 1 + ((s_ij x_ij + s_ik x_ik) +
 * s_jk x_jk) with x_pq formed as lrs_separate_triangles forms it (the same fused multiply-add chain
 * over the columns, the same division): for an inequality that call returns at the same factor,
 * slack is bitwise minus its violation.  lambda[t] = LAMBDA[m0 + t].  Each may be NULL.  On the
 * device and the context's stream, a dot a thread: the same bits on every run.  A context without
 * cuts: 0, nothing written.
 * lrs_round_signs and lrs_separate_triangles accept the SDP cone of a context that registered its
 * cuts (its constraints are the n diagonal ones and exactly the list's) and act as on the plain
 * problem at the same factor; a problem loaded with such constraints already in it stays refused.
 * Refusals of lrs_cuts_append: -2 above, -3 a sharded context, -4 more than one SDP cone, -5 an LP
 * block of the problem's own, -6 carry without solver state, -7 not diagonally constrained (or not
 * by constraints 1 .. n alone), -8 a b_i <= 0, -9 a dense or constant objective, -10 dense or
 * rank-one constraint matrices.  lrs_cuts_drop: -13 a context without cuts, -6.  lrs_cuts_state:
 * -6, -11 a selector other than LRS_R .. LRS_V.  A refused call changes nothing.
 * lrs_certified_bound: for such a context, with or without cuts, the weak-duality bound of the
 * current LAMBDA in the instance file's units (lrs_result.dobj's; a reopt scale undone):
 *   bound = b^T lambda + (sum_i d_i) min(0, lambda_min(S)) + 4 sum_t min(0, lambda_{m0 + t}),
 * S = C - sum_i lambda_i A_i on the SDP cone: tr X = sum_i d_i is fixed by the diagonal and every
 * slack lies in [0, 4] since |x_pq| <= 1.  lambda_min is lrs_op_dual_infeasibility's per-cone
 * value (*lam_min, may be NULL) and *converged (may be NULL) that eigen-solve's flag: 1 when its
 * Ritz residual met tol max(eps^(2/3), |theta|); 0 when the restart cap ran out -- the Ritz value
 * is then only an UPPER bound of lambda_min and `bound` is not certified.  With converged = 1 the
 * Ritz value theta is taken as lambda_min as it stands: its residual, at most 1e-2 max(eps^(2/3),
 * |theta|), is not subtracted, so the bound is certified to within (sum_i d_i) times that.  Refusals: -3, -4, -5,
 * -6, -7, -8, -10 as above. */
#define LRS_CUT_MAX_TOTAL 262144
int lrs_solve_warm(lrs_ctx *ctx, const lrs_params *p, lrs_result *res);
int lrs_cuts_append(lrs_ctx *ctx, const int *cuts /* [n][4]: i < j < k 0-based, type 0..3 */, int n, int carry,
                    int *n_added);
int lrs_cuts_drop(lrs_ctx *ctx, const unsigned char *drop /* [n_cuts] */, int carry, int *n_dropped);
int lrs_cuts_get(lrs_ctx *ctx, int *cuts, int cap, int *n_cuts);
int lrs_cuts_state(lrs_ctx *ctx, int which, double *slack /* [n_cuts] */, double *lambda /* [n_cuts] */);
int lrs_certified_bound(lrs_ctx *ctx, double *bound, double *lam_min, int *converged);
/* ---- Rank reduction: the factors rotated to the principal axes of their Gram.
 * No reference counterpart.  With G = X^T X = Q diag(w) Q^T, w descending, X Q has the same X X^T;
 * its leading k columns are the best rank-k approximation and the trace lost is sum_{j >= k} w_j.
 * lrs_sym_eig (host only, no context, like lrs_round_dirs): a symmetric r x r (row- or column-
 * major, it is symmetric; the mean of the two triangles is taken), w[r] its eigenvalues in
 * descending order, q (may be NULL) column-major r x r, column j the unit eigenvector of w[j] with
 * its component of largest magnitude positive (the first one on a tie).  Householder
 * tridiagonalisation and implicit QL with accumulated vectors; the same bits on every call.  -2:
 * r < 1 or a NULL a / w.
 * `which`: LRS_R takes the source R, LRS_U the source (U + V) / 2, the phase-2 point; anything else
 * is refused with -11.
 * lrs_factor_spectrum changes nothing: per cone the device Gram (k_gram), then lrs_sym_eig's
 * routine.  eigs[sum_k r_k] cone by cone, descending, small negative values as they come; the LP
 * cone contributes its one 1 x 1 Gram entry.  counts[k]: eigenvalues > rel_tol times the cone's
 * largest.  Each may be NULL.
 * lrs_factor_compress: for each SDP cone k_new = new_ranks[k] when given and > 0, else min(r,
 * max(1, count(rel_tol) + slack)); the LP cone stays at rank 1 and its rows are copied bit for bit
 * (LRS_R).  Every cone is rotated, also where k_new = r.  Afterwards the context's ranks are the new
 * ones (rank_max untouched: AUG_RANK can grow them again), R = U = V = the compressed source,
 * bitwise equal, LAMBDA is kept bit for bit, every other work buffer is zero as after lrs_set_rank,
 * and what is keyed on the workspace is dropped as lrs_set_rank drops it.  A reopt scale is left as
 * it is.  The factors do not go through the host: the old R, U, V stay alive across the
 * reallocation, k_rot (FP64 matrix cores) writes old -> new, then they are freed (peak memory: the
 * new workspace plus three old factors; host traffic: the r x r Grams down, Q up).  Outputs, each
 * may be NULL: ranks_out[K]; eigs as above (at the OLD ranks); lost[K] = the sum of the dropped
 * eigenvalues, max(., 0) each; q cone by cone, column-major r_k x r_k (old ranks).
 * Refusals (nothing changed): -3 a sharded context, -6 ranks not set, -11 a bad selector, -2 a
 * new_ranks[k] < 0 or above the current rank, an LP entry other than 0 or 1, rel_tol outside
 * [0, 1), slack < 0 (-1: the header's general failures).  Contexts with registered cuts, dense-A,
 * rank-one and dense-objective cones are accepted: only the factor layout changes.
 * lrs_solve_warm clips an over-wide start to its leading columns: compress first, then the leading
 * columns are the principal ones.
 * lrs_set_rank_shrink(rel_tol, slack): rel_tol <= 0 is off, the default.  On, lrs_solve and
 * lrs_solve_warm do this once, right before the ALM-to-ADMM hand-over, on an unsharded context
 * whose time limit has not hit: the counts of R are taken, and if some cone's min(r, max(1, count +
 * slack)) is below its rank the point is compressed to those ranks (log line "rank shrink: a ->
 * b").  The phase-2 trajectory and final_rank then show the lower ranks; the reopt rounds run on
 * from there.  lrs_solve_batch ignores the setting: batch members keep their ranks.  Off, no output
 * differs by a byte.  -2: rel_tol >= 1 or NaN, slack < 0.
 * lrs_compress_timing: the last lrs_factor_compress's k_rot launches between two HIP events (ms)
 * and their algorithmic bytes, 8 n (r + k) per cone (8 n (2 r + k) from LRS_U). */
int lrs_sym_eig(int r, const double *a, double *w, double *q);
int lrs_factor_spectrum(lrs_ctx *ctx, int which, double rel_tol,
                        double *eigs /* [sum_k r_k], cone by cone, descending */,
                        int *counts /* [K]: eigenvalues > rel_tol * the cone's largest */);
int lrs_factor_compress(lrs_ctx *ctx, int which, const int *new_ranks /* [K] or NULL */, double rel_tol, int slack,
                        int *ranks_out /* [K] */, double *eigs /* as above, may be NULL */,
                        double *lost /* [K], may be NULL */, double *q /* may be NULL */);
int lrs_set_rank_shrink(lrs_ctx *ctx, double rel_tol, int slack);
int lrs_compress_timing(lrs_ctx *ctx, double *rot_ms, double *rot_bytes);
/* trajectory (phase 1 then phase 2) after lrs_solve: curr and oracle ranks */
int lrs_trajectory(lrs_ctx *ctx, int phase, int *curr_rank, int *oracle_rank, int cap);
/* JSON like lorads_logging.c:618-712 */
int lrs_write_json(lrs_ctx *ctx, const char *path, const char *problem_id, const char *file_path,
                   const lrs_result *res, const lrs_params *p);

/* Phase-1 throughput: runs `warmup` then `steps` ALM inner iterations at the
 * current rank (phase1Tol effectively off), timing the steps with device events.
 * kernel_ms (optional) receives per-kernel average durations of the A(UU^T)
 * SDDMM kernel measured with HIP events on the solver stream. */
int lrs_alm_throughput(lrs_ctx *ctx, const lrs_params *p, long warmup, long steps, double *seconds,
                       long *done, double *sddmm_avg_ms, double *iter_avg_ms);

/* Benchmark hook on the phase-1 budget (lrs_params.almInnerBudget): when the ALM inner
 * loop reaches the budget, the solve synchronises its stream and calls
 * hook(user, inner_iterations_done).  A return value larger than the count continues the
 * SAME solve (same iterate, L-BFGS ring and control block) up to that new absolute budget;
 * anything else ends phase 1 as without a hook.  This lets a caller time exactly K inner
 * iterations after W warmup iterations with no solver setup inside the timed region.
 * NULL removes the hook.  (No reference counterpart: benchmarking only.) */
typedef long (*lrs_budget_hook)(void *user, long inner_done);
int lrs_set_budget_hook(lrs_ctx *ctx, lrs_budget_hook hook, void *user);
/* The last completed ALM inner iteration of the last solve (after a budget stop: trip
 * almInnerBudget): out4 = {tau, ||G||^2, l_1 primal infeasibility, beta of the newest
 * L-BFGS pair}; newest_pair = 0 if that pair is (LRS_S0, LRS_Y0), 1 if (LRS_S1, LRS_Y1).
 * (Test hook for the per-iteration parity against the reference's inner loop,
 * lorads_alm.c:1302-1379.) */
int lrs_alm_last_step(lrs_ctx *ctx, double *out4, int *newest_pair);
/* Wait for every operation enqueued on the context's stream. */
int lrs_sync(lrs_ctx *ctx);

/* Mirror the iteration log into a file (the reference's --logfile). */
int lrs_set_log_path(lrs_ctx *ctx, const char *path);

/* Kernel selection of the ALM inner iteration (same arithmetic either way):
 * 0 = automatic (the latency-regime kernels k_lat_a/k_lat_b when every row's lane group is
 * resident at once, else the general row kernels), 1 = general row kernels only,
 * 2 = general row kernels in their bandwidth-regime form (stages split in two launches),
 * 3 = as 2 with the long-row neighbour kernels k_wide_a/k_wide_b wherever the layout allows,
 * 4 = the single-workgroup inner loop where it fits, 5 = as 0 with one lane group a row even
 * where denser rows would get a team of lane groups, so that the latency-regime kernels also take
 * such cones (diagnostics and tests: the teams are the faster form there).
 * The environment variable LRS_NO_LAT=1 forces 1 for every context. */
int lrs_set_kernel_path(lrs_ctx *ctx, int path);
/* The path the last enqueued ALM inner iteration of this context took (0 latency-regime
 * kernels, 1 general row kernels; -1 none enqueued yet). */
int lrs_get_kernel_path(lrs_ctx *ctx, int *used);
/* *used = 1 when every launch of the last enqueued ALM inner iteration was the latency kernels'
 * PLAIN instantiation (path 0 on cones whose slots carry at most one constraint entry and at most
 * one local constraint, without dense-row slices and without a dense objective), else 0.  The
 * environment variable LRS_LAT_PLAIN=0 selects the general instantiation (same results). */
int lrs_lat_plain_used(lrs_ctx *ctx, int *used);
/* *used = 1 when the last enqueued ALM inner iteration ran the latency kernels (path 0) with their
 * wave sums as transposed butterflies (wave_tsum: the same pair tree as one wave sum a value, so
 * the same bits), else 0.  The environment variable LRS_LAT_TSUM=0 selects one wave sum a value. */
int lrs_lat_tsum_used(lrs_ctx *ctx, int *used);
/* The lane layout of `cone`'s factor rows at the context's current ranks (after lrs_set_rank or a
 * solve): every factor array of the cone is row-major n x ld on the device, a row held by G lanes
 * with E doubles each, ld = G E >= the cone's rank, the columns [rank, ld) zero.  G, E and ld may
 * each be NULL.  Diagnostics and tests (which template instantiation of the kernels a rank runs;
 * the environment variable LRS_LAYOUT=GxE forces one wherever it holds the rank). */
int lrs_get_layout(lrs_ctx *ctx, int cone, int *G, int *E, int *ld);
/* The LP block's ADMM column sweep as the next launch will run it (read-only; every pointer may be
 * NULL).  *lp_cone = the LP block's cone, -1 without one (the other outputs are then 0).  *staged =
 * 1 when the sweep's operands fit the LDS limit (152 KB, lowered by the environment variable
 * LRS_LP_LDS_MAX in bytes, read per launch; 0 forces the other variant) and the walk reads them
 * there, 0 when it walks global memory.  *lds_bytes = what the staged variant needs for this
 * problem, *entries = the LP block's constraint entries on the device, *dense_dropped = the
 * constraint entries of its columns present in >= m/4 constraints, which the reference's column
 * typing drops (their squared norm stays in the update's denominator).  Diagnostics and tests. */
int lrs_lp_sweep_info(lrs_ctx *ctx, int *lp_cone, int *staged, long *lds_bytes, long *entries, long *dense_dropped);
/* *max_abs = the largest |x| over the padding columns [rank, ld) of every row of factor `which`
 * (LRS_R .. LRS_Y1) in every cone, read back from the device as it is stored; a NaN counts as
 * infinite.  Every kernel reduces over whole padded rows, so this is 0 at all times (tests). */
int lrs_factor_padding(lrs_ctx *ctx, int which, double *max_abs);

/* Standalone A(UU^T) on R (the constraint-entry kernel k_auv_con, all cones): reps
 * launches back to back between two HIP events, average ms per launch; and its
 * algorithmic bytes (factor rows touched once + entry data + outputs). */
int lrs_time_auut(lrs_ctx *ctx, int reps, double *avg_ms);
int lrs_auut_bytes(lrs_ctx *ctx, double *bytes);

/* Standalone r x r Gram R^T R of one cone (build_gram_from_factor, lorads_logging.c:216-240;
 * k_gram on the FP64 matrix cores, then the fixed-order partial reduction): avg_ms = ms per
 * Gram (kernel + reduction), gram_ms = ms of the MFMA kernel alone (may be NULL). */
int lrs_time_gram(lrs_ctx *ctx, int cone, int reps, double *avg_ms, double *gram_ms);

/* The FP64 matrix-core ceiling on this device, measured: TFLOP/s of back-to-back
 * v_mfma_f64_16x16x4f64 on every CU (8 independent accumulators a wave, 2 waves a SIMD).
 * Diagnostics for the Gram's roofline; no reference counterpart. */
int lrs_mfma_f64_peak(lrs_ctx *ctx, double *tflops);
/* The same probe at `waves_per_simd` (1..8) waves a SIMD with `chains` (4 or 8) independent
 * accumulators a wave, plus the shader clock under that load (s_memtime against the 100 MHz
 * wall clock, MHz) and the cycles a SIMD spends per v_mfma_f64_16x16x4f64: the matrix-core
 * rate separated from the clock (bench.py "mfma_probe").  No reference counterpart. */
int lrs_mfma_f64_probe(lrs_ctx *ctx, int waves_per_simd, int chains, double *tflops, double *mhz,
                       double *cycles_per_mfma);
/* The latency kernels' two wave-sum forms on the caller's inputs, one small launch: `ref` from one
 * wave sum a value, `out` from the transposed butterfly (nv values each, 1 <= nv <= 16), for a
 * bitwise comparison.  form 0, the control wave's prologue: in[nv][n], the partials of
 * 1 <= n <= 256 producer blocks.  form 1, the block tail: in[nv][64 n], the accumulators of the
 * threads of 1 <= n <= 8 waves; value v summed per wave, then over the waves in wave order. */
int lrs_wave_tsum_probe(lrs_ctx *ctx, int form, int nv, int n, const double *in, double *ref, double *out);

/* Dense objective (a cone whose C is kept as a full n x n matrix: LRS_DENSE_C=1, or n >= 1024
 * with C filling >= 1/4 of the lower triangle): ms per C R product on the FP64 matrix cores
 * (k_cgemm, 2 n^2 r flop), averaged over `reps`.  Fails when the cone has no dense objective. */
int lrs_time_dense(lrs_ctx *ctx, int cone, int reps, double *avg_ms);

/* Dense constraint matrices (the reference's SDP_COEFF_DENSE, data/lorads_sdp_data.c:1187-1191:
 * an A_i with more than 10 % of the cone's lower triangle, strictly).  A cone on the dense-A
 * path (LRS_DENSE_A=1; unset: at least 320 000 entries in the cone's dense A_i; LRS_DENSE_A=0: never) keeps those A_i out of the slot
 * pattern as a stack of full n x n matrices and evaluates them on the FP64 matrix cores
 * (k_dcon_ax); its ALM inner loop is the operator-composed one.  Sharded
 * contexts refuse such a problem.
 * lrs_dense_a_info: the cone's number of dense coefficients (whichever path), whether it took
 * the dense path at load, and the stack's bytes (0 off the path); outputs may be NULL.
 * lrs_time_dense_a: ms per k_dcon_ax launch over the cone's whole stack on R (A_i R and the
 * dots <R, A_i R>), averaged over `reps` back-to-back launches; fails when the cone is not on
 * the dense path.
 * lrs_dense_a_plan: host-only (no device, no context) classification of the instance at `path`:
 * cons (may be NULL) receives up to cap 0-based constraint indices of the cone's dense A_i. */
int lrs_dense_a_info(lrs_ctx *ctx, int cone, int *n_dense, int *on_dense_path, long *stack_bytes);
int lrs_time_dense_a(lrs_ctx *ctx, int cone, int reps, double *avg_ms);
int lrs_dense_a_plan(const char *path, int cone, int *n_dense, int *on_dense_path, int *cons, int cap);

/* Rank-one dense constraint matrices.  Every coefficient the rule above types
 * dense is tested for A_i = sigma a a^T (pivot on the largest |A_pp|, accepted iff max |A_jk -
 * sigma a_j a_k| <= 1e-13 max|A|).  A cone that factors them keeps V = [a_1 .. a_p] (n x p) in
 * place of p full matrices -- n p doubles, not p n^2 -- and evaluates them as skinny products on
 * the FP64 matrix cores (k_r1_vtx, k_r1_apply).  LRS_RANK1_A=0: no detection; =1: every cone with
 * such a coefficient factors them (its other dense coefficients follow LRS_DENSE_A); unset: the
 * cones LRS_DENSE_A selects factor theirs.  Read when a problem is loaded.  Such a cone runs the
 * operator-composed inner loop, and sharded contexts refuse it, as for the dense-A path.
 * lrs_dense_a_info's n_dense still counts these coefficients; its stack_bytes does not.
 * lrs_rank1_info: the cone's number of rank-one dense coefficients (whichever path; 0 under
 * LRS_RANK1_A=0), whether it keeps a factor, and the factor's bytes (0 without); outputs may be
 * NULL.
 * lrs_rank1_plan: host-only (no device, no context) detection on the instance at `path`: cons and
 * sigma (each may be NULL) receive up to cap 0-based constraint indices, ascending, and signs.
 * lrs_time_rank1: ms per V^T R launch (k_r1_vtx with its finish) averaged over `reps` back-to-back
 * launches, and that launch's algorithmic bytes n (ldp + ld) 8 (may be NULL); fails when the cone
 * has no factor.
 * lrs_load_coo_rank1: lrs_load_coo plus nterm terms tsigma[t] a_t a_t^T on (constraint tcon[t] >=
 * 1, SDP block tblk[t], 1-based), the vectors concatenated in tvec, each of length dims[tblk[t]].
 * Refused: a term on constraint 0 (the objective), a term in the LP block, a (constraint, block)
 * that also has explicit entries.  A term whose expansion the reference's rule types sparse (z
 * nonzeros in a, z (z + 1) / 2 <= 0.1 n (n + 1) / 2) is expanded into entries and takes the slot
 * path; every other term is factored whatever LRS_RANK1_A says, and its n^2 entries are never
 * formed.  Ranks and norms come out as for the expanded entries. */
int lrs_rank1_info(lrs_ctx *ctx, int cone, int *n_rank1, int *on_factor_path, long *factor_bytes);
int lrs_rank1_plan(const char *path, int cone, int *n_rank1, int *on_factor_path, int *cons, double *sigma, int cap);
int lrs_time_rank1(lrs_ctx *ctx, int cone, int reps, double *avg_ms, double *bytes);
int lrs_load_coo_rank1(lrs_ctx *ctx, int m, int nblk, const int *dims, const double *b, long nnz, const int *con,
                       const int *blk, const int *row, const int *col, const double *val, int nterm, const int *tcon,
                       const int *tblk, const double *tsigma, const double *tvec);

/* Per-stage timing of the split ALM inner iteration: runs `steps` inner iterations at
 * the current rank like lrs_alm_throughput, with HIP events on the solver stream
 * around each of the four launches (S1 direction+SDDMM, S2 q-gather, S3 update+
 * adjoint, S4 gradient).  stage_ms[4] = average ms per launch; *done = iterations. */
int lrs_profile_stages(lrs_ctx *ctx, const lrs_params *p, long steps, double *stage_ms, long *done);

/* In-memory problem in SDPA entry semantics (replaces LReadSDPA for callers that
 * already hold the data, io/lorads_file_io.c:59-455): nblk blocks of sizes dims
 * (the last may be negative: an LP block of -dims[nblk-1] columns, entry row = column, col
 * unused), b[m], and nnz entries (con, blk, row, col, val) with 1-based blk/row/col and con 0 =
 * F0 (C = -F0). */
int lrs_load_coo(lrs_ctx *ctx, int m, int nblk, const int *dims, const double *b, long nnz, const int *con,
                 const int *blk, const int *row, const int *col, const double *val);

/* Which kernels the upload chose for the long-row cones: *auv = 1 when
 * some cone's constraint entries are in 2-D LDS tiles (A(XY^T) by k_auv_tile), *slot = 1
 * when some cone's lower pattern is (stage A / B and S X by k_tile_a / k_tile_b1/b2).  No
 * reference counterpart (the reference's 10 % dense rule picks a BLAS-3 branch instead,
 * data/lorads_sdp_data.c:1187-1193). */
int lrs_tile_info(lrs_ctx *ctx, int *auv, int *slot);
/* *used = 1 when the last enqueued ALM iteration ran its stages over those tiles (k_tile_a,
 * k_tile_b1/b2: the stage plan picked the long-row kernels for a tiled cone), else 0. */
int lrs_tile_used(lrs_ctx *ctx, int *used);

/* Algorithmic HBM bytes per launch of the split-iteration stages A, G, B at the
 * current ranks (the roofline numerators, DESIGN.md "Kernels"). */
int lrs_stage_bytes(lrs_ctx *ctx, double *bytes);

/* Per-launch duration (ms) of the split-iteration stages A, G, B on the current solver
 * state (call after lrs_alm_throughput): each stage is relaunched `reps` times back to
 * back between two HIP events on the solver stream (the stages are idempotent for a
 * fixed control block).  stage_ms[1] = 0 when there are no multi-slot constraints. */
int lrs_time_stages(lrs_ctx *ctx, int reps, double *stage_ms);

/* Diagnostics: in-kernel phase timestamps of the last split iteration (block 0,
 * 100 MHz wall clock), out[4][16], and (blk, optional) per-block entry/exit stamps
 * blk[4][1024][2].  Returns 64 from the diagnostics build (liblrsdp_timing.so), 0
 * from the product build. */
int lrs_debug_phase_times(lrs_ctx *ctx, unsigned long long *out, unsigned long long *blk);

/* ---- Sharded solve of one instance over several GPUs.
 * Replaces the reference's single-process operator slots for one cone split by rows:
 * every process loads the whole problem (lrs_load_sdpa / lrs_load_coo), then calls one
 * lrs_shard_* with its rank; the context then owns a contiguous block of rows (+ the
 * halo of neighbour rows) and the constraints inside it, and lrs_solve /
 * lrs_alm_throughput run whole solves (ALM + ADMM + reopt rounds + the dual
 * infeasibility) with, per inner iteration, one halo exchange of direction rows and
 * all-reduces of the stage totals (line search; L-BFGS dots + residual; shared
 * constraints' sums).  Any number of SDP cones, each split alike; constraints may span row
 * blocks (shared: every holder sums its owned entries, the sums meet in an all-reduce);
 * a dense objective is held as each shard's owned row block of C with every row in the
 * halo; long-row cones keep their 2-D tile stage kernels over the owned rows.  The ADMM CG
 * runs on owned rows with its dot products all-reduced; the Lanczos of the dual
 * infeasibility on owned rows with a vector halo.  DESIGN.md §6.  Every shard
 * must make the same calls in the same order (the collectives are matched by order). */
/* RCCL: rank 0 creates the id (128 bytes) and broadcasts it; every rank then calls
 * lrs_shard_rccl on its own GPU (ncclCommInitRank is collective). */
int lrs_comm_unique_id(char *id_out);
int lrs_shard_rccl(lrs_ctx *ctx, int world, int rank, const char *id);
/* One-process loopback transport (tests): `world` contexts on one GPU, one host thread
 * each; lrs_shard_loopback is collective over the group's threads. */
int lrs_loopback_create(int world, lrs_loopback **out);
void lrs_loopback_destroy(lrs_loopback *g);
int lrs_shard_loopback(lrs_ctx *ctx, lrs_loopback *g, int rank);
/* world, rank, first global row, owned rows, halo rows of this context (1, 0, 0, n, 0 unsharded) */
int lrs_shard_info(lrs_ctx *ctx, int *world, int *rank, int *row0, int *nown, int *nhalo);
/* ranks the context's transport counts itself (RCCL: ncclCommCount; loopback: its group's
 * world; 1 unsharded), so a launcher can check that every GPU joined the communicator */
int lrs_shard_comm_ranks(lrs_ctx *ctx, int *count);
/* Recording of the transport's operations (sharded contexts): on != 0 clears the log and records
 * every later operation, 0 stops.  lrs_shard_comm_log: *n = entries recorded; out (may be NULL)
 * receives min(cap, *n) records of 5 longs {kind, peer, cone, count, offset}: kind 0 = the start
 * of one halo-exchange group (cone = the vector's cone or -1 for factor rows, count = its ops),
 * 1 = send to peer, 2 = receive from peer (count doubles; offset: send-buffer position, or the
 * landing rows' local offset x ld), 3 / 4 = device / host all-reduce of count doubles.  Both
 * transports issue their groups from one op list, so the loopback transport's log is the
 * sequence of ncclSend / ncclRecv / ncclAllReduce calls the RCCL transport makes. */
int lrs_shard_comm_record(lrs_ctx *ctx, int on);
/* Inner-loop calls whose one-workgroup-per-cone launch timed out in its
 * workgroups' exchange and was rerun from the kept state on the multi-launch iteration (the
 * context then stays on it).  LRS_XWG_SPIN=k sets the exchange's spin limit to 2^k polls
 * (default 26; -1: no wait) -- k = -1 forces the fallback (tests). */
int lrs_xwg_fallbacks(lrs_ctx *ctx, int *count);
int lrs_shard_comm_log(lrs_ctx *ctx, long *out, long cap, long *n);
/* Host-only (no device, no context) view of the row partition of a sharded solve of the
   instance at `path`: counts[8] = {n_global, first owned global row, owned rows, local rows
   (owned + halo), send rows (all peers), shared constraints, local constraints, world}, then
   (arrays may be null) bounds[world+1], local_gid[local rows], send_ptr[world+1],
   send_gid[send rows] (global ids, grouped by peer), shared_gid[shared], con_gid[local
   constraints], primary[local constraints] (1: this shard counts it in sums).  Replaces the
   reference's nothing: LoRADS has no multi-process path. */
int lrs_shard_plan(const char *path, int world, int rank, long *counts, int *bounds, int *local_gid,
                   int *send_ptr, int *send_gid, int *shared_gid, int *con_gid, int *primary);

#ifdef __cplusplus
}
#endif
#endif

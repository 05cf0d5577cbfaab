// lrs_device.h -- device-side data model and kernel launchers for the MI355X
// (gfx950) low-rank SDP inner solver.  Host code (lrs_solver.cpp) owns all
// scalar control; the hot path runs as the kernels declared here.
//
// Data layout in HBM (DESIGN.md "Data layout"):
//  * factors R, D, G, L-BFGS s/y, U, V: ROW-major n x ld per cone (ld = G*E >= r,
//    zero padded), all cones concatenated in one buffer ("factor buffer").  A row
//    is read by one lane group of G lanes, E consecutive doubles per lane.
//  * pattern ("slots"): the union of the lower-triangle nonzeros of C and every
//    A_i of a cone, ordered row-major (row i, col <= i); all cones' slots
//    concatenated in one global slot space.
//  * symmetric adjacency per cone (row i -> (j, slot)) for the row-owned SpMM;
//    its prefix with j <= i is the lower part used by the row-owned SDDMM.
//  * constraints: CSR over global slots with the symmetric weight folded in
//    ((2 - delta_ij) * a, data/lorads_sdp_data.c:803-856) for A(.) ; the inverse
//    slot -> (constraint, a) CSR for A^*(y) (data/lorads_sdp_data.c:878-922).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

namespace lrs {

constexpr int kBlock = 256;          // threads per block (4 waves)
constexpr int kMaxPartialBlocks = 4096;
constexpr int kMaxPartialVals = 16;

// ---- ALM inner-loop control block (double array, double-buffered by iteration parity)
enum CtrlIdx {
    C_ACTIVE = 0,   // 1 while the inner L-BFGS loop runs
    C_EXIT,         // exit reason (ExitReason)
    C_INNER,        // alm_state.innerIter
    C_LOCAL,        // localIter
    C_CLEAR,        // clearLBFGS
    C_HEAD,         // L-BFGS ring head (next slot to write)
    C_GCUR,         // which G buffer holds the current gradient
    C_PENDING,      // previous iteration left partials to fold
    C_RCVAL,        // rho_certificate_val
    C_LAG,          // ||G||^2
    C_PINF1,        // l_1 primal infeasibility
    C_PINFINF,      // l_inf primal infeasibility
    C_BETA0, C_BETA1,   // 1/<y,s> per ring slot
    C_YY0, C_YY1,       // <y,y> per ring slot
    C_NODENUM,
    C_CG, C_CS0, C_CY0, C_CS1, C_CY1,  // D = -(cG G + cs0 s0 + cy0 y0 + cs1 s1 + cy1 y1)
    C_DG,           // <D, G> after LBFGSDirectionUseGrad
    C_LASTTAU,
    // dots of the current gradient with the ring (stash, valid when PENDING == 2)
    C_DSG, C_DYG, C_DSOG, C_DYOG, C_DSOY, C_DYOY,
    // written by the gather stage of the split iteration (authoritative after it ran)
    C_ACT2,         // ACTIVE after the phase-1 (l_inf pinf) test of the completed iteration
    C_EXIT2,        // exit reason after that test
    C_RRDONE,       // 1 if this iteration's first stage refreshed A(RR^T) and the residual
    C_RCUR,         // which factor buffer (R, R2) holds the current iterate
    C_NCTRL = 40
};
enum ExitReason {
    EXIT_NONE = 0,
    EXIT_CONVERGED = 1,   // rho_certificate_val - tol <= endALMSubTol (while condition)
    EXIT_PHASE1 = 2,      // l_inf pinf <= phase1Tol  -> END_ALM
    EXIT_LOCAL800 = 3,    // localIter > 800          -> break
    EXIT_TINYTAU = 4,     // |tau| < endTauTol        -> UpdateRho
    EXIT_NUMERR = 5,      // no root                  -> RET_CODE_NUM_ERR
    EXIT_BUDGET = 6,      // bench budget of inner iterations reached
    EXIT_XWG = 7          // one-workgroup-per-cone loop: the workgroups' exchange timed out (an error)
};
// ---- parameters read by the device loop
enum ParIdx {
    P_RHO = 0, P_RCTOL, P_ENDSUB, P_ENDTAU, P_PH1TOL, P_BN1, P_BNINF, P_CNINF,
    P_HIGHACC, P_BUDGET, P_L, P_GAP, P_NPAR = 16
};
// ---- line-search result, double-buffered by parity: tau, rootNum, flag
enum LsIdx { LS_TAU = 0, LS_ROOTNUM, LS_FLAG, LS_N = 4 };
// ---- finals of the standalone launchers (offsets into the per-context tmpfin scratch)
constexpr int kMaxCones = 256;
constexpr int kFinN = 416;           // per-context finals of the line search / direction kernels (FinIdx)
// TF_DOTC + k: cone k's <X, C Y> of a dense objective (op_constr_xx), read with the gather's sums
enum TmpFinIdx {
    TF_SD = 0, TF_GATHER = 2 * kMaxCones, TF_RESID, TF_DOT, TF_DOTC, TF_SPMM = TF_DOTC + kMaxCones,
    TF_N = TF_SPMM + kMaxCones
};
constexpr int kMaxShards = 64;       // processes of one sharded solve
constexpr int kLongRow = 32;         // constraint rows longer than this get a wave each

struct Layout {
    int G = 1, E = 1, ld = 1;
};
Layout choose_layout(int r);

struct DevCone {
    int n = 0, r = 0, ld = 0, G = 0, E = 0;
    bool lp = false;    // the LP block as the diagonal cone at rank 1 (lrs_problem.cpp build_problem)
    // LP cone: per row (LP column) its local slot or -1 (a column without data), and per row
    // the column's squared 2-norm (lp_cone_presolve nrm2Square, lorads_lp_conic.c:132-133)
    int *lp_slot = nullptr;
    double *lp_nrm2 = nullptr;
    // LP cone: its entries' range [lp_e0, lp_e0 + lp_ne) of the slot CSR (upload_problem; the
    // sweep's launch takes it from here), and the entries its LP_COEFF_DENSE columns lost
    long lp_e0 = 0, lp_ne = 0, lp_dense_dropped = 0;
    // rows the kernels compute: [row0, row0 + nown) -- the whole cone, or in a sharded
    // solve this process's rows (the others, the halo, are read as neighbours only)
    int row0 = 0, nown = 0;
    long foff = 0;      // offset (doubles) of this cone in the factor buffer
    int slot_off = 0, P = 0;
    // every slot has at most one constraint entry and at most one local constraint (slot1.y,
    // loc1.y never -2): the latency kernels' PLAIN instantiations apply
    bool plain = false;
    int *adj_ptr = nullptr, *adj_low = nullptr, *adj_col = nullptr, *adj_slot = nullptr;
    long adj_nnz = 0;
    // constraint i of this cone is the single entry (i, i), every i (m = n): k_auv_diag
    bool auv_diag = false;
    // most adjacency entries of one row (all, and lower incl. the diagonal); 0 = unknown
    int maxdeg = 0, maxlow = 0;
    // dense rows (far more entries than the rest, e.g. a hub vertex): the latency kernels
    // spread their entries over extra slice blocks.  A: rows whose lower part has more than
    // kDenseRow entries; B: rows whose adjacency has.  Host ids (for the grids) and device copies.
    std::vector<int> dra_h, drb_h;
    std::vector<int> dra_n, drb_n;       // their entry counts (A: lower incl. diagonal, B: all)
    int *dra = nullptr, *drb = nullptr;
    long gl_need = 0;                    // doubles of slice gradients the B slices can need (any layout)
    // dense objective (lrs_problem.h), not in the slots: 1 = C as a full n x n row-major
    // matrix, 2 = the constant C = c_alpha J (rank-one products, no matrix)
    int dense_c = 0;
    double *Cd = nullptr;
    double c_alpha = 0.0;
    // dense constraint coefficients (lrs_problem.h HostCone::dA), not in the slots: kd full
    // n x n row-major symmetric matrices, coefficient j at dA + j n^2, of constraint dA_con[j]
    int kd = 0;
    double *dA = nullptr;
    int *dA_con = nullptr;
    std::vector<int> dA_con_h;
    const double *dSd = nullptr;         // while the dual infeasibility runs: S_d = -sum_j lambda_j A_j (n x n)
    // rank-one dense coefficients (lrs_problem.h HostCone::rV), in neither the slots nor the stack:
    // rV n x rldp row-major (row i: a_1[i] .. a_rp[i], padding 0; rldp a multiple of 16), term t
    // = r_sigma[t] a_t a_t^T of constraint r_con[t] (ascending)
    int rp = 0, rldp = 0;
    double *rV = nullptr, *r_sigma = nullptr;
    int *r_con = nullptr;
    // while the dual infeasibility runs: the weights w (S_r = sum_t w[con_t] sigma_t a_t a_t^T),
    // a p-vector for V^T v and k_r1_vtx's chunk partials
    const double *r1w = nullptr;
    double *r1T = nullptr, *r1part = nullptr;
    // long rows (>= kTileMinDeg adjacency entries per row on average): per row, the first entry
    // at or past column x n / kNX, x = 0..kNX ([n][kNX + 1]); the column-tiled k_wide_* kernels
    int *colseg = nullptr;
    // A(X Y^T) over 2-D tiles (many constraint entries per row, e.g. C5): the cone's constraint
    // entries bucketed by (row tile, column tile) of kAuvT rows each, items of at most kAuvItem
    // entries {row0, col0, begin, end}, per tiled entry its local (row, col) packed 16:16 and its
    // constraint entry (cone order), and the per-entry values in cone entry order (scratch)
    int auv_items = 0;
    long auv_ebase = 0;                  // first constraint entry of this cone (con_ptr[k m])
    int *auv_item = nullptr;             // [items][4]
    unsigned *auv_pq = nullptr;          // [Zk]
    int *auv_pos = nullptr;              // [Zk]
    double *auv_val = nullptr;           // [Zk]
    // the lower pattern in the same 2-D tiles (k_tile_a, stage A of the long-row path): items
    // {row0, col0, begin, end}, per tiled slot its local (row, col) 16:16 and its global slot
    int sa_items = 0;
    int sa_n = 0;                        // tiled slots (sa_slot's length)
    int *sa_item = nullptr;
    int sa_nsub = 0;                     // the items cut at kTileSub slots (k_tile_a's sub-items)
    int *sa_sub = nullptr;
    int sa_ngrp = 0;                     // runs of <= kTileGrp sub-items of one row tile: [ngrp + 1] starts
    int *sa_grp = nullptr;
    unsigned *sa_pq = nullptr;
    int *sa_slot = nullptr;
    // stage B's gradient S R_new over the symmetric pattern in the same tiles (k_tile_b2): one
    // block per (row tile I, column group x of kNX), its tile pairs {col0, row-pointer offset}
    // ([nt * kNX][2] ranges into sb_tp), per tile pair kAuvT + 1 row pointers into the entries
    // {local column, slot}; sa_S holds the slot values of S = C + A^*(M1) between the two kernels
    int sb_blocks = 0;
    int *sb_blk = nullptr, *sb_tp = nullptr, *sb_rp = nullptr, *sb_ent = nullptr;
    double *sa_S = nullptr;
    // sharded solve: the tiles cover the owned rows only -- sa_* the owned rows' lower slots,
    // sb_* the row tiles from sb_I0 on; sx_slot the slots whose lower row is a halo row (the
    // upper entries of owned rows), whose S k_slot_sv forms for k_tile_b2
    int sb_I0 = 0;
    int sx_n = 0;
    int *sx_slot = nullptr;
    // single-workgroup ADMM half-step (launch_small_cg; small unsharded cones, lrs_problem.cpp):
    // the constraint slots (slots with a constraint entry, cg_ncs) and their symmetric adjacency
    // per row packed (col << 16 | constraint slot); the cone's constraints in compact order (the
    // cg_ns short ones, then the long ones; cg_cl_con their ids) with their entries packed
    // (constraint slot << 1 | diagonal) and weights (2 - delta) a; per constraint slot its
    // (compact constraint, a) pairs; the objective as constant (cg_cconst 1: slot form, alpha =
    // Craw[cg_cslot]; 2: the rank-one form) or its entries per row (col, global slot)
    int cg_ok = 0, cg_ncs = 0, cg_ncl = 0, cg_ns = 0, cg_nce = 0, cg_nsc = 0, cg_nadj = 0, cg_cconst = 0, cg_cslot = 0;
    int *cg_cadj_ptr = nullptr, *cg_cadj = nullptr, *cg_cl_con = nullptr, *cg_cl_ptr = nullptr, *cg_ce = nullptr;
    int *cg_sp = nullptr, *cg_sj = nullptr, *cg_cc_ptr = nullptr, *cg_cc = nullptr;
    double *cg_ce_w = nullptr, *cg_sa = nullptr;
    // a cone with constraint-entry tiles (auv_items): the global slots holding C entries, for
    // <C, X Y^T> straight from the factor rows (launch_cobj)
    int cobj_n = 0;
    int *cobj_slot = nullptr;
};
constexpr int kScMaxN = 256;         // rows of a cone the single-workgroup ADMM half-step takes
constexpr int kMaxRankLd = 512;      // widest factor row (choose_layout: 64 lanes x 8 doubles)
constexpr int kAuvT = 128;           // rows of one side of an A(X Y^T) tile
constexpr int kAuvC = 32;            // factor columns staged in LDS at a time
constexpr int kAuvThreads = 512;
constexpr int kAuvNpt = 8;           // entries per thread of one item
constexpr int kAuvItem = kAuvThreads * kAuvNpt;
constexpr int kTileSub = 1024;       // slots of one k_tile_a sub-item (one a thread)
constexpr int kTileGrp = 2;          // most sub-items of one k_tile_a group (one row tile)
constexpr int kAuvMinN = 2048;       // tiled when n >= this and the lower triangle's tiles hold on average
constexpr int kAuvMinPerTile = 768;  //   >= this many entries (constraint entries for A(X Y^T), pattern slots
                                     //   for the stage kernels: 3x reuse of each staged row); C5 ~1850, a
                                     //   C5-structured m = 1e5 ~98 (slower tiled); LRS_AUV_TILES /
                                     //   LRS_SLOT_TILES = 0/1 override
constexpr int kCgSplitSlabs = 8;      // k_cgemm2's most K-slices (DevWork::CGK slabs)
constexpr int kNX = 8;              // column blocks of the tiled long-row kernels (one per XCD)
constexpr int kTileMinDeg = 32;
constexpr int kDenseRow = 64;        // entries of a row past which the latency kernels slice it
constexpr int kSliceMinB = 28;       // fewest entries of one B slice block (G = 64: 7 groups x 4)
constexpr int kMaxDenseRows = 32;    // more dense rows than this: the general row kernels

// Sharded solve (one process per GPU, rows of the cone split into contiguous blocks):
// the collectives the split iteration calls between its stages, provided by the host
// (lrs_solver.cpp: RCCL, or the one-process loopback transport of the tests).
struct ShardHooks {
    void *self = nullptr;
    // direction rows D of this shard's halo from their owners (and its rows to theirs)
    int (*halo)(void *self, double *D, hipStream_t st) = nullptr;
    // in-place sum over the shards of n contiguous doubles in device memory
    int (*allreduce)(void *self, double *buf, int n, hipStream_t st) = nullptr;
};

struct DevProblem {
    const ShardHooks *shard = nullptr;   // non-null in a sharded solve
    int no_lat = 0;                      // kernel path (lrs_set_kernel_path): 1 never the latency kernels, 2 + bandwidth regime, 3 + long-row kernels, 4 the single-workgroup inner loop, 5 auto without teams
    int *slot_g = nullptr;               // [Ptot][2] every slot's (row, col) in the all-cones row space
    mutable int last_path = -1;          // path of the last enqueued iteration (0 lat, 1 general)
    mutable int last_tiles = 0;          // the last enqueued iteration ran stage A / B over the 2-D tiles
    mutable int last_plain = 0;          // ... every latency launch of it as the PLAIN instantiation
    mutable int last_tsum = 0;           // ... its latency launches' wave sums by wave_tsum (LRS_LAT_TSUM)
    int m = 0, K = 0;
    int lp_cone = -1;   // the LP block's cone (the last), -1 without one
    long NRpad = 0;     // factor buffer length (doubles)
    int Ptot = 0;
    long Z = 0;
    double *b = nullptr;
    double *Cw = nullptr, *Craw = nullptr;                   // [Ptot]
    int *con_ptr = nullptr, *con_slot = nullptr;             // [m+1], [Z]
    double *con_w = nullptr;                                 // [Z]
    int *slot_ptr = nullptr, *slot_con = nullptr;            // [Ptot+1], [Z]
    double *slot_a = nullptr;                                // [Z]
    // single-slot ("local") constraints per slot, and the list of the others
    int mg = 0;                                              // number of global constraints
    int glob_maxlen = 0;                                     // most entries of one global constraint
    int *glob = nullptr;                                     // [mg]
    int *loc_ptr = nullptr, *loc_con = nullptr;              // [Ptot+1], [m - mg]
    double *loc_w = nullptr;                                 // (2 - delta) a of that one entry
    int *slot_rc = nullptr;                                  // [Ptot][2] (row, col) in the cone
    double *slot1 = nullptr;                                 // [Ptot][2] {a, con} of a slot's single
                                                             //   constraint entry (con -1 none, -2 several)
    double *loc1 = nullptr;                                  // [Ptot][2] {w, con} of its single local constraint
    int *con1_pq = nullptr;                                  // [K*m][2] single-entry rows: (p, q); -1 other; -2 long
    int *long_rows = nullptr;                                // constraints with > kLongRow entries in a cone,
    std::vector<int> long_ptr_h;                             //   grouped by cone: long_ptr_h[k]..[k+1]
    double *con1_w = nullptr;                                // [K*m] their weight
    // sharded solve: constraints held by several shards ("shared", lrs_problem.h ShardPlan)
    int nsh = 0;                                             // shared constraints (same on every shard)
    int *sh_idx = nullptr;                                   // [m] local constraint -> shared index, -1
    double *cmask = nullptr;                                 // [m] 1 where this shard counts the constraint
    double *bprim = nullptr;                                 // [m] b * cmask (b^T lambda counted once)
    double *g3 = nullptr;                                    // [3][m] owned-slot sums RR, RD, DD (global cons)
    double *gpack = nullptr;                                 // [nsh][3] the shared ones, all-reduced
    double *spack = nullptr;                                 // [nsh] one m-vector's shared entries
    std::vector<DevCone> cones;
    int ndense = 0;                                          // cones with a dense objective (DevCone::Cd)
    int ndensea = 0;                                         // cones on the dense-A path (DevCone::dA) or with a rank-one factor (DevCone::rV)
    bool tiles = false;                                      // column-tiled long-row kernels (LRS_TILES=1 at alloc)
    double *gp = nullptr;                                    // DevWork::GP (kNX partial factors), the tiled S X's scratch
    double *cgk = nullptr;                                   // DevWork::CGK: k_cgemm2's split-K slabs (kCgSplitSlabs x NRpad)
    double dense_scale = 1.0;                                // objScale_dualvar's factor on those C
    // K > 1: all cones as one block-diagonal row space (global rows and columns); used by
    // the split iteration when every cone has the same (G, E) row layout
    DevCone merged;
    bool has_merged = false;
    bool cone_sep = false;                                   // every constraint's entries lie in one cone
};

// Scratch shared by the kernels of one solve.
struct DevWork {
    double *R = nullptr, *D = nullptr, *G[2] = {nullptr, nullptr};
    double *R2 = nullptr;      // second factor buffer of the split iteration (R double-buffered)
    // dense-objective cones (DevCone::Cd): C R of the current iterate (carried C R + tau C D
    // through the inner loop, recomputed by op_grad) and C D of the iteration; zero elsewhere
    double *CR = nullptr, *CD = nullptr;
    double *CGK = nullptr;   // k_cgemm2's split-K slabs (dense cones of >= 2048 rows): kCgSplitSlabs x NR
    // dense-A cones (DevCone::dA), sized for the largest: dT the products T_i = A_i X (kd x n x ld),
    // dSd one full matrix sum_i w_i A_i (n x n), dpart k_dcon_ax's tile partials
    double *dT = nullptr, *dSd = nullptr, *dpart = nullptr;
    // cones with a rank-one factor (DevCone::rV), sized for the largest: rTx, rTz the products
    // V^T X, V^T Z (rldp x ld each), rTy V^T Y of the ADMM half-step (kept over its CG), rpart
    // k_r1_vtx's chunk partials
    double *rTx = nullptr, *rTz = nullptr, *rTy = nullptr, *rpart = nullptr;
    // column-tiled long-row kernels: kNX partial S R_new factors (kNX * NRpad), null when no cone
    // has long rows
    double *GP = nullptr;
    double *ls[2] = {nullptr, nullptr}, *ly[2] = {nullptr, nullptr};
    double *U = nullptr, *V = nullptr, *X = nullptr;         // ADMM / scratch factors
    double *cg_r = nullptr, *cg_p = nullptr, *cg_Q = nullptr, *cg_b = nullptr, *M2 = nullptr;
    double *uvt0 = nullptr, *uvt1 = nullptr, *uvt2 = nullptr, *S = nullptr;   // [Ptot]
    double *uvp = nullptr;   // [Ptot][2] the tiled stage A's (sym(RD^T), DD^T) per slot, for k_it_g
    double *lam = nullptr, *cvs = nullptr, *q1 = nullptr, *q2 = nullptr, *M1 = nullptr, *wtmp = nullptr;
    double *cvc = nullptr;                                   // per-cone A(UV^T), K*m
    double *lpw = nullptr;                                   // the LP sweep's scratch (lp_sweep_scratch)
    double *part = nullptr;    // [kMaxPartialVals][kMaxPartialBlocks] partial sums (scratch A)
    double *partB = nullptr;   // second partial buffer (scratch B)
    double *partC = nullptr;   // third partial buffer (scratch C)
    double *ctrl = nullptr;    // [2][C_NCTRL]
    double *lsres = nullptr;   // [2][LS_N]
    double *par = nullptr;     // [P_NPAR]
    double *gram = nullptr;    // gram partials
    double *rec = nullptr;     // [m][4] per-constraint {A(RR^T), q1, q2, -lam - rho b}
    double *cgc = nullptr;     // [8] device CG control (CgIdx)
    double *tot = nullptr;     // [32] sharded solve: summed stage totals (A: 0..7, B: 16..25)
    double *gl = nullptr;      // latency kernels: partial gradients of the dense rows' slices [slices][ld]
    long gl_len = 0;
};

// ---------------------------- launchers -----------------------------------
// All launchers enqueue on `st` and return hipSuccess / an error code.

// uvt_out0[slot] (and uvt_out1) over the cone's pattern; objective partials
// sum_slot Cw*uvt -> part[0 or 1][pblk_off + b].  mode: 0 = sym(X Y^T),
// 1 = X X^T (Y ignored), 2 = sym(X Y^T) into out0 and Y Y^T into out1.
int launch_sddmm(const DevProblem &P, int cone, int mode, const double *X, const double *Y,
                 double *out0, double *out1, double *part, int pblk_off, int *nblk_used,
                 hipStream_t st);
// out[i] = scale * sum_e w_e uvt[slot_e] for every constraint (A(.)), plus
// partial sum of (b - out)^2 if vio_part != nullptr (primal residual).
int launch_gather(const DevProblem &P, const double *uvt, double scale, double *out,
                  const double *b_for_vio, double *vio_part, hipStream_t st, int *nblk_used);
// Constraint-entry A(.) of one cone without the pattern pass: every constraint's
// entries of cone `cone` read their two factor rows directly (mode 0: sym(X Y^T),
// mode 1: X X^T).  out[i] = (accumulate ? out[i] : 0) + scale * value_of_this_cone; optional
// residual sum (b - out)^2 -> tmpfin TF_GATHER.  Bitwise equal to sddmm + gather_cone.
int launch_auv_con(const DevProblem &P, int cone, int mode, const double *X, const double *Y, double scale,
                   int accumulate, double *out, const double *b_for_vio, double *vio_part, hipStream_t st,
                   const double *guard = nullptr, double *sum_upd = nullptr);   // sum_upd[i] += new - old out[i]
// <C, sym(X Y^T)> (mode 0) or <C, X X^T> (mode 1) of a cone with constraint-entry tiles over
// its C entries only (DevCone::cobj_slot), into tmpfin TF_SD + 2 cone (as launch_sddmm's sums)
int launch_cobj(const DevProblem &P, int cone, int mode, const double *X, const double *Y, double *part,
                hipStream_t st);
// S[slot] = (withC ? Craw[slot] : 0) + sum_(con,a) w[con] * a
int launch_wsum(const DevProblem &P, const double *w, int withC, double *S, hipStream_t st);
// out = scale * S X (+ addX * X) per cone, partial ||out||^2 -> part[0][pblk_off+b]
int launch_spmm(const DevProblem &P, int cone, const double *S, const double *X, double scale,
                const double *addX, double addScale, double *out, double *part, int pblk_off,
                int *nblk_used, hipStream_t st);
// generic BLAS-1 over the factor buffer / m-vectors with partial dots
int launch_axpby(long n, double a, const double *x, double b, double *y, hipStream_t st);
int launch_dot(long n, const double *x, const double *y, double *part, hipStream_t st, int *nblk_used,
               int fin = TF_DOT);
int launch_fill(long n, double v, double *x, hipStream_t st);
// lam += rho (b - cvs)
int launch_dual_update(const DevProblem &P, double rho, double *lam, const double *cvs, hipStream_t st);
// M1 = -lam - rho b + rho cvs   (ALMSetGrad, lorads_alm.c:38-50)
int launch_alm_m1(const DevProblem &P, double rho, const double *lam, const double *cvs, double *M1,
                  hipStream_t st);
// r x r Gram X^T X (avg=0) or ((U+V)/2)^T((U+V)/2) (avg=1) of one cone, one launch:
// gram[0, r*r) <- the Gram, gram[r*r, ...) chunk partials (gram_buf_len(rmax) doubles)
constexpr int kGramMaxChunks = 64;
size_t gram_buf_len(int rmax);
int launch_gram(const DevProblem &P, int cone, const double *X, const double *Y, int avg,
                double *gram, int *nblk_used, hipStream_t st, bool reduce = true);
// Y = X Q on one cone's rows (k_rot): X (or (X + X2)/2, X2 non-null) n x ld
// row-major with rp = 4 ceil(r / 4) <= ld columns read, Q row-major rp x rot_q_ld(ldn) (zero rows
// past r, zero columns past k), Y n x ldn row-major, columns [k, ldn) written 0.  The pointers are
// the cone's own rows (no cone offset is added).  rot_q_ld: Q's row pitch for an output pitch ldn.
int rot_q_ld(int ldn);
int launch_rot(int n, int r, int ld, int k, int ldn, const double *X, const double *X2, const double *Q,
               double *Y, hipStream_t st);
// sustained v_mfma_f64_16x16x4f64 rate: every CU, 2 waves a SIMD, 8 accumulators a wave
int mfma_f64_peak(hipStream_t st, double *tflops);
int mfma_f64_probe(hipStream_t st, int wps, int chains, double *tflops, double *mhz, double *cyc_per_mfma);
int wave_tsum_probe(hipStream_t st, int form, int nv, int n, const double *in, double *ref, double *out);
// dense objective of cone `cone` (DevCone::Cd): Y = scale C X + beta Y on the cone's rows
// (X, Y full factor buffers; columns r..ld of Y written 0)
int launch_dense_cx(const DevProblem &P, int cone, const double *X, double *Y, double beta, hipStream_t st);
// ALM iteration, between stage A and B: CD = scale C D of every dense cone, and the partials
// <R, CD>, <D, CD> (slots 0, 1 of 8) of stage A's objective terms at partial offset `off`
// (R: the current iterate by the control block); returns the partial blocks written
// dense constraint coefficients of cone `cone` (DevCone::dA, kd matrices; lrs_kernels.hip
// "dense constraint coefficients").  launch_dcon_ax: T_i = A_i X for the nmat matrices at A
// (the cone's stack, or one n x n matrix), X / Z full factor buffers; the tiles' partial dots
// <X, T_i>, <Z, T_i> into dpart (2 nmat dcon_tiles doubles); T (optional) cone-local, matrix i
// at T + i n ld.  launch_dcon_fin: the partials per matrix in tile order, out0[con_i] (+)= s0
// <X, T_i>, out1[con_i] (+)= s1 <Z, T_i>, out1b[con_i] += s1 <Z, T_i> (each optional).
int dcon_tiles(const DevCone &c);
int launch_dcon_ax(const DevProblem &P, int cone, int nmat, const double *A, const double *X, const double *Z,
                   double *T, double *dpart, hipStream_t st);
int launch_dcon_fin(const DevProblem &P, int cone, const double *dpart, double s0, double *out0, double s1,
                    double *out1, double *out1b, int accumulate, hipStream_t st);
// Sd (n x n) = sum_i w[con_i] A_i, i ascending
int launch_dcon_wsum(const DevProblem &P, int cone, const double *w, double *Sd, hipStream_t st);
// out rows of the cone = beta out + scale sum_i w[con_i] T_i (out, dotx full factor buffers);
// with dotx and part: the blocks' partial <dotx, out> in part[0 .. *nblk)
int launch_dcon_comb(const DevProblem &P, int cone, const double *w, const double *T, double scale, double beta,
                     double *out, const double *dotx, double *part, int *nblk, hipStream_t st);
// out[con_i] (+)= <p, T_i>, outb[con_i] += it (optional)
int launch_dcon_dots(const DevProblem &P, int cone, const double *T, const double *p, double *out, double *outb,
                     int accumulate, hipStream_t st);
// rank-one dense coefficients of a cone (DevCone::rV, rp terms; lrs_kernels.hip "rank-one dense
// coefficients").  launch_r1_vtx: Tx = V^T X and, with Z, Tz = V^T Z in the same
// pass over V (X, Z cone-local, n x ld, r columns; Tx, Tz rldp x ld); part: r1_part_len doubles.
// launch_r1_vals: per term t, v0 = sigma_t <Tx_t, Tx_t>, v1 = sigma_t <Tx_t, Tz_t> (Tz null: Tx);
// out0[con_t] (+)= s0 v0, out1[con_t] (+)= s1 v1, out1b[con_t] += s1 v1 (each optional), a
// constraint's terms in index order.  launch_r1_apply: out = beta out + scale V diag(w[con_t]
// sigma_t) T on the cone's rows (out, dotx cone-local); with dotx and part: the blocks' partial
// <dotx, out> in part[0 .. *nblk) (launch_cg_mv's layout).
long r1_part_len(const DevCone &c, int r);
int launch_r1_vtx(const DevCone &c, int r, int ld, const double *X, const double *Z, double *Tx, double *Tz,
                  double *part, hipStream_t st);
int launch_r1_vals(const DevCone &c, int r, int ld, const double *Tx, const double *Tz, double s0, double *out0,
                   double s1, double *out1, double *out1b, int accumulate, hipStream_t st);
int launch_r1_apply(const DevCone &c, int r, int ld, const double *w, const double *T, double scale, double beta,
                    double *out, const double *dotx, double *part, int *nblk, hipStream_t st);
int dense_cd_blocks(const DevProblem &P);
int launch_dense_cd(const DevProblem &P, const DevWork &W, const double *ctrl, int off, hipStream_t st);

// ---- fused ALM inner iteration (device-side control; see lrs_kernels.hip) ----
struct AlmIterArgs {
    const DevProblem *P;
    DevWork *W;
    hipEvent_t *ev;    // optional: 5 events recorded before S1..S4 and after S4
    double *hmirror = nullptr;   // optional: device pointer of a pinned host slot; stage B
    double seq = 0;              // mirrors the control block there, then writes seq after it
};
// Four launches per inner iteration (lrs_kernels.hip "split iteration").
int enqueue_alm_iteration(const AlmIterArgs &a, int parity, hipStream_t st);
// whether stage A is split into direction + SDDMM launches (bandwidth regime)
bool alm_stage_a_split(const DevProblem &P);
bool alm_stage_b_split(const DevProblem &P);   // stage B likewise (line search + update, gradient)
// a subset of the stages (mask bit 0 = A, 1 = G, 2 = B), for per-stage timing
int enqueue_alm_stages(const AlmIterArgs &a, int parity, int mask, hipStream_t st);

// ---- single-workgroup persistent inner loop (lrs_kernels.hip "Single-workgroup"): small
// problems (R and D of every cone in one CU's LDS, ld <= 64, no full dense C) ----
bool small_alm_fits(const DevProblem &P, DevWork &W);
// workgroups of the single-workgroup inner loop for this problem (> 1: one per cone, the
// exchanges between them), 0 when it does not fit
int small_alm_workgroups(const DevProblem &P, DevWork &W);
int launch_small_alm(const DevProblem &P, DevWork &W, const double *ctrl_in, double *ctrl_out, double *ls_out,
                     hipStream_t st);
// The same loop for many contexts at once (lrs_solve_batch): member i's launch
// arguments as launch_small_alm would form them, the launches combined by kernel instantiation,
// one block a member.  host_ctrl receives the member's final control block (C_NCTRL doubles).
// launch_small_alm_batch returns when the round's launches and copies have completed; the
// members' streams must be idle.  *launches is advanced by the combined launches made, *widest
// raised to the largest one's blocks.
struct SmallBatch;
struct SmallBatchMember {
    const DevProblem *P;
    DevWork *W;
    const double *ctrl_in;
    double *ctrl_out, *ls_out, *host_ctrl;
};
int small_batch_create(SmallBatch **out, int cap);
void small_batch_destroy(SmallBatch *b);
int launch_small_alm_batch(SmallBatch *b, const SmallBatchMember *mem, int n, int *launches);
// The ADMM iterations of many contexts at once (the batch's ADMM rendezvous): member i's two
// half-step launches and its evaluation launch as admm_update_var / admm_eval form them
// (small_admm_fits: every cone on k_small_cg with one variant, k_small_eval), combined into a
// side-0 and a side-1 launch per kernel variant and one evaluation launch, a block a cone, each
// bitwise the member's own.  host_tot receives the member's evaluation sums ([K][4], three used),
// host_cg its W.cgc[CG_TOTAL].  Returns when the round's streams (its own, not the ALM round's)
// have drained; the members' streams must be idle.  *launches is advanced by the launches made.
struct SmallAdmmMember {
    const DevProblem *P;
    DevWork *W;
    double rho, tol;
    int maxit;
    double *host_tot, *host_cg;
};
bool small_admm_fits(const DevProblem &P);
int launch_small_admm_batch(SmallBatch *b, const SmallAdmmMember *mem, int n, int *launches);
// since small_admm_batch_reset: the most kernel variants in one round, the most blocks in one launch
void small_admm_batch_shape(const SmallBatch *b, int *variants, int *blocks);
void small_admm_batch_reset(SmallBatch *b);

// ---- device-resident CG (lrs_kernels.hip "Device-resident CG") ----
enum CgIdx { CG_ACTIVE = 0, CG_ITERS, CG_BNORM, CG_RR, CG_QTR0, CG_QTR1, CG_TOTAL, CG_N = 8 };
int launch_cg_mv(const DevProblem &P, int cone, const double *w, const double *V, const double *Xin, double *Q,
                 double *part, const double *cgc, int guarded, hipStream_t st, int *nblk);
int launch_cg_nrm1(long nr, const double *b, double *part, hipStream_t st, int *nblk);
int launch_cg_upd(long nr, double *X, double *r, const double *p, const double *Q, const double *partB, int nblkB,
                  double *partC, double *cgc, int par, int it, hipStream_t st, int *nblk);
int launch_cg_conv(long nr, const double *r, double *p, const double *partC, int nblkC, double *cgc, double tol,
                   int par, int restart, hipStream_t st);
int launch_cg_resid(long nr, const double *b, const double *Q, double *r, double *p, double *partC, double *cgc,
                    const double *partA, int nblkA, int init, hipStream_t st, int *nblk);
int launch_cg_resid2(long nr, const double *r, double *p, const double *partC, int nblkC, double *cgc, double tol,
                     int par, int init, hipStream_t st);
// single-workgroup ADMM half-step of cone `cone` (LORADSUpdateSDPVarOne + CGSolve + the cone's
// constraint refresh, one launch): side 0 solves U with V fixed, 1 V with U fixed; the RHS into
// W.cg_b, this solve's CG iterations into W.cgc[CG_ITERS], added to W.cgc[CG_TOTAL]
bool small_cg_fits(const DevProblem &P, int cone);
int launch_small_cg(const DevProblem &P, DevWork &W, int cone, int side, double rho, double tol, int maxit,
                    hipStream_t st);
// every cone's half-step of one side in one launch (a block a cone; cones whose constraints
// each lie in one cone, all fitting k_small_cg with the same variant)
bool small_cg_batch_fits(const DevProblem &P);
// the ADMM iteration's evaluation (R = (U + V) / 2, A(R R^T) into cvs / cvc, and per cone
// {sum (b - A(X))^2, <C, R R^T>, b^T lambda} into out[4k..]) in one launch, a block a cone
bool small_eval_fits(const DevProblem &P);
int launch_small_eval(const DevProblem &P, DevWork &W, const double *U, const double *V, double *out, hipStream_t st);
// the LP block's ADMM update: the reference's closed-form column sweep (k_lp_admm), both sides
int launch_lp_admm(const DevProblem &P, DevWork &W, double rho, hipStream_t st);
long lp_sweep_scratch(const DevProblem &P);
// which variant the next launch takes (1 operands staged in LDS, 0 the global-memory walk) under
// the current LRS_LP_LDS_MAX, and the LDS bytes the staged variant needs for this problem
void lp_sweep_plan(const DevProblem &P, int *staged, long *lds_bytes);
int launch_small_cg_batch(const DevProblem &P, DevWork &W, int side, double rho, double tol, int maxit,
                          hipStream_t st);

// ---- sign rounding of a factor (lrs_kernels.hip "Sign rounding") ----
// T trials (a multiple of 64) of one cone, their signs as bit words bits[T / 64][n] (bit t of
// word w: trial 64 w + t, set = +1).  launch_round_prep: wadj[e] = Craw[slot_e] sb[i] sb[j] per
// adjacency entry (Craw the unscaled slot values, sb[n] = sqrt(b_i)).  launch_round_proj: the
// signs of X dirT (X the cone's rows, n x ld; dirT r x T row-major).  launch_round_value:
// values[t] = <C, x_t x_t^T> through part (T round_chunks(n) doubles), summed in chunk order.
// launch_round_descent: Gauss-Seidel one-flip descent on the words in place, at most max_sweeps
// sweeps; sweeps[T / 64] = the sweeps each word's wave ran.
int round_chunks(int n);
int launch_round_prep(const DevCone &c, const double *Craw, const double *sb, double *wadj, hipStream_t st);
int launch_round_proj(const DevCone &c, const double *X, int T, const double *dirT, unsigned long long *bits,
                      hipStream_t st);
int launch_round_value(const DevCone &c, int T, const double *wadj, const unsigned long long *bits, double *part,
                       double *values, hipStream_t st);
int launch_round_descent(const DevCone &c, int T, const double *wadj, unsigned long long *bits, int max_sweeps,
                         int *sweeps, hipStream_t st);

// ---- triangle-inequality separation (lrs_kernels.hip "Triangle-inequality separation") ----
// launch_tri_gram: x = D^-1/2 X X^T D^-1/2 of one cone (X its rows, n x ld; sb[n] = sqrt(b_i)) as a
// full tri_pad(n)^2 matrix, zero past n.  launch_tri_scan: one pass over every i < j < k and type
// with v > minv.  Its key is 128 bits: hi = ~bits(v), lo = ((i n + j) n + k) 4 + type.  mode 0:
// gcnt[0] += the count, gcnt[1] = max bits(v), ghist[d] += the keys whose digit (hi >> shift) &
// mask is d.  mode 1: the same histogram of part's (0: hi, 1: lo) digit over the keys with
// (part >> pshift) == prefix (part 1: and hi == fixed_hi).  mode 2: the records {bits(v), lo} with
// (part >> pshift) <= prefix (part 1: hi < fixed_hi, or equal and that) appended to rec[cap] at
// *cursor, which keeps counting past cap.  The caller zeroes ghist, gcnt and cursor.
constexpr int kTriTile = 32;      // tile edge of the scan (why not 64)
constexpr int kTriBins = 4096;    // a radix digit is at most 12 bits
struct TriPass {
    unsigned long long prefix, fixed_hi;
    int part, pshift, shift;
    unsigned mask, cap;
};
int tri_pad(int n);
int launch_tri_gram(const DevCone &c, const double *X, const double *sb, double *x, hipStream_t st);
int launch_tri_scan(int mode, int n, double minv, const TriPass &P, const double *x, unsigned long long *ghist,
                    unsigned long long *gcnt, unsigned *cursor, void *rec, hipStream_t st);

// ---- registered triangle cuts (lrs_kernels.hip "Registered triangle cuts") ----
// launch_cut_state: for the T cuts {i, j, k, type} (i < j < k < n, 16-byte aligned) at the cone's
// rows X (n x ld, r columns read) with sb[n] = sqrt(b_i): slack[t] = 1 + sigma . x in
// k_tri_gram's and k_tri_scan's arithmetic (bitwise minus the separation's violation), and, where
// the pointers are given, lam_out[t] = lam_in[t], lp_out[t] = lp_in[t ldlp].  launch_cut_carry:
// lam[t] = src[t] >= 0 ? lam_old[src[t]] : 0; lp[t ldlp] = (src[t] >= 0 && keep_lp) ?
// lp_old[src[t]] : sqrt(max(slack[t], 0)).
int launch_cut_state(int T, int r, int ld, const int *cuts, const double *X, const double *sb, const double *lam_in,
                     const double *lp_in, int ldlp, double *slack, double *lam_out, double *lp_out, hipStream_t st);
int launch_cut_carry(int T, const double *slack, const int *src, const double *lam_old, const double *lp_old,
                     int keep_lp, double *lam, double *lp, int ldlp, hipStream_t st);

// ---- dual infeasibility (Lanczos for lambda_min of S per cone) ----
// y = S x over one cone's adjacency (S on the global slots, x / y cone-local vectors)
int launch_symv(const DevProblem &P, int cone, const double *S, const double *x, double *y, hipStream_t st);
// w -= Q (Q^T w): Q column-major n x k (leading dimension ldq); part >= 64 k doubles, h >= k
int launch_reorth(int n, int k, const double *Q, long ldq, double *w, double *part, double *h, hipStream_t st);
// thick-restart Lanczos (ARPACK dsaupd semantics, lrs_solver.cpp trl_min): one step's launches.
// Vectors are cone-local rows; norm / dots / sub / restart take pointers pre-offset to the first
// owned row and n = owned rows; symv runs the cone's owned rows [row0, row0 + nown) itself.
constexpr int kTrlMaxV = 64;   // basis vectors at most (ncv = 40 in the reference)
int trl_nblk(int n);           // partial blocks per column of launch_trl_dots
int launch_trl_norm(int n, const double *w, const double *b2, double *vj, hipStream_t st);
// y = S (x / sqrt(*b2)) (+ scale C v on a dense cone); vj (optional) = x / sqrt(*b2); b2 = null: 1
int launch_trl_symv(const DevProblem &P, int cone, const double *S, const double *x, const double *b2, double *vj,
                    double *y, hipStream_t st);
int launch_trl_dots(int n, const double *V, long ldv, int k, const double *y, double *part, hipStream_t st);
int launch_trl_fold(int k, int nb, const double *part, double *tot, hipStream_t st);
int launch_trl_sub(int n, const double *V, long ldv, int k, const double *part, int nb, double *y, double *Hc,
                   int pass, double *npart, double *bw2, hipStream_t st);
int launch_trl_restart(int n, const double *V, long ldv, int m, const double *Y, int kk, double *Vt, hipStream_t st);

// per-context scratch of the standalone reductions for the calling thread (no module-level fallback)
void bind_scratch(unsigned *tickets, double *tmpfin, double *rpart, double *fin);
// sharded solve helpers
int launch_pack_rows(int nrows, int ld, const int *rows, const double *src, double *dst, hipStream_t st);
// sharded: sum an m-vector's shared-constraint entries over the shards (no-op otherwise)
int sync_shared(const DevProblem &P, double *v, hipStream_t st);
// fold one scalar's per-block partials into out[0] (sharded CG, before its all-reduce)
int launch_fold1(const double *part, int nblk, double *out, hipStream_t st);
// par[P_NPAR] and ctl[C_NCTRL] (host arrays) into dpar / dctl, stream-ordered, as one launch
int launch_put_ctrl(const double *par, const double *ctl, double *dpar, double *dctl, hipStream_t st);
int launch_sum_shards(int n, int world, const double *const *src, double *out, hipStream_t st);

const char *last_device_error();
// diagnostics build only: copies g_phase[4][16] (returns 64), else returns 0
int read_phase_times(unsigned long long *out, unsigned long long *blk);

}  // namespace lrs

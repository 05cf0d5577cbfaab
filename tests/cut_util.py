"""NumPy restatements for the cutting-plane loop (include/lrsdp.h lrs_cuts_*, lrs_certified_bound,
DESIGN.md §4.14) for the tests.  They read a problem in the (m, dims, b, entries) form of
instances.py -- the plain MaxCut-class problem or instances.add_triangle_cuts' output -- a factor and
a vector of multipliers, never the device."""
import numpy as np

import tri_util as tu


def flat_entries(problem):
    """The problem's entries as a list of (con, blk, i, j, v), 1-based as in the file."""
    out = []
    for con, blk, ii, jj, vv in problem[3]:
        con = np.asarray(con)
        blk = np.broadcast_to(np.asarray(blk), con.shape)
        out += list(zip(con.tolist(), blk.tolist(), np.asarray(ii).tolist(), np.asarray(jj).tolist(),
                        np.asarray(vv, dtype=float).tolist()))
    return out


def slack(X, b, cuts):
    """slack_t = 1 + ((s_ij x_ij + s_ik x_ik) + s_jk x_jk) for the rows {i, j, k, type} of cuts."""
    x = tu.xmat(X, b)
    cuts = np.asarray(cuts, dtype=np.int64).reshape(-1, 4)
    i, j, k, ty = cuts.T
    s = tu.SIGNS[ty]
    return 1.0 + ((s[:, 0] * x[i, j] + s[:, 1] * x[i, k]) + s[:, 2] * x[j, k])


def dense_S(problem, lam):
    """S = C - sum_i lam_i A_i on the SDP block (block 1) as a full symmetric matrix, from the
    file's entries: C = -F0, an off-diagonal entry stands for both triangles."""
    m, dims, _, _ = problem
    n = int(dims[0])
    lam = np.asarray(lam, dtype=np.float64)
    assert lam.shape == (m,)
    S = np.zeros((n, n))
    for con, blk, i, j, v in flat_entries(problem):
        if blk != 1:
            continue
        w = -v if con == 0 else -lam[con - 1] * v
        S[i - 1, j - 1] += w
        if i != j:
            S[j - 1, i - 1] += w
    return S


def lp_dual_slack(problem, lam):
    """The LP block's dual slacks c_j - sum_i lam_i a_ij by column (empty without an LP block)."""
    m, dims, _, _ = problem
    if len(dims) < 2:
        return np.zeros(0)
    z = np.zeros(-int(dims[1]))
    for con, blk, i, j, v in flat_entries(problem):
        if blk == 2:
            z[i - 1] += -v if con == 0 else -np.asarray(lam)[con - 1] * v
    return z


def bound(problem, lam, m0=None):
    """(bound, lambda_min): b^T lam + (sum_i b_i) min(0, lambda_min(S)) + 4 sum_t min(0, lam_{m0 + t})
    with lambda_min from eigvalsh of the dense S; m0 (default: the SDP block's size) the number of
    diagonal constraints, each X_ii = b_i with coefficient 1."""
    m, dims, b, _ = problem
    n = int(dims[0])
    m0 = n if m0 is None else m0
    lam = np.asarray(lam, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    lmin = float(np.linalg.eigvalsh(dense_S(problem, lam))[0])
    val = float(b @ lam) + float(b[:n].sum()) * min(0.0, lmin) + 4.0 * float(np.minimum(lam[m0:], 0.0).sum())
    return val, lmin

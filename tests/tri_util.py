"""NumPy restatement of the triangle-inequality separation (include/lrsdp.h
lrs_separate_triangles) for the tests.  It reads the instance file and a factor,
never the device: b comes from the SDPA entries, x = D^-1/2 X X^T D^-1/2 from the factor, and all
4 C(n, 3) violations are formed at once, so it is for small n only."""
import numpy as np

import round_util as ru

# sign of x_ij, x_ik, x_jk per type
SIGNS = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])


def diag_b(path, cone=0):
    """b_i by row of a diagonally constrained cone of the file."""
    return ru.cone_data(path, cone)["b"]


def xmat(X, b):
    """x_ij = <X_i, X_j> / (sqrt(b_i) sqrt(b_j))."""
    sb = np.sqrt(np.asarray(b, dtype=np.float64))
    return (X @ X.T) / np.outer(sb, sb)


def triples(n):
    """All i < j < k as three arrays, in lexicographic order."""
    ii, jj, kk = [], [], []
    for i in range(n - 2):
        a, c = np.triu_indices(n - i - 1, 1)
        ii.append(np.full(a.size, i, dtype=np.int64))
        jj.append(a + i + 1)
        kk.append(c + i + 1)
    return np.concatenate(ii), np.concatenate(jj), np.concatenate(kk)


def all_violations(X, b):
    """(i, j, k, v): v[t, type] = -1 - ((s_ij x_ij + s_ik x_ik) + s_jk x_jk) for every triple t, in
    the order of the header's formula; flattened row-major, v is in ascending (i, j, k, type)."""
    x = xmat(X, b)
    i, j, k = triples(X.shape[0])
    a, bb, c = x[i, j], x[i, k], x[j, k]
    v = np.empty((i.size, 4))
    for ty in range(4):
        s = SIGNS[ty]
        v[:, ty] = -1.0 - ((s[0] * a + s[1] * bb) + s[2] * c)
    return i, j, k, v


def separate(X, b, max_cuts, min_violation=0.0):
    """(cuts (n_cuts, 4) int32, violation (n_cuts,), n_violated, max_violation) under the total
    order: v descending, then (i, j, k, type) ascending."""
    i, j, k, v = all_violations(X, b)
    flat = v.ravel()
    q = np.flatnonzero(flat > min_violation)          # ascending index
    order = q[np.argsort(-flat[q], kind="stable")]    # stable: ties keep the ascending index
    top = order[:max_cuts]
    t, ty = top // 4, top % 4
    cuts = np.stack([i[t], j[t], k[t], ty], axis=1).astype(np.int32).reshape(-1, 4)
    return cuts, flat[top].copy(), int(q.size), float(flat[q].max()) if q.size else 0.0


def margin(X, b, max_cuts, min_violation=0.0):
    """(gap, dist): the smallest difference between neighbours among the first max_cuts + 1
    qualifying violations in sorted order (inf with fewer than two), and the smallest distance of
    any of the 4 C(n, 3) violations from min_violation.  Both far above the rounding error of a
    violation means that the order and the count cannot depend on the summation order."""
    flat = all_violations(X, b)[3].ravel()
    qual = np.sort(flat[flat > min_violation])[::-1][:max_cuts + 1]
    gap = float(np.min(-np.diff(qual))) if qual.size > 1 else float("inf")
    return gap, float(np.abs(flat - min_violation).min())


def rounding_bound(r):
    """|device - restatement| on one violation for rows of norm sqrt(b_i): three dots of r products
    and two additions (the issue's bound)."""
    return 3.0 * (r + 4) * 2.0 ** -52


def brute_force_min(cd):
    """min over x in {-1, +1}^n of <C, x x^T> from round_util.cone_data's objective entries (b = 1),
    by enumeration with x_0 = +1 (n <= 21 or so)."""
    n = cd["n"]
    codes = np.arange(1 << (n - 1), dtype=np.int64)
    S = np.ones((n, codes.size), dtype=np.int8)
    for i in range(1, n):
        S[i] = 1 - 2 * ((codes >> (i - 1)) & 1)
    val = np.zeros(codes.size)
    for i, j, v in zip(cd["ci"], cd["cj"], cd["cv"]):
        val += (v if i == j else 2.0 * v) * (S[i] * S[j])
    return float(val.min())

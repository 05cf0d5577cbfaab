"""NumPy restatement of the sign rounding (include/lrsdp.h lrs_round_signs) for
the tests.  It reads the instance file, never the device: C = -F0 and b come from the SDPA
entries, the signs from R @ dirs, the descent is the sequential sweep per trial."""
import numpy as np

M64 = (1 << 64) - 1


def read_sdpa(path):
    """(m, dims, b, entries) of a plain .dat-s file; entries: list of (con, blk, i, j, v), 1-based."""
    with open(path) as f:
        lines = [ln for ln in f if ln.strip() and ln[0] not in '*"']
    tok = lambda s: s.replace("{", " ").replace("}", " ").replace("(", " ").replace(")", " ").replace(",", " ").split()
    m = int(tok(lines[0])[0])
    nblk = int(tok(lines[1])[0])
    dims = [int(t) for t in tok(lines[2])[:nblk]]
    b = np.array([float(t) for t in tok(lines[3])[:m]])
    ents = []
    for ln in lines[4:]:
        t = tok(ln)
        ents.append((int(t[0]), int(t[1]), int(t[2]), int(t[3]), float(t[4])))
    return m, dims, b, ents


def cone_data(path, cone=0):
    """The rounding's view of cone `cone`: n, sb = sqrt(b_i) by row, and the objective's lower
    entries (row >= col, merged, columns ascending per row) as arrays ci, cj, cv with C = -F0."""
    m, dims, b, ents = read_sdpa(path)
    n = dims[cone]
    C = {}
    brow = np.full(n, np.nan)
    for con, blk, i, j, v in ents:
        if blk != cone + 1 or abs(v) < 1e-12:
            continue
        i, j = max(i, j) - 1, min(i, j) - 1
        if con == 0:
            C[(i, j)] = C.get((i, j), 0.0) - v
        else:
            assert i == j and v == 1.0 and np.isnan(brow[i]), "not a diagonally constrained cone"
            brow[i] = b[con - 1]
    assert not np.isnan(brow).any() and (brow > 0).all()
    keys = sorted(C)
    ci = np.array([k[0] for k in keys], dtype=np.int64)
    cj = np.array([k[1] for k in keys], dtype=np.int64)
    cv = np.array([C[k] for k in keys])
    return dict(n=n, sb=np.sqrt(brow), b=brow, ci=ci, cj=cj, cv=cv)


def margin(R, dirs):
    """min over (i, t) of |<R_i, g_t>| / (|R_i| |g_t|): how far every sign is from a tie."""
    P = np.abs(R @ dirs)
    P /= np.linalg.norm(R, axis=1)[:, None]
    P /= np.linalg.norm(dirs, axis=0)[None, :]
    return float(P.min())


def signs(R, dirs):
    """(n, T) array of +-1: +1 where <R_i, g_t> >= 0."""
    return np.where(R @ dirs >= 0, 1.0, -1.0)


def values(cd, S):
    """value_t = sum_i C_ii b_i + 2 sum_{j<i} C_ij sqrt(b_i b_j) s_i s_j for the columns of S."""
    w = np.where(cd["ci"] == cd["cj"], 1.0, 2.0) * cd["cv"] * (cd["sb"][cd["ci"]] * cd["sb"][cd["cj"]])
    return (w[:, None] * (S[cd["ci"]] * S[cd["cj"]])).sum(axis=0)


def adjacency(cd):
    """Per row the (column, C_ij sqrt(b_i b_j)) pairs of the symmetric objective, j != i, columns
    ascending: the order the descent sums f in."""
    adj = [[] for _ in range(cd["n"])]
    for i, j, v in zip(cd["ci"].tolist(), cd["cj"].tolist(), cd["cv"].tolist()):
        if i != j:
            w = v * (cd["sb"][i] * cd["sb"][j])
            adj[i].append((j, w))
            adj[j].append((i, w))
    return [sorted(a) for a in adj]


def descent(cd, S, max_sweeps=50):
    """The sequential one-flip descent, every trial (column of S) on its own: rows in order, f =
    sum_{j != i} C_ij sqrt(b_i b_j) s_j in column order, s_i flipped iff -4 s_i f < 0.  Returns the
    final S and the sweeps each trial used (the sweep that flips nothing counts)."""
    S = S.copy()
    adj = adjacency(cd)
    T = S.shape[1]
    used = np.zeros(T, dtype=np.int64)
    live = np.ones(T, dtype=bool)
    for _ in range(max_sweeps):
        if not live.any():
            break
        flipped = np.zeros(T, dtype=bool)
        for i in range(cd["n"]):
            f = np.zeros(T)
            for j, w in adj[i]:
                f = f + w * S[j]
            flip = live & (-4.0 * S[i] * f < 0)
            S[i, flip] = -S[i, flip]
            flipped |= flip
        used[live] += 1
        live &= flipped
    return S, used


def one_flip_gains(cd, S):
    """(n, T): the change of value_t when s_i alone is flipped, -4 s_i f_i."""
    adj = adjacency(cd)
    out = np.zeros_like(S)
    for i in range(cd["n"]):
        f = np.zeros(S.shape[1])
        for j, w in adj[i]:
            f = f + w * S[j]
        out[i] = -4.0 * S[i] * f
    return out


def bits_to_signs(bits, trials):
    """(trials // 64, n) uint64 words -> (n, trials) array of +-1 (bit set: +1)."""
    W, n = bits.shape
    S = np.empty((n, trials))
    for w in range(W):
        for t in range(64):
            S[:, 64 * w + t] = np.where((bits[w] >> np.uint64(t)) & np.uint64(1), 1.0, -1.0)
    return S


def signs_to_bits(S):
    n, T = S.shape
    bits = np.zeros((T // 64, n), dtype=np.uint64)
    for t in range(T):
        bits[t // 64] |= (S[:, t] > 0).astype(np.uint64) << np.uint64(t % 64)
    return bits


def _mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def round_dirs_py(seed, r, trials):
    """The documented generator of lrs_round_dirs, restated: an (r, trials) array."""
    import math
    out = np.empty((r, trials))
    s = _mix(seed & M64)
    for t in range(trials):
        for c in range(r):
            h = _mix(s ^ ((t << 32) + c))
            a = _mix(h)
            b = _mix(a)
            u1 = ((a >> 11) + 1) * 2.0 ** -53
            u2 = (b >> 11) * 2.0 ** -53
            out[c, t] = math.sqrt(-2.0 * math.log(u1)) * math.cos(6.283185307179586 * u2)
    return out

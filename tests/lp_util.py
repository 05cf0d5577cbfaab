"""NumPy restatement of the LP block's ADMM column sweep (the reference's
LORADSUpdateSDPLPVar LP loop, lorads_alg_common.c:356-374, and LORADSUpdateLPVarOne,
lorads_admm.c:759-792) for the tests.  Everything here reads a problem in the (m, dims, b, entries)
form of instances.py and the input vectors only, never the device.

lp_problem builds small problems with one SDP block and an LP block of given column shapes;
lp_columns derives what the sweep reads from a problem (per column its cost, its entries in
constraint order and ||a_j||^2, with the reference's column typing: a column present in >= m/4
constraints loses its entries and keeps its norm); lp_sweep walks the columns in the reference's
operation order in a chosen floating-point type; constr_values is A(U V^T) of the whole problem
(what the sweep starts from)."""
from types import SimpleNamespace

import numpy as np

EPS = float(np.finfo(np.float64).eps)


def lp_problem(n_sdp, m, cols, b=None, sdp=None, seed=0):
    """(m, dims, b, entries) with one SDP block of n_sdp rows and an LP block of len(cols) columns.

    cols: per LP column (c, ents): c its cost or None (no objective entry), ents a list of (con, a)
    with 0-based constraints, in any order, duplicates allowed (the loader sums them); (None, [])
    is a column without data.  sdp: list of (con, i, j, v), 0-based, i <= j, con = -1 the
    objective; default: a seeded diagonal objective, X_ii in constraint i for i < min(m, n_sdp)
    and an off-diagonal entry in every fifth constraint.  b: the right-hand sides (default
    seeded, in [0.5, 1.5])."""
    rng = np.random.default_rng(seed)
    if b is None:
        b = rng.uniform(0.5, 1.5, size=m)
    if sdp is None:
        sdp = [(-1, i, i, float(rng.uniform(0.5, 2.0))) for i in range(n_sdp)]
        sdp += [(i, i, i, 1.0) for i in range(min(m, n_sdp))]
        if n_sdp > 1:
            sdp += [(i, i % (n_sdp - 1), n_sdp - 1, float(rng.uniform(-1.0, 1.0))) for i in range(0, m, 5)]
    s = np.array([(con + 1, i + 1, j + 1) for con, i, j, _ in sdp], dtype=np.int64).reshape(-1, 3)
    entries = [(s[:, 0], 1, s[:, 1], s[:, 2], np.array([v for *_, v in sdp], dtype=np.float64))]
    con, col, val = [], [], []
    for j, (c, ents) in enumerate(cols):
        if c is not None:
            con.append(0); col.append(j + 1); val.append(-float(c))     # F0 = -c (the reader's C = -F0)
        for i, a in ents:
            assert 0 <= i < m
            con.append(i + 1); col.append(j + 1); val.append(float(a))
    col = np.array(col, dtype=np.int64)
    entries.append((np.array(con, dtype=np.int64), 2, col, col, np.array(val, dtype=np.float64)))
    return m, [n_sdp, -len(cols)], np.asarray(b, dtype=np.float64), entries


def read_problem(path):
    """A plain SDPA .dat-s file (one entry a line, as instances.write_sdpa writes it) in the
    (m, dims, b, entries) form."""
    with open(path) as f:
        lines = [ln for ln in f if ln.strip() and ln.lstrip()[0] not in '*"']
    m, nb = int(lines[0].split()[0]), int(lines[1].split()[0])
    dims = [int(x) for x in lines[2].replace(",", " ").split()[:nb]]
    b = np.array([float(x) for x in lines[3].replace(",", " ").split()[:m]])
    t = np.array([ln.split() for ln in lines[4:]], dtype=np.float64).reshape(-1, 5)
    ints = t[:, :4].astype(np.int64)
    return m, dims, b, [(ints[:, 0], ints[:, 1], ints[:, 2], ints[:, 3], t[:, 4])]


def _flat(problem):
    con, blk, ii, jj, vv = [], [], [], [], []
    for c, bk, i, j, v in problem[3]:
        c = np.asarray(c, dtype=np.int64).ravel()
        con.append(c)
        blk.append(np.broadcast_to(np.asarray(bk, dtype=np.int64), c.shape))
        ii.append(np.asarray(i, dtype=np.int64).ravel())
        jj.append(np.asarray(j, dtype=np.int64).ravel())
        vv.append(np.asarray(v, dtype=np.float64).ravel())
    return [np.concatenate(x) for x in (con, blk, ii, jj, vv)]


def lp_columns(problem):
    """What the sweep reads of the problem's LP block (the last block, of negative size), from the
    problem alone: n columns, c[n], con[j] / a[j] the entries of column j in constraint order with
    duplicates summed, nrm2[n] = sqrt(sum a^2)^2 over those entries, and the reference's column
    typing (lp_cone_presolve, lorads_lp_conic.c:110-133): a column present in >= m/4 constraints
    is typed dense, whose entries the reference never reads; such a column keeps nrm2 and loses
    con / a.  dense = those columns, dropped = their entries, slots = the columns that keep a cost
    entry or a constraint entry."""
    m, dims = int(problem[0]), [int(d) for d in problem[1]]
    assert dims[-1] < 0 and all(d > 0 for d in dims[:-1])
    n, lpb = -dims[-1], len(dims)
    con, blk, ii, jj, vv = _flat(problem)
    z = blk == lpb
    con, ii, jj, vv = con[z], ii[z], jj[z], vv[z]
    assert (ii == jj).all() and (1 <= ii).all() and (ii <= n).all()
    c = np.zeros(n)
    has_c = np.zeros(n, dtype=bool)
    per = [dict() for _ in range(n)]
    for q in np.argsort(con, kind="stable"):
        j, i, v = int(ii[q]) - 1, int(con[q]) - 1, float(vv[q])
        if i < 0:
            c[j] += -v
            has_c[j] = True
        else:
            per[j][i] = per[j].get(i, 0.0) + v
    cons, avals, nrm2, dense, dropped = [], [], np.zeros(n), [], 0
    for j in range(n):
        keys = sorted(per[j])
        a = np.array([per[j][i] for i in keys], dtype=np.float64)
        s = 0.0
        for x in a.tolist():
            s += x * x
        t = float(np.sqrt(np.float64(s)))
        nrm2[j] = t * t
        if keys and len(keys) / m >= 0.25:
            dense.append(j)
            dropped += len(keys)
            keys, a = [], np.zeros(0)
        cons.append(np.array(keys, dtype=np.int64))
        avals.append(a)
    slots = [j for j in range(n) if has_c[j] or cons[j].size]
    return SimpleNamespace(m=m, n=n, c=c, con=cons, a=avals, nrm2=nrm2, dense=dense, dropped=dropped, slots=slots,
                           entries=int(sum(x.size for x in cons)))


def lp_sweep(cols, b, lam, rho, u, v, cvs, dtype=np.float64):
    """The column sweep in the reference's operation order, every operation rounded to `dtype`
    (np.float64 or np.longdouble): for each column j in order, u_j with v_j fixed, the constraint
    sums refreshed, then v_j with u_j fixed, the sums refreshed.  Returns new (u, v, cvs)."""
    T = dtype
    b, lam = np.asarray(b, dtype=T), np.asarray(lam, dtype=T)
    u, v, cvs = np.array(u, dtype=T), np.array(v, dtype=T), np.array(cvs, dtype=T)
    rho, one, neg = T(rho), T(1.0), T(-1.0)
    for j in range(cols.n):
        con = cols.con[j].tolist()
        a = np.asarray(cols.a[j], dtype=T)
        c, n2 = T(cols.c[j]), T(cols.nrm2[j])
        for side in (0, 1):
            uv = u[j] * v[j]
            w = T(0.0)
            w = w + c                                    # lp_cone_ObjCoeffSum
            for q, i in enumerate(con):                  # M1_i, then LPdataMatSparseWeightSum
                m1 = -b[i]
                m1 = m1 + cvs[i]
                m1 = m1 + neg * (uv * a[q])
                m1 = m1 * rho
                m1 = m1 + neg * lam[i]
                w = w + a[q] * m1
            y = v[j] if side == 0 else u[j]
            M2 = w * y
            M2 = M2 - rho * y
            blin = neg * M2 / rho
            x = blin / (one + n2 * y * y)
            if side == 0:
                u[j] = x
            else:
                v[j] = x
            uvn = u[j] * v[j]
            for q, i in enumerate(con):                  # constrValSum -= the column's old values
                cvs[i] = cvs[i] + neg * (uv * a[q])
            for q, i in enumerate(con):                  # ... += its new ones
                cvs[i] = cvs[i] + one * (uvn * a[q])
    return u, v, cvs


def constr_values(problem, cols, U, V, rank, dtype=np.float64):
    """A(U V^T) of the whole problem in `dtype`: U, V the factors as the library takes them (each
    SDP block n x rank column-major, then the LP values); an SDP entry (i, j, a) gives
    a <u_i, v_i> on the diagonal and a (<u_i, v_j> + <u_j, v_i>) off it (the file's entry stands
    for both triangles of the symmetrised U V^T); LP column j gives a_ij u_j v_j through the typed
    columns `cols` (a dense column gives nothing).  Sums per cone in entry order, then over cones."""
    T = dtype
    m, dims = int(problem[0]), [int(d) for d in problem[1]]
    con, blk, ii, jj, vv = _flat(problem)
    out = np.zeros(m, dtype=T)
    off = 0
    for k, n in enumerate(dims[:-1]):
        Uk = np.asarray(U[off:off + n * rank], dtype=T).reshape(n, rank, order="F")
        Vk = np.asarray(V[off:off + n * rank], dtype=T).reshape(n, rank, order="F")
        off += n * rank
        acc = np.zeros(m, dtype=T)
        for q in np.nonzero((blk == k + 1) & (con > 0))[0]:
            i, j, a = int(ii[q]) - 1, int(jj[q]) - 1, T(vv[q])
            d = T(0.0)
            for p in range(rank):
                d = d + Uk[i, p] * Vk[j, p]
            if i != j:
                e = T(0.0)
                for p in range(rank):
                    e = e + Uk[j, p] * Vk[i, p]
                d = d + e
            acc[con[q] - 1] = acc[con[q] - 1] + a * d
        out = out + acc
    ul, vl = np.asarray(U[off:], dtype=T), np.asarray(V[off:], dtype=T)
    acc = np.zeros(m, dtype=T)
    for j in range(cols.n):
        uv = ul[j] * vl[j]
        for q, i in enumerate(cols.con[j].tolist()):
            acc[i] = acc[i] + T(cols.a[j][q]) * uv
    return out + acc


def rel_max(x, ref):
    """max |x - ref| relative to max(1, max |ref|), in the wider of the two types."""
    x, ref = np.asarray(x), np.asarray(ref)
    d = np.abs(x.astype(np.longdouble) - ref.astype(np.longdouble))
    return float(d.max(initial=0.0) / max(1.0, float(np.abs(ref).max(initial=0.0))))


def sweep_floor(cols, b, lam, rho, u, v, cvs):
    """(floor, (u, v, cvs) in longdouble): the largest rel_max over u, v and the constraint sums
    between the float64 and the longdouble restatement on the same inputs -- what rounding every
    operation to float64 costs on this case; the device's bar is 8 floor + 4 eps."""
    lo = lp_sweep(cols, b, lam, rho, u, v, cvs, np.float64)
    hi = lp_sweep(cols, b, lam, rho, u, v, cvs, np.longdouble)
    return max(rel_max(x, r) for x, r in zip(lo, hi)), hi


def bar(floor):
    return 8.0 * floor + 4.0 * EPS

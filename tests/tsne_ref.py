"""Host restatement of the t-SNE definition of include/srx.h (sections 1 to 5) in numpy, written from the header text and
independent of the device code: the perplexity affinities and the joint P, the uniform pyramid with Python-integer cell sums,
the walk (as a frontier of (point, cell) pairs, level by level), the attraction, the gains / momentum update, the KL pass and
the two deterministic starts.  Every DECISION is taken in f64 (the cell of a point, the accept test, the sign test of the
gains); ``dtype=np.longdouble`` widens only the arithmetic of the terms, their sums and the updates, so that
D = max |f64 - longdouble| measures rounding and not flipped decisions."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MASK = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
MAX_LEVELS = 12
COUNTERS = ("cells_accepted", "cells_exact", "pairs_exact")


def golden():
    return json.load(open(os.path.join(GOLD, "tsne_kat.json")))


def mix_int(z):
    z &= MASK
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & MASK
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & MASK
    return z ^ (z >> 31)


# ---- 5. starts ---------------------------------------------------------------------------------------------------------------------
def random_start(n, seed):
    c = np.array([((mix_int(seed + G * (c + 1)) >> 11) * 2.0 ** -53 - 0.5) * 2e-4 for c in range(2 * n)], dtype=np.float64)
    return c.reshape(n, 2)


def pca_start(scores):
    s = np.asarray(scores, dtype=np.float64)[:, :2]
    return s * (1e-4 / np.abs(s).max())


# ---- 1. affinities -----------------------------------------------------------------------------------------------------------------
def default_perplexity(k):
    return min(30.0, k / 3.0)


def entropy(x, beta):
    """H(beta) of rows x = D - m (rows x k), beta one per row: log S + beta * sum(x e) / S."""
    e = np.exp(-(beta[:, None] * x))
    S = e.sum(axis=1)
    return np.log(S) + beta * (x * e).sum(axis=1) / S


def conditional(idx, dist, u):
    """Rows in column order.  Returns (cols n x k, p n x k, beta n, info) with info["bound"] the per-row factor
    max_j |dp_j / dH| (inf where the row has no root) that turns an error in H into one in p."""
    idx = np.asarray(idx, dtype=np.int64)
    dist = np.asarray(dist, dtype=np.float64)
    n, k = idx.shape
    order = np.argsort(idx, axis=1, kind="stable")
    cols = np.take_along_axis(idx, order, axis=1)
    d = np.take_along_axis(dist, order, axis=1)
    D = d * d
    m = D.min(axis=1)
    tie = D == m[:, None]
    c = tie.sum(axis=1)
    x = D - m[:, None]
    logu = np.log(np.float64(u))
    root = c < u
    p = np.where(tie, 1.0 / c[:, None], 0.0)
    beta = np.full(n, np.inf)
    bound = np.full(n, np.inf)
    r = np.flatnonzero(root)
    if r.size:
        xr = x[r]
        lo, hi = np.ones(r.size), np.ones(r.size)
        with np.errstate(over="ignore", under="ignore"):
            H = entropy(xr, lo)
            up = H > logu
            for _ in range(2200):                       # bracket by factors of two
                g = up & (entropy(xr, hi) > logu) & (hi < 1e300)
                if not g.any():
                    break
                lo[g] = hi[g]
                hi[g] = hi[g] * 2.0
            for _ in range(2200):
                g = ~up & (entropy(xr, lo) <= logu) & (lo > 1e-300)
                if not g.any():
                    break
                hi[g] = lo[g]
                lo[g] = lo[g] * 0.5
            for _ in range(200):                        # bisection to the last bit of the bracket
                mid = lo + 0.5 * (hi - lo)
                Hm = entropy(xr, mid)
                g = Hm > logu
                lo = np.where(g, mid, lo)
                hi = np.where(g, hi, mid)
            b = lo + 0.5 * (hi - lo)
            e = np.exp(-(b[:, None] * xr))
            pr = e / e.sum(axis=1)[:, None]
        beta[r] = b
        p[r] = pr
        ED = (pr * xr).sum(axis=1)
        var = (pr * (xr - ED[:, None]) ** 2).sum(axis=1)
        dp = pr * (ED[:, None] - xr)                    # dp_j / dbeta
        with np.errstate(divide="ignore", invalid="ignore"):
            bound[r] = np.abs(dp).max(axis=1) / (b * var)          # |dH / dbeta| = beta Var_p(D)
    return cols, p, beta, {"rows_no_root": int((~root).sum()), "bound": bound, "x": x, "root": root}


def row_entropy(x, beta):
    """H of single rows from a fetched beta (the test's own check of |H - log u| <= 1e-9)."""
    with np.errstate(over="ignore", under="ignore"):
        return entropy(x, beta)


# ---- 2. joint P ----------------------------------------------------------------------------------------------------------------------
def joint(cols, p, n):
    """(indptr, indices, data, info) of P = (p + p^T) / (2 n) on the union pattern, zeros dropped (dense: n is small here)."""
    A = np.zeros((n, n))
    M = np.zeros((n, n), dtype=bool)
    rows = np.repeat(np.arange(n), cols.shape[1])
    A[rows, cols.ravel()] = p.ravel()
    M[rows, cols.ravel()] = True
    U = M | M.T
    P = (A + A.T) / np.float64(2 * n)
    keep = U & (P != 0.0)
    indptr = np.zeros(n + 1, dtype=np.uint64)
    indptr[1:] = np.cumsum(keep.sum(axis=1))
    ii, jj = np.nonzero(keep)
    info = {"nnz": int(keep.sum()), "n_mutual": int((M & M.T).sum()) // 2, "entries_dropped": int((U & ~keep).sum())}
    return indptr, jj.astype(np.uint32), P[ii, jj], info


def affinities(idx, dist, u=0.0):
    idx = np.asarray(idx)
    n, k = idx.shape
    if u == 0.0:
        u = default_perplexity(k)
    cols, p, beta, ci = conditional(idx, dist, u)
    indptr, indices, data, info = joint(cols, p, n)
    info.update(rows_no_root=ci["rows_no_root"], n=n, k=k, perplexity=float(u))
    return (indptr, indices, data), beta, info, (cols, p, ci)


# ---- 3. the pyramid and the walk -----------------------------------------------------------------------------------------------------
def auto_levels(n):
    L = 1
    while L < MAX_LEVELS and 4 ** (L + 1) < n:
        L += 1
    return L


def _spread(v):
    out = np.zeros_like(v)
    for b in range(16):
        out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(2 * b)
    return out


def pyramid(Y, L):
    """lo, side, U (n x 2 uint64), and per level l = 1..L: the sorted codes of the cells that hold a point, their count m
    (Python integers), and com (f64, from Python-integer sums)."""
    Y = np.asarray(Y, dtype=np.float64)
    lo = Y.min(axis=0)
    ext = np.float64((Y.max(axis=0) - lo).max())
    side = ext * (1.0 + 2.0 ** -20) if ext != 0.0 else np.float64(1.0)
    U = np.minimum(np.floor(((Y - lo) / side) * 2.0 ** 32), 2.0 ** 32 - 1).astype(np.uint64)
    levels = {}
    for l in range(1, L + 1):
        cx, cy = U[:, 0] >> np.uint64(32 - l), U[:, 1] >> np.uint64(32 - l)
        code = _spread(cx) | (_spread(cy) << np.uint64(1))
        codes, inv = np.unique(code, return_inverse=True)
        m = [0] * codes.size
        SX, SY = [0] * codes.size, [0] * codes.size
        for i, c in enumerate(inv):
            m[c] += 1
            SX[c] += int(U[i, 0])
            SY[c] += int(U[i, 1])
        mf = np.array([float(v) for v in m])
        unit = side * 2.0 ** -32
        com = np.stack([lo[0] + (np.array([float(v) for v in SX]) / mf) * unit,
                        lo[1] + (np.array([float(v) for v in SY]) / mf) * unit], axis=1)
        levels[l] = {"codes": codes, "m": mf, "com": com, "code_of": code}
    return lo, side, U, levels


def repulsion(Y, theta, L, dtype=np.float64):
    """rep (n x 2), z (n), Z and the three counters at Y (positions in `dtype`; the decisions use their f64 values)."""
    Yt = np.asarray(Y, dtype=dtype)
    Y64 = Yt.astype(np.float64)
    n = Y64.shape[0]
    lo, side, U, lev = pyramid(Y64, L)
    theta2 = np.float64(theta) * np.float64(theta)
    rep = np.zeros((n, 2), dtype=dtype)
    z = np.zeros(n, dtype=dtype)
    ctr = dict.fromkeys(COUNTERS, 0)
    # the members of the finest cells in ascending index
    fin = lev[L]
    order = np.argsort(fin["code_of"], kind="stable")
    first = np.searchsorted(fin["code_of"][order], fin["codes"], side="left")
    last = np.searchsorted(fin["code_of"][order], fin["codes"], side="right")
    pi = np.repeat(np.arange(n), 4)
    code = np.tile(np.arange(4, dtype=np.uint64), n)
    one = dtype(1)
    for l in range(1, L + 1):
        cell = lev[l]
        at = np.searchsorted(cell["codes"], code)
        at_c = np.minimum(at, cell["codes"].size - 1)
        full = cell["codes"][at_c] == code                       # an empty cell is skipped
        pi, code, at = pi[full], code[full], at_c[full]
        d64 = Y64[pi] - cell["com"][at]
        d2_64 = d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1]
        sl = side * 2.0 ** -l
        acc = sl * sl < theta2 * d2_64
        # accepted cells
        a = np.flatnonzero(acc)
        ctr["cells_accepted"] += int(a.size)
        d = Yt[pi[a]] - cell["com"][at[a]].astype(dtype)
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        q = one / (one + d2)
        m = cell["m"][at[a]].astype(dtype)
        mqq = m * q * q
        np.add.at(rep, pi[a], mqq[:, None] * d)
        np.add.at(z, pi[a], m * q)
        rest = np.flatnonzero(~acc)
        if l == L:
            ctr["cells_exact"] += int(rest.size)
            cnt = (last - first)[at[rest]]
            pp = np.repeat(pi[rest], cnt)
            start = np.repeat(first[at[rest]], cnt)
            within = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            jj = order[start + within]
            ok = jj != pp
            pp, jj = pp[ok], jj[ok]
            ctr["pairs_exact"] += int(pp.size)
            d = Yt[pp] - Yt[jj]
            q = one / (one + (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]))
            np.add.at(rep, pp, (q * q)[:, None] * d)
            np.add.at(z, pp, q)
        else:
            pi = np.repeat(pi[rest], 4)
            code = (np.repeat(code[rest], 4) << np.uint64(2)) + np.tile(np.arange(4, dtype=np.uint64), rest.size)
    Z = z.sum()
    info = dict(ctr, levels=L, side=float(side), lo=(float(lo[0]), float(lo[1])))
    return rep, z, Z, info


def dense_repulsion(Y, dtype=np.float64):
    """The exact O(n^2) sums, every pair, without any pyramid."""
    Yt = np.asarray(Y, dtype=dtype)
    d = Yt[:, None, :] - Yt[None, :, :]
    q = dtype(1) / (dtype(1) + (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]))
    np.fill_diagonal(q, 0)
    return ((q * q)[:, :, None] * d).sum(axis=1), q.sum(axis=1)


# ---- 4. attraction, the update, the KL pass ------------------------------------------------------------------------------------------
def attraction(P, Y, dtype=np.float64):
    indptr, indices, data = P
    Yt = np.asarray(Y, dtype=dtype)
    n = Yt.shape[0]
    rows = np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))
    d = Yt[rows] - Yt[indices.astype(np.int64)]
    q = dtype(1) / (dtype(1) + (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]))
    attr = np.zeros((n, 2), dtype=dtype)
    np.add.at(attr, rows, (data.astype(dtype) * q)[:, None] * d)
    return attr


def kl(P, Y, Z, dtype=np.float64):
    indptr, indices, data = P
    Yt = np.asarray(Y, dtype=dtype)
    rows = np.repeat(np.arange(Yt.shape[0]), np.diff(indptr.astype(np.int64)))
    d = Yt[rows] - Yt[indices.astype(np.int64)]
    q = dtype(1) / (dtype(1) + (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]))
    w = data.astype(dtype)
    return (w * ((np.log(w) - np.log(q)) + np.log(dtype(Z)))).sum()


def auto_eta(n):
    return max(n / 48.0, 50.0)


def layout(P, Y0, n_iter=1000, theta=0.5, levels=0, exaggeration=12.0, exaggeration_iters=250, learning_rate=0.0, stop_after=0,
           dtype=np.float64, keep=()):
    """Iterations 1 .. (stop_after or n_iter).  Returns (Y, info, {t: Y^t for t in keep})."""
    Y = np.array(Y0, dtype=dtype)
    n = Y.shape[0]
    L = levels or auto_levels(n)
    eta = dtype(learning_rate if learning_rate else auto_eta(n))
    gain = np.ones((n, 2), dtype=dtype)
    vel = np.zeros((n, 2), dtype=dtype)
    kept, ctr = {}, dict.fromkeys(COUNTERS, 0)
    run = stop_after or n_iter
    for t in range(1, run + 1):
        early = t <= exaggeration_iters
        alpha, mu = dtype(exaggeration if early else 1.0), dtype(0.5 if early else 0.8)
        rep, z, Z, ctr = repulsion(Y, theta, L, dtype)
        attr = attraction(P, Y, dtype)
        grad = dtype(4) * (alpha * attr - rep / Z)
        flip = (grad.astype(np.float64) > 0) != (vel.astype(np.float64) > 0)          # the sign test, in f64
        gain = np.where(flip, gain + dtype(0.2), gain * dtype(0.8))
        gain = np.maximum(gain, dtype(0.01))
        vel = mu * vel - (eta * gain) * grad
        Y = Y + vel
        if t in keep:
            kept[t] = Y.copy()
    rep, z, Z, last = repulsion(Y, theta, L, dtype)
    info = {"n": n, "n_iter": n_iter, "iters_run": run, "levels": L, "eta": float(eta), "Z": Z, "kl": kl(P, Y, Z, dtype),
            "side": last["side"]}
    info.update({c: ctr[c] for c in COUNTERS})
    return Y, info, kept


# ---- quality, recomputed densely on the host -----------------------------------------------------------------------------------------
def exact_kl(P, Y):
    """KL(P || Q) with the exact Z of Y (dense)."""
    _, zz = dense_repulsion(Y)
    return float(kl(P, Y, zz.sum()))


def purity(Y, labels, k=10):
    """The share of points whose k nearest neighbours in the embedding all carry their label."""
    Y = np.asarray(Y, dtype=np.float64)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1, kind="stable")[:, :k]
    return float((labels[nn] == labels[:, None]).all(axis=1).mean())


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def host_knn(x, k):
    """Exact k nearest neighbours without self (dense; the fixtures are small): (idx n x k, dist n x k)."""
    x = np.asarray(x, dtype=np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return idx.astype(np.uint32), np.sqrt(np.take_along_axis(d2, idx, axis=1))


def clumps(n, dim, n_clumps=6, seed=0, spread=10.0):
    """n points in n_clumps separated Gaussian clumps in `dim` dimensions, with their labels."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clumps, dim)) * spread
    labels = np.arange(n) % n_clumps
    return centres[labels] + rng.standard_normal((n, dim)), labels


# ---- the named inputs of the affinity tests (shared by the CPU check of the 1 % cap and the GPU tests) -------------------------------
AFFINITY_CASES = ("n3", "k2", "k64", "n257", "n1025", "edges", "edges_shuffled")


def affinity_case(name):
    """(idx n x k uint32, dist n x k f64, perplexity).  "edges": the 257-point list with a row whose neighbours all tie, rows
    with c = 4, 5 and 6 tied minima at u = 5 (just below: a root; at and above: none), a row of exact duplicates (all D = 0);
    a k-NN list joins many pairs in one direction only.  "edges_shuffled": the same rows in another order."""
    if name == "n3":
        return np.array([[1, 2], [2, 0], [0, 1]], np.uint32), np.array([[1.0, 2.0], [0.5, 1.0], [2.0, 0.5]]), 1.5
    if name == "k2":
        idx, dist = host_knn(clumps(50, 3, seed=5)[0], 2)
        return idx, dist, 1.5
    if name == "k64":
        idx, dist = host_knn(clumps(130, 8, seed=6)[0], 64)
        return idx, dist, 0.0
    if name == "n257":
        idx, dist = host_knn(clumps(257, 10, seed=0)[0], 15)
        return idx, dist, 5.0
    if name == "n1025":
        idx, dist = host_knn(clumps(1025, 10, seed=1)[0], 30)
        return idx, dist, 10.0
    idx, dist, u = affinity_case("n257")
    dist = dist.copy()
    dist[0, :] = dist[0, 3]                     # all tie
    for row, c in ((1, 4), (2, 5), (3, 6)):
        dist[row, :c] = dist[row, 0]            # c tied minima, the others farther
        dist[row, c:] = dist[row, 0] * (1.5 + 0.1 * np.arange(dist.shape[1] - c))
    dist[4, :] = 0.0                            # exact duplicates
    if name == "edges_shuffled":
        rng = np.random.default_rng(9)
        perm = np.stack([rng.permutation(idx.shape[1]) for _ in range(idx.shape[0])])
        return np.take_along_axis(idx, perm, axis=1), np.take_along_axis(dist, perm, axis=1), u
    assert name == "edges", name
    return idx, dist, u


P_ROW_CAP = 1e-6                                # a row whose bound on |dp| exceeds this is checked through its entropy alone


def p_row_tolerance(bound):
    """The per-row tolerance of p_{j|i}: both sides solve H to 1e-9, so dH <= 2e-9, with a factor 5 of safety."""
    return 5.0 * 2e-9 * bound + 1e-15


# ---- the named layouts of the force tests ---------------------------------------------------------------------------------------------
FORCE_LAYOUTS = ("coincident", "clump70", "boundaries", "constant_x", "extent_1e-4", "extent_1e4")


def force_layout(name, n):
    rng = np.random.default_rng(17)
    Y = rng.standard_normal((n, 2))
    if name == "generic":
        return Y
    if name == "coincident":                    # ext = 0
        return np.tile(np.array([[0.25, -1.5]]), (n, 1))
    if name == "clump70":                       # more than a wave of coincident points inside one finest cell
        Y[40:110] = Y[40]
        return Y
    if name == "boundaries":
        # ext = 2^20 makes side = 2^20 + 1 exactly, and y = side * j / 2^12 is exact: U = j * 2^20, a cell edge of every level
        # up to 12; the corner point carries the maximum of both coordinates
        Y = (2.0 ** 20 + 1.0) * rng.integers(0, 2 ** 12, (n, 2)) / 2.0 ** 12
        Y[0], Y[1], Y[2], Y[3] = (0.0, 0.0), (2.0 ** 20, 2.0 ** 20), (0.0, 2.0 ** 20), ((2.0 ** 20 + 1.0) / 2.0, (2.0 ** 20 + 1.0) / 2.0)
        return Y
    if name == "constant_x":
        Y[:, 0] = 3.0
        return Y
    if name == "extent_1e-4":
        return Y * (1e-4 / np.ptp(Y, axis=0).max())
    assert name == "extent_1e4", name
    return Y * (1e4 / np.ptp(Y, axis=0).max())

"""Host restatement of the BBKNN section of include/srx.h (numpy / scipy), independent of the device code: the batch-balanced
list by brute force in the difference-form f64 distance with the (distance, index) order, its graph through graph_ref.py, and
the trimming both in the closed form of the header and as the bbknn package's two-pass loop (restated from its public
source; the package itself is not installed and nothing here was compared with it).

The device tests use coordinates that are small integers times a power of two, so every squared distance is exact in f64
whatever the order of the additions or their contraction into fused multiply-adds, and the comparison is bit for bit."""
import numpy as np
import scipy.sparse as sp

import graph_ref


# ---- the list -----------------------------------------------------------------------------------------------------------------
def dist2(q, x):
    """|q_i - x_j|^2 summed in coordinate order, n_q x n_x."""
    q, x = np.asarray(q, dtype=np.float64), np.asarray(x, dtype=np.float64)
    d2 = np.zeros((q.shape[0], x.shape[0]))
    for c in range(x.shape[1]):
        t = q[:, c][:, None] - x[None, :, c]
        d2 += t * t
    return d2


def bbknn_list(x, batch, n_batches, k_within=3, n_dims=None):
    """(indices n x K uint32, distances n x K f64), K = k_within * n_batches - 1: from every other batch the k_within nearest
    points, from the own batch the k_within - 1 nearest other than the point itself, chosen by (dist2, index); the row ascending
    by (sqrt(dist2), index)."""
    x = np.asarray(x, dtype=np.float64)
    if n_dims:
        x = x[:, :n_dims]
    n = len(x)
    batch = np.zeros(n, dtype=np.int64) if batch is None else np.asarray(batch, dtype=np.int64)
    idx_parts, d2_parts = [], []
    for b in range(n_batches):
        members = np.nonzero(batch == b)[0]                       # ascending: the local order is the order of the indices
        assert len(members) >= k_within, "a batch has fewer than k_within points"
        d2 = dist2(x, x[members])
        own = np.nonzero(batch == b)[0]
        d2[own, np.arange(len(members))] = np.inf                 # self is left out by identity
        order = np.argsort(d2, axis=1, kind="stable")[:, :k_within]
        part_i, part_d = members[order], np.take_along_axis(d2, order, axis=1)
        keep = np.ones((n, k_within), dtype=bool)
        keep[own, k_within - 1] = False                           # one fewer from the own batch
        idx_parts.append((part_i, keep))
        d2_parts.append(part_d)
    K = k_within * n_batches - 1
    idx = np.zeros((n, K), dtype=np.int64)
    d2 = np.zeros((n, K))
    for i in range(n):
        ii = np.concatenate([p[i][k[i]] for p, k in idx_parts])
        dd = np.concatenate([d[i][k[i]] for d, (_, k) in zip(d2_parts, idx_parts)])
        assert len(ii) == K and np.isfinite(dd).all()
        idx[i], d2[i] = ii, dd
    dist = np.sqrt(d2)
    order = np.lexsort((idx, dist), axis=1)
    return np.take_along_axis(idx, order, axis=1).astype(np.uint32), np.take_along_axis(dist, order, axis=1)


def pairs_searched(sizes, k_within):
    n = int(np.sum(sizes))
    return n * n - (int((np.asarray(sizes, dtype=np.int64) ** 2).sum()) if k_within == 1 else 0)


def n_searches(sizes, k_within):
    """Per batch: the queries before its block, its own block (k_within > 1), the queries behind it; empty ranges are skipped."""
    sizes = [int(s) for s in sizes]
    n, at, c = sum(sizes), 0, 0
    for s in sizes:
        c += (at > 0) + (k_within > 1) + (n - at - s > 0)
        at += s
    return c


def graph(idx, dist):
    """graph_ref.graph of the list: (D, C, per-row dict, A, info)."""
    return graph_ref.graph(idx, dist)


# ---- trimming -----------------------------------------------------------------------------------------------------------------
def thresholds(indptr, data, trim):
    indptr = np.asarray(indptr, dtype=np.int64)
    t = np.zeros(len(indptr) - 1)
    for i in np.nonzero(np.diff(indptr) > trim)[0]:
        t[i] = np.sort(data[indptr[i]:indptr[i + 1]])[-trim]     # the trim-th largest, with multiplicity
    return t


def trim_closed(csr, trim, wave_capacity=0, short_capacity=0):
    """The closed form: (indptr uint64, indices uint32, data f64) and the counters of srx_trim_info."""
    indptr, indices, data = (np.asarray(a) for a in csr)
    ptr = indptr.astype(np.int64)
    n = len(ptr) - 1
    L = np.diff(ptr)
    t = thresholds(ptr, data, trim)
    rows = np.repeat(np.arange(n), L)
    keep = (data >= t[rows]) & (data >= t[indices.astype(np.int64)])
    newL = np.bincount(rows[keep], minlength=n).astype(np.int64) if n else np.zeros(0, dtype=np.int64)
    out_ptr = np.concatenate([[0], np.cumsum(newL)]).astype(np.uint64)
    over = L > trim
    info = {"trim": int(trim), "rows_over_trim": int(over.sum()), "nnz_before": int(ptr[-1]), "nnz_after": int(keep.sum()),
            "entries_trimmed": int((~keep).sum()), "max_row_nnz_before": int(L.max()) if n else 0,
            "max_row_nnz_after": int(newL.max()) if n else 0, "rows_emptied": int(((newL == 0) & (L > 0)).sum()),
            "rows_wave": int((over & (L <= wave_capacity)).sum()),
            "rows_short": int((over & (L > wave_capacity) & (L <= short_capacity)).sum()),
            "rows_long": int((over & (L > short_capacity)).sum())}
    return (out_ptr, indices[keep].astype(np.uint32), data[keep].astype(np.float64)), info


def trim_bbknn_loop(csr, trim):
    """bbknn's `trimming`: the thresholds once, then twice "zero what lies below the row's threshold, drop the zeros,
    transpose".  Returns the CSR triple with sorted indices."""
    indptr, indices, data = (np.asarray(a) for a in csr)
    n = len(indptr) - 1
    cnts = sp.csr_matrix((np.array(data, dtype=np.float64), indices.astype(np.int64), indptr.astype(np.int64)), shape=(n, n))
    vals = np.zeros(n)
    for i in range(n):
        row = cnts.data[cnts.indptr[i]:cnts.indptr[i + 1]]
        if trim < len(row):
            vals[i] = row[np.argsort(row, kind="stable")[-trim]]
    for _ in range(2):
        for i in range(n):
            row = cnts.data[cnts.indptr[i]:cnts.indptr[i + 1]]     # a view: written in place
            row[row < vals[i]] = 0.0
        cnts.eliminate_zeros()
        cnts = cnts.T.tocsr()
    cnts.sort_indices()
    return cnts.indptr.astype(np.uint64), cnts.indices.astype(np.uint32), cnts.data.astype(np.float64)


def symmetric_from_list(idx, weights):
    """A symmetric test matrix from a directed list: the larger of the two directed weights of every pair joined in either
    direction (both entries the same bits), as a CSR triple with sorted indices."""
    idx = np.asarray(idx, dtype=np.int64)
    n, k = idx.shape
    a = sp.csr_matrix((np.asarray(weights, dtype=np.float64).ravel(), idx.ravel(), np.arange(0, n * k + 1, k)), shape=(n, n))
    c = a.maximum(a.T).tocsr()
    c.sort_indices()
    return c.indptr.astype(np.uint64), c.indices.astype(np.uint32), c.data.astype(np.float64)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def labels(kind, sizes, seed=0):
    """One label per point with the given batch sizes: "contiguous" blocks, "interleaved" round-robin while a batch has points
    left, or "hashed" (a seeded shuffle of the contiguous labels)."""
    sizes = [int(s) for s in sizes]
    cont = np.repeat(np.arange(len(sizes)), sizes)
    if kind == "contiguous":
        return cont.astype(np.uint32)
    if kind == "hashed":
        return np.random.default_rng(seed).permutation(cont).astype(np.uint32)
    assert kind == "interleaved"
    left, out = list(sizes), []
    while len(out) < len(cont):
        for b in range(len(sizes)):
            if left[b]:
                left[b] -= 1
                out.append(b)
    return np.array(out, dtype=np.uint32)


def lattice(rng, n, d, span, exp=0):
    """n points with integer coordinates in -span .. span times 2^exp: every squared distance is exact in f64."""
    return np.ldexp(rng.integers(-span, span + 1, (n, d)).astype(np.float64), exp)


def clumps_two_batches(rng, per=100, shift=5.0):
    """Two batches drawn from the same three clumps (radius <= 1, centres 100 apart), the second batch shifted by `shift`
    along an axis of its own: (points n x 3, batch, clump), n = 6 * per, in a shuffled order."""
    centres = np.array([[0.0, 0.0], [100.0, 0.0], [0.0, 100.0]])
    pts, bat, clu = [], [], []
    for b in (0, 1):
        for c in range(3):
            r = np.sqrt(rng.random(per))
            phi = rng.random(per) * 2 * np.pi
            p = np.zeros((per, 3))
            p[:, 0] = centres[c, 0] + r * np.cos(phi)
            p[:, 1] = centres[c, 1] + r * np.sin(phi)
            p[:, 2] = b * shift
            pts.append(p)
            bat += [b] * per
            clu += [c] * per
    order = rng.permutation(6 * per)
    x = np.round(np.concatenate(pts)[order] * 1024.0) / 1024.0     # dyadic coordinates: exact squared distances
    return x, np.array(bat, dtype=np.uint32)[order], np.array(clu)[order]

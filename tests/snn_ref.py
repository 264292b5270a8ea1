"""Two independent restatements of the shared-nearest-neighbour graph that include/srx.h defines (srx_snn_from_knn), neither of
which shares a line with the device code:

  * ``by_sets``: Python ``set``s and ``fractions``, for tiny inputs: the definition read aloud;
  * ``by_scipy``: ``A @ A.T`` on int64 incidence matrices, the diagonal removed, J by the same f64 division (numpy's), the
    optional restriction to ``P u P^T``; its CSR is what the device result is compared with, bit for bit.

``idx`` is the k-NN list, n x k, rows in any order.
"""
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

JACCARD, NUMBER = 0, 1
SHARED, KNN = 0, 1
DEFAULT_PRUNE = 1.0 / 15.0


def set_size(k, include_self):
    return k + (1 if include_self else 0)


def jaccard_f64(s, K):
    """(double)s / (double)(2K - s): Python's float division of two exact integers is the one IEEE division."""
    return float(s) / float(2 * K - s)


def min_shared(k, include_self, prune):
    """The smallest s in 1..K whose J, the exact fraction rounded once to f64, is >= prune; K + 1 if none."""
    K = set_size(k, include_self)
    for s in range(1, K + 1):
        if float(Fraction(s, 2 * K - s)) >= prune:      # Fraction -> float rounds correctly, once
            return s
    return K + 1


def by_sets(idx, include_self=True, pairs=SHARED, prune=DEFAULT_PRUNE, weight=JACCARD):
    """{(i, j): (s, exact J as a Fraction, stored f64 value)} over the stored ordered pairs, and the considered-pair count."""
    idx = [[int(j) for j in row] for row in idx]
    n = len(idx)
    k = len(idx[0]) if n else 0
    K = set_size(k, include_self)
    N = [set(row) | ({i} if include_self else set()) for i, row in enumerate(idx)]
    out, considered = {}, 0
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            s = len(N[i] & N[j])
            if s < 1:
                continue
            if pairs == KNN and not (j in idx[i] or i in idx[j]):
                continue
            considered += 1
            J = Fraction(s, 2 * K - s)
            if float(J) >= prune:
                out[(i, j)] = (s, J, float(J) if weight == JACCARD else float(s))
    return out, considered // 2


def incidence(idx, include_self):
    idx = np.asarray(idx, dtype=np.int64)
    n, k = idx.shape
    A = sp.csr_matrix((np.ones(n * k, dtype=np.int64), (np.repeat(np.arange(n), k), idx.ravel())), shape=(n, n))
    if include_self:
        A = A + sp.identity(n, dtype=np.int64, format="csr")
    return A.tocsr()


def by_scipy(idx, include_self=True, pairs=SHARED, prune=DEFAULT_PRUNE, weight=JACCARD):
    """(indptr uint64, indices uint32, data f64, info dict) of the SNN graph."""
    idx = np.asarray(idx, dtype=np.int64)
    n, k = idx.shape
    K = set_size(k, include_self)
    A = incidence(idx, include_self)
    S = (A @ A.T).tocoo()
    off = S.row != S.col
    r, c, s = S.row[off], S.col[off], S.data[off].astype(np.int64)
    pos = s > 0
    r, c, s = r[pos], c[pos], s[pos]
    if pairs == KNN:
        P = incidence(idx, False)
        U = (P + P.T).tocsr()
        joined = np.asarray(U[r, c]).ravel() > 0 if len(r) else np.zeros(0, dtype=bool)
        r, c, s = r[joined], c[joined], s[joined]
    considered = len(s)
    max_shared = int(s.max()) if considered else 0      # over the considered pairs, kept or not
    J = s.astype(np.float64) / (2 * K - s).astype(np.float64)
    keep = J >= prune
    r, c, s, J = r[keep], c[keep], s[keep], J[keep]
    order = np.lexsort((c, r))
    r, c, s, J = r[order], c[order], s[order], J[order]
    counts = np.bincount(r, minlength=n)
    indptr = np.zeros(n + 1, dtype=np.uint64)
    indptr[1:] = np.cumsum(counts)
    data = J if weight == JACCARD else s.astype(np.float64)
    indeg = np.bincount(idx.ravel(), minlength=n)
    members = indeg + (1 if include_self else 0)                  # |{j : m in N(j)}|
    cand = np.asarray(A @ members).ravel()
    info = {"n": n, "k": k, "set_size": K, "min_shared": min_shared(k, include_self, prune), "max_shared": max_shared,
            "pairs_considered": considered // 2, "pairs_kept": len(r) // 2, "nnz": len(r),
            "max_row_nnz": int(counts.max()) if n else 0, "max_in_degree": int(indeg.max()) if n else 0,
            "max_candidates": int(cand.max()) if n else 0, "sum_candidates": int(cand.sum()),
            "rows_empty": int((counts == 0).sum())}
    return indptr, c.astype(np.uint32), np.ascontiguousarray(data, dtype=np.float64), info


def random_list(rng, n, k):
    """n rows of k distinct neighbours j != i, uniformly, rows unsorted."""
    out = np.empty((n, k), dtype=np.uint32)
    for i in range(n):
        pick = rng.choice(n - 1, size=k, replace=False)
        out[i] = pick + (pick >= i)
    return out


def brute_knn(points, k):
    """The exact k-NN list of the rows of `points` (self excluded), by (squared distance, index)."""
    x = np.asarray(points, dtype=np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    return np.argsort(d2, axis=1, kind="stable")[:, :k].astype(np.uint32)


def clumps(rng, n, n_clumps, d=8, spread=0.05, gap=10.0):
    """n points in n_clumps well-separated clumps; (points, clump of each point)."""
    lab = np.arange(n) % n_clumps
    centres = rng.normal(size=(n_clumps, d)) * gap
    return centres[lab] + rng.normal(size=(n, d)) * spread, lab

"""Host reference of the Wilcoxon rank-sum definition in include/srx.h (srx_rank_genes_wilcoxon): a dense numpy sort per gene,
the doubled rank sums R2 and the tie terms T in integers, and the score in the stated operation order (numpy rounds every
operation once and never contracts).  Test-side only: the product never imports it."""
import numpy as np
import scipy.sparse as sp

STORE_DTYPE = {1: np.float32, 2: np.float64}          # SRX_STORE_F32, SRX_STORE_F64: each storage compares in its own precision


def dense(X, store=2):
    """The N x G column values as the device holds them: stored values rounded to the storage, implicit zeros as 0."""
    X = sp.csr_matrix(X)
    return sp.csr_matrix((X.data.astype(STORE_DTYPE[store]), X.indices, X.indptr), shape=X.shape).toarray()


def rank_sums(D, labels, n_groups):
    """D: dense N x G (any float dtype; -0.0 == 0.0 as numpy compares them).  Returns (R2 (n_groups, G) uint64, T (G,) uint64):
    r2 = 2 b + t + 1 per cell from the sorted distinct values of the column and their multiplicities."""
    D = np.asarray(D)
    labels = np.asarray(labels, np.int64)
    N, G = D.shape
    R2 = np.zeros((n_groups, G), np.int64)
    T = np.zeros(G, np.uint64)
    for j in range(G):
        if N == 0:
            continue
        _, inverse, t = np.unique(D[:, j], return_inverse=True, return_counts=True)
        t = t.astype(np.int64)
        b = np.cumsum(t) - t
        np.add.at(R2[:, j], labels, (2 * b + t + 1)[inverse.ravel()])
        T[j] = np.uint64(sum(int(x) ** 3 - int(x) for x in t))
    return R2.astype(np.uint64), T


def score(R2, T, sizes, n_rows, tie_correct):
    """The score table of srx.h; T may be None without tie_correct."""
    N = int(n_rows)
    R2 = np.asarray(R2, np.uint64).astype(np.int64)
    n_g = np.asarray(sizes, np.uint64).astype(np.int64)[:, None]
    n_r = N - n_g
    degenerate = (n_g == 0) | (n_r == 0)
    num = (R2 - n_g * (N + 1)).astype(np.float64) * 0.5
    if tie_correct and N >= 2:
        tc = 1.0 - np.asarray(T, np.uint64).astype(np.float64)[None, :] / float(N ** 3 - N)
    else:
        tc = np.ones((1, R2.shape[1]))
    d = (((n_g * n_r).astype(np.float64) * float(N + 1)) / 12.0) * tc
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(~degenerate & (d > 0), num / np.sqrt(d), 0.0)
    return s, int(degenerate.sum())


def reference(X, labels, n_groups, store=2, tie_correct=False):
    """Everything at once for a sparse matrix: {"ranksum2", "ties", "score", "groups_degenerate"}."""
    D = dense(X, store)
    R2, T = rank_sums(D, labels, n_groups)
    sizes = np.bincount(np.asarray(labels, np.int64), minlength=n_groups)
    s, deg = score(R2, T, sizes, D.shape[0], tie_correct)
    return {"ranksum2": R2, "ties": T, "score": s, "groups_degenerate": deg}

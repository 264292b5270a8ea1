"""Host reference of the marker-gene definition in include/srx.h (srx_group_moments / srx_rank_genes_groups): exact grouped
moments, the statistics in the stated operation order (numpy rounds every operation once and never contracts), the ranking
order and the fixed-point scales.  Test-side only: the product never imports it."""
import math

import numpy as np
import scipy.sparse as sp


def scales(max_abs, n_rows):
    """(sum_scale_log2, sq_scale_log2) of srx.h: e = the smallest integer with max_abs < 2^e (0 for 0), no lower than -30;
    L = ceil(log2(max(N, 1)))."""
    e = max(math.frexp(float(max_abs))[1], -30)          # max_abs = f 2^e with 0.5 <= f < 1
    L = max(int(n_rows), 1)
    L = (L - 1).bit_length()
    return 62 - e - L, 62 - 2 * e - L


def sizes_of(labels, n_groups):
    return np.bincount(np.asarray(labels, np.int64), minlength=n_groups).astype(np.uint64)


def exact_moments_int(X, labels, n_groups):
    """Integer-valued data: (cnt, sum, sumsq) per (group, gene) in int64, exact."""
    X = sp.csr_matrix(X)
    n = X.shape[0]
    onehot = sp.csr_matrix((np.ones(n, np.int64), (np.asarray(labels, np.int64), np.arange(n))), shape=(n_groups, n))
    Xi = sp.csr_matrix((np.rint(X.data).astype(np.int64), X.indices, X.indptr), shape=X.shape)
    assert np.array_equal(Xi.data.astype(X.data.dtype), X.data)
    ones = sp.csr_matrix((np.ones(X.nnz, np.int64), X.indices, X.indptr), shape=X.shape)
    sq = sp.csr_matrix((Xi.data * Xi.data, X.indices, X.indptr), shape=X.shape)
    dense = lambda m: np.asarray((onehot @ m).todense(), dtype=np.int64)
    return dense(ones), dense(Xi), dense(sq)


def exact_moments_fsum(X, labels, n_groups):
    """Any finite data: cnt (int64) and the correctly rounded sums of x and of fl(x * x) per (group, gene) (math.fsum)."""
    X = sp.csr_matrix(X)
    labels = np.asarray(labels, np.int64)
    G = X.shape[1]
    cnt = np.zeros((n_groups, G), np.int64)
    s = np.zeros((n_groups, G))
    q = np.zeros((n_groups, G))
    for g in range(n_groups):
        sub = sp.csc_matrix(X[np.flatnonzero(labels == g)])
        for j in range(G):
            v = sub.data[sub.indptr[j]:sub.indptr[j + 1]].astype(np.float64)
            cnt[g, j] = v.size
            s[g, j] = math.fsum(v)
            q[g, j] = math.fsum(v * v)
    return cnt, s, q


def statistics(sizes, cnt, s, q, n_rows, logged, rest=None):
    """The tables of srx.h from per-group moments.  sizes (n_groups,), cnt / s / q (n_groups, G) as f64-representable numbers.
    `rest` = (cnt_rest, s_rest, q_rest) where the caller holds them (the device forms them from its fixed-point integers);
    otherwise total - group in f64, which is exact for integer-valued data below 2^53."""
    sizes = np.asarray(sizes, np.float64)
    cnt, s, q = (np.asarray(a, np.float64) for a in (cnt, s, q))
    if rest is None:
        rest = tuple(a.sum(axis=0, keepdims=True) - a for a in (cnt, s, q))
    cnt_r, s_r, q_r = (np.asarray(a, np.float64) for a in rest)
    n_g = sizes[:, None]
    n_r = float(n_rows) - n_g
    degenerate = (n_g < 2) | (n_r < 2)

    def side(c, S, Q, n):
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = np.where(n > 0, S / n, 0.0)
            pct = np.where(n > 0, c / n, 0.0)
            v = (Q / n - mean * mean) * (n / (n - 1.0))
        var = np.where(~degenerate & (v > 0), v, 0.0)
        return mean, var, pct

    mean, var, pct = side(cnt, s, q, n_g)
    mean_r, var_r, pct_r = side(cnt_r, s_r, q_r, n_r)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = var / n_g + var_r / n_r
        score = np.where(~degenerate & (d > 0), (mean - mean_r) / np.sqrt(d), 0.0)
        if logged:
            lfc = np.log2((np.expm1(mean) + 1e-9) / (np.expm1(mean_r) + 1e-9))
        else:
            lfc = np.log2((mean + 1e-9) / (mean_r + 1e-9))
    return {"mean": mean, "var": var, "mean_rest": mean_r, "var_rest": var_r, "score": score, "lfc": lfc, "pct": pct,
            "pct_rest": pct_r, "groups_degenerate": int(degenerate.sum())}


def order(score):
    """Per group the gene indices by (score descending, index ascending)."""
    score = np.asarray(score)
    idx = np.arange(score.shape[1])
    return np.stack([np.lexsort((idx, -row)) for row in score])

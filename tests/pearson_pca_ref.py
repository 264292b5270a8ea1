"""Numpy restatement of the residual PCA of include/srx.h (srx_pca_pearson, srx_pearson_gram) and the inputs of its tests.

``residuals`` is pearson_ref's long-double definition with the ``selected`` totals added (the sums over the listed genes only:
the definition applied to the sub-matrix, whose column sums are the whole matrix's).  ``covariance`` / ``pca`` are the stated
formulas in f64 with ``np.linalg.eigh``; ``sign_rule`` is the library's.  ``planted_counts`` draws the PCA tests' matrix."""
import numpy as np

import pearson_ref as R

U = 2.0 ** -53
TOTALS = ("all", "selected")


def residuals(X, genes, theta=None, clip=None, totals="all", dtype=np.longdouble):
    """Z (n x k) of the listed genes in ``dtype``; the default clip is sqrt(n) under both totals."""
    X = np.asarray(X)
    genes = np.asarray(genes, dtype=np.int64)
    theta, clip = R.used_opts(X.shape[0], theta, clip)
    if totals == "all":
        return R.residuals(X, theta, clip, dtype)[:, genes]
    assert totals == "selected", totals
    return R.residuals(X[:, genes], theta, clip, dtype)


def gram(Z):
    """(Z^T Z, |Z|^T |Z|, column sums, column sums of |Z|) in the type of Z."""
    A = np.abs(Z)
    return Z.T @ Z, A.T @ A, Z.sum(axis=0), A.sum(axis=0)


def gram_bound(n, absgram):
    """(n + 32) u (|Z|^T |Z|)_ij: the dot-product bound for n terms plus twice the 8-ulp element bound."""
    return (n + 32) * U * np.asarray(absgram, dtype=np.float64)


def colsum_bound(n, abssum):
    return (n + 8) * U * np.asarray(abssum, dtype=np.float64)


def covariance(Z, center=True):
    """(C, m): C = (Z^T Z - n m m^T) / (n - 1), m the column means (zeros without centring)."""
    Z = np.asarray(Z, dtype=np.float64)
    n = Z.shape[0]
    m = Z.sum(axis=0) / n if center else np.zeros(Z.shape[1])
    return (Z.T @ Z - n * np.outer(m, m)) / (n - 1), m


def sign_rule(V):
    """Each column flipped so that its entry of largest magnitude (the first of equals) is positive."""
    V = np.array(V, dtype=np.float64)
    for c in range(V.shape[1]):
        if V[int(np.argmax(np.abs(V[:, c]))), c] < 0:
            V[:, c] = -V[:, c]
    return V


def pca(Z, n_pc, center=True):
    """dict(values (all, descending), evr, components k x n_pc, scores n x n_pc, mean) by eigh of C."""
    Z = np.asarray(Z, dtype=np.float64)
    C, m = covariance(Z, center)
    w, V = np.linalg.eigh(C)
    w, V = w[::-1], V[:, ::-1]
    V = sign_rule(V[:, :n_pc])
    return {"values": w, "evr": w[:n_pc] / np.trace(C), "components": V, "scores": (Z - m) @ V, "mean": m}


def min_relative_gap(values, n_pc):
    """The smallest (w_p - w_{p+1}) / w_p over the first n_pc eigenvalues (the one behind them included, where there is one)."""
    w = np.asarray(values, dtype=np.float64)
    last = min(n_pc, w.size - 1)
    return float(np.min((w[:last] - w[1:last + 1]) / w[:last]))


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
PLANTED_SHAPE = (600, 240)
PLANTED_SEED = 8           # chosen so that every tested case keeps a relative eigenvalue gap >= 1e-3 (asserted by the tests)
PLANTED_RANK = 5


def planted_counts(seed=PLANTED_SEED):
    """Poisson counts (int64, 600 x 240) around a rank-5 mean: five cell programmes over log-normal depths."""
    n, G = PLANTED_SHAPE
    rng = np.random.default_rng(seed)
    W = rng.gamma(1.0, 1.0, size=(n, PLANTED_RANK))
    H = rng.gamma(0.5, 1.0, size=(PLANTED_RANK, G)) + 0.05
    depth = np.exp(rng.normal(0.0, 0.4, size=n))
    lam = (W @ H) * depth[:, None]
    lam *= 3.0 / lam.mean()
    return rng.poisson(lam).astype(np.int64)


def planted_genes(k):
    """k distinct genes of the planted matrix in a fixed, unsorted order."""
    return np.random.default_rng(77).permutation(PLANTED_SHAPE[1])[:k].astype(np.uint64)


def gram_case(n, k):
    """(X, genes) of a Gram test: pearson_ref's draw with a few genes more than are listed, the list unsorted; from 8 x 8 on
    the all-zero gene 0 is listed and cell 0 is empty."""
    G = max(k + 3, 8)
    X = R.make_counts(n, G)
    rest = np.random.default_rng(1000 * n + k).permutation(np.arange(1, G))[:k - 1]
    genes = np.concatenate([rest[:k // 2], [0], rest[k // 2:]]).astype(np.uint64)
    return X, genes

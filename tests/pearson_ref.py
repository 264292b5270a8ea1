"""Numpy restatement of the Pearson-residual definition of include/srx.h, and the inputs of the Pearson tests.

``residuals`` / ``variances`` evaluate the definition in any float type: ``np.longdouble`` is what the device is bounded
against, ``np.float64`` is evaluated once for information (how much of each bound numpy's own f64 arithmetic uses).
``select`` is the stated order.  ``make_counts`` draws the inputs; ``properties`` says what an input holds, from this
restatement alone."""
import numpy as np

U = 2.0 ** -53


def sums(X, dtype=np.longdouble):
    """(r, g, T) of a dense n x G array in ``dtype``."""
    X = np.asarray(X, dtype=dtype)
    r, g = X.sum(axis=1), X.sum(axis=0)
    return r, g, r.sum()


def used_opts(n, theta=None, clip=None):
    """The values in use: theta 0 / None = 100, clip 0 / None = sqrt(n)."""
    theta = 100.0 if theta in (None, 0, 0.0) else float(theta)
    clip = float(np.sqrt(float(n))) if clip in (None, 0, 0.0) else float(clip)
    return theta, clip


def mu_of(X, dtype=np.longdouble):
    r, g, T = sums(X, dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = np.outer(r, g) / T
    return np.where(np.isnan(mu), dtype(0), mu)


def residuals(X, theta=None, clip=None, dtype=np.longdouble):
    """z (n x G) in ``dtype``: mu = (r g) / T, s = sqrt(mu + mu mu / theta), z = clip((x - mu) / s), z = 0 where mu == 0."""
    X = np.asarray(X, dtype=dtype)
    theta, clip = used_opts(X.shape[0], theta, clip)
    mu = mu_of(X, dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(mu) if np.isinf(theta) else np.sqrt(mu + (mu * mu) / dtype(theta))
        z = (X - mu) / s
    z = np.minimum(np.maximum(z, dtype(-clip)), dtype(clip))
    return np.where(mu > 0, z, dtype(0))


def variances(z):
    """v_j = sum z^2 / n - (sum z / n)^2 over all n cells; exactly 0 for a column of zeros."""
    n = z.shape[0]
    return (z * z).sum(axis=0) / n - (z.sum(axis=0) / n) ** 2


def select(v, g, n):
    """The first n genes with g > 0 by descending v, equal variances in ascending index, in rank order."""
    v, g = np.asarray(v), np.asarray(g)
    order = np.argsort(-v, kind="stable")
    order = order[g[order] > 0]
    return order[:n].astype(np.uint64)


def element_bound(z_ref, mu, theta, n=0, G=0, integer=True):
    """8u (|z| + min(sqrt(mu), sqrt(theta))); non-integer inputs: 8 + 2 (n + G) for the rounding of the three sums."""
    c = 8.0 if integer else 8.0 + 2.0 * (n + G)
    return c * U * (np.abs(z_ref).astype(np.float64) + np.minimum(np.sqrt(np.asarray(mu, dtype=np.float64)), np.sqrt(theta)))


def variance_bound(z_ref, cnt, sum_quantum=0.0, sq_quantum=0.0):
    """4 (n + 16) u mean(z^2) + (cnt / n) (sq_quantum + 2 |mean z| sum_quantum), per gene."""
    n = z_ref.shape[0]
    z = np.asarray(z_ref, dtype=np.float64)
    return 4.0 * (n + 16) * U * (z * z).mean(axis=0) + (np.asarray(cnt) / n) * (sq_quantum + 2.0 * np.abs(z.mean(axis=0)) * sum_quantum)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
FEATURES_FROM = 8     # a shape holds the six special rows / columns below from 8 x 8 on; a smaller one is a plain draw


def make_counts(n, G, seed=0, density=1.0):
    """Integer counts (dense int64 n x G) from a Poisson-gamma draw with log-normal depths.  From 8 x 8 on the input also
    holds: gene 0 all-zero; cell 0 empty; gene 1 stored in every non-empty cell; gene 2 with a single entry (a 1, in the
    shallowest cell); cell 1 holding every gene but gene 0; one outlier count (cell 2, gene 3)."""
    rng = np.random.default_rng(1000003 * n + 101 * G + seed)
    p = rng.gamma(0.6, 1.0, size=G) + 0.02
    p /= p.sum()
    depth = np.exp(rng.normal(np.log(density * max(3.0 * G, 60.0)), 0.6, size=n))
    lam = np.outer(depth, p) * rng.gamma(2.0, 0.5, size=(n, G))
    X = rng.poisson(lam).astype(np.int64)
    if n >= FEATURES_FROM and G >= FEATURES_FROM:
        X[:, 0] = 0
        X[:, 1] = np.maximum(X[:, 1], 1)
        X[1, 1:] = np.maximum(X[1, 1:], 1)
        X[2, 3] += 40 * int(max(X.max(), 5))
        X[:, 2] = 0
        X[0, :] = 0
        rs = X.sum(axis=1)
        rs[:3] = np.iinfo(np.int64).max
        X[int(np.argmin(rs)), 2] = 1
    return X


def to_csr(X, dtype):
    """(n, G, indptr, indices, values) of a dense array, entries in row-major order (sorted within a row)."""
    X = np.asarray(X)
    rows, cols = np.nonzero(X)
    indptr = np.zeros(X.shape[0] + 1, dtype=np.uint64)
    np.cumsum(np.bincount(rows, minlength=X.shape[0]), out=indptr[1:])
    return X.shape[0], X.shape[1], indptr, cols.astype(np.uint64), X[rows, cols].astype(dtype)


def to_csc(X, dtype):
    """(n, G, col_offsets, row_indices, values): the CSC arrays of X."""
    G, n, indptr, indices, values = to_csr(np.asarray(X).T, dtype)
    return n, G, indptr, indices, values


def properties(X):
    """What the GPU tests assert of an input before they touch the device, from the restatement alone."""
    n, G = X.shape
    g = X.sum(axis=0)
    z_def = residuals(X, None, None)
    z_one = residuals(X, None, 1.0)
    c = float(np.sqrt(float(n)))
    return {"upper_clip_default": bool((z_def == np.longdouble(c)).any()),
            "upper_clip_one": bool((z_one == 1).any()), "lower_clip_one": bool((z_one == -1).any()),
            "zero_genes": int((g == 0).sum()), "expressed_genes": int((g > 0).sum()),
            "empty_cells": int((X.sum(axis=1) == 0).sum()), "full_genes": int(((X > 0).sum(axis=0) >= n - 1).sum()),
            "single_genes": int(((X > 0).sum(axis=0) == 1).sum()), "full_cells": int(((X > 0).sum(axis=1) >= G - 2).sum())}      # (every gene but the all-zero and the single-entry one)


# The sizes at which the kernels of pearson.hip take another path (the constants of that file, restated): the dense pass stages
# 1024 cells at a time and cuts the cells into chunks that are multiples of that, a workgroup owns 1024 genes (a thread 4 of them,
# 256 apart); the CSR correction gives a workgroup a block of at least 64 rows and one of the matrix's gene tiles (at most 10000
# genes: 10001 genes are two tiles); the block kernel makes 256 outputs per workgroup.
TILES = {"dense_cell_step": 1024, "dense_gene_tile": 1024, "dense_gene_stride": 256, "sparse_row_block": 64,
         "sparse_gene_tile": 10000, "block_tile": 256}
ISSUE_SHAPES = [(1, 1), (5, 3), (63, 64), (64, 63), (65, 65), (257, 300), (1000, 300), (3000, 130), (20000, 64)]
EDGE_SHAPES = ([(n, 40) for n in (1023, 1024, 1025)] + [(40, G) for G in (1023, 1024, 1025)] + [(33, G) for G in (255, 256, 257)] +
               [(n, 33) for n in (127, 128, 129)] + [(20, G) for G in (9999, 10000, 10001)] + [(15, 17), (16, 16), (257, 1)])
SHAPES = ISSUE_SHAPES + EDGE_SHAPES
CROSS_SHAPES = [(65, 65), (257, 300), (1000, 300)]        # every theta x clip x storage x handle
THETAS = (100.0, 10.0, float("inf"))
CLIPS = (None, 1.0, float("inf"))


def has_features(n, G):
    return n >= FEATURES_FROM and G >= FEATURES_FROM

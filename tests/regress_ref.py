"""Numpy restatement of the regression / scale / clip section of include/srx.h (srx_regress_fit, srx_regress_residuals,
srx_regress_gram, srx_pca_regress) and the inputs of its tests.

``evaluate`` walks the definition step by step in the given dtype: ``np.longdouble`` is the reference, ``np.float64`` the naive
evaluation whose own distance from the reference measures what the p x p solve costs on a case (the factor K of the GPU tests).
The p x p system is solved by elimination (the Cholesky factor of the diagonally scaled matrix, as the definition states).  The
PCA, the sign rule and the eigenvalue gaps are pearson_pca_ref's."""
import os

import numpy as np

import pearson_pca_ref as P

U = 2.0 ** -53
MIN_PIVOT = 1e-10
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Refused(Exception):
    """A covariate the definition refuses: ``args[0]`` is its index, ``args[1]`` 'constant' or 'collinear'."""


def cholesky_scaled(A):
    """(sqrt(diag A), L, pivots) with L L^T = D^-1/2 A D^-1/2, in the type of A."""
    p = A.shape[0]
    for q in range(p):
        if not A[q, q] > 0:
            raise Refused(q, "constant")
    d = np.sqrt(np.diag(A)) if p else np.zeros(0, dtype=A.dtype)
    L = np.zeros_like(A)
    piv = np.ones(p, dtype=A.dtype)
    for j in range(p):
        v = A[j, j] / d[j] / d[j]
        for t in range(j):
            v = v - L[j, t] * L[j, t]
        piv[j] = v
        if not v >= MIN_PIVOT:
            raise Refused(j, "collinear")
        L[j, j] = np.sqrt(v)
        for i in range(j + 1, p):
            w = A[i, j] / d[i] / d[j]
            for t in range(j):
                w = w - L[i, t] * L[j, t]
            L[i, j] = w / L[j, j]
    return d, L, piv


def solve_scaled(d, L, W):
    """beta (p x k) with A beta = W by the factor of ``cholesky_scaled``."""
    p = L.shape[0]
    u = np.zeros_like(W)
    for q in range(p):
        v = W[q] / d[q]
        for t in range(q):
            v = v - L[q, t] * u[t]
        u[q] = v / L[q, q]
    for q in range(p - 1, -1, -1):
        v = u[q].copy()
        for t in range(q + 1, p):
            v = v - L[t, q] * u[t]
        u[q] = v / L[q, q]
    return u / d[:, None] if p else u


def constant_genes(X):
    return np.all(X == X[0:1], axis=0)


def evaluate(X, cov, scale=True, max_value=0.0, dtype=np.longdouble):
    """Every quantity of the definition for the dense n x k block X (f64 values as stored) and the n x p covariates."""
    X64 = np.asarray(X, dtype=np.float64)
    n, k = X64.shape
    C64 = np.asarray(cov, dtype=np.float64).reshape(n, -1)
    p = C64.shape[1]
    X, C = X64.astype(dtype), C64.astype(dtype)
    # Every sum over the cells runs in ascending cell order, one term after the other, as the definition states it (np.cumsum
    # accumulates that way; np.sum and BLAS add pairwise / in blocks, which in f64 is MORE accurate than any fixed ascending order
    # and would make the f64 evaluation a flattering yardstick for the solve's cost).
    col_sum = lambda M: np.cumsum(M, axis=0)[-1] if M.shape[0] else np.zeros(M.shape[1:], dtype=dtype)
    dot = lambda Wt, M: (np.stack([col_sum(Wt[:, q:q + 1] * M) for q in range(Wt.shape[1])]) if Wt.shape[1]
                         else np.zeros((0, M.shape[1]), dtype=dtype))
    cbar = col_sum(C) / dtype(n)
    ct = C - cbar
    A = dot(ct, ct)
    d, L, piv = cholesky_scaled(A)
    xbar = col_sum(X) / dtype(n)
    W = dot(ct, X)
    beta = solve_scaled(d, L, W)
    const = constant_genes(X64)
    fitted = np.zeros_like(X)                              # q ascending
    for q in range(p):
        fitted = fitted + ct[:, q:q + 1] * beta[q:q + 1, :]
    r = (X - xbar) - fitted
    r[:, const] = 0
    if scale:
        v = col_sum(r * r) / dtype(n - 1)
        s = np.where(v == 0, dtype(1), np.sqrt(v))
    else:
        v = np.zeros(k, dtype=dtype)
        s = np.ones(k, dtype=dtype)
    z_raw = r / s
    mv = float(max_value or 0.0)
    clipped = np.abs(z_raw) > mv if mv > 0 else np.zeros(z_raw.shape, dtype=bool)
    z = np.clip(z_raw, -mv, mv) if mv > 0 else z_raw
    return {"cbar": cbar, "ct": ct, "A": A, "piv": piv, "xbar": xbar, "W": W, "beta": beta, "const": const, "r": r, "s": s, "z": z,
            "z_raw": z_raw, "clipped": clipped, "mag_r": np.abs(X) + np.abs(xbar) + np.abs(ct) @ np.abs(beta),
            "W_abs": (np.abs(ct) + np.abs(C).mean(axis=0)).T @ np.abs(X), "A_abs": (np.abs(ct) + np.abs(C).mean(axis=0)).T @ np.abs(ct),
            "cbar_abs": np.abs(C).sum(axis=0) / n, "Ainv_abs": np.abs(np.linalg.inv(np.asarray(A, dtype=np.float64))) if p else np.zeros((0, 0))}


def measured_factor(X, cov, scale=True):
    """(K, the raw ratios).  K["r"] = K["s"] = K["beta"]: 8 x the largest ratio the f64 evaluation of the definition reaches
    against the long-double one on this case over r, s and beta, each in units of u x the magnitude the GPU test uses; floor 8.
    K["ctr"]: the factor of the normal-equation gate (below).  Never measured against the device."""
    a, b = evaluate(X, cov, scale, 0.0, np.longdouble), evaluate(X, cov, scale, 0.0, np.float64)
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    out = {}
    mag = f64(a["mag_r"])
    out["r"] = float(np.max(f64(np.abs(b["r"].astype(np.longdouble) - a["r"])) / (U * np.maximum(mag, 1e-300)), initial=0.0))
    out["s"] = float(np.max(f64(np.abs(b["s"].astype(np.longdouble) - a["s"]) / a["s"]) / U, initial=0.0))
    mb = beta_magnitude(a)
    out["beta"] = float(np.max(f64(np.abs(b["beta"].astype(np.longdouble) - a["beta"])) / (U * np.maximum(mb, 1e-300)), initial=0.0))
    # the normal equations on the f64 evaluation's own residuals, in the unit of that gate (u |Ct|^T |r|): where the fit is nearly
    # exact (n = p + 2) the residuals are far smaller than the terms they are made of, and so is that unit
    ct, r = f64(a["ct"]).astype(np.longdouble), b["r"].astype(np.longdouble)
    out["ctr"] = float(np.max(f64(np.abs(ct.T @ r)) / (U * np.maximum(f64(np.abs(ct).T @ np.abs(r)), 1e-300)), initial=0.0)) if ct.shape[1] else 0.0
    one = max(8.0, 8.0 * max(out["r"], out["s"], out["beta"]))          # ONE factor per case: the largest ratio of the three
    K = {"r": one, "s": one, "beta": one, "ctr": max(one, 8.0 * out["ctr"])}
    return K, out


def beta_magnitude(ref):
    """|A^-1| (|Ct|^T |X|): the size of what the solve adds up, p x k."""
    return ref["Ainv_abs"] @ np.asarray(ref["W_abs"], dtype=np.float64) if ref["beta"].shape[0] else np.zeros(ref["beta"].shape)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def splitmix64(x):
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def hashed_covariate(n, seed=7):
    """100 (splitmix64(seed 2^32 + i) >> 11) / 2^53 for i < n."""
    return np.array([100.0 * (splitmix64((seed << 32) + i) >> 11) / 2.0 ** 53 for i in range(n)], dtype=np.float64)


def planted():
    """dict(X: the fixture's log1p values as a dense 600 x 240 f64 array, sum_row)."""
    z = np.load(os.path.join(GOLD, "planted_600x240.npz"))
    n, G = int(z["n_rows"]), int(z["n_cols"])
    X = np.zeros((n, G), dtype=np.float64)
    indptr = z["indptr"].astype(np.int64)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    X[rows, z["indices"].astype(np.int64)] = z["log_values"]
    return {"X": X, "sum_row": z["sum_row"].astype(np.float64)}


def planted_covariates(p, seed=7):
    """p in {0, 2}: the cells' total counts and the hashed covariate."""
    pl = planted()
    return np.stack([pl["sum_row"], hashed_covariate(pl["X"].shape[0], seed)], axis=1)[:, :p]


PCA_CASES = [(k, p, mv) for k in (64, 240) for p in (0, 2) for mv in (0.0, 3.0)]
PCA_SEED = 7           # the hashed covariate's seed: changed, not the conditions, should a case miss one (test_regress_cpu.py)


def walk_covariates(X, p):
    """n x p for the shape walk: the cells' sums of X, then hashed covariates with seeds 7, 8, ..."""
    n = X.shape[0]
    cols = [X.sum(axis=1)] + [hashed_covariate(n, 7 + q) for q in range(max(p - 1, 0))]
    return np.stack(cols, axis=1)[:, :p] if p else np.zeros((n, 0))


def walk_case(n, k, dtype=np.float64):
    """(X dense f64 as stored at `dtype`, genes uint64 unsorted, position of the listed constant gene or None): log1p of
    pearson_pca_ref.gram_case's counts (from 8 x 8 on: gene 0 all-zero and listed, cell 0 empty).  For k >= 16 one more gene
    holds 1.5 in every cell and takes the place of the list's last gene: cell 0 then stores that entry alone."""
    Xc, genes = P.gram_case(n, k)
    X = np.log1p(Xc.astype(np.float64))
    const_pos = None
    if k >= 16:
        X = np.concatenate([X, np.full((n, 1), 1.5)], axis=1)
        genes = genes.copy()
        const_pos = k - 1 if genes[k - 1] != 0 else k - 2
        genes[const_pos] = X.shape[1] - 1
    return X.astype(dtype).astype(np.float64), genes, const_pos

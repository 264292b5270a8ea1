"""Host restatement of the neighbour-graph definition of include/srx.h (numpy / scipy), independent of the device code:
rho, c, the root of S(s) = log2(k + 1) by bisection in f64 until the bracket is one ulp wide, the floor, the directed
weights, C = A + A^T - A o A^T with exact zeros removed, D, and the counters of srx_graph_info."""
import numpy as np
import scipy.sparse as sp


def _S(c, one, x, s):
    with np.errstate(divide="ignore", over="ignore", under="ignore", invalid="ignore"):
        return c + np.where(one, 0.0, np.exp(-x / s[:, None])).sum(axis=1)


def scales(dist):
    """dist: n x k distances (any order within a row).  Returns a dict of per-row arrays and the n x k weights.  "lo" and
    "hi" are the final bracket of the root (adjacent doubles unless the bisection met S == T on the way; 0 where the row
    has no root): sigma_star is one of the two."""
    d = np.asarray(dist, dtype=np.float64)
    n, k = d.shape
    T = np.log2(k + 1.0)
    rho = np.where(d > 0, d, np.inf).min(axis=1) if k else np.zeros(n)
    all_zero = ~np.isfinite(rho)
    rho[all_zero] = 0.0
    one = d <= rho[:, None]
    c = one.sum(axis=1).astype(np.float64)
    x = np.where(one, 0.0, d - rho[:, None])
    has_root = ~all_zero & (c < T)
    sig, sig_lo, sig_hi = np.zeros(n), np.zeros(n), np.zeros(n)
    r = np.nonzero(has_root)[0]
    if len(r):
        cr, oner, xr = c[r], one[r], x[r]
        lo = xr.max(axis=1)
        hi = lo.copy()
        below = _S(cr, oner, xr, lo) < T
        for _ in range(2200):                       # bracket upwards where S(lo) < T
            m = below & (hi <= lo)
            if not m.any():
                break
            cand = lo * 2.0
            ok = _S(cr, oner, xr, cand) >= T
            hi = np.where(m & ok, cand, hi)
            lo = np.where(m & ~ok, cand, lo)
        for _ in range(2200):                       # ... downwards where S(hi) >= T
            m = ~below & (lo >= hi)
            if not m.any():
                break
            cand = hi * 0.5
            ok = (_S(cr, oner, xr, cand) < T) | (cand == 0)
            lo = np.where(m & ok, cand, lo)
            hi = np.where(m & ~ok, cand, hi)
        for _ in range(200):                        # bisection until the bracket is one ulp wide
            mid = lo + 0.5 * (hi - lo)
            m = (mid > lo) & (mid < hi)
            if not m.any():
                break
            up = _S(cr, oner, xr, mid) < T
            lo = np.where(m & up, mid, lo)
            hi = np.where(m & ~up, mid, hi)
        better_lo = np.abs(_S(cr, oner, xr, lo) - T) < np.abs(_S(cr, oner, xr, hi) - T)
        sig[r] = np.where(better_lo & (lo > 0), lo, hi)
        sig_lo[r], sig_hi[r] = lo, hi
    floor = 1e-3 * d.sum(axis=1) / (k + 1.0)
    clamped = ~all_zero & (floor > sig)
    sigma = np.where(all_zero, 0.0, np.maximum(sig, floor))
    a = weights(d, rho, sigma)
    return {"T": T, "rho": rho, "c": c, "sigma_star": sig, "floor": floor, "sigma": sigma, "has_root": has_root,
            "clamped": clamped, "all_zero": all_zero, "lo": sig_lo, "hi": sig_hi}, a


def weights(d, rho, sigma):
    """a_ij from the distances and the two scales (also how the tests recover the device's weights)."""
    one = d <= rho[:, None]
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        a = np.exp(-(d - rho[:, None]) / sigma[:, None])
    return np.where(one, 1.0, a)


def graph(idx, dist):
    """The whole restatement: returns (D csr, C csr, per-row dict, A csr with explicit zeros kept, info dict)."""
    idx = np.asarray(idx, dtype=np.int64)
    n, k = idx.shape
    sc, a = scales(dist)
    ptr = np.arange(0, n * k + 1, k, dtype=np.int64)
    # (copies: sort_indices works in place and must not reorder the caller's arrays)
    D = sp.csr_matrix((np.array(dist, dtype=np.float64).ravel(), idx.ravel().copy(), ptr), shape=(n, n))
    A = sp.csr_matrix((a.ravel(), idx.ravel().copy(), ptr.copy()), shape=(n, n))
    D.sort_indices()
    A.sort_indices()
    C = (A + A.T - A.multiply(A.T)).tocsr()
    C.eliminate_zeros()
    C.sort_indices()
    B = sp.csr_matrix((np.ones(n * k), idx.ravel(), ptr), shape=(n, n))      # the k-NN edges as a pattern
    union = (B + B.T).nnz
    info = {"n": n, "k": k, "nnz_distances": n * k, "nnz_connectivities": int(C.nnz),
            "n_mutual": int(B.multiply(B.T).nnz) // 2, "rows_no_root": int((~sc["has_root"]).sum()),
            "rows_clamped": int(sc["clamped"].sum()), "rows_all_zero": int(sc["all_zero"].sum()),
            "entries_dropped": int(union - C.nnz), "max_row_nnz": int(np.diff(C.indptr).max()) if n else 0}
    return D, C, sc, A, info

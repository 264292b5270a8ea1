"""Host restatement of the "new cells on a fitted data set" section of include/srx.h in numpy, independent of the device code:
the row in ascending reference order, the nearest entry, the membership scale by the header's bracket-and-halve rule, the
weights, the start, srx_umap's schedule and epoch on the bipartite entries (the building blocks of tests/umap_ref.py, imported),
the exact counters and the label vote.

Every function takes a ``dtype``.  np.float64 IS the definition: the same operations in the same order, the 64-slot butterfly
sums included.  np.longdouble measures the definition's own error: positions, weights and sums are long double, and the root is
then bisected until its bracket is one long-double ulp wide instead of stopping at |S - T| <= 1e-13, so that
D = max |f64 - longdouble| includes how far the f64 rule's stop leaves sigma from the root itself (two valid evaluations of the
rule can stop one halving apart when an S lands within rounding of the stop's threshold).  The schedule (which entry acts in which
epoch) is a function of the f64 weights in either case, as in umap_ref.layout."""
import numpy as np

import umap_ref as U

WAVE = 64
GROUP = 8                     # SRX_UMAP_GROUP
CHUNK = 64                    # SRX_UMAP_TRANSFORM_CHUNK
STOP = 1e-13                  # the f64 rule's stop on |S(mid) - T|


def default_epochs(n_query):
    return 100 if n_query <= 10000 else 30


def butterfly(v):
    """Row sums of an n x m array (m <= 64) in the order of the device's wave_sum: the row padded with zeros to 64 slots, then
    for off = 32, 16, 8, 4, 2, 1 every slot becomes itself plus slot (s xor off); slot 0 (any slot) holds the sum."""
    v = np.asarray(v)
    n, m = v.shape
    p = np.zeros((n, WAVE), dtype=v.dtype)
    p[:, :m] = v
    s = np.arange(WAVE)
    off = WAVE // 2
    while off:
        p = p + p[:, s ^ off]
        off //= 2
    return p[:, 0]


def sort_rows(idx, dist):
    """(columns, distances) of every row in ascending reference index: slot order."""
    idx = np.asarray(idx)
    order = np.argsort(idx, axis=1, kind="stable")
    return np.take_along_axis(idx, order, axis=1), np.take_along_axis(np.asarray(dist), order, axis=1)


def _S(one, far, x, s):
    with np.errstate(divide="ignore", over="ignore", under="ignore", invalid="ignore"):
        terms = np.where(far, np.exp(-x / s[:, None]), x.dtype.type(0))
    return butterfly(np.where(one, x.dtype.type(1), terms))


def root(one, far, x, T, dtype=np.float64):
    """The header's rule for every row (all of them have a root): returns the upper end of the last bracket."""
    ty = np.dtype(dtype).type
    big = ty(np.finfo(np.float64).max)
    lo = x.max(axis=1)
    hi = lo.copy()
    below = _S(one, far, x, lo) < T
    live = below.copy()
    for _ in range(2200):                           # S(lo) < T: double hi until S(hi) >= T
        if not live.any():
            break
        with np.errstate(over="ignore"):
            cand = lo * ty(2)
            done = ~(cand <= big) | (_S(one, far, x, cand) >= T)
        hi = np.where(live, cand, hi)
        lo = np.where(live & ~done, cand, lo)
        live = live & ~done
    live = ~below
    for _ in range(2200):                           # else: halve lo until S(lo) < T
        if not live.any():
            break
        cand = hi * ty(0.5)
        done = (cand == 0) | (_S(one, far, x, cand) < T)
        lo = np.where(live, cand, lo)
        hi = np.where(live & ~done, cand, hi)
        live = live & ~done
    live = np.ones(len(lo), dtype=bool)
    exact = np.dtype(dtype) != np.float64           # long double: the root itself, no early stop
    for _ in range(128 if not exact else 400):
        mid = lo + ty(0.5) * (hi - lo)
        live = live & (mid > lo) & (mid < hi)
        if not live.any():
            break
        S = _S(one, far, x, mid)
        stop = live & (np.abs(S - T) <= ty(STOP)) & (not exact)
        up = S < T
        hi = np.where(stop | (live & ~up), mid, hi)
        lo = np.where(live & ~stop & up, mid, lo)
        live = live & ~stop
    return hi


def membership(idx, dist, dtype=np.float64):
    """Per-row dict of the membership stage: cols (slot order), d, nearest (slot), T, has_root, clamped, all_zero, sigma_star,
    floor, sigma, w (n x kq)."""
    ty = np.dtype(dtype).type
    cols, d64 = sort_rows(idx, np.asarray(dist, dtype=np.float64))
    d = d64.astype(dtype)
    n, kq = d.shape
    T = np.log2(ty(kq))
    nearest = np.argmin(d, axis=1) if n else np.zeros(0, dtype=np.int64)   # the first minimum: the lowest index among equals
    in_sum = np.ones((n, kq), dtype=bool)
    in_sum[np.arange(n), nearest] = False
    all_zero = ~(d.max(axis=1) > 0) if n else np.zeros(0, dtype=bool)
    far = in_sum & (d > 0)
    one = in_sum & ~far
    c = one.sum(axis=1)
    x = np.where(far, d, ty(0))
    has_root = ~all_zero & (c.astype(dtype) < T)
    sig = np.zeros(n, dtype=dtype)
    r = np.nonzero(has_root)[0]
    if len(r):
        sig[r] = root(one[r], far[r], x[r], T, dtype)
    with np.errstate(over="ignore"):
        sum_d = np.where(np.isinf(butterfly(d64)), ty(np.inf), butterfly(d))     # a sum that overflows in f64 is +inf in any dtype
        floor = ty(1e-3) * sum_d / ty(kq)
    clamped = ~all_zero & (floor > sig)
    sigma = np.where(all_zero, ty(0), np.where(clamped, floor, sig))
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        w = np.where(d > 0, np.exp(-d / sigma[:, None]), ty(1))
    return {"cols": cols, "d": d, "nearest": nearest, "T": T, "one": one, "far": far, "has_root": has_root, "clamped": clamped,
            "all_zero": all_zero, "sigma_star": sig, "floor": floor, "sigma": sigma, "w": w}


def start(w, cols, Yref, nearest, dtype=np.float64):
    """(y0 n x dim, the rows that start at their nearest entry because W == 0)."""
    w = np.asarray(w, dtype=dtype)
    Y = np.asarray(Yref, dtype=dtype)
    n, kq = w.shape
    W = butterfly(w)
    from_nearest = W == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        f = w / W[:, None]
    y0 = np.zeros((n, Y.shape[1]), dtype=dtype)
    for c in range(Y.shape[1]):
        y0[:, c] = butterfly(f * Y[cols, c])
    if from_nearest.any():
        rows = np.nonzero(from_nearest)[0]
        y0[rows] = Y[cols[rows, nearest[rows]]]
    return y0, from_nearest


def epochs(cols, w, Yref, Y0, a, b, n_epochs, gamma=1.0, rate=5, alpha0=0.25, seed=0, stop_after=0, dtype=np.float64, first_epoch=1):
    """Epochs first_epoch .. (stop_after or n_epochs) of the n_epochs schedule on the query positions Y0; w: the f64 weights (the
    schedule).  Returns (Y, counters)."""
    cols = np.asarray(cols, dtype=np.int64)
    nq, kq = cols.shape
    nnz, n_ref = nq * kq, len(Yref)
    ty = np.dtype(dtype).type
    Yr = np.asarray(Yref, dtype=dtype)
    Y = np.array(Y0, dtype=dtype, copy=True)
    E, last = int(n_epochs), int(stop_after or n_epochs)
    info = {"entries_active": 0, "samples": 0, "negatives": 0, "epochs_run": 0, "w_max": 0.0}
    if nnz == 0:
        return Y, info
    w = np.asarray(w, dtype=np.float64).ravel()
    rows = np.repeat(np.arange(nq, dtype=np.int64), kq)
    ind = cols.ravel()
    r = U.ratios(w)
    info["w_max"] = float(w.max())
    info["entries_active"] = int((np.floor(np.float64(E) * r) > 0).sum())
    a_, b_, bm1 = ty(np.float64(a)), ty(np.float64(b)), ty(np.float64(b) - 1.0)
    att, rep = ty(-2.0 * np.float64(a) * np.float64(b)), ty(2.0 * np.float64(gamma) * np.float64(b))
    one, four, eps = ty(1.0), ty(4.0), ty(np.float64(0.001))
    for t in range(first_epoch, last + 1):
        alpha = np.float64(alpha0) * (1.0 - np.float64(t - 1) / np.float64(E))
        e = np.nonzero(U.sampled(r, t))[0]
        i, j = rows[e], ind[e]
        delta = np.zeros_like(Y)
        yi = Y[i]
        d = yi - Yr[j]
        d2 = U._d2(d)
        ok = d2 > 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            q = np.where(ok, att * d2 ** bm1 / (a_ * d2 ** b_ + one), ty(0.0))
        g = np.clip(q[:, None] * d, -four, four)
        g[~ok] = 0
        U._add_rows(delta, i, ty(alpha) * g)                    # the head move alone: the reference does not move
        info["samples"] += len(e)
        if rate:
            k = U.negative_targets(seed, t, nnz, e, rate, n_ref).astype(np.int64)
            for p in range(rate):
                d = yi - Yr[k[:, p]]                            # a target is a reference point: none is skipped
                d2 = U._d2(d)
                ok = d2 > 0
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    q = np.where(ok, rep / ((eps + d2) * (a_ * d2 ** b_ + one)), ty(0.0))
                g = np.clip(q[:, None] * d, -four, four)
                g[~ok] = 0
                U._add_rows(delta, i, ty(alpha) * g)
        Y = Y + delta
        info["epochs_run"] += 1
    info["negatives"] = info["samples"] * int(rate)
    return Y, info


COUNTERS = ("entries_active", "samples", "negatives", "rows_no_root", "rows_clamped", "rows_all_zero", "rows_start_nearest")


def transform(idx, dist, Yref, a, b, n_epochs=0, gamma=1.0, rate=5, alpha0=0.25, seed=0, stop_after=0, dtype=np.float64):
    """The whole restatement.  Returns (Y, info, parts) with parts = the membership dict plus "start"."""
    idx = np.asarray(idx)
    nq, kq = idx.shape
    Yref = np.asarray(Yref, dtype=np.float64)
    E = int(n_epochs) or default_epochs(nq)
    m = membership(idx, dist, dtype)
    w_sched = m["w"] if np.dtype(dtype) == np.float64 else membership(idx, dist, np.float64)["w"]
    y0, from_nearest = start(m["w"], m["cols"], Yref, m["nearest"], dtype)
    Y, c = epochs(m["cols"], w_sched, Yref, y0, a, b, E, gamma, rate, alpha0, seed, stop_after, dtype)
    info = {"n_query": nq, "n_ref": len(Yref), "kq": kq, "dim": Yref.shape[1], "n_epochs": E,
            "epochs_run": c["epochs_run"] if nq else 0, "entries_active": c["entries_active"], "samples": c["samples"],
            "negatives": c["negatives"], "rows_no_root": int((~m["has_root"]).sum()), "rows_clamped": int(m["clamped"].sum()),
            "rows_all_zero": int(m["all_zero"].sum()), "rows_start_nearest": int(from_nearest.sum()), "w_max": c["w_max"]}
    parts = dict(m)
    parts["start"] = y0
    return Y, info, parts


def vote(idx, ref_labels):
    """(label, count) per row: the label that occurs most often among the row's references, ties to the lowest label."""
    idx = np.asarray(idx, dtype=np.int64)
    lab = np.asarray(ref_labels)[idx]
    out = np.zeros((len(idx), 2), dtype=np.uint32)
    for i, row in enumerate(lab):
        vals, cnts = np.unique(row, return_counts=True)
        m = cnts.max()
        out[i] = (vals[cnts == m].min(), m)
    return out[:, 0].copy(), out[:, 1].copy()

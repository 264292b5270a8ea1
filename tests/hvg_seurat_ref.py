"""Host reference of the Seurat v3 gene selection as include/srx.h restates it (srx_select_hvg_seurat_v3, srx_loess_direct,
srx_clipped_group_moments): every step in numpy in the stated operation order (numpy rounds each operation once and never
contracts), the fixed-point sums as exact integers.  Test-side only: the product never imports it.

The integer sums are int64: the scales of srx.h keep every total below 2^62, so int64 addition is exact integer addition."""
import math

import numpy as np
import scipy.sparse as sp

import markers_ref

RANK_TOL = 2.0 ** -33          # the degree rule of srx.h


# ---- step 2: direct loess ----------------------------------------------------------------------------------------------------------
def window(m, span):
    return min(m, max(1, int(math.floor(span * m + 1e-5))))


def loess_direct(x, y, span, dtype=np.float64, degrees=None):
    """e_j of srx.h for every point, evaluated in `dtype` (np.longdouble: the second reference the tolerance comes from).  The
    sums run over the weighted points in ascending (x, index): the device's differ in their order only.  `degrees`: an int
    array of m entries that receives the degree the rule on the moments chose for every point."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    m = x.size
    out = np.zeros(m, dtype)
    if m == 0:
        return out
    order = np.lexsort((np.arange(m), x))
    xs, ys = x[order].astype(dtype), y[order].astype(dtype)
    q = window(m, span)
    one, tol = dtype(1), dtype(RANK_TOL)
    for p in range(m):
        d = np.abs(xs - xs[p])
        h = np.partition(d, q - 1)[q - 1]
        if h > 0:
            sel = d < h
            t = (xs[sel] - xs[p]) / h
            u = np.abs(t)
            c = one - (u * u) * u
            w = (c * c) * c
        else:
            sel = d == 0
            t = np.zeros(int(sel.sum()), dtype)
            w = np.ones(int(sel.sum()), dtype)
        yy = ys[sel]
        wt = w * t
        wt2 = wt * t
        wt3 = wt2 * t
        m0, m1, m2, m3, m4 = w.sum(), wt.sum(), wt2.sum(), wt3.sum(), (wt3 * t).sum()
        b0, b1, b2 = (w * yy).sum(), (wt * yy).sum(), (wt2 * yy).sum()
        c00 = m2 * m4 - m3 * m3
        c01 = m1 * m4 - m2 * m3
        c02 = m1 * m3 - m2 * m2
        det = (m0 * c00 - m1 * c01) + m2 * c02
        d2 = m0 * m2 - m1 * m1
        if det > tol * ((m0 * m2) * m4):
            fit, deg = ((b0 * c00 - m1 * (b1 * m4 - b2 * m3)) + m2 * (b1 * m3 - b2 * m2)) / det, 2
        elif d2 > tol * (m0 * m2):
            fit, deg = (b0 * m2 - b1 * m1) / d2, 1
        else:
            fit, deg = b0 / m0, 0
        if degrees is not None:
            degrees[order[p]] = deg
        out[order[p]] = fit
    return out


def loess_degree(x, span):
    """The degree the rule gives every point, and the number of distinct weighted abscissae, for the tests' own checks."""
    x = np.asarray(x, np.float64)
    m = x.size
    q = window(m, span)
    deg, distinct = np.zeros(m, int), np.zeros(m, int)
    for p in range(m):
        d = np.abs(x - x[p])
        h = np.partition(d, q - 1)[q - 1]
        sel = d < h if h > 0 else d == 0
        distinct[p] = np.unique(x[sel]).size
        deg[p] = min(2, distinct[p] - 1)
    return deg, distinct


def loess_polyfit(x, y, span):
    """The same fit by np.polyfit on the weighted points, where they hold three distinct abscissae or more (NaN elsewhere):
    an implementation that shares nothing with loess_direct but the window and the weights."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    m = x.size
    q = window(m, span)
    out = np.full(m, np.nan)
    for p in range(m):
        d = np.abs(x - x[p])
        h = np.partition(d, q - 1)[q - 1]
        if not h > 0:
            continue
        sel = d < h
        if np.unique(x[sel]).size < 3:
            continue
        t = (x[sel] - x[p]) / h
        w = (1 - np.abs(t) ** 3) ** 3
        out[p] = np.polyval(np.polyfit(t, y[sel], 2, w=np.sqrt(w)), 0.0)
    return out


def loess_bound(cases):
    """The tolerance of a device fit against loess_direct in f64: 8 x the largest |f64 - long double| over the given
    (x, y, span) cases.  Device and reference differ in the order of eight sums only; the factor is headroom for another
    summation tree.  Never computed from the device's output."""
    worst = 0.0
    for x, y, span in cases:
        a = loess_direct(x, y, span)
        b = loess_direct(x, y, span, np.longdouble)
        if a.size:
            worst = max(worst, float(np.abs(a.astype(np.longdouble) - b).max()))
    return 8.0 * worst, worst


# ---- steps 1 and 3: the fixed-point sums -------------------------------------------------------------------------------------------
def fixed(v, scale_log2):
    """round(v 2^s), ties to even, as int64 (|.| < 2^62 by the choice of the scales)."""
    return np.rint(np.ldexp(np.asarray(v, np.float64), int(scale_log2))).astype(np.int64)


def grouped_int(X, labels, n_groups, scales, clip=None):
    """(S_int, Q_int) per (group, gene) of min(x, clip[group, gene]) (clip None: of x) at the two scales."""
    X = sp.csr_matrix(X)
    X.sort_indices()
    labels = np.asarray(labels, np.int64)
    rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    g, j = labels[rows], X.indices.astype(np.int64)
    v = X.data.astype(np.float64)
    if clip is not None:
        v = np.minimum(v, np.asarray(clip, np.float64)[g, j])
    S = np.zeros((n_groups, X.shape[1]), np.int64)
    Q = np.zeros((n_groups, X.shape[1]), np.int64)
    np.add.at(S, (g, j), fixed(v, scales[0]))
    np.add.at(Q, (g, j), fixed(v * v, scales[1]))
    return S, Q


def unfix(a, scale_log2):
    return np.ldexp(np.asarray(a, np.int64).astype(np.float64), -int(scale_log2))


def scales_of(X):
    X = sp.csr_matrix(X)
    return markers_ref.scales(float(np.abs(X.data).max()) if X.nnz else 0.0, X.shape[0])


def moments(S, Q, sizes):
    """mean and var of step 1 from the f64 sums (sizes: cells per batch, or the cell count for the totals)."""
    n = np.asarray(sizes, np.float64).reshape(-1, 1) if np.ndim(sizes) else np.float64(sizes)
    mean = S / n
    with np.errstate(invalid="ignore"):
        var = (Q / n - mean * mean) * (n / (n - 1.0))
    return mean, var


def trend(mean, var, span, dtype=np.float64):
    """e per (batch, gene): the direct loess over the genes with var > 0, 0 elsewhere."""
    e = np.zeros(mean.shape, dtype)
    for b in range(mean.shape[0]):
        ok = var[b] > 0
        e[b, ok] = loess_direct(np.log10(mean[b, ok]), np.log10(var[b, ok]), span, dtype)
    return e


def reg_var_of(fitted):
    """10^e as numpy's pow gives it: the one operation of the method that is not correctly rounded anywhere."""
    return 10.0 ** fitted


def clip_of(mean, reg_var, sizes):
    n = np.asarray(sizes, np.float64).reshape(-1, 1)
    return np.sqrt(reg_var) * np.sqrt(n) + mean


def nv_of(mean, reg_var, clip_sum, clip_sumsq, sizes):
    n = np.asarray(sizes, np.float64).reshape(-1, 1)
    return ((n * (mean * mean) + clip_sumsq) - (2.0 * clip_sum) * mean) / ((n - 1.0) * reg_var)


# ---- steps 4 and 5: integer logic ----------------------------------------------------------------------------------------------------
def ranks_of(nv):
    """rank[b, j] = the number of genes before j under (nv descending, gene index ascending)."""
    nv = np.asarray(nv)
    out = np.zeros(nv.shape, np.uint32)
    idx = np.arange(nv.shape[1])
    for b in range(nv.shape[0]):
        out[b, np.lexsort((idx, -nv[b]))] = idx
    return out


def combine(rank, n_top):
    """(nbatches u32, median f64 with NaN where nbatches == 0)."""
    rank = np.asarray(rank, np.int64)
    G = rank.shape[1]
    top = min(int(n_top), G)
    nb = (rank < top).sum(axis=0).astype(np.uint32)
    med = np.full(G, np.nan)
    for j in range(G):
        r = np.sort(rank[rank[:, j] < top, j])
        if r.size:
            med[j] = (int(r[(r.size - 1) // 2]) + int(r[r.size // 2])) / 2.0
    return nb, med


def final_order(median, nbatches, paper=False):
    """Every gene in the final order."""
    G = median.size
    idx = np.arange(G)
    med = np.where(np.isnan(median), np.inf, median)
    nbn = -np.asarray(nbatches, np.int64)
    return np.lexsort((idx, med, nbn)) if paper else np.lexsort((idx, nbn, med))


def select(median, nbatches, n_top, paper=False):
    return final_order(median, nbatches, paper)[:min(int(n_top), median.size)].astype(np.uint64)


def run(X, batch, n_batches, n_top, span=0.3, paper=False):
    """The whole definition from the counts: a dict of every table of srx_seurat_v3_tables and the selection."""
    X = sp.csr_matrix(X)
    N, G = X.shape
    batch = np.zeros(N, np.int64) if batch is None else np.asarray(batch, np.int64)
    sc = scales_of(X)
    sizes = np.bincount(batch, minlength=n_batches)
    S, Q = grouped_int(X, batch, n_batches, sc)
    mean, var = moments(unfix(S, sc[0]), unfix(Q, sc[1]), sizes)
    fitted = trend(mean, var, span)
    reg_var = reg_var_of(fitted)
    clip = clip_of(mean, reg_var, sizes)
    Sc, Qc = grouped_int(X, batch, n_batches, sc, clip)
    cs, cq = unfix(Sc, sc[0]), unfix(Qc, sc[1])
    nv = nv_of(mean, reg_var, cs, cq, sizes)
    rank = ranks_of(nv)
    nb, med = combine(rank, n_top)
    means, variances = moments(unfix(S.sum(axis=0), sc[0]), unfix(Q.sum(axis=0), sc[1]), N)
    vn = np.zeros(G)
    for b in range(n_batches):
        vn = vn + nv[b]
    return {"sizes": sizes, "scales": sc, "mean": mean, "var": var, "fitted": fitted, "reg_var": reg_var, "clip": clip, "clip_sum": cs, "clip_sumsq": cq,
            "nv": nv, "rank": rank, "nbatches": nb, "median": med, "means": means, "variances": variances,
            "variances_norm": vn / n_batches, "selected": select(med, nb, n_top, paper)}


# ---- inputs the tests share ----------------------------------------------------------------------------------------------------------
def hashed_batches(n, k):
    """A batch per cell from a multiplicative hash of its index: interleaved, unequal sizes, the same everywhere."""
    i = np.arange(n, dtype=np.uint64)
    return (((i * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(k)).astype(np.uint32)


LOESS_SIZES = (1, 2, 3, 4, 63, 64, 65, 257, 1100)          # 1100: more points than a workgroup (and a wave) is wide


def loess_cases():
    """(name, x, y, span) of every case of the loess kernel's own test: the sizes at four spans (0.3, 1.0, one giving q = 1, one
    giving q = 2), and the degenerate and tied inputs."""
    rng = np.random.default_rng(2024)
    out = []
    for m in LOESS_SIZES:
        x = rng.uniform(-3.0, 2.0, m)
        y = 0.8 * x + 0.3 * np.sin(2.0 * x) + rng.normal(0.0, 0.2, m)
        for tag, span in (("s03", 0.3), ("s10", 1.0), ("q1", 1.2 / m), ("q2", 2.2 / m)):
            if span <= 1.0:
                out.append(("m%d_%s" % (m, tag), x, y, span))
    x = rng.uniform(0.0, 1.0, 40)
    y = rng.normal(0.0, 1.0, 40)
    xr = x.copy()
    xr[5:25] = 0.5                                           # a run of 20 identical x, q = 12: h == 0 on the run
    out.append(("run_longer_than_q", xr, y, 0.3))
    xq = x.copy()
    xq[5:17] = 0.5                                           # a run of exactly q = 12
    out.append(("run_of_exactly_q", xq, y, 0.3))
    x2 = np.where(np.arange(40) % 3 == 0, 0.25, 0.75)        # two distinct abscissae: degree 1 at span 1, degree 0 below
    out.append(("two_values_span1", x2, y, 1.0))
    out.append(("two_values_span03", x2, y, 0.3))
    xt = rng.uniform(-1.0, 1.0, 130)
    xt[[3, 77, 128]] = xt[40]                                # tied fit points at different input positions
    out.append(("tied_points", xt, rng.normal(0.0, 1.0, 130), 0.3))
    out.append(("three_points_q3", np.array([0.0, 1.0, 3.0]), np.array([1.0, 2.0, 0.5]), 1.0))
    return out

"""The definition of srx_autocorr (include/srx.h), written twice.

1. ``tables`` / ``stats``: the five per-gene integer tables and the graph sums exactly as the header states them (every product
   an IEEE double product, rint ties-to-even, the scales), as Python integers, and the statistics from them in
   ``fractions.Fraction``: what the device must reproduce, the tables bit for bit, the statistics within ``bounds``.
2. ``literal_fraction`` / ``literal_f64``: the textbook double sums over the dense, mean-centred column, in Fraction (exact)
   and in numpy f64.

Tolerances.
``bounds``: the header's own statement of what its long double arithmetic loses GIVEN the tables.
``quanta_bounds``: how far the statistics of the tables may lie from the statistics of the stored values themselves, derived
per gene from the table quanta (header: |table - exact| <= terms 2^-(scale + 1)) and den, by first-order propagation with
every partial derivative bounded by absolute values, times 2 for the second-order terms (each relative perturbation involved
is below 2^-20 at the sizes the tests use, so the neglected part is below 2^-19 of the bound).  The terms are counted from
above: N for S, Q, A, B, nnz / 2 for P, nnz for W, a row's length for d_i.
``f64_slack``: what the numpy f64 evaluation of the literal sums may lose itself: (terms + 8) 2^-53 of the sum of the absolute
values of the terms of each sum (the standard bound for recursive summation, pairwise does better), propagated the same way.
"""
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

TILE_GENES = 10000                 # genes.hip: kMaxTileGenes; the walk owns one gene tile of the matrix
WAVES = 16                         # autocorr.hip: kAcThreads / 64, one neighbour per wave


def fx_exponent(v):
    """The smallest integer e with v < 2^e (0 for 0), no lower than -30."""
    return max(math.frexp(float(v))[1], -30) if v else 0


def ceil_log2(n):
    return max(int(n) - 1, 0).bit_length()


def scales(max_abs, max_w, max_d, N, nnz):
    ex, ew, ed = fx_exponent(max_abs), fx_exponent(max_w), fx_exponent(max_d)
    LN, LE = ceil_log2(N), ceil_log2(nnz)
    return {"s_sum": 62 - ex - LN, "s_sumsq": 62 - 2 * ex - LN, "s_dsum": 62 - ed - ex - LN, "s_dsumsq": 62 - ed - 2 * ex - LN,
            "s_cross": 62 - ew - 2 * ex - LE, "s_w": 62 - ew - LE, "s_1": 62 - 2 * ew - LE, "s_2": 62 - 2 * ed - LN}


def _fix(v, s):
    """rint(v 2^s) as int64: the scaling by a power of two is exact, np.rint is ties-to-even, and the result is an integer
    below 2^63 by the scale rule."""
    return np.rint(np.ldexp(np.asarray(v, np.float64), s)).astype(np.int64)


def _pyint(a):
    return [int(v) for v in a]


def graph_sums(W):
    """dq, W, S1, max d of a symmetric scipy CSR graph, and the scales that depend on the graph alone."""
    W = sp.csr_matrix(W)
    n = W.shape[0]
    w = W.data.astype(np.float64)
    ew, LE = fx_exponent(w.max()), ceil_log2(W.nnz)
    s_w, s_1 = 62 - ew - LE, 62 - 2 * ew - LE
    rows = np.repeat(np.arange(n), np.diff(W.indptr))
    dq = np.zeros(n, np.int64)
    np.add.at(dq, rows, _fix(w, s_w))
    d = np.ldexp(dq.astype(np.float64), -s_w)                  # f64(dq) converted once (ties to even), then scaled exactly
    return {"dq": dq, "d": d, "w_int": int(dq.sum()), "s1_int": int(_fix(w * w, s_1).sum()), "max_weight": float(w.max()),
            "max_degree": float(d.max())}


def tables(X, W):
    """The five tables (lists of Python integers) and the info of the header for the stored values of the scipy CSR X (already
    at the storage precision, held as f64) and the symmetric scipy CSR graph W with sorted rows."""
    X = sp.csr_matrix(X)
    W = sp.csr_matrix(W)
    W.sort_indices()
    N, G = X.shape
    x = X.data.astype(np.float64)
    gs = graph_sums(W)
    max_abs = float(np.abs(x).max()) if x.size else 0.0
    sc = scales(max_abs, gs["max_weight"], gs["max_degree"], N, W.nnz)
    rows = np.repeat(np.arange(N), np.diff(X.indptr))
    cols = X.indices.astype(np.int64)
    d = gs["d"][rows]
    xx = x * x
    t = {k: np.zeros(G, np.int64) for k in ("sum_int", "sumsq_int", "dsum_int", "dsumsq_int", "cross_int")}
    np.add.at(t["sum_int"], cols, _fix(x, sc["s_sum"]))
    np.add.at(t["sumsq_int"], cols, _fix(xx, sc["s_sumsq"]))
    np.add.at(t["dsum_int"], cols, _fix(d * x, sc["s_dsum"]))
    np.add.at(t["dsumsq_int"], cols, _fix(d * xx, sc["s_dsumsq"]))
    for i in range(N):
        gi = X.indices[X.indptr[i]:X.indptr[i + 1]]
        xi = x[X.indptr[i]:X.indptr[i + 1]]
        for e in range(W.indptr[i], W.indptr[i + 1]):
            j = int(W.indices[e])
            if j <= i or not gi.size:
                continue
            gj = X.indices[X.indptr[j]:X.indptr[j + 1]]
            common, ai, aj = np.intersect1d(gi, gj, assume_unique=True, return_indices=True)
            if common.size:
                prod = xi[ai] * x[X.indptr[j]:X.indptr[j + 1]][aj]                  # the product of the two values, rounded first
                np.add.at(t["cross_int"], common, _fix(float(W.data[e]) * prod, sc["s_cross"]))
    s2 = int(_fix(gs["d"] * gs["d"], sc["s_2"]).sum())
    out = {k: _pyint(v) for k, v in t.items()}
    out["info"] = dict(sc, n=N, n_genes=G, nnz=int(W.nnz), max_abs=max_abs, max_weight=gs["max_weight"], max_degree=gs["max_degree"],
                       w_int=gs["w_int"], s1_int=gs["s1_int"], s2_int=s2)
    return out


def _unscale(v, s):
    return Fraction(v) / Fraction(2) ** s


def moments_of_graph(info):
    """(s0, s1, s2, E[I], Var[I], E[C], Var[C]) as Fractions."""
    N = Fraction(info["n"])
    s0 = _unscale(info["w_int"], info["s_w"])
    s1 = 2 * _unscale(info["s1_int"], info["s_1"])
    s2 = 4 * _unscale(info["s2_int"], info["s_2"])
    e_i = Fraction(-1) / (N - 1)
    var_i = (N * N * s1 - N * s2 + 3 * s0 * s0) / ((N * N - 1) * s0 * s0) - e_i * e_i
    var_c = ((2 * s1 + s2) * (N - 1) - 4 * s0 * s0) / (2 * (N + 1) * s0 * s0)
    return s0, s1, s2, e_i, var_i, Fraction(1), var_c


def _sqrt(fr):
    getcontext().prec = 60
    return (Decimal(fr.numerator) / Decimal(fr.denominator)).sqrt()


def _z(stat, e, var):
    if stat is None or var <= 0:
        return None
    getcontext().prec = 60
    d = stat - e
    return float(Decimal(d.numerator) / Decimal(d.denominator) / _sqrt(var))


def stats(t):
    """Per gene (I, C, z_I, z_C, terms): I and C Fractions or None for a constant gene, z floats (60-digit decimal square
    root) or None; terms = the (t1, t2, t3, den) of the header, for its bound."""
    info = t["info"]
    N = Fraction(info["n"])
    s0, _, _, e_i, var_i, e_c, var_c = moments_of_graph(info)
    out = []
    for g in range(len(t["sum_int"])):
        if not t["sumsq_int"][g]:                                  # Q = 0: den = -S^2 / N <= 0 (most genes of the wide test shapes)
            out.append((None, None, None, None, None))
            continue
        S, Q = _unscale(t["sum_int"][g], info["s_sum"]), _unscale(t["sumsq_int"][g], info["s_sumsq"])
        A, B = _unscale(t["dsum_int"][g], info["s_dsum"]), _unscale(t["dsumsq_int"][g], info["s_dsumsq"])
        P = _unscale(t["cross_int"][g], info["s_cross"])
        den = Q - S * S / N
        if den <= 0:
            out.append((None, None, None, None, None))
            continue
        t1, t2, t3 = 2 * P, 2 * S * A / N, S * S * s0 / (N * N)
        I = N * (t1 - t2 + t3) / (s0 * den)
        Cc = (N - 1) * (B - 2 * P) / (s0 * den)
        out.append((I, Cc, _z(I, e_i, var_i), _z(Cc, e_c, var_c), (t1, t2, t3, den)))
    return out


def bounds(t, st):
    """The header's bounds given the tables, per gene: (b_I, b_C, b_zI, b_zC) as floats (None for a constant gene).  z adds the
    rounding of Var, the square root and the quotient (2^-50 relative) to stat's bound over sd."""
    info = t["info"]
    N = Fraction(info["n"])
    s0, _, _, _, var_i, _, var_c = moments_of_graph(info)
    out = []
    for I, Cc, zi, zc, terms in st:
        if I is None:
            out.append(None)
            continue
        t1, t2, t3, den = terms
        b_i = abs(I) / 2 ** 52 + (N / (s0 * den)) * (abs(t1) + abs(t2) + abs(t3)) / 2 ** 60
        b_c = abs(Cc) / 2 ** 52
        b_zi = float(b_i) / math.sqrt(var_i) + abs(zi) * 2.0 ** -50 if zi is not None else None
        b_zc = float(b_c) / math.sqrt(var_c) + abs(zc) * 2.0 ** -50 if zc is not None else None
        out.append((float(b_i), float(b_c), b_zi, b_zc))
    return out


# ---- the literal double sums --------------------------------------------------------------------------------------------------
def literal_fraction(Xd, Wd):
    """(I, C) per gene, Fractions or None, from the textbook sums over the dense X (N x G) and dense W (N x N), exactly."""
    N, G = len(Xd), len(Xd[0])
    Wf = [[Fraction(v) for v in row] for row in Wd]
    edges = [(i, j, Wf[i][j]) for i in range(N) for j in range(N) if Wf[i][j]]
    s0 = sum(w for _, _, w in edges)
    out = []
    for g in range(G):
        x = [Fraction(Xd[i][g]) for i in range(N)]
        m = sum(x) / N
        z = [v - m for v in x]
        den = sum(v * v for v in z)
        if den <= 0:
            out.append((None, None))
            continue
        I = Fraction(N) / s0 * sum(w * z[i] * z[j] for i, j, w in edges) / den
        Cc = Fraction(N - 1) * sum(w * (x[i] - x[j]) ** 2 for i, j, w in edges) / (2 * s0 * den)
        out.append((I, Cc))
    return out


def literal_f64(X, W):
    """(I, C, parts) per gene in numpy f64 over the dense centred columns; parts = the absolute sums f64_slack needs."""
    Xd = np.asarray(sp.csr_matrix(X).todense(), np.float64)
    W = sp.csr_matrix(W).astype(np.float64)
    N = Xd.shape[0]
    s0 = W.sum()
    Z = Xd - Xd.mean(axis=0)
    den = (Z * Z).sum(axis=0)
    num = (Z * (W @ Z)).sum(axis=0)
    coo = W.tocoo()
    diff = Xd[coo.row] - Xd[coo.col]
    numc = (coo.data[:, None] * diff * diff).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        I = N / s0 * num / den
        Cc = (N - 1) * numc / (2 * s0 * den)
    absW = abs(W)
    parts = {"num_abs": (np.abs(Z) * (absW @ np.abs(Z))).sum(axis=0), "numc": numc, "den": den, "s0": s0}
    return I, Cc, parts


def quanta_bounds(t, X, W):
    """Per gene (b_I, b_C): how far the statistics of the tables may lie from those of the stored values (module docstring)."""
    info = t["info"]
    X = sp.csr_matrix(X)
    W = sp.csr_matrix(W)
    N = info["n"]
    q = lambda s: 2.0 ** -(info[s] + 1)
    row_len = np.diff(W.indptr)
    dd = row_len * q("s_w")                                          # per cell: |d_i - exact row sum|
    absX = abs(X)
    dS, dQ = N * q("s_sum"), N * q("s_sumsq")
    dA = N * q("s_dsum") + np.asarray(absX.T @ dd).ravel()
    dB = N * q("s_dsumsq") + np.asarray(absX.multiply(absX).T @ dd).ravel()
    dP = info["nnz"] / 2 * q("s_cross")
    dW = info["nnz"] * q("s_w")
    s0 = float(_unscale(info["w_int"], info["s_w"]))
    out = []
    for g in range(len(t["sum_int"])):
        S, Q = float(_unscale(t["sum_int"][g], info["s_sum"])), float(_unscale(t["sumsq_int"][g], info["s_sumsq"]))
        A, B = float(_unscale(t["dsum_int"][g], info["s_dsum"])), float(_unscale(t["dsumsq_int"][g], info["s_dsumsq"]))
        P = float(_unscale(t["cross_int"][g], info["s_cross"]))
        m = S / N
        den = Q - N * m * m
        if not den > 0:
            out.append(None)
            continue
        dm = dS / N
        dden = dQ + 2 * abs(m) * dS
        num_i = 2 * P - 2 * m * A + m * m * s0
        dnum_i = 2 * dP + 2 * abs(m) * dA[g] + 2 * abs(A) * dm + 2 * abs(m) * s0 * dm + m * m * dW
        num_c = B - 2 * P
        dnum_c = dB[g] + 2 * dP
        b_i = (N / s0) * (dnum_i / den + abs(num_i) * dden / den ** 2) + abs(N * num_i / (s0 * den)) * dW / s0
        b_c = ((N - 1) / s0) * (dnum_c / den + abs(num_c) * dden / den ** 2) + abs((N - 1) * num_c / (s0 * den)) * dW / s0
        out.append((2 * b_i, 2 * b_c))
    return out


def f64_slack(parts, N, nnz):
    """Per gene (s_I, s_C): what literal_f64 may lose (module docstring).  den and numc are sums of non-negative terms, so
    their absolute sums are themselves."""
    u = 2.0 ** -53
    den, s0 = parts["den"], parts["s0"]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_den = (N + 8) * u * 3                                     # centring, squaring, summing
        s_i = (N / s0) * parts["num_abs"] / den * ((nnz + N + 8) * u * 3 + rel_den)
        s_c = (N - 1) * parts["numc"] / (2 * s0 * den) * ((nnz + 8) * u * 3 + rel_den)
    return s_i, s_c


# ---- generators ------------------------------------------------------------------------------------------------------------------
def symmetric_graph(n, lists, weight):
    """A symmetric CSR graph from {i: iterable of j} (each pair made symmetric, no diagonal); weight(i, j) with i < j."""
    pairs = {}
    for i, js in lists.items():
        for j in js:
            i, j = int(i), int(j)
            if i != j:
                a, b = (i, j) if i < j else (j, i)
                pairs[(a, b)] = weight(a, b)
    r = [a for a, b in pairs] + [b for a, b in pairs]
    c = [b for a, b in pairs] + [a for a, b in pairs]
    v = list(pairs.values()) * 2
    W = sp.csr_matrix((np.array(v, np.float64), (np.array(r, np.int64), np.array(c, np.int64))), shape=(n, n))
    W.sort_indices()
    return W


def random_graph(rng, n, k, dyadic=True):
    """Each vertex names k random others; weights k / 8 (dyadic) or UMAP-like values in (0, 1]."""
    lists = {i: rng.choice(np.delete(np.arange(n), i), size=min(k, n - 1), replace=False) for i in range(n)}
    if dyadic:
        return symmetric_graph(n, lists, lambda a, b: ((a * 7 + b * 3) % 8 + 1) / 8.0)
    return symmetric_graph(n, lists, lambda a, b: float(np.exp(-((a * 31 + b * 17) % 97) / 19.0)))


def as_storage(X, store):
    """The stored values as f64: rounded to f32 first at store 1."""
    X = sp.csr_matrix(X).astype(np.float64)
    X.sort_indices()
    if store == 1:
        X.data = X.data.astype(np.float32).astype(np.float64)
    return X

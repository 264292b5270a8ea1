"""Host restatement of the UMAP layout definition of include/srx.h in vectorised numpy, independent of the device code: the
stateless schedule, the hashed negative samples, the synchronous epoch in any float dtype (f64 is the definition; longdouble
measures its rounding error; f32 shows why the device works in f64), the exact counters, both deterministic starts, the
curve's target, a planted-data generator and the hand-made 12-vertex graph of the golden file."""
import json
import os

import numpy as np
import scipy.sparse as sp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
MASK = (1 << 64) - 1


def mix(z):
    """splitmix64's finaliser on a uint64 array (arithmetic mod 2^64)."""
    z = np.array(z, dtype=np.uint64, ndmin=1, copy=True)
    z ^= z >> np.uint64(30)
    z *= M1
    z ^= z >> np.uint64(27)
    z *= M2
    z ^= z >> np.uint64(31)
    return z


def mix_int(z):
    """The same in Python integers: what the known answers of the golden file were worked out with."""
    z &= MASK
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & MASK
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & MASK
    return z ^ (z >> 31)


def target_int(seed, t, nnz, e, R, p, n):
    """The negative sample of (entry e, epoch t, p) in Python integers."""
    z = mix_int(seed + 0x9E3779B97F4A7C15 * (1 + (t * nnz + e) * R + p))
    return ((z >> 32) * n) >> 32


def negative_targets(seed, t, nnz, e, R, n):
    """len(e) x R targets of the sampled entries e (uint64 array) in epoch t."""
    e = np.asarray(e, dtype=np.uint64)
    first = (np.uint64(t) * np.uint64(nnz) + e) * np.uint64(R) + np.uint64(1)
    idx = first[:, None] + np.arange(R, dtype=np.uint64)[None, :]
    z = mix((np.uint64(seed & MASK) + GOLDEN * idx).ravel()).reshape(idx.shape)
    return ((z >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)


def ratios(w):
    """r_e = w_e / w_max, one f64 division."""
    w = np.asarray(w, dtype=np.float64)
    return w / w.max() if w.size else w


def sampled(r, t):
    """Entry e acts in epoch t iff floor(t r_e) > floor((t - 1) r_e), in f64."""
    return np.floor(np.float64(t) * r) > np.floor(np.float64(t - 1) * r)


def random_start(n, dim, seed):
    c = np.arange(n * dim, dtype=np.uint64)
    z = mix(np.uint64(seed & MASK) + GOLDEN * (c + np.uint64(1)))
    return (-10.0 + 20.0 * ((z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53)).reshape(n, dim)


def pca_start(scores, dim):
    """scores[:, :dim] * (10 / max |score| over those columns)."""
    s = np.ascontiguousarray(np.asarray(scores, dtype=np.float64)[:, :dim])
    return s * (10.0 / np.abs(s).max())


def default_epochs(n):
    return 500 if n <= 10000 else 200


def _csr(W):
    if isinstance(W, (tuple, list)):
        indptr, indices, data = W
    else:
        W = sp.csr_matrix(W)
        W.sort_indices()
        indptr, indices, data = W.indptr, W.indices, W.data
    return np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64), np.asarray(data, dtype=np.float64)


def _add_rows(delta, rows, terms):
    if delta.dtype == np.float64:            # bincount adds in the order of the terms, as add.at does, and is much faster
        for c in range(delta.shape[1]):
            delta[:, c] += np.bincount(rows, weights=terms[:, c], minlength=delta.shape[0])
    else:
        np.add.at(delta, rows, terms)


def _d2(d):
    s = d[:, 0] * d[:, 0]
    for c in range(1, d.shape[1]):
        s = s + d[:, c] * d[:, c]
    return s


def layout(W, Y0, a, b, n_epochs, gamma=1.0, rate=5, alpha0=1.0, seed=0, stop_after=0, dtype=np.float64, first_epoch=1, keep=()):
    """Epochs first_epoch .. (stop_after or n_epochs) of the n_epochs schedule from Y0 (the positions BEFORE first_epoch).
    Returns (Y, info, kept) with kept[t] = Y^t for t in `keep`.  Scalars (a, b, gamma, alpha_t, the schedule) are f64 values;
    the positions and every operation on them are `dtype`."""
    indptr, indices, w = _csr(W)
    n, nnz = len(indptr) - 1, len(indices)
    Y = np.array(Y0, dtype=dtype, copy=True)
    Y = Y if Y.ndim == 2 else Y.reshape(n, -1)
    E, last = int(n_epochs), int(stop_after or n_epochs)
    info = {"n": n, "nnz": nnz, "entries_active": 0, "samples": 0, "negatives": 0, "negatives_skipped": 0, "n_epochs": E,
            "epochs_run": 0, "dim": Y.shape[1], "w_max": 0.0}
    kept = {}
    if nnz == 0 or n == 0:
        return Y, info, {t: Y.copy() for t in keep}
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    r = ratios(w)
    info["w_max"] = float(w.max())
    info["entries_active"] = int((np.floor(np.float64(E) * r) > 0).sum())
    T = np.dtype(dtype).type
    a_, b_, bm1 = T(np.float64(a)), T(np.float64(b)), T(np.float64(b) - 1.0)
    att, rep = T(-2.0 * np.float64(a) * np.float64(b)), T(2.0 * np.float64(gamma) * np.float64(b))
    one, four, eps = T(1.0), T(4.0), T(np.float64(0.001))
    for t in range(first_epoch, last + 1):
        alpha = np.float64(alpha0) * (1.0 - np.float64(t - 1) / np.float64(E))
        e = np.nonzero(sampled(r, t))[0]
        i, j = rows[e], indices[e]
        delta = np.zeros_like(Y)
        yi = Y[i]
        d = yi - Y[j]
        d2 = _d2(d)
        ok = d2 > 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            q = np.where(ok, att * d2 ** bm1 / (a_ * d2 ** b_ + one), T(0.0))
        g = np.clip(q[:, None] * d, -four, four)
        g[~ok] = 0
        _add_rows(delta, i, T(2.0 * alpha) * g)
        info["samples"] += len(e)
        if rate:
            k = negative_targets(seed, t, nnz, e, rate, n).astype(np.int64)
            for p in range(rate):
                kp = k[:, p]
                own = kp == i
                info["negatives_skipped"] += int(own.sum())
                d = yi - Y[kp]
                d2 = _d2(d)
                ok = (d2 > 0) & ~own
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    q = np.where(ok, rep / ((eps + d2) * (a_ * d2 ** b_ + one)), T(0.0))
                g = np.clip(q[:, None] * d, -four, four)
                g[~ok] = 0
                _add_rows(delta, i, T(alpha) * g)
        Y = Y + delta
        info["epochs_run"] += 1
        if t in keep:
            kept[t] = Y.copy()
    info["negatives"] = info["samples"] * int(rate) - info["negatives_skipped"]
    return Y, info, kept


COUNTERS = ("entries_active", "samples", "negatives", "negatives_skipped")


def curve_target(spread, min_dist):
    """(x, y) the curve is fitted to: 300 equally spaced x in [0, 3 spread]."""
    x = np.linspace(0.0, 3.0 * spread, 300)
    return x, np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))


def curve(x, a, b):
    return 1.0 / (1.0 + a * x ** (2.0 * b))


# ---- fixtures -----------------------------------------------------------------------------------------------------------
def knn_graph(x, k=15):
    """A symmetric weighted k-NN graph of the points, numpy / scipy only: w_ij = exp(-(d_ij - rho_i) / mean_i) on the k
    nearest, then the fuzzy union A + A^T - A o A^T (both halves computed from the same bits, so W is bit-symmetric)."""
    from scipy.spatial import cKDTree
    n = len(x)
    dist, idx = cKDTree(x).query(x, k=k + 1)
    dist, idx = dist[:, 1:], idx[:, 1:]
    rho = dist[:, :1]
    scale = np.maximum((dist - rho).mean(axis=1, keepdims=True), 1e-12)
    A = sp.csr_matrix((np.exp(-(dist - rho) / scale).ravel(), (np.repeat(np.arange(n), k), idx.ravel())), shape=(n, n))
    A = sp.triu(A + A.T - A.multiply(A.T), k=1).tocsr()
    W = (A + A.T).tocsr()
    W.eliminate_zeros()
    W.sort_indices()
    return W


def planted(seed=5, n=800, d=10, n_clusters=8, centre_scale=6.0, k=15):
    """(points, labels, W): Gaussian clusters and their k-NN graph."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clusters, d)) * centre_scale
    lab = rng.integers(0, n_clusters, n)
    x = centres[lab] + rng.standard_normal((n, d))
    return x, lab, knn_graph(x, k)


def sym_csr(n, edges):
    """Symmetric CSR of (i, j, w) edges, each stored in both directions with the same bits."""
    i = np.array([e[0] for e in edges] + [e[1] for e in edges], dtype=np.int64)
    j = np.array([e[1] for e in edges] + [e[0] for e in edges], dtype=np.int64)
    w = np.array([e[2] for e in edges] * 2, dtype=np.float64)
    W = sp.csr_matrix((w, (i, j)), shape=(n, n))
    W.sort_indices()
    return W


def graph12():
    """The hand-made 12-vertex graph: vertex 11 isolated, vertex 10 a row of one, the entry (8, 9) at 1e-7 w_max (never
    acts), vertices 2 and 3 start at the same position (d2 = 0), vertices 4 and 5 start 1e-9 apart.  Returns (W, Y0 n x 3);
    the 2-D start is its first two columns."""
    edges = [(0, 1, 1.0), (0, 2, 0.75), (1, 2, 0.5), (2, 3, 1.0), (3, 4, 0.25), (4, 5, 1.0), (5, 6, 0.625), (6, 7, 0.375),
             (7, 0, 0.875), (4, 6, 0.3), (1, 5, 0.45), (8, 9, 1e-7), (8, 0, 0.55), (9, 3, 0.7), (10, 6, 0.9), (2, 7, 0.05)]
    W = sym_csr(12, edges)
    Y0 = random_start(12, 3, 77) * 0.5
    Y0[3] = Y0[2]
    Y0[5] = Y0[4]
    Y0[5, 0] += 1e-9
    return W, Y0


def star_rows(G, hub=300):
    """A hub with `hub` leaves plus vertices whose rows are exactly G - 1, G, G + 1 and 2 G + 1 long (their neighbours are
    fresh leaves of their own); weights vary so that the schedule differs from entry to entry."""
    edges, nxt = [], 0
    centres = []
    for length in (hub, G - 1, G, G + 1, 2 * G + 1):
        centres.append((nxt, length))
        nxt += 1
    for c, length in centres:
        for s in range(length):
            edges.append((c, nxt, 0.05 + 0.95 * ((s * 7 + c * 3) % 20) / 19.0))
            nxt += 1
    return sym_csr(nxt, edges)


def every_length(max_len=130):
    """Rows of every length 1 .. max_len (centre c has c + 1 leaves of its own)."""
    edges, nxt = [], max_len
    for c in range(max_len):
        for s in range(c + 1):
            edges.append((c, nxt, 0.05 + 0.95 * ((s * 5 + c) % 17) / 16.0))
            nxt += 1
    return sym_csr(nxt, edges)


def ring(n):
    """A ring of n >= 3 vertices; n = 2: one edge; n = 1: no entry."""
    if n < 2:
        return sp.csr_matrix((n, n))
    if n == 2:
        return sym_csr(2, [(0, 1, 1.0)])
    return sym_csr(n, [(i, (i + 1) % n, 0.2 + 0.8 * ((i * 3) % 11) / 10.0) for i in range(n)])


def golden():
    return json.load(open(os.path.join(GOLD, "umap_kat.json")))


def quality(x, Y, labels, subsample=None):
    """(trustworthiness with 15 neighbours against the points x, silhouette of the labels) of the layout Y."""
    from sklearn.manifold import trustworthiness
    from sklearn.metrics import silhouette_score
    if subsample is not None:
        x, Y, labels = x[subsample], Y[subsample], labels[subsample]
    return float(trustworthiness(x, Y, n_neighbors=15)), float(silhouette_score(Y, labels))


def quality_floor(values):
    """min - (max - min) over the reference's seeds: the shape of the Louvain quality floor."""
    lo, hi = min(values), max(values)
    return lo - (hi - lo)

"""Host side of the doublet tests, independent of the device code: a numpy / scipy restatement of the section "Doublet
detection" of include/srx.h (the parent hash, the union-add of CSR row pairs, the scores of a neighbour list, the histogram
threshold exactly as that section words it, the brute-force neighbour search) and the planted data set the chain is run on."""
import math

import numpy as np
import scipy.sparse as sp

M64 = (1 << 64) - 1
G64 = 0x9E3779B97F4A7C15
MAX_ROUNDS = 10000


def mix_int(z):
    """splitmix64's finaliser on a Python int (mod 2^64)."""
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def rnd(x):
    """The section's round(): floor(x + 0.5)."""
    return int(math.floor(x + 0.5))


def parents(n, n_sim, seed):
    """p(s, c) = ((mix(seed + G (1 + 2 s + c)) >> 32) * n) >> 32 as an n_sim x 2 uint64 array."""
    out = np.zeros((n_sim, 2), dtype=np.uint64)
    for s in range(n_sim):
        for c in range(2):
            out[s, c] = (((mix_int(seed + G64 * (1 + 2 * s + c)) >> 32) * n) & M64) >> 32
    return out


def simulate(x, par, dtype):
    """X[a] + X[b] row by row in the storage type `dtype`: the union of the two patterns with ascending columns, a + b
    rounded once where both are stored, stored entries kept whatever their sum.  Returns (indptr int64, indices int32, data)."""
    x = x.tocsr()
    x.sort_indices()
    data = x.data.astype(dtype)
    indptr, cols, vals = [0], [], []
    for a, b in np.asarray(par, dtype=np.int64):
        ca, va = x.indices[x.indptr[a]:x.indptr[a + 1]], data[x.indptr[a]:x.indptr[a + 1]]
        cb, vb = x.indices[x.indptr[b]:x.indptr[b + 1]], data[x.indptr[b]:x.indptr[b + 1]]
        u = np.union1d(ca, cb)
        v = np.zeros(u.size, dtype=dtype)
        v[np.searchsorted(u, ca)] += va                  # 0 + a is a
        v[np.searchsorted(u, cb)] += vb                  # then a + b, one rounding
        cols.append(u)
        vals.append(v)
        indptr.append(indptr[-1] + u.size)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return np.array(indptr, dtype=np.int64), cat(cols, np.int32), cat(vals, dtype)


def scores(idx, n_obs, rho, se_rho, r):
    """(Ld, se_Ld) of every row of the list, section 4 in the order written."""
    idx = np.asarray(idx)
    k_adj = idx.shape[1]
    k_d = (idx >= n_obs).sum(axis=1).astype(np.float64)
    q = (k_d + 1.0) / (k_adj + 2.0)
    D = 1.0 - rho - q * (1.0 - rho - rho / r)
    Ld = q * rho / r / D
    se_q = np.sqrt(q * (1.0 - q) / (k_adj + 3.0))
    t1 = se_q / q * (1.0 - rho)
    t2 = se_rho / rho * (1.0 - q)
    se_Ld = q * rho / r / (D * D) * np.sqrt(t1 * t1 + t2 * t2)
    return Ld, se_Ld


def histogram(x):
    """(counts as doubles, centres, min, width) of the 256 equal bins over [min, max]."""
    mn, mx = float(x.min()), float(x.max())
    w = mx - mn
    b = np.minimum(255.0, np.floor((x - mn) / w * 256.0)).astype(np.int64)
    s = np.bincount(b, minlength=256).astype(np.float64)
    centres = np.array([mn + (i + 0.5) * w / 256.0 for i in range(256)])
    return s, centres


def maxima(s):
    out, rising = [], True
    for i in range(255):
        if rising:
            if s[i + 1] < s[i]:
                out.append(i)
                rising = False
        elif s[i + 1] > s[i]:
            rising = True
    return out


def _threshold(x, smooth):
    x = np.asarray(x, dtype=np.float64).ravel()
    if x.size < 2 or not np.isfinite(x).all() or x.max() == x.min():
        return float("nan"), 0, 0
    s, centres = histogram(x)
    r = 0
    while True:
        s = smooth(s)
        r += 1
        m = maxima(s)
        if len(m) < 3 or r >= MAX_ROUNDS:
            break
    if len(m) != 2 or r >= MAX_ROUNDS:
        return float("nan"), 0, r
    return float(centres[m[0] + int(np.argmin(s[m[0]:m[1] + 1]))]), 1, r


def smooth_restated(s):
    """s'[i] = (s[i-1] + s[i] + s[i+1]) / 3, summed left to right, the ends repeated."""
    p = np.concatenate(([s[0]], s, [s[-1]]))
    return ((p[:-2] + p[1:-1]) + p[2:]) / 3.0


def threshold(x):
    """(threshold, found, rounds): section 5 as it is worded."""
    return _threshold(x, smooth_restated)


def threshold_ndimage(x):
    """The same through scipy.ndimage.uniform_filter1d (scikit-image's own smoothing: a running sum, other rounding)."""
    from scipy.ndimage import uniform_filter1d
    return _threshold(x, lambda s: uniform_filter1d(s, 3))


def call(Ld_obs, se_obs, Ld_sim, t):
    """(predicted, z, detected_rate, detectable_fraction, overall_rate) for threshold t."""
    pred = Ld_obs > t
    z = (Ld_obs - t) / se_obs
    if t != t:
        return pred, z, float("nan"), float("nan"), float("nan")
    det, frac = float(pred.sum()) / Ld_obs.size, float((Ld_sim > t).sum()) / Ld_sim.size
    return pred, z, det, frac, det / frac


def knn_brute(pts, k):
    """(indices, distances) of the exact k nearest of every point among the others: distances sqrt(sum_j (q_j - r_j)^2) summed in
    f64 in ascending coordinate order, each product rounded before it is added, ordered by (distance, index)."""
    n, d = pts.shape
    d2 = np.zeros((n, n))
    for j in range(d):
        t = pts[:, j][:, None] - pts[None, :, j]
        d2 += t * t
    dist = np.sqrt(d2)
    dist[np.arange(n), np.arange(n)] = np.inf
    order = np.argsort(dist, axis=1, kind="stable")[:, :k]
    return order.astype(np.uint32), np.take_along_axis(dist, order, axis=1), dist


def auc(score, positive):
    """ROC AUC with ties counted half (the Mann-Whitney form)."""
    from scipy.stats import rankdata
    r = rankdata(score)
    n1 = int(positive.sum())
    n0 = score.size - n1
    return float((r[positive].sum() - n1 * (n1 + 1) / 2.0) / (n1 * n0))


# ---- the planted data set ---------------------------------------------------------------------------------------------------------
N_PLANTED = 48


def planted(seed, n=480, G=240):
    """(counts csr f64, doublet flags): 4 clusters, gamma(0.3) profiles with 40 cluster-specific genes times 8, normalised;
    depths uniform in 150..399, Poisson counts; the first 48 cells replaced by the sum of two later cells of different clusters."""
    rng = np.random.default_rng(seed)
    prof = rng.gamma(0.3, size=(4, G))
    for c in range(4):
        prof[c, rng.choice(G, 40, replace=False)] *= 8.0
    prof /= prof.sum(axis=1, keepdims=True)
    cl = rng.integers(0, 4, n)
    depth = rng.integers(150, 400, n)
    x = rng.poisson(depth[:, None] * prof[cl]).astype(np.float64)
    for i in range(N_PLANTED):
        while True:
            a, b = rng.integers(N_PLANTED, n, 2)
            if cl[a] != cl[b]:
                break
        x[i] = x[a] + x[b]
    flags = np.zeros(n, dtype=bool)
    flags[:N_PLANTED] = True
    m = sp.csr_matrix(x)
    m.sort_indices()
    return m, flags


# ---- the embedding, restated ------------------------------------------------------------------------------------------------------
def normalize_log1p(x, target=1e4):
    y = np.asarray(x.todense(), dtype=np.float64)
    s = y.sum(axis=1)
    f = np.where(s == 0, 0.0, target / np.where(s == 0, 1.0, s))
    return np.log1p(y * f[:, None])


def hvg_nz(y, n_top):
    """The n_top genes of largest variance over their non-zero entries (population form), ties to the lower index."""
    nz = y != 0
    cnt = np.maximum(nz.sum(axis=0), 1)
    mean = y.sum(axis=0) / cnt
    var = (y * y).sum(axis=0) / cnt - mean * mean
    return np.sort(np.argsort(-var, kind="stable")[:n_top])


def pca_fit(y, n_pc):
    """(scores, V, mu, sd) of the standardised PCA of the columns of y."""
    mu, sd = y.mean(axis=0), y.std(axis=0)
    sd = np.where(sd == 0, 1.0, sd)
    z = (y - mu) / sd
    _, _, vt = np.linalg.svd(z, full_matrices=False)
    V = vt[:n_pc].T
    return z @ V, V, mu, sd


def project(x, sel, V, mu, sd, target=1e4):
    sd = np.where(sd == 0, 1.0, sd)
    return ((normalize_log1p(x, target)[:, sel] - mu) / sd) @ V


def chain(x, seed=0, sim_ratio=2.0, k=11, rho=0.05, se_rho=0.02, n_hvg=120, n_pc=10, target=1e4):
    """The whole method on the host; a dict of every intermediate."""
    n = x.shape[0]
    n_sim = rnd(sim_ratio * n)
    r = n_sim / n
    par = parents(n, n_sim, seed)
    ip, ix, dv = simulate(x, par, np.float64)
    xs = sp.csr_matrix((dv, ix, ip), shape=(n_sim, x.shape[1]))
    y = normalize_log1p(x, target)
    sel = hvg_nz(y, n_hvg)
    obs, V, mu, sd = pca_fit(y[:, sel], n_pc)
    pts = np.vstack([obs, project(xs, sel, V, mu, sd, target)])
    k_adj = rnd(k * (1.0 + r))
    idx = knn_brute(pts, k_adj)[0]
    Ld, se = scores(idx, n, rho, se_rho, r)
    t, found, rounds = threshold(Ld[n:])
    pred, z, det, frac, overall = call(Ld[:n], se[:n], Ld[n:], t)
    return {"n_sim": n_sim, "r": r, "parents": par, "points": pts, "k_adj": k_adj, "knn": idx, "Ld": Ld, "se": se, "threshold": t,
            "found": found, "rounds": rounds, "predicted": pred, "z": z, "rates": (det, frac, overall)}


# ---- named inputs of the threshold tests ------------------------------------------------------------------------------------------
THRESHOLD_CASES = ("separated", "overlapping", "one_clump", "all_equal", "n0", "n1", "n2", "nan", "spikes", "plateau", "slow")


def threshold_case(name):
    rng = np.random.default_rng(77)
    if name == "separated":
        return np.concatenate([rng.normal(0.1, 0.02, 600), rng.normal(0.8, 0.03, 200)])
    if name == "overlapping":
        return np.concatenate([rng.normal(0.3, 0.08, 700), rng.normal(0.55, 0.08, 300)])
    if name == "one_clump":                                # a triangle of bin counts: one maximum from the first round on
        b = np.arange(256)
        return np.concatenate([[0.0, 1.0], np.repeat((b + 0.5) / 256, 1 + np.minimum(b, 255 - b))])
    if name == "all_equal":
        return np.full(50, 0.3)
    if name in ("n0", "n1", "n2"):
        return np.array([0.2, 0.9][:int(name[1])])
    if name == "nan":
        x = threshold_case("separated")
        x[17] = np.nan
        return x
    if name == "spikes":                                   # bins 0 and 255 alone
        return np.concatenate([np.zeros(100), np.ones(60)])
    if name == "plateau":                                  # two pairs of equal neighbouring bins: both maxima are plateaus
        w = 1.0 / 256
        return np.concatenate([[0.0, 1.0], np.repeat([(10.5) * w, (11.5) * w], 40), np.repeat([(200.5) * w, (201.5) * w], 25)])
    if name == "slow":                                     # the scores of 33-neighbour lists: 34 distinct values, far apart in bins
        k_d = np.concatenate([rng.binomial(33, 0.15, 800), rng.binomial(33, 0.85, 300)])
        idx = (np.arange(33)[None, :] < k_d[:, None]).astype(np.uint32)         # k_d entries "at or above n_obs = 1"
        return scores(idx, 1, 0.05, 0.02, 2.0)[0]
    raise KeyError(name)

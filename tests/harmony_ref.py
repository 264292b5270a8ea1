"""The Harmony batch integration of include/srx.h (section "Harmony"), restated in numpy from the header text alone.

`ft` switches the float type between np.float64 and np.longdouble: the gap between the two runs on one input is the
yardstick of the device tests (tests/test_harmony_gpu.py).  Nothing here is fast; every sum is numpy's own.
"""
import numpy as np

MASK = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
MAX_ROUNDS = 64


def mix(z):
    """splitmix64's finaliser on a uint64 array."""
    z = z.astype(np.uint64)
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return z


def hashes(seed, a, n):
    """H(a, i) for i = 0..n-1."""
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=np.uint64)
        arg = np.full(n, (1 + (a << 32)) & MASK, dtype=np.uint64) + i
        return mix(np.full(n, seed & MASK, dtype=np.uint64) + np.full(n, GOLD, dtype=np.uint64) * arg)


def default_clusters(n):
    return max(1, min((n + 15) // 30, 100))          # round(n / 30), halves up, in integers


def cosine_rows(X):
    s = np.zeros(X.shape[0], dtype=X.dtype)
    for c in range(X.shape[1]):                      # ascending coordinate order
        s = s + X[:, c] * X[:, c]
    nrm = np.sqrt(s)
    out = np.zeros_like(X)
    nz = nrm > 0
    out[nz] = X[nz] / nrm[nz, None]
    return out


def normalise_centroids(S, Y_old):
    Y = Y_old.copy()
    s = np.zeros(S.shape[0], dtype=S.dtype)
    for c in range(S.shape[1]):
        s = s + S[:, c] * S[:, c]
    nrm = np.sqrt(s)
    nz = nrm > 0
    Y[nz] = S[nz] / nrm[nz, None]
    return Y


def softmax_rows(L):
    L = L - L.max(axis=1, keepdims=True)
    e = np.exp(L)
    return e / e.sum(axis=1, keepdims=True)


def tables(R, onehot):
    """sum over the cells of each batch of R_ik: K x B."""
    return R.T @ onehot


def objective(R, dist, O, E, batch, sigma, theta):
    a = (R * dist).sum()
    lr = np.zeros_like(R)
    pos = R > 0
    lr[pos] = np.log(R[pos])
    b = sigma * (R * lr).sum()
    c = sigma * theta * (R * np.log((O + 1) / (E + 1))[:, batch].T).sum()
    return a + b + c


def ridge_closed_form(m, S, lam):
    """m: K x B, S: K x B x d.  W: K x B x d of the definition's correction."""
    ft = S.dtype.type
    lam = ft(lam)
    den = m + lam
    s = (lam * m / den).sum(axis=1)
    num = (lam * S / den[:, :, None]).sum(axis=1)
    W = np.zeros_like(S)
    ok = s != 0
    w0 = np.zeros_like(num)
    w0[ok] = num[ok] / s[ok, None]
    W[ok] = (S[ok] - m[ok][:, :, None] * w0[ok][:, None, :]) / den[ok][:, :, None]
    return W


def ridge_dense(m_k, S_k, lam):
    """harmonypy's moe_correct_ridge system of ONE cluster, solved densely: rows 1..B of the (B + 1) x d solution."""
    B = m_k.shape[0]
    A = np.zeros((B + 1, B + 1))
    A[0, 0] = m_k.sum()
    A[0, 1:] = m_k
    A[1:, 0] = m_k
    A[1:, 1:] = np.diag(m_k + lam)
    rhs = np.vstack([S_k.sum(axis=0, keepdims=True), S_k])
    return np.linalg.solve(A, rhs)[1:]


def run(Z, batch, B, ft=np.float64, theta=2.0, sigma=0.1, lam=1.0, epsilon_cluster=1e-5, epsilon_harmony=1e-4, seed=0,
        n_clusters=0, n_blocks=0, max_rounds=0, max_cluster_iters=0, init_iters=0, n_dims=0):
    Z = np.asarray(Z, dtype=np.float64)
    n, d_full = Z.shape
    d = n_dims or d_full
    Z = Z[:, :d].astype(ft)
    batch = np.asarray(batch, dtype=np.int64)
    K = n_clusters or default_clusters(n)
    nb = n_blocks or 20
    max_rounds = max_rounds or 10
    max_ci = max_cluster_iters or 20
    init_iters = 0 if init_iters < 0 else (init_iters or 10)
    theta, sigma, lam = ft(theta), ft(sigma), ft(lam)
    assert K <= n and batch.max(initial=0) < B
    Nb = np.bincount(batch, minlength=B)
    P = Nb.astype(ft) / ft(n)
    onehot = np.zeros((n, B), dtype=ft)
    onehot[np.arange(n), batch] = 1

    Zh = cosine_rows(Z)
    h0 = hashes(seed, 0, n)
    start = np.lexsort((np.arange(n), h0))[:K]
    Y = Zh[start].copy()
    for _ in range(init_iters):
        c = np.argmax(Zh @ Y.T, axis=1)              # first maximum: ties to the lowest k
        S = np.zeros((K, d), dtype=ft)
        for k in range(K):
            S[k] = Zh[c == k].sum(axis=0)
        Y = normalise_centroids(S, Y)
    dist = 2 * (1 - Zh @ Y.T)
    R = softmax_rows(-dist / sigma)
    O = tables(R, onehot)
    E = np.outer(R.sum(axis=0), P)

    out = {"n": n, "d": d, "K": K, "B": B, "n_blocks": nb, "round_iters": [], "round_objective": [], "objectives": [],
           "ratios_cluster": [], "ratios_harmony": [], "converged": 0}
    t = 0
    Zc = Z.copy()
    for r in range(1, max_rounds + 1):
        objs = []
        for j in range(1, max_ci + 1):
            Y = normalise_centroids(R.T @ Zh, Y)
            dist = 2 * (1 - Zh @ Y.T)
            q = (hashes(seed, 1 + t, n) % np.uint64(nb)).astype(np.int64)
            for blk in range(nb):
                idx = np.nonzero(q == blk)[0]
                if idx.size == 0:
                    continue
                Rb, oh = R[idx], onehot[idx]
                O = O - tables(Rb, oh)
                E = E - np.outer(Rb.sum(axis=0), P)
                Rn = softmax_rows(-dist[idx] / sigma + theta * np.log((E + 1) / (O + 1))[:, batch[idx]].T)
                R[idx] = Rn
                O = O + tables(Rn, oh)
                E = E + np.outer(Rn.sum(axis=0), P)
            t += 1
            objs.append(objective(R, dist, O, E, batch, sigma, theta))
            if j >= 6:
                old = objs[j - 6] + objs[j - 5] + objs[j - 4]
                new = objs[j - 3] + objs[j - 2] + objs[j - 1]
                ratio = (old - new) / abs(old)
                out["ratios_cluster"].append(float(ratio))
                if epsilon_cluster > 0 and ratio < epsilon_cluster:
                    break
        out["round_iters"].append(len(objs))
        out["round_objective"].append(objs[-1])
        out["objectives"].append(objs)
        # correction, from the original Z
        m = tables(R, onehot)
        S = np.zeros((K, B, d), dtype=ft)
        for b in range(B):
            ib = np.nonzero(batch == b)[0]
            if ib.size:
                S[:, b, :] = R[ib].T @ Z[ib]
        W = ridge_closed_form(m, S, lam)
        Zc = Z.copy()
        for b in range(B):
            ib = np.nonzero(batch == b)[0]
            if ib.size:
                Zc[ib] = Z[ib] - R[ib] @ W[:, b, :]
        Zh = cosine_rows(Zc)
        if r >= 2:
            hp, hr = out["round_objective"][-2], out["round_objective"][-1]
            ratio = (hp - hr) / abs(hp)
            out["ratios_harmony"].append(float(ratio))
            if epsilon_harmony > 0 and ratio < epsilon_harmony:
                out["converged"] = 1
                break
    out.update(Z_corr=Zc, R=R, Y=Y, O=O, E=E, rounds=len(out["round_iters"]), cluster_iters=t)
    return out


TABLES = ("Z_corr", "R", "Y", "O", "E")


def gaps(a, b):
    """Largest |a - b| over largest |a| per table and for the round objectives: the f64-against-longdouble yardstick."""
    g = {}
    for name in TABLES:
        x, y = np.asarray(a[name], dtype=np.longdouble), np.asarray(b[name], dtype=np.longdouble)
        g[name] = float(np.abs(x - y).max(initial=0) / max(np.abs(x).max(initial=0), np.finfo(np.float64).tiny))
    x = np.array(a["round_objective"], dtype=np.longdouble)          # h_r: what srx_harmony_info reports
    y = np.array(b["round_objective"], dtype=np.longdouble)
    g["objectives"] = float(np.abs(x - y).max(initial=0) / max(np.abs(x).max(initial=0), np.finfo(np.float64).tiny))
    return g


# ---- data ------------------------------------------------------------------------------------------------------------
def planted(n=600, d=10, n_types=3, n_batches=2, seed=1, offset=3.0):
    """Cell types with N(0, 4^2) centres, one offset of length `offset` per batch, unit noise.  (Z, batch, type)."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 4.0, (n_types, d))
    off = rng.normal(0.0, 1.0, (n_batches, d))
    off *= offset / np.linalg.norm(off, axis=1, keepdims=True)
    typ = rng.integers(0, n_types, n)
    batch = rng.integers(0, n_batches, n)
    Z = centres[typ] + off[batch] + rng.normal(0.0, 1.0, (n, d))
    return Z, batch.astype(np.uint32), typ


def planted_two():
    return planted(600, 10, 3, 2, 1)


def planted_seven():
    """Seven labels of which one (5) is empty: batch 5 is relabelled to 4."""
    Z, batch, typ = planted(1000, 50, 4, 7, 3)
    batch = batch.copy()
    batch[batch == 5] = 4
    return Z, batch, typ


def knn_brute(X, k):
    """Brute-force k nearest neighbours (self excluded), ties to the lower index."""
    X = np.asarray(X, dtype=np.float64)
    g = X @ X.T
    sq = np.diag(g)
    d2 = sq[:, None] + sq[None, :] - 2 * g
    np.fill_diagonal(d2, np.inf)
    return np.argsort(d2, axis=1, kind="stable")[:, :k]


def mixing_and_purity(X, batch, typ, k=15):
    """(share of neighbours from another batch, share of neighbours of the same type)."""
    nb = knn_brute(X, k)
    return float((batch[nb] != batch[:, None]).mean()), float((typ[nb] == typ[:, None]).mean())

"""Host restatement of the Louvain definition of include/srx.h (numpy / scipy), independent of the device code: synchronous
sweeps by parity with the strict-gain, lowest-id and singleton rules, aggregation with self weights, levels kept while Q
rises, final labels by (size descending, smallest member); an independent `modularity`; and the fixtures the tests share."""
import json
import os

import numpy as np
import scipy.sparse as sp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def modularity(W, labels, gamma=1.0):
    """Q = sum_c [in_c / 2m - gamma (tot_c / 2m)^2] of a labelling, straight from the formula (f64)."""
    W = sp.coo_matrix(W)
    labels = np.asarray(labels, dtype=np.int64)
    n = W.shape[0]
    k = np.bincount(W.row, weights=W.data, minlength=n)
    twom = k.sum()
    if twom == 0 or n == 0:
        return 0.0
    inside = W.data[labels[W.row] == labels[W.col]].sum()
    tot = np.bincount(labels, weights=k)
    return float(inside / twom - gamma * ((tot / twom) ** 2).sum())


def gains(W, k, twom, comm, gamma, active=None):
    """For every (active) vertex with at least one admissible target: (vertex, best target, g(best)), and g(own) of all
    vertices.  W: CSR without diagonal; k: degrees including self weights."""
    n = W.shape[0]
    coo = W.tocoo()
    rows, cols, data = coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data
    if active is not None:
        m = active[rows]
        rows, cols, data = rows[m], cols[m], data[m]
    tot = np.bincount(comm, weights=k, minlength=n)
    size = np.bincount(comm, minlength=n)
    key, inv = np.unique(rows * n + comm[cols], return_inverse=True)
    w_to = np.bincount(inv.ravel(), weights=data, minlength=len(key))
    ur, uc = key // n, key % n
    own = comm[ur]
    is_own = uc == own
    w_own = np.zeros(n)
    w_own[ur[is_own]] = w_to[is_own]
    g_own = w_own - gamma * k * (tot[comm] - k) / twom
    cand = ~is_own & ~((size[own] == 1) & (size[uc] == 1) & (uc < own))
    ur, uc, g = ur[cand], uc[cand], (w_to - gamma * k[ur] * tot[uc] / twom)[cand]
    order = np.lexsort((uc, -g, ur))
    ur, uc, g = ur[order], uc[order], g[order]
    first = np.ones(len(ur), dtype=bool)
    first[1:] = ur[1:] != ur[:-1]
    return ur[first], uc[first], g[first], g_own


def max_excess(W, comm, gamma=1.0):
    """max over vertices of g(best admissible target) - g(own) on a graph without self weights (-inf if no target)."""
    W = sp.csr_matrix(W)
    k = np.asarray(W.sum(axis=1)).ravel()
    v, _, g, g_own = gains(W, k, k.sum(), np.asarray(comm, dtype=np.int64), gamma)
    return float((g - g_own[v]).max()) if len(v) else -np.inf


def _level_q(W, selfw, comm, gamma, k, twom):
    coo = W.tocoo()
    inside = coo.data[comm[coo.row] == comm[coo.col]].sum() + selfw.sum()
    tot = np.bincount(comm, weights=k)
    return float(inside / twom - gamma * ((tot / twom) ** 2).sum())


def _level(W, selfw, gamma, max_sweeps):
    n = W.shape[0]
    k = selfw + np.asarray(W.sum(axis=1)).ravel()
    twom = k.sum()
    comm = np.arange(n, dtype=np.int64)
    ids = np.arange(n)
    sweeps = moves = quiet = t = 0
    while t < max_sweeps and quiet < 2:
        v, c, g, g_own = gains(W, k, twom, comm, gamma, (ids + t) % 2 == 0)
        go = g > g_own[v]
        comm = comm.copy()
        comm[v[go]] = c[go]
        sweeps += 1
        moves += int(go.sum())
        quiet = 0 if go.any() else quiet + 1
        t += 1
    return comm, k, twom, sweeps, moves


def final_labels(comm):
    """Communities numbered by (size descending, smallest member)."""
    comm = np.asarray(comm)
    _, first, inv, cnt = np.unique(comm, return_index=True, return_inverse=True, return_counts=True)
    order = np.lexsort((first, -cnt))
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    return rank[inv.ravel()].astype(np.uint32)


def louvain(W, gamma=1.0, min_gain=0.0, max_levels=32, max_sweeps=200):
    """Returns (labels uint32, info dict) as srx_louvain_csr defines them."""
    W = sp.csr_matrix(W, dtype=np.float64)
    n = W.shape[0]
    info = {"n": n, "n_levels": 0, "sweeps": 0, "moves": 0, "level_communities": [], "level_modularity": [], "modularity": 0.0}
    cell = np.arange(n, dtype=np.int64)
    selfw = np.zeros(n)
    q_prev = None
    for _ in range(max_levels):
        if n == 0 or W.sum() + selfw.sum() == 0:
            break
        comm, k, twom, sweeps, moves = _level(W, selfw, gamma, max_sweeps)
        if q_prev is None:
            q_prev = _level_q(W, selfw, np.arange(W.shape[0]), gamma, k, twom)
        if moves == 0:
            break
        q = _level_q(W, selfw, comm, gamma, k, twom)
        if not q > q_prev + min_gain:
            break
        _, compact = np.unique(comm, return_inverse=True)
        compact = compact.ravel()
        nc = int(compact.max()) + 1
        cell = compact[cell]
        q_prev = q
        info["n_levels"] += 1
        info["sweeps"] += sweeps
        info["moves"] += moves
        info["level_communities"].append(nc)
        info["level_modularity"].append(q)
        if nc <= 1:
            break
        S = sp.csr_matrix((np.ones(len(compact)), (np.arange(len(compact)), compact)), shape=(len(compact), nc))
        Wc = sp.csr_matrix(S.T @ W @ S)
        selfw = Wc.diagonal() + S.T @ selfw
        Wc.setdiag(0.0)
        Wc.eliminate_zeros()
        Wc.sort_indices()
        W = Wc
    labels = final_labels(cell)
    info["n_communities"] = int(labels.max()) + 1 if n else 0
    info["modularity"] = q_prev if q_prev is not None else 0.0
    return labels, info


# ---- fixtures -----------------------------------------------------------------------------------------------------------
def planted_clusters(seed, n, d, n_clusters=12, centre_scale=6.0):
    """Gaussian clusters around centres drawn at `centre_scale`; returns (points, planted labels)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clusters, d)) * centre_scale
    lab = rng.integers(0, n_clusters, n)
    return centres[lab] + rng.standard_normal((n, d)), lab


def connectivities(x, k=15):
    """The connectivities of graph_ref over sklearn's brute k-NN list of the points."""
    from sklearn.neighbors import NearestNeighbors

    import graph_ref
    nn = NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(x)
    dist, idx = nn.kneighbors(n_neighbors=k)
    Cm = sp.csr_matrix(graph_ref.graph(idx, dist)[1])
    Cm.sort_indices()
    return Cm


KARATE_EDGES = None


def karate(unit):
    """Zachary's karate club from tests/golden/louvain_nx.json (edges with the stored weights), as symmetric CSR."""
    e = np.array(json.load(open(os.path.join(GOLD, "louvain_nx.json")))["karate_edges"], dtype=np.float64)
    i, j, w = e[:, 0].astype(int), e[:, 1].astype(int), (np.ones(len(e)) if unit else e[:, 2])
    n = int(max(i.max(), j.max())) + 1
    W = sp.coo_matrix((np.r_[w, w], (np.r_[i, j], np.r_[j, i])), shape=(n, n)).tocsr()
    W.sort_indices()
    return W


def ring_of_cliques(n_cliques=8, size=6):
    n = n_cliques * size
    A = np.zeros((n, n))
    for c in range(n_cliques):
        A[c * size:(c + 1) * size, c * size:(c + 1) * size] = 1.0
        a, b = c * size + size - 1, ((c + 1) % n_cliques) * size
        A[a, b] = A[b, a] = 1.0
    np.fill_diagonal(A, 0.0)
    return sp.csr_matrix(A)


def two_cliques():
    A = np.zeros((7, 7))
    A[:3, :3] = 1.0
    A[3:, 3:] = 1.0
    np.fill_diagonal(A, 0.0)
    return sp.csr_matrix(A)


FIXTURES = {
    "separated_3000": lambda: planted_clusters(11, 3000, 50, 12, 6.0),
    "separated_20011": lambda: planted_clusters(12, 20011, 50, 12, 6.0),
    "overlapping_6000": lambda: planted_clusters(13, 6000, 50, 12, 0.6),
}


def fixture_graph(name):
    """(W, planted labels or None) of a named fixture of the golden file."""
    if name in FIXTURES:
        x, lab = FIXTURES[name]()
        return connectivities(x, 15), lab
    if name == "karate_stored":
        return karate(False), None
    if name == "karate_unit":
        return karate(True), None
    raise KeyError(name)


def golden():
    return json.load(open(os.path.join(GOLD, "louvain_nx.json")))


def quality_floor(name):
    """The least Q the quality rule admits: q_min - (q_max - q_min) over networkx's five seeds; q - 1e-9 where they agree."""
    q = [s["modularity"] for s in golden()["fixtures"][name]["seeds"]]
    lo, hi = min(q), max(q)
    return lo - (hi - lo) if hi > lo else lo - 1e-9


def ari(a, b):
    """Adjusted Rand index of two labellings."""
    a, b = np.asarray(a), np.asarray(b)
    _, ai = np.unique(a, return_inverse=True)
    _, bi = np.unique(b, return_inverse=True)
    M = sp.coo_matrix((np.ones(len(a)), (ai.ravel(), bi.ravel()))).toarray()
    c2 = lambda v: (v * (v - 1) / 2).sum()
    s, ra, rb, tot = c2(M), c2(M.sum(axis=1)), c2(M.sum(axis=0)), len(a) * (len(a) - 1) / 2
    exp = ra * rb / tot
    return float((s - exp) / (0.5 * (ra + rb) - exp)) if 0.5 * (ra + rb) != exp else 1.0

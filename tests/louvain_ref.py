"""Host restatement of the Louvain definition of include/srx.h (numpy / scipy), independent of the device code: synchronous
sweeps by parity with the strict-gain, lowest-id and singleton rules, aggregation with self weights, levels kept while Q
rises, final labels by (size descending, smallest member); an independent `modularity`; the fixtures the tests share; and
the seeded cases with dyadic weights (`exact_cases`) on which the device must agree with this restatement exactly."""
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


def aggregate(W, selfw, comm):
    """The next level's graph: (W without diagonal, self weights, compact ids of `comm`)."""
    _, compact = np.unique(comm, return_inverse=True)
    compact = compact.ravel()
    nc = int(compact.max()) + 1
    S = sp.csr_matrix((np.ones(len(compact)), (np.arange(len(compact)), compact)), shape=(len(compact), nc))
    Wc = sp.csr_matrix(S.T @ W @ S)
    selfc = Wc.diagonal() + S.T @ selfw
    Wc.setdiag(0.0)
    Wc.eliminate_zeros()
    Wc.sort_indices()
    return Wc, selfc, compact


def louvain(W, gamma=1.0, min_gain=0.0, max_levels=32, max_sweeps=200):
    """Returns (labels uint32, info dict) as srx_louvain_csr defines them.  Beside the keys of srx_louvain_info the dict has
    `level_sweeps` (of the kept levels) and `min_margin`: the smallest |q - (q_prev + min_gain)| over every keep-or-discard
    decision taken, the discarded last level included (inf if none was taken)."""
    W = sp.csr_matrix(W, dtype=np.float64)
    n = W.shape[0]
    info = {"n": n, "n_levels": 0, "sweeps": 0, "moves": 0, "level_communities": [], "level_modularity": [], "modularity": 0.0,
            "level_sweeps": [], "min_margin": np.inf}
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
        info["min_margin"] = min(info["min_margin"], abs(q - (q_prev + min_gain)))
        if not q > q_prev + min_gain:
            break
        Wc, selfc, compact = aggregate(W, selfw, comm)
        nc = Wc.shape[0]
        cell = compact[cell]
        q_prev = q
        info["n_levels"] += 1
        info["sweeps"] += sweeps
        info["moves"] += moves
        info["level_communities"].append(nc)
        info["level_modularity"].append(q)
        info["level_sweeps"].append(sweeps)
        if nc <= 1:
            break
        W, selfw = Wc, selfc
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


# ---- exact cases ----------------------------------------------------------------------------------------------------------
# Every weight is a multiple of 2^-20 and 2m < 2^32: k_i, tot_c, w_{i->c} and all coarse weights are then exact in f64 and in
# the device's fixed point, g(c) sees the same bits on both sides, and labels, sweeps, moves and level counts must be equal.
DYADIC = 2.0 ** 20


def sym_csr(n, r, c, w):
    """Symmetric sorted CSR of the undirected edges (r, c, w); no pair may occur twice."""
    W = sp.coo_matrix((np.r_[w, w], (np.r_[r, c], np.r_[c, r])), shape=(n, n)).tocsr()
    W.sort_indices()
    return W


def random_edges(rng, n, mean_degree):
    """About n * mean_degree / 2 distinct pairs i < j, in a seeded order."""
    m = n * mean_degree // 2
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    _, first = np.unique(lo * n + hi, return_index=True)
    first = np.sort(first[lo[first] != hi[first]])
    return lo[first], hi[first]


def random_graph(seed, n, mean_degree, weights):
    rng = np.random.default_rng(seed)
    r, c = random_edges(rng, n, mean_degree)
    return sym_csr(n, r, c, weights(rng, len(r)))


ROW_CLASS_LENGTHS = (31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 3999)


def row_classes(seed, extras_first):
    """A random background of 4000 vertices (mean degree 6, weights 1..3) and one extra vertex per length of
    ROW_CLASS_LENGTHS with exactly that many entries, numbered after the background or before it."""
    nb, ne = 4000, len(ROW_CLASS_LENGTHS)
    rng = np.random.default_rng(seed)
    r, c = random_edges(rng, nb, 6)
    er = np.concatenate([np.full(L, nb + x) for x, L in enumerate(ROW_CLASS_LENGTHS)])
    ec = np.concatenate([rng.choice(nb, L, replace=False) for L in ROW_CLASS_LENGTHS])
    r, c = np.r_[r, er], np.r_[c, ec]
    w = rng.integers(1, 4, len(r)).astype(np.float64)
    if extras_first:
        r, c = (r + ne) % (nb + ne), (c + ne) % (nb + ne)
    return sym_csr(nb + ne, r, c, w)


def clique_links(seed, n_cliques, link_degree, size=5, inner=8.0):
    """Cliques of `size` with inner weight `inner`, joined by random unit links between vertices of different cliques, about
    `link_degree` of them at every vertex."""
    rng = np.random.default_rng(seed)
    n = n_cliques * size
    i, j = np.triu_indices(size, 1)
    base = np.repeat(np.arange(n_cliques) * size, len(i))
    r, c = base + np.tile(i, n_cliques), base + np.tile(j, n_cliques)
    w = np.full(len(r), inner)
    a, b = random_edges(rng, n, link_degree)
    keep = a // size != b // size
    return sym_csr(n, np.r_[r, a[keep]], np.r_[c, b[keep]], np.r_[w, np.ones(int(keep.sum()))])


def chain(n):
    """Edges (2i, 2i + 1) of weight 4 and (2i + 1, 2i + 2) of weight 1."""
    r = np.arange(n - 1)
    return sym_csr(n, r, r + 1, np.where(r % 2 == 0, 4.0, 1.0))


def quantised(name):
    """A real-valued fixture with W_q = rint(W 2^20) / 2^20 (entries that round to zero leave, on both sides)."""
    W = fixture_graph(name)[0].copy()
    W.data = np.rint(W.data * DYADIC) / DYADIC
    W.eliminate_zeros()
    W.sort_indices()
    return W


EXACT_CASES = {
    "ties_int": lambda: random_graph(101, 3000, 6, lambda rng, m: rng.integers(1, 4, m).astype(np.float64)),
    "unit": lambda: random_graph(102, 2000, 8, lambda rng, m: np.ones(m)),
    "dyadic": lambda: random_graph(103, 3000, 6, lambda rng, m: rng.integers(1, 4097, m) * 2.0 ** -10),
    "row_classes_last": lambda: row_classes(104, False),
    "row_classes_first": lambda: row_classes(104, True),
    "coarse_long_rows": lambda: clique_links(105, 200, 20),
    "chain_300k": lambda: chain(300_000),
    "separated_3000_q20": lambda: quantised("separated_3000"),
    "overlapping_6000_q20": lambda: quantised("overlapping_6000"),
    "karate_unit": lambda: karate(True),
}
_EXACT_GRAPHS = {}


def exact_graph(name):
    """The graph of a named exact case, built once per process; callers leave it unchanged."""
    if name not in _EXACT_GRAPHS:
        _EXACT_GRAPHS[name] = EXACT_CASES[name]() if name in EXACT_CASES else GUARD_CASES[name][0]()
    return _EXACT_GRAPHS[name]


# (case, options of louvain() / louvain_csr() by louvain()'s names): every run the device is compared on
TIES_INT_MIN_GAIN = 0.01            # ties_int at gamma 1 raises Q by 0.0216 at its fourth level and by 0.0079 at its fifth
EXACT_RUNS = [
    ("ties_int", {"gamma": 0.5}), ("ties_int", {}), ("ties_int", {"gamma": 2.0}),
    ("ties_int", {"max_levels": 1}), ("ties_int", {"max_levels": 2}), ("ties_int", {"max_levels": 3}),
    ("ties_int", {"min_gain": TIES_INT_MIN_GAIN}),
    ("unit", {}), ("dyadic", {}), ("row_classes_last", {}), ("row_classes_first", {}), ("coarse_long_rows", {}),
    ("chain_300k", {}), ("separated_3000_q20", {}), ("separated_3000_q20", {"max_levels": 1, "max_sweeps": 3}), ("overlapping_6000_q20", {}), ("karate_unit", {}),
]
PREFIX_CASES = ("ties_int", "row_classes_last", "row_classes_first", "coarse_long_rows")
PREFIX_SWEEPS = (1, 2, 3, 4, 7)

_EXACT_RESULTS = {}


def exact_result(name, opts):
    """ref.louvain of a case with the given options, computed once per process and shared; callers leave it unchanged."""
    key = (name, tuple(sorted(opts.items())))
    if key not in _EXACT_RESULTS:
        _EXACT_RESULTS[key] = louvain(exact_graph(name), **opts)
    return _EXACT_RESULTS[key]


def _edges(n, edges):
    e = np.array(edges, dtype=np.float64)
    return sym_csr(n, e[:, 0].astype(np.int64), e[:, 1].astype(np.int64), e[:, 2])


def _path(n_edges):
    return _edges(n_edges + 1, [(i, i + 1, 1.0) for i in range(n_edges)])


# Small graphs on which the singleton guard and the lowest-id rule decide the outcome: name -> (graph, [(options, labels)]).
# The labels were worked out by hand from include/srx.h (the traces are in tests/test_louvain_cpu.py); "tie_third" is
# 0 -15- 2 -40- 1 -20- 4 with 3 isolated: 2m = 150 makes g(c) exact, and in sweep 1 vertex 1, alone, meets g({0, 2}) =
# 40 - 60 * 70 / 150 = 12 = 20 - 60 * 20 / 150 = g({4}).
GUARD_CASES = {
    "path_2": (lambda: _path(2), [({"max_levels": 1, "max_sweeps": 1}, [0, 0, 1]), ({}, [0, 0, 0])]),
    "path_3": (lambda: _path(3), [({"max_levels": 1, "max_sweeps": 1}, [0, 0, 1, 1]), ({}, [0, 0, 1, 1])]),
    "path_4": (lambda: _path(4), [({"max_levels": 1, "max_sweeps": 1}, [0, 0, 1, 1, 2]), ({}, [0, 0, 0, 1, 1])]),
    "star_hub_last": (lambda: _edges(5, [(i, 4, 1.0) for i in range(4)]),
                      [({"max_levels": 1, "max_sweeps": 1}, [0, 1, 0, 2, 0]), ({}, [0, 0, 0, 0, 0])]),
    "star_hub_first": (lambda: _edges(5, [(0, i, 1.0) for i in range(1, 5)]),
                       [({"max_levels": 1, "max_sweeps": 1}, [0, 0, 1, 2, 3]), ({}, [0, 0, 0, 0, 0])]),
    "tie_third": (lambda: _edges(5, [(0, 2, 15.0), (1, 2, 40.0), (1, 4, 20.0)]),
                  [({"max_levels": 1, "max_sweeps": 1}, [0, 1, 0, 2, 3]), ({"max_levels": 1, "max_sweeps": 2}, [0, 0, 0, 1, 2]),
                   ({}, [0, 0, 0, 1, 0])]),
}


def prefix_runs():
    """First-level sweep prefixes: the labelling after 1, 2, 3, 4 and 7 sweeps (sweeps 1 and 2 move disjoint halves)."""
    return [(name, {"max_levels": 1, "max_sweeps": s}) for name in PREFIX_CASES for s in PREFIX_SWEEPS]


def guard_runs():
    return [(name, opts, np.array(want, dtype=np.uint32)) for name, (_, runs) in GUARD_CASES.items() for opts, want in runs]


def run_id(run):
    return run[0] + "".join("-%s=%s" % kv for kv in sorted(run[1].items()))

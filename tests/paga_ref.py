"""PAGA as include/srx.h defines it, in Python integers and fractions: independent of the library.

E by a plain loop over the stored entries, float(int) for every conversion (correctly rounded, as the C conversions are),
Kruskal in the stated order, and the hash of the start positions in Python integers.  Tables are dicts keyed by (g, h), so a
case with 4096 groups costs what its connected pairs cost.
"""
from fractions import Fraction

import numpy as np

ROWS_PER_WORKGROUP = 512          # paga.hip's kPagaRows: a workgroup of the walk takes at most this many rows of one group
MASK = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def counts_of(indptr, indices, labels, G):
    """E as a dict {(g, h): count} and the sizes, by a plain loop over the entries."""
    E = {}
    lab = [int(x) for x in labels]
    ptr = [int(x) for x in indptr]
    ind = [int(x) for x in indices]
    for i in range(len(lab)):
        g = lab[i]
        for e in range(ptr[i], ptr[i + 1]):
            key = (g, lab[ind[e]])
            E[key] = E.get(key, 0) + 1
    sizes = [0] * G
    for g in lab:
        sizes[g] += 1
    return E, sizes


def dense_counts(E, G):
    out = np.zeros((G, G), dtype=np.uint64)
    for (g, h), c in E.items():
        out[g, h] = c
    return out


def sparse_counts(counts):
    counts = np.asarray(counts)
    return {(int(g), int(h)): int(counts[g, h]) for g, h in zip(*np.nonzero(counts))}


def from_counts(E, sizes, G, exact=False):
    """Everything after the counts.  E: {(g, h): count}; sizes: G integers.  Returns a dict with out_edges (list), the three
    tables as {(g, h): float} over their non-zero entries (tree at g < h only) and info (the counters of srx_paga_info).
    exact: also the tables as Fractions, before any rounding (`expected_exact`, `ratio_exact`)."""
    sizes = [int(s) for s in sizes]
    N = sum(sizes)
    es = [0] * G
    nnz = inner = 0
    for (g, h), c in E.items():
        es[g] += c
        nnz += c
        if g == h:
            inner += c
    pairs = sorted({(min(g, h), max(g, h)) for (g, h), c in E.items() if g != h and c > 0})
    conn, expected, edges = {}, {}, []
    exp_exact, ratio_exact = {}, {}
    clipped = 0
    for g, h in pairs:
        v = E.get((g, h), 0) + E.get((h, g), 0)
        num = es[g] * sizes[h] + es[h] * sizes[g]
        ex = float(num) / float(N - 1)
        r = float(v) / ex
        c = 1.0 if r > 1.0 else r
        clipped += r > 1.0
        expected[(g, h)] = expected[(h, g)] = ex
        conn[(g, h)] = conn[(h, g)] = c
        if exact:
            exp_exact[(g, h)] = Fraction(num, N - 1)
            ratio_exact[(g, h)] = Fraction(v) / Fraction(num, N - 1)
        if c > 0.0:
            edges.append((-c, g, h))
    edges.sort()
    root = list(range(G))

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x

    tree = {}
    for negc, g, h in edges:
        a, b = find(g), find(h)
        if a != b:
            root[max(a, b)] = min(a, b)
            tree[(g, h)] = -negc
    info = {"n": N, "nnz": nnz, "n_groups": G, "groups_empty": sum(s == 0 for s in sizes), "edges_inner": inner,
            "edges_inter": nnz - inner, "pairs_connected": len(pairs), "pairs_clipped": int(clipped), "tree_edges": len(tree),
            "components": G - len(tree)}
    out = {"sizes": sizes, "out_edges": es, "connectivities": conn, "expected": expected, "tree": tree, "info": info}
    if exact:
        out["expected_exact"], out["ratio_exact"] = exp_exact, ratio_exact
    return out


def dense(table, G):
    out = np.zeros((G, G))
    for (g, h), v in table.items():
        out[g, h] = v
    return out


def mix(z):
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def init_positions(labels, conn, pos, seed):
    """srx_paga_init_positions: conn G x G and pos G x dim as arrays; every f64 operation is one numpy scalar operation."""
    conn, pos = np.asarray(conn, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    G, dim = pos.shape
    nb = []
    for g in range(G):
        best, at = 0.0, None
        for h in range(G):
            if conn[g, h] > best:
                best, at = conn[g, h], h
        nb.append(at)
    out = np.zeros((len(labels), dim))
    half = np.float64(0.5)
    for i, g in enumerate(int(x) for x in labels):
        for c in range(dim):
            if nb[g] is None:
                out[i, c] = pos[g, c]
                continue
            dist = pos[g, c] - pos[nb[g], c]
            u = np.float64(mix(seed + GOLD * (i * dim + c + 1)) >> 11) * np.float64(2.0 ** -53)
            out[i, c] = (pos[g, c] - half * dist) + (u - half) * dist
    return out

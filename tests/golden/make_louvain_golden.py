"""Generates tests/golden/louvain_nx.json: the quality yardstick of the Louvain tests.

For every fixture of tests/louvain_ref.py (the k = 15 connectivities of Gaussian-cluster point sets, rebuilt from seeds, and
Zachary's karate club with its stored and with unit weights) it holds the modularity and the number of communities that
networkx.community.louvain_communities reaches for seeds 0..4, with networkx's own modularity function.  The karate club's
edge list is stored too, so that the tests need no networkx.
Run where networkx is installed:  python tests/golden/make_louvain_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
OUT = os.path.join(HERE, "louvain_nx.json")
SEEDS = (0, 1, 2, 3, 4)
NAMES = ("separated_3000", "separated_20011", "overlapping_6000", "karate_stored", "karate_unit")


def karate_edges():
    import networkx as nx
    g = nx.karate_club_graph()
    return [[int(u), int(v), float(d.get("weight", 1.0))] for u, v, d in sorted(g.edges(data=True))]


def run_networkx(W):
    import networkx as nx
    g = nx.from_scipy_sparse_array(W)
    out = []
    for seed in SEEDS:
        parts = nx.community.louvain_communities(g, weight="weight", resolution=1.0, seed=seed)
        out.append({"seed": seed, "modularity": float(nx.community.modularity(g, parts, weight="weight")),
                    "n_communities": len(parts)})
    return out


def build(names=NAMES, edges=None):
    import networkx as nx

    import louvain_ref
    edges = karate_edges() if edges is None else edges
    doc = {"networkx": nx.__version__, "k": 15, "seeds": list(SEEDS), "karate_edges": edges, "fixtures": {}}
    for name in names:
        if name.startswith("karate"):
            import scipy.sparse as sp
            e = np.array(edges)
            i, j = e[:, 0].astype(int), e[:, 1].astype(int)
            w = np.ones(len(e)) if name == "karate_unit" else e[:, 2]
            W = sp.coo_matrix((np.r_[w, w], (np.r_[i, j], np.r_[j, i])), shape=(34, 34)).tocsr()
        else:
            W, _ = louvain_ref.fixture_graph(name)
        doc["fixtures"][name] = {"n": int(W.shape[0]), "nnz": int(W.nnz), "seeds": run_networkx(W)}
        print(name, W.shape[0], W.nnz, [round(s["modularity"], 6) for s in doc["fixtures"][name]["seeds"]], flush=True)
    return doc


if __name__ == "__main__":
    json.dump(build(), open(OUT, "w"), indent=1)
    print(OUT)

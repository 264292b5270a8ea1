"""Writes tsne_kat.json: known answers of the t-SNE definition (include/srx.h) worked out on the CPU.

  start     the hashed start of three (n, seed) in Python integers (tests/tsne_ref.mix_int: no numpy arithmetic)
  quality   600 points in six separated clumps in 10 dimensions (tsne_ref.clumps, numpy's seeded generator), k = 30, u = 10:
            the exact KL (dense Z) and the label purity (the share of points whose 10 nearest neighbours in the embedding all
            carry their label) after the full default run of the f64 reference at theta = 0.5, from five hashed seeds
            (11 .. 15; the device test runs three others), and their ranges; beside them scikit-learn's TSNE(method="exact")
            at the same perplexity: the KL of ITS embedding under OUR P, and its purity.  The reference's purity range must
            reach scikit-learn's purity, or this script fails.

    python tests/golden/make_tsne_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tsne_ref as ref  # noqa: E402

N, DIM, K, U, DATA_SEED = 600, 10, 30, 10.0, 0
SEEDS = [11, 12, 13, 14, 15]


def start_kat():
    return [{"n": n, "seed": str(seed), "y": ref.random_start(n, seed).ravel().tolist()} for n, seed in ((1, 0), (3, 9), (2, 2 ** 64 - 1))]


def quality():
    x, labels = ref.clumps(N, DIM, seed=DATA_SEED)
    idx, dist = ref.host_knn(x, K)
    P, _, info, _ = ref.affinities(idx, dist, U)
    runs = []
    for seed in SEEDS:
        Y, li, _ = ref.layout(P, ref.random_start(N, seed))
        runs.append({"seed": seed, "kl": ref.exact_kl(P, Y), "purity": ref.purity(Y, labels), "kl_theta": float(li["kl"])})
        print(runs[-1], flush=True)
    out = {"n": N, "dim": DIM, "k": K, "perplexity": U, "data_seed": DATA_SEED, "theta": 0.5, "runs": runs, "nnz": info["nnz"],
           "kl_range": [min(r["kl"] for r in runs), max(r["kl"] for r in runs)],
           "purity_range": [min(r["purity"] for r in runs), max(r["purity"] for r in runs)]}
    from sklearn.manifold import TSNE
    emb = TSNE(n_components=2, perplexity=U, method="exact", init="random", random_state=0).fit_transform(x).astype(np.float64)
    out["sklearn_kl"] = ref.exact_kl(P, emb)
    out["sklearn_purity"] = ref.purity(emb, labels)
    print("sklearn exact: KL under our P %.4f, purity %.4f" % (out["sklearn_kl"], out["sklearn_purity"]))
    assert out["purity_range"][1] >= out["sklearn_purity"], (out["purity_range"], out["sklearn_purity"])
    return out


if __name__ == "__main__":
    kat = {"start": start_kat(), "quality": quality()}
    with open(os.path.join(HERE, "tsne_kat.json"), "w") as f:
        json.dump(kat, f, indent=1)
        f.write("\n")

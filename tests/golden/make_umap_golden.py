"""Writes umap_kat.json: known answers of the UMAP layout definition (include/srx.h) worked out on the CPU.

  hash      splitmix64's finaliser and negative-sample targets in Python integers (tests/umap_ref.mix_int / target_int:
            no numpy), which the vectorised reference must reproduce
  graph12   the hand-made 12-vertex graph of umap_ref.graph12() in 2 and 3 dimensions: Y^1, Y^3 of the definition evaluated in
            np.longdouble (rounded to f64 for storage) and the exact counters, E = 3, R = 5, seed 9, a = 1.577, b = 0.895
  quality   trustworthiness (15 neighbours) and silhouette of the planted labels after E = 200 epochs from the random start, for
            eight seeds, of the f64 reference on the planted 800-point graph and on louvain_ref's separated_20011 (scored on a
            fixed 2 000-vertex subsample), with the floors min - (max - min) the device must reach

    python tests/golden/make_umap_golden.py [--skip-large]
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import umap_ref as ref  # noqa: E402

A, B = 1.577, 0.895
SEEDS = list(range(1, 9))
SUBSAMPLE_SEED, SUBSAMPLE = 2024, 2000


def hash_kat():
    zs = [0, 1, 0x9E3779B97F4A7C15, 2 ** 64 - 1, 123456789012345]
    out = {"mix": [[str(z), str(ref.mix_int(z))] for z in zs], "targets": []}
    for seed, t, nnz, e, R, p, n in [(0, 1, 10, 0, 5, 0, 12), (9, 3, 32, 31, 5, 4, 12), (2 ** 64 - 1, 200, 17768, 17767, 32, 31, 800),
                                     (77, 1, 1, 0, 1, 0, 2), (5, 1048576, 2 ** 40, 2 ** 40 - 1, 32, 7, 2 ** 32 - 2)]:
        out["targets"].append({"seed": str(seed), "t": t, "nnz": nnz, "e": e, "R": R, "p": p, "n": n,
                               "k": ref.target_int(seed, t, nnz, e, R, p, n)})
    return out


def graph12_kat():
    W, Y0 = ref.graph12()
    out = {"a": A, "b": B, "n_epochs": 3, "rate": 5, "seed": 9}
    for dim in (2, 3):
        y0 = np.ascontiguousarray(Y0[:, :dim])
        _, info, kept = ref.layout(W, y0, A, B, 3, rate=5, seed=9, dtype=np.longdouble, keep=(1, 3))
        out["dim%d" % dim] = {"Y1": kept[1].astype(np.float64).tolist(), "Y3": kept[3].astype(np.float64).tolist(),
                              "counters": {k: info[k] for k in ref.COUNTERS}}
    return out


def quality_runs(x, lab, W, sub):
    a, b = A, B
    rows = []
    for seed in SEEDS:
        Y0 = ref.random_start(W.shape[0], 2, seed)
        Y, info, _ = ref.layout(W, Y0, a, b, 200, rate=5, seed=seed)
        tw, sil = ref.quality(x, Y, lab, sub)
        rows.append({"seed": seed, "trustworthiness": tw, "silhouette": sil, "samples": info["samples"], "max_abs": float(np.abs(Y).max())})
        print(rows[-1], flush=True)
    tw0, sil0 = ref.quality(x, ref.random_start(W.shape[0], 2, SEEDS[0]), lab, sub)
    return {"n": int(W.shape[0]), "nnz": int(W.nnz), "a": a, "b": b, "seeds": rows, "start_trustworthiness": tw0, "start_silhouette": sil0,
            "floor_trustworthiness": ref.quality_floor([r["trustworthiness"] for r in rows]),
            "floor_silhouette": ref.quality_floor([r["silhouette"] for r in rows])}


def main():
    path = os.path.join(HERE, "umap_kat.json")
    old = json.load(open(path)) if os.path.exists(path) else {}
    out = {"hash": hash_kat(), "graph12": graph12_kat(), "quality": dict(old.get("quality", {}))}
    x, lab, W = ref.planted()
    out["quality"]["planted_800"] = quality_runs(x, lab, W, None)
    if "--skip-large" not in sys.argv:
        import louvain_ref
        x, lab = louvain_ref.FIXTURES["separated_20011"]()
        W = louvain_ref.connectivities(x, 15)
        sub = np.sort(np.random.default_rng(SUBSAMPLE_SEED).choice(len(x), SUBSAMPLE, replace=False))
        out["quality"]["separated_20011"] = dict(quality_runs(x, lab, W, sub), subsample_seed=SUBSAMPLE_SEED, subsample=SUBSAMPLE)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Times of the UMAP transform (srx_umap_transform_knn) against a fitted data set of --ref cells: clustered points in --dims
dimensions stand for the PCA scores, their first two coordinates scaled to +-10 for the fitted layout (neighbours in the
scores are neighbours in the layout, as in a real one), the queries are reference points plus noise and their k-NN lists come
from srx_knn_points.  Per query count (min / median of --runs calls after --warmup): the membership kernel, the epochs at the
default chunk length and at chunk length 1 (one launch per epoch), the sampled (entry, epoch) pairs per second.  --host also
times the numpy restatement (tests/ingest_ref.py) at the first query count.  Report only: prints one JSON document.

    python scripts/ingest_time.py [--ref 1300000 --queries 10000,100000,1300000 --kq 16 --runs 5 --warmup 1 --host]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def min_med(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", type=int, default=1_300_000)
    ap.add_argument("--queries", default="10000,100000,1300000")
    ap.add_argument("--kq", type=int, default=16)
    ap.add_argument("--dims", type=int, default=10)
    ap.add_argument("--clusters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=3003)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import knn_points, umap_transform
    ctx = sr.Context.default()
    rng = np.random.default_rng(a.seed)
    centres = rng.standard_normal((a.clusters, a.dims)) * 6.0
    ref = centres[rng.integers(0, a.clusters, a.ref)] + rng.standard_normal((a.ref, a.dims))
    layout = np.ascontiguousarray(ref[:, :2] * (10.0 / np.abs(ref[:, :2]).max()))
    out = {"n_ref": a.ref, "kq": a.kq, "dim": 2, "lanes_per_query": F.UMAP_GROUP, "chunk_epochs": F.UMAP_TRANSFORM_CHUNK, "cases": []}
    for pos, nq in enumerate(int(v) for v in a.queries.split(",")):
        pick = rng.integers(0, a.ref, nq)
        q = ref[pick] + 0.5 * rng.standard_normal((nq, a.dims))
        t0 = time.perf_counter()
        idx, dist, _ = knn_points(ctx, ref, q, k=a.kq)
        knn_s = time.perf_counter() - t0

        def call(chunk):
            memb, ep, wall, info = [], [], [], None
            for i in range(a.warmup + a.runs):
                t0 = time.perf_counter()
                _, info = umap_transform(ctx, idx, dist, layout, chunk_epochs=chunk)
                w = time.perf_counter() - t0
                if i >= a.warmup:
                    memb.append(info["membership_ms"])
                    ep.append(info["ms"] - info["membership_ms"])
                    wall.append(w * 1e3)
            return memb, ep, wall, info

        memb, ep, wall, info = call(0)
        _, ep1, wall1, info1 = call(1)
        assert info1["samples"] == info["samples"]
        case = {"n_query": nq, "n_epochs": info["n_epochs"], "entries_active": info["entries_active"], "samples": info["samples"],
                "knn_points_s": round(knn_s, 3), "membership_ms": min_med(memb), "epochs_ms": min_med(ep),
                "epochs_ms_chunk_1": min_med(ep1), "call_wall_ms": min_med(wall), "call_wall_ms_chunk_1": min_med(wall1),
                "samples_per_s": round(info["samples"] / (min(ep) * 1e-3)), "samples_per_s_chunk_1": round(info["samples"] / (min(ep1) * 1e-3)),
                "rows_no_root": info["rows_no_root"], "rows_clamped": info["rows_clamped"]}
        if a.host and pos == 0:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import ingest_ref
            t0 = time.perf_counter()
            _, hi, _ = ingest_ref.transform(idx, dist, layout, info["a"], info["b"])
            case["numpy_restatement_s"] = round(time.perf_counter() - t0, 2)
            assert hi["samples"] == info["samples"]
        out["cases"].append(case)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

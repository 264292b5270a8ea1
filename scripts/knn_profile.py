"""Time of the exact k-nearest-neighbour search over the resident PCA scores (srx_knn_result after a pipeline step): device time
of the SRX_K_KNN class and wall time including the D2H of indices and distances, warm, median of --reps calls; achieved f32
FLOP/s on 2 N^2 d_padded; the share of rows the f64 pass recomputed; and (unless --no-sklearn) the wall time of sklearn's
brute-force search on the same points with --threads threads.

    python scripts/knn_profile.py [--cells 1300000] [--genes 28000] [--density 0.03] [--n-hvg 2000] [--n-pc 50] [--k 15]
                                  [--reps 5] [--no-sklearn] [--threads 16]

Prints one JSON line.  The matrix is srx_synth's (the bench's c3 shape by default), f32 storage."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import singlerust_amd as sr                                         # noqa: E402
from singlerust_amd import _ffi as F                                # noqa: E402
from singlerust_amd.memory.processing import neighbors              # noqa: E402


def padded_k(d):
    return next(w for w in (8, 20, 36, 52, 68, 132) if d < w)       # restates knn_padded_width over kKnnInstances (knn_internal.hpp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_300_000)
    ap.add_argument("--genes", type=int, default=28_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--n-hvg", type=int, default=2000)
    ap.add_argument("--n-pc", type=int, default=50)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    ctx = sr.Context.default()
    lib = F.lib()
    p = F.SynthParams()
    lib.srx_synth_defaults(C.byref(p), 3003, a.cells, a.genes, a.density)
    h = C.c_void_p()
    F.check(lib.srx_synth_generate(ctx.handle, C.byref(p), 0, a.cells, F.F32, F.STORE_F32, C.byref(h)), ctx.handle)
    ad = sr.IMAnnData(sr.DeviceCsr(ctx, h), None, None, [], [])
    opts = F.PcaOpts(a.n_pc, -1, -1, -1, 0, 0, 0, 0.0, 12345)
    res = F.PipelineResult()
    F.check(lib.srx_pipeline(ad.x().handle, 1e4, a.n_hvg, C.byref(opts), C.byref(res)), ctx.handle)
    n_pc = int(res.pca.n_pc)
    info = neighbors(ad, a.k)["info"]                                # warm: scratch allocation, code-object load
    walls, dev = [], []
    ctx.prof_enable(1 << F.K_KNN)
    for _ in range(a.reps):
        ctx.synchronize()
        ctx.prof_reset()
        t0 = time.perf_counter()
        info = neighbors(ad, a.k)["info"]
        walls.append((time.perf_counter() - t0) * 1e3)
        dev.append(ctx.prof_get(F.K_KNN)[0])
    ctx.prof_enable(0)
    flop = 2.0 * a.cells * a.cells * padded_k(n_pc)
    out = {"cells": a.cells, "n_pc": n_pc, "k": a.k, "d_padded": padded_k(n_pc), "n_candidates": info["n_candidates"],
           "knn_class_ms": {"min": round(min(dev), 2), "median": round(float(np.median(dev)), 2)},
           "wall_ms_with_d2h": {"min": round(min(walls), 2), "median": round(float(np.median(walls)), 2)},
           "f32_tflops_on_class_time": round(flop / (float(np.median(dev)) * 1e-3) / 1e12, 1),
           "rows_recomputed": info["rows_recomputed"], "recomputed_share": info["rows_recomputed"] / max(a.cells, 1)}
    if not a.no_sklearn:
        from sklearn.neighbors import NearestNeighbors
        from threadpoolctl import threadpool_limits
        x = np.zeros((a.cells, n_pc))
        F.check(lib.srx_result_fetch(ad.x().handle, F.ptr(x), None, None, None, None, None), ctx.handle)
        with threadpool_limits(limits=a.threads):
            t0 = time.perf_counter()
            nn = NearestNeighbors(n_neighbors=a.k + 1, algorithm="brute", n_jobs=a.threads).fit(x)
            sk = nn.kneighbors(return_distance=False, n_neighbors=a.k)
            out["sklearn_brute_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["speedup_vs_sklearn"] = round(out["sklearn_brute_wall_ms"] / out["wall_ms_with_d2h"]["median"], 1)
        got = ad.obsm["knn_indices"]
        out["rows_with_sklearn_set"] = int(sum(set(r) == set(s) for r, s in zip(got, sk)))
    print(json.dumps(out))
    if "speedup_vs_sklearn" in out and out["speedup_vs_sklearn"] <= 1.0:
        sys.exit("the device search (D2H included) is not faster than sklearn's brute force on the host")


if __name__ == "__main__":
    main()

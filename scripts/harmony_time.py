#!/usr/bin/env python
"""Times of the Harmony integration (srx_harmony_result) on the c3-shaped synthetic matrix: pipeline -> scores resident ->
Harmony at its defaults with --batches hashed batch labels.  Reported (min / median of --runs calls after --warmup): info.ms,
ms per cluster iteration, and the rate at which the iterations stream R and Zhat, counted as the least any implementation
moves per cluster iteration: R read once and written once (2 n K 8 bytes) and Zhat read once (n d 8 bytes).  The k-NN search
over the corrected block is timed beside it (wall clock of srx_knn_harmony without outputs).
Report only: prints one JSON document.

    python scripts/harmony_time.py [--cells 1300000 --genes 28000 --density 0.03 --batches 8 --runs 2 --warmup 1]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def min_med(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4)}


def hashed_batches(n, n_batches, seed):
    """batch of cell i = splitmix64(seed + i) mod n_batches"""
    import numpy as np
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(seed)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z % np.uint64(n_batches)).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_300_000)
    ap.add_argument("--genes", type=int, default=28_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=3003)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--clusters", type=int, default=0)
    ap.add_argument("--max-rounds", type=int, default=0)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-knn", action="store_true")
    a = ap.parse_args()
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing.harmony import _info_dict, _opts
    lib = F.lib()
    ctx = sr.Context.default()
    p = F.SynthParams()
    lib.srx_synth_defaults(C.byref(p), a.seed, a.cells, a.genes, a.density)
    h = C.c_void_p()
    F.check(lib.srx_synth_generate(ctx.handle, C.byref(p), 0, a.cells, F.F32, F.STORE_F32, C.byref(h)), ctx.handle)
    m = sr.DeviceCsr(ctx, h)
    m.prepare()
    opts, res = F.PcaOpts(50, -1, -1, -1, 0, 0, 0, 0.0, 12345), F.PipelineResult()
    F.check(lib.srx_pipeline(m.handle, 1e4, 2000, C.byref(opts), C.byref(res)), ctx.handle)
    batch = hashed_batches(a.cells, a.batches, a.seed)
    o = _opts(n_clusters=a.clusters, max_rounds=a.max_rounds)
    ms, wall, info, hm = [], [], F.HarmonyInfo(), C.c_void_p()
    for i in range(a.warmup + a.runs):
        if hm:
            lib.srx_harmony_free(hm)
        hm = C.c_void_p()
        t0 = time.perf_counter()
        F.check(lib.srx_harmony_result(m.handle, F.ptr(batch), a.batches, C.byref(o), C.byref(hm), C.byref(info)), ctx.handle)
        if i >= a.warmup:
            ms.append(info.ms)
            wall.append((time.perf_counter() - t0) * 1e3)
    d = _info_dict(info)
    iters = max(d["cluster_iters"], 1)
    stream = iters * (2.0 * a.cells * d["n_clusters"] * 8 + a.cells * d["d"] * 8)
    out = {"cells": a.cells, "d": d["d"], "n_batches": a.batches, "n_clusters": d["n_clusters"], "n_blocks": d["n_blocks"],
           "rounds": d["rounds"], "round_iters": d["round_iters"], "converged": d["converged"], "cluster_iters": d["cluster_iters"],
           "info_ms": min_med(ms), "call_wall_ms": min_med(wall), "ms_per_cluster_iter": round(min(ms) / iters, 4),
           "stream_bytes_per_iter": stream / iters, "stream_GBps": round(stream / (min(ms) * 1e-3) / 1e9, 2)}
    if not a.no_knn:
        ko, ki = F.KnnOpts(a.k, 0, 0, 0), F.KnnInfo()
        t = []
        for i in range(2):
            t0 = time.perf_counter()
            F.check(lib.srx_knn_harmony(hm, C.byref(ko), None, None, C.byref(ki)), ctx.handle)
            t.append((time.perf_counter() - t0) * 1e3)
        out["knn_harmony_wall_ms"] = round(min(t), 3)
        out["knn_rows_recomputed"] = int(ki.rows_recomputed)
    print(json.dumps(out, indent=1))
    lib.srx_harmony_free(hm)


if __name__ == "__main__":
    main()

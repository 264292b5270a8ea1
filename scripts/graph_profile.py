"""Time of the neighbour-graph build over the resident PCA scores (srx_neighbors_result after a pipeline step): device time of
the SRX_K_GRAPH class next to the SRX_K_KNN class of the same call, the algorithmic bytes of the build against the HBM
rate, wall time of the call, of fetching both matrices, and (unless --no-host) of building the same graph on the host with the
numpy / scipy restatement the tests use (tests/graph_ref.py) from the fetched k-NN list.

    python scripts/graph_profile.py [--cells 1300000] [--genes 28000] [--density 0.03] [--n-hvg 2000] [--n-pc 50] [--k 15]
                                    [--reps 3] [--no-host]

Prints one JSON line.  The matrix is srx_synth's (the bench's c3 shape by default), f32 storage.  Per-kernel times come from
running this script under `rocprofv3 --kernel-trace --stats` (profiles/graph.md)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import singlerust_amd as sr                                         # noqa: E402
from singlerust_amd import _ffi as F                                # noqa: E402
from singlerust_amd.memory.processing.neighbors import Graph        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_300_000)
    ap.add_argument("--genes", type=int, default=28_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--n-hvg", type=int, default=2000)
    ap.add_argument("--n-pc", type=int, default=50)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
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
    kopts = F.KnnOpts(a.k, 0, 0, 0)

    def once():
        gh = C.c_void_p()
        F.check(lib.srx_neighbors_result(ad.x().handle, C.byref(kopts), None, C.byref(gh)), ctx.handle)
        return Graph(ctx, gh)

    g = once()                                                       # warm: scratch allocation, code-object load
    walls, dev_graph, dev_knn, gbytes = [], [], [], 0.0
    ctx.prof_enable((1 << F.K_KNN) | (1 << F.K_GRAPH))
    for _ in range(a.reps):
        g.free()
        ctx.synchronize()
        ctx.prof_reset()
        t0 = time.perf_counter()
        g = once()
        walls.append((time.perf_counter() - t0) * 1e3)
        dev_knn.append(ctx.prof_get(F.K_KNN)[0])
        ms, _, gbytes = ctx.prof_get(F.K_GRAPH)
        dev_graph.append(ms)
    ctx.prof_enable(0)
    info = g.info()
    t0 = time.perf_counter()
    d = g.fetch(F.GRAPH_DISTANCES)
    c = g.fetch(F.GRAPH_CONNECTIVITIES)
    fetch_ms = (time.perf_counter() - t0) * 1e3
    med = float(np.median(dev_graph))
    out = {"cells": a.cells, "k": a.k, "graph": info,
           "graph_class_ms": {"min": round(min(dev_graph), 2), "median": round(med, 2)},
           "knn_class_ms": {"min": round(min(dev_knn), 2), "median": round(float(np.median(dev_knn)), 2)},
           "graph_share_of_knn": round(med / float(np.median(dev_knn)), 4),
           "wall_ms_knn_plus_graph": {"min": round(min(walls), 2), "median": round(float(np.median(walls)), 2)},
           "algorithmic_mbytes": round(gbytes / 1e6, 1), "algorithmic_gb_per_s": round(gbytes / (med * 1e-3) / 1e9, 1),
           "ms_at_8_tb_per_s": round(gbytes / 8e12 * 1e3, 3), "fetch_both_ms": round(fetch_ms, 1)}
    if not a.no_host:
        import graph_ref
        from threadpoolctl import threadpool_limits
        idx = d[1].reshape(a.cells, a.k)
        dist = d[2].reshape(a.cells, a.k)
        with threadpool_limits(limits=16):
            t0 = time.perf_counter()
            _, Cr, _, _, want = graph_ref.graph(idx, dist)
            out["host_restatement_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["host_matches"] = bool(want == info and np.array_equal(Cr.indices, c[1].astype(Cr.indices.dtype))
                                   and float(np.abs(Cr.data - c[2]).max()) <= 2e-8)
        out["speedup_vs_host"] = round(out["host_restatement_wall_ms"] / med, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

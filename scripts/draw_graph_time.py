#!/usr/bin/env python
"""Times of the ForceAtlas2 layout (srx_draw_graph*) on the c3-shaped synthetic matrix: pipeline -> neighbours (k) ->
connectivities -> layout, everything resident.  Report only: prints one JSON document.

Default mode: --runs calls of srx_draw_graph after --warmup, each of --iters iterations from the hashed start (or, with
--clumped-start, from a given start of --clumps hashed Gaussian clumps of sd 1 on a circle of radius 50: the geometry of a
clumped layout without running one); info.ms (hipEvent time of the device work) as min / median, the time per iteration, and
the four walk counters per point of the last iteration.

--walk LAYOUT: walk against walk.  The same Y, theta and levels through srx_draw_graph_forces (k_fa_walk) and
srx_tsne_forces (k_tsne_walk), alternating, --runs times after --warmup.  LAYOUT is "pca" (the t-SNE PCA start: smooth),
"tsne50" (the layout after the 50 t-SNE iterations of scripts/tsne_time.py) or "tsne25" (the same run stopped at the end of
its 25 exaggerated iterations: the most clumped layout of that run).  Neither diagnostic reports a device time of its own (both copy their
inputs), so the kernels' times are read from a kernel trace of this mode, a run of its own per layout:
`rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python scripts/draw_graph_time.py --walk tsne50 ...`, then
`python profiles/summarize_rocpd.py DIR/.../NAME_results.db --last RUNS`; the wall times printed here include the copies.

--networkx N: the host baseline, networkx.forceatlas2_layout (dense, 100 iterations) on the k-NN connectivities of N generic
points (no GPU work besides building that graph).

    python scripts/draw_graph_time.py [--cells 100000 --genes 28000 --density 0.03 --k 15 --theta 1.2 --iters 500]
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


def clumped_start(np, n, clumps):
    rng = np.random.default_rng(7)
    ang = 2.0 * np.pi * (np.arange(n) % clumps) / clumps
    return np.ascontiguousarray(50.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1) + rng.standard_normal((n, 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100_000)
    ap.add_argument("--genes", type=int, default=28_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=3003)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--theta", type=float, default=1.2)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--levels", type=int, default=0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clumped-start", action="store_true")
    ap.add_argument("--clumps", type=int, default=20)
    ap.add_argument("--walk", choices=("pca", "tsne25", "tsne50"))
    ap.add_argument("--perplexity", type=float, default=21.0)
    ap.add_argument("--networkx", type=int, default=0)
    a = ap.parse_args()
    import numpy as np

    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory import processing as P
    from singlerust_amd.memory.processing.neighbors import Graph
    lib = F.lib()
    ctx = sr.Context.default()

    if a.networkx:
        import networkx as nx
        import scipy.sparse as sp
        n = a.networkx
        idx, dist, _ = P.knn_points(ctx, np.random.default_rng(1).standard_normal((n, 10)), None, a.k)
        ip, ind, dat = P.connectivities_from_knn(ctx, idx, dist).fetch(F.GRAPH_CONNECTIVITIES)
        G = nx.from_scipy_sparse_array(sp.csr_matrix((dat, ind.astype(np.int64), ip.astype(np.int64)), shape=(n, n)))
        t0 = time.perf_counter()
        nx.forceatlas2_layout(G, max_iter=100, scaling_ratio=2.0, gravity=1.0, weight="weight", seed=0)
        host_s = time.perf_counter() - t0
        _, info = P.draw_graph_csr(ctx, (ip, ind, dat), None, n_iter=100)
        _, info = P.draw_graph_csr(ctx, (ip, ind, dat), None, n_iter=100)
        print(json.dumps({"n": n, "k": a.k, "nnz": int(ind.size), "iterations": 100, "networkx": nx.__version__,
                          "networkx_wall_s": round(host_s, 3), "device_ms_theta_1.2": round(info["ms"], 3)}, indent=1))
        return

    p = F.SynthParams()
    lib.srx_synth_defaults(C.byref(p), a.seed, a.cells, a.genes, a.density)
    h = C.c_void_p()
    F.check(lib.srx_synth_generate(ctx.handle, C.byref(p), 0, a.cells, F.F32, F.STORE_F32, C.byref(h)), ctx.handle)
    m = sr.DeviceCsr(ctx, h)
    m.prepare()
    opts, res = F.PcaOpts(50, -1, -1, -1, 0, 0, 0, 0.0, 12345), F.PipelineResult()
    F.check(lib.srx_pipeline(m.handle, 1e4, 2000, C.byref(opts), C.byref(res)), ctx.handle)
    gh = C.c_void_p()
    t0 = time.perf_counter()
    F.check(lib.srx_neighbors_result(m.handle, C.byref(F.KnnOpts(a.k, 0, 0, 0)), None, C.byref(gh)), ctx.handle)
    graph_s = time.perf_counter() - t0
    graph = Graph(ctx, gh)
    gi = graph.info()
    n = a.cells

    if a.walk:
        ts = P.tsne_affinities_graph(graph, a.perplexity)
        if a.walk == "pca":
            Y, _ = P.tsne_run(ts, m, "pca", n_iter=1, learning_rate=1e-300)          # nothing moves: the start itself
        else:
            Y, _ = P.tsne_run(ts, m, "pca", theta=0.5, n_iter=50, exaggeration_iters=25, stop_after=25 if a.walk == "tsne25" else 0)
        W = graph.fetch(F.GRAPH_CONNECTIVITIES)
        wall = {"fa": [], "tsne": []}
        for i in range(a.warmup + a.runs):
            t0 = time.perf_counter()
            _, _, _, _, fi = P.draw_graph_forces(ctx, W, Y, a.theta, a.levels)
            t1 = time.perf_counter()
            _, _, _, ti = P.tsne_forces(ts, Y, a.theta, a.levels)
            t2 = time.perf_counter()
            if i >= a.warmup:
                wall["fa"].append((t1 - t0) * 1e3)
                wall["tsne"].append((t2 - t1) * 1e3)
        print(json.dumps({"cells": n, "k": a.k, "layout": a.walk, "theta": a.theta, "levels": fi["levels"], "side": fi["side"],
                          "fa": {c: round(fi[c] / n, 2) for c in ("cells_accepted", "cells_exact", "pairs_exact", "pairs_coincident")},
                          "tsne": {c: round(ti[c] / n, 2) for c in ("cells_accepted", "cells_exact", "pairs_exact")},
                          "wall_ms_with_copies": {k: min_med(v) for k, v in wall.items()}}, indent=1))
        return

    y0 = clumped_start(np, n, a.clumps) if a.clumped_start else None
    o = F.Fa2Opts(a.theta, 2.0, 1.0, 1.0, 0, a.iters, 0, a.levels, F.FA2_INIT_GIVEN if a.clumped_start else F.FA2_INIT_RANDOM, 0, 0)
    ms, info = [], F.Fa2Info()
    for i in range(a.warmup + a.runs):
        F.check(lib.srx_draw_graph(graph.handle, C.byref(o), F.ptr(y0), None, C.byref(info)), ctx.handle)
        if i >= a.warmup:
            ms.append(info.ms)
    print(json.dumps({"cells": n, "k": a.k, "theta": a.theta, "levels": int(info.levels), "nnz": int(gi["nnz_connectivities"]),
                      "total_mass": int(info.total_mass), "start": "clumped (given)" if a.clumped_start else "hashed",
                      "graph_wall_s": round(graph_s, 3), "iters": a.iters, "call_ms": min_med(ms),
                      "ms_per_iter": round(min(ms) / max(a.iters, 1), 4), "speed": info.speed, "side": info.side,
                      "cells_accepted_per_point": round(info.cells_accepted / n, 2), "cells_exact_per_point": round(info.cells_exact / n, 3),
                      "pairs_exact_per_point": round(info.pairs_exact / n, 2),
                      "pairs_coincident_per_point": round(info.pairs_coincident / n, 4)}, indent=1))


if __name__ == "__main__":
    main()

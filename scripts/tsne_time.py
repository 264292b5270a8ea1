#!/usr/bin/env python
"""Times of the t-SNE layout (srx_tsne_*) on the c3-shaped synthetic matrix: pipeline -> neighbours (k) -> affinities
(perplexity u) -> layout from the PCA start, everything resident.  Reported (min / median of --runs calls after --warmup):
the affinities' wall time, info.ms of a call of --iters iterations and of a call stopped after one, the time per iteration from
their difference, the same with theta = 1e9 (every walk ends at the four level-1 cells, so the difference to the run at
--theta is the traversal; what is left is the pyramid build plus attraction + update), and the three walk counters per point of
the last iteration.  The split of the rest by kernel is read from a kernel trace of this script
(`rocprofv3 --kernel-trace --stats -- python scripts/tsne_time.py --runs 1 --warmup 0 --skip-flat`: the k_tsne_* rows; the
run at theta = 1e9 evolves another layout, so its difference is an estimate and the trace is the measurement).  --sklearn adds
scikit-learn's barnes_hut wall time on the host on the fetched scores; --affinities-only stops before the layout (the size at
which the uniform pyramid's dense cells make an iteration take minutes: profiles/tsne.md).  Report only: prints one JSON document.

    python scripts/tsne_time.py [--cells 1300000 --genes 28000 --density 0.03 --k 64 --perplexity 21 --theta 0.5 --iters 50]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_300_000)
    ap.add_argument("--genes", type=int, default=28_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=3003)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--perplexity", type=float, default=21.0)
    ap.add_argument("--theta", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--levels", type=int, default=0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--skip-flat", action="store_true", help="no second pair of calls at theta = 1e9 (for a kernel trace)")
    ap.add_argument("--affinities-only", action="store_true", help="stop after the affinities (no layout)")
    a = ap.parse_args()
    import numpy as np

    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
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
    graph = C.c_void_p()
    t0 = time.perf_counter()
    F.check(lib.srx_neighbors_result(m.handle, C.byref(F.KnnOpts(a.k, 0, 0, 0)), None, C.byref(graph)), ctx.handle)
    graph_s = time.perf_counter() - t0
    aff_ms = []
    ts = C.c_void_p()
    for i in range(a.warmup + a.runs):
        if ts:
            lib.srx_tsne_free(ts)
        ts = C.c_void_p()
        t0 = time.perf_counter()
        F.check(lib.srx_tsne_affinities_graph(graph, a.perplexity, C.byref(ts)), ctx.handle)
        if i >= a.warmup:
            aff_ms.append((time.perf_counter() - t0) * 1e3)
    ti = F.TsneInfo()
    F.check(lib.srx_tsne_info_get(ts, C.byref(ti)), ctx.handle)

    if a.affinities_only:
        print(json.dumps({"cells": a.cells, "k": a.k, "perplexity": a.perplexity, "nnz": int(ti.nnz), "n_mutual": int(ti.n_mutual),
                          "rows_no_root": int(ti.rows_no_root), "graph_wall_s": round(graph_s, 3),
                          "affinities_wall_ms": min_med(aff_ms)}, indent=1))
        lib.srx_tsne_free(ts)
        lib.srx_graph_free(graph)
        return

    def call(stop_after, theta):
        o = F.TsneOpts(theta, 12.0, 0.0, 0, a.iters, min(250, a.iters // 2), stop_after, a.levels, F.TSNE_INIT_PCA, 0)
        ms, info = [], F.TsneRunInfo()
        for i in range(a.warmup + a.runs):
            F.check(lib.srx_tsne_run(ts, m.handle, C.byref(o), None, None, C.byref(info)), ctx.handle)
            if i >= a.warmup:
                ms.append(info.ms)
        return ms, info

    def per_iter(theta):
        full, info = call(0, theta)
        one, _ = call(1, theta)
        # a call of s iterations runs s + 1 force evaluations (the last one for Z and the KL): a.iters - 1 more steps
        return (min(full) - min(one)) / max(a.iters - 1, 1), full, one, info

    it, full, one, info = per_iter(a.theta)
    it_flat = it if a.skip_flat else per_iter(1e9)[0]
    out = {"cells": a.cells, "k": a.k, "perplexity": a.perplexity, "theta": a.theta, "levels": int(info.levels), "nnz": int(ti.nnz),
           "rows_no_root": int(ti.rows_no_root), "graph_wall_s": round(graph_s, 3), "affinities_wall_ms": min_med(aff_ms),
           "iters": a.iters, "call_ms": min_med(full), "one_iter_call_ms": min_med(one), "ms_per_iter": round(it, 4),
           "ms_per_iter_without_traversal": round(it_flat, 4), "traversal_ms_per_iter": round(it - it_flat, 4),
           "cells_accepted_per_point": round(info.cells_accepted / a.cells, 2), "cells_exact_per_point": round(info.cells_exact / a.cells, 3),
           "pairs_exact_per_point": round(info.pairs_exact / a.cells, 2), "Z": info.Z, "kl": info.kl, "eta": info.eta}
    if a.sklearn:
        from sklearn.manifold import TSNE
        scores = np.zeros((a.cells, 50))
        F.check(lib.srx_result_fetch(m.handle, F.ptr(scores), None, None, None, None, None), ctx.handle)
        t0 = time.perf_counter()
        TSNE(perplexity=a.perplexity, method="barnes_hut", init="pca", random_state=0).fit(scores)
        out["sklearn_barnes_hut_wall_s"] = round(time.perf_counter() - t0, 2)
    print(json.dumps(out, indent=1))
    lib.srx_tsne_free(ts)
    lib.srx_graph_free(graph)


if __name__ == "__main__":
    main()

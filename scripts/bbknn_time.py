"""Time of BBKNN over the resident scores (srx_bbknn_result after a pipeline step): the hipEvent stage times of srx_bbknn_info
(sort, search, merge, graph, trim and the whole call), warm, median of --reps calls, at the default trim, with no trim and at
trim = K (where most rows are over trim and go through the selection).  Beside it, in the same run on the same scores, the
yardstick: srx_neighbors_result at k = K (wall time: the call drains the stream before it returns).  With --ref-cells N > 0 the
numpy restatement of tests/bbknn_ref.py builds the list of a smaller fit on the host and the two lists are compared.

    python scripts/bbknn_time.py [--cells 1300000 100000] [--genes 28000] [--density 0.03] [--n-hvg 2000] [--n-pc 50]
                                 [--batches 8] [--k-within 3] [--reps 5] [--ref-cells 10000]
                                 [--what both|bbknn|neighbors] [--trims default_trim no_trim trim_K]

Prints one JSON line.  The matrix is srx_synth's (the bench's c3 shape by default), f32 storage; the batch labels are a hash of
the cell number, so every batch is spread over the whole matrix."""
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
from singlerust_amd.memory.processing.neighbors import Graph, _bbknn_dict        # noqa: E402

STAGES = ("ms", "ms_sort", "ms_search", "ms_merge", "ms_graph", "ms_trim")


def fitted(ctx, a, cells):
    lib = F.lib()
    p = F.SynthParams()
    lib.srx_synth_defaults(C.byref(p), 3003, cells, a.genes, a.density)
    h = C.c_void_p()
    F.check(lib.srx_synth_generate(ctx.handle, C.byref(p), 0, cells, F.F32, F.STORE_F32, C.byref(h)), ctx.handle)
    ad = sr.IMAnnData(sr.DeviceCsr(ctx, h), None, None, [], [])
    opts = F.PcaOpts(a.n_pc, -1, -1, -1, 0, 0, 0, 0.0, 12345)
    res = F.PipelineResult()
    F.check(lib.srx_pipeline(ad.x().handle, 1e4, a.n_hvg, C.byref(opts), C.byref(res)), ctx.handle)
    return ad


def hashed_batches(n, B):
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)
    return (h % np.uint64(B)).astype(np.uint32)


def bbknn_once(ctx, ad, batch, B, kw, trim):
    opts = F.BbknnOpts(kw, 0, trim)
    info = F.BbknnInfo()
    h = C.c_void_p()
    t0 = time.perf_counter()
    F.check(F.lib().srx_bbknn_result(ad.x().handle, F.ptr(batch), B, C.byref(opts), C.byref(info), C.byref(h)), ctx.handle)
    wall = (time.perf_counter() - t0) * 1e3
    Graph(ctx, h).free()
    return info, wall


def neighbors_once(ctx, ad, k):
    kopts = F.KnnOpts(k, 0, 0, 0)
    h = C.c_void_p()
    t0 = time.perf_counter()
    F.check(F.lib().srx_neighbors_result(ad.x().handle, C.byref(kopts), None, C.byref(h)), ctx.handle)
    wall = (time.perf_counter() - t0) * 1e3
    Graph(ctx, h).free()
    return wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[1_300_000, 100_000])
    ap.add_argument("--genes", type=int, default=28_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--n-hvg", type=int, default=2000)
    ap.add_argument("--n-pc", type=int, default=50)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--k-within", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-cells", type=int, default=10_000)
    ap.add_argument("--what", choices=("both", "bbknn", "neighbors"), default="both")     # one of the two alone: for a kernel trace
    ap.add_argument("--trims", nargs="+", default=["default_trim", "no_trim", "trim_K"])
    a = ap.parse_args()
    ctx = sr.Context.default()
    B, kw = a.batches, a.k_within
    K = kw * B - 1
    out = {"batches": B, "neighbors_within_batch": kw, "K": K, "runs": []}
    for cells in a.cells:
        ad = fitted(ctx, a, cells)
        batch = hashed_batches(cells, B)
        run = {"cells": cells}
        for name, trim in (("default_trim", -1), ("no_trim", 0), ("trim_K", K)):
            if a.what == "neighbors" or name not in a.trims:
                continue
            bbknn_once(ctx, ad, batch, B, kw, trim)                       # warm: scratch allocation, code-object load
            rows, info = [], None
            for _ in range(a.reps):
                info, wall = bbknn_once(ctx, ad, batch, B, kw, trim)
                rows.append([getattr(info, s) for s in STAGES] + [wall])
            med = np.median(np.array(rows), axis=0)
            d = _bbknn_dict(info)
            run[name] = {"ms": {s: round(float(v), 3) for s, v in zip(STAGES + ("wall",), med)},
                         "info": {k: v for k, v in d.items() if k not in STAGES}}
        if a.what != "bbknn":
            neighbors_once(ctx, ad, K)
            walls = [neighbors_once(ctx, ad, K) for _ in range(a.reps)]
            run["neighbors_result_k%d_wall_ms" % K] = round(float(np.median(walls)), 3)
        out["runs"].append(run)
        del ad
    if a.ref_cells > 0:
        import bbknn_ref as ref
        from singlerust_amd.memory.processing import bbknn_points
        n = a.ref_cells
        ad = fitted(ctx, a, n)
        scores = np.zeros((n, a.n_pc))
        F.check(F.lib().srx_result_fetch(ad.x().handle, F.ptr(scores), None, None, None, None, None), ctx.handle)
        batch = hashed_batches(n, B)
        idx, dist, _, info = bbknn_points(ctx, scores, batch, kw, None, 0, B, graph=False)
        t0 = time.perf_counter()
        want_i, want_d = ref.bbknn_list(scores, batch, B, kw)
        host_ms = (time.perf_counter() - t0) * 1e3
        out["numpy"] = {"cells": n, "host_ms": round(host_ms, 1), "device_ms": round(info["ms"], 3),
                        "indices_equal": bool(np.array_equal(idx, want_i)),
                        "distance_max_rel_diff": float(np.max(np.abs(dist - want_d) / np.maximum(want_d, 1e-300)))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Time of the shared-nearest-neighbour graph over the resident k-NN list (srx_neighbors_result after a pipeline step, then
srx_snn_graph on the handle): srx_snn_info's hipEvent times (the whole call; the reverse lists, the count pass and the fill pass
of it), warm, median of --reps calls, for every k of --k, with the counters that say what the list looks like (in-degrees,
candidates per row, the rows of each route).  Beside it the bytes the call must move (the list in, C out) against the streaming
rate k_row_sum reaches, and the bytes the two passes gather (4 B per candidate, twice).  With --scipy-cells N > 0 a second,
smaller list is fetched and scipy forms A A^T, the Jaccard values and the pruned CSR on the host; the two results are compared.

    python scripts/snn_time.py [--cells 1300000] [--genes 28000] [--density 0.03] [--n-hvg 2000] [--n-pc 50] [--k 15 19]
                               [--prune 0.0666...] [--reps 3] [--scipy-cells 100000]

Prints one JSON line.  The matrix is srx_synth's (the bench's c3 shape by default), f32 storage: the list is the real search's
over clumped scores, so the in-degrees are a k-NN graph's, not a random list's.  Per-kernel times come from running this script
under `rocprofv3 --kernel-trace --stats` (profiles/snn.md)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import singlerust_amd as sr                                         # noqa: E402
from singlerust_amd import _ffi as F                                # noqa: E402
from singlerust_amd.memory.processing._common import flat_info      # noqa: E402
from singlerust_amd.memory.processing.neighbors import Graph        # noqa: E402

STREAM_TBS = 5.8          # k_row_sum's read rate (the kernel table)


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


def knn_graph(ctx, ad, k):
    kopts = F.KnnOpts(k, 0, 0, 0)
    gh = C.c_void_p()
    F.check(F.lib().srx_neighbors_result(ad.x().handle, C.byref(kopts), None, C.byref(gh)), ctx.handle)
    return Graph(ctx, gh)


def snn_once(ctx, g, opts, info):
    h = C.c_void_p()
    t0 = time.perf_counter()
    F.check(F.lib().srx_snn_graph(g.handle, C.byref(opts), C.byref(info), C.byref(h)), ctx.handle)
    wall = (time.perf_counter() - t0) * 1e3
    return Graph(ctx, h), wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_300_000)
    ap.add_argument("--genes", type=int, default=28_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--n-hvg", type=int, default=2000)
    ap.add_argument("--n-pc", type=int, default=50)
    ap.add_argument("--k", type=int, nargs="+", default=[15, 19])
    ap.add_argument("--prune", type=float, default=1.0 / 15.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scipy-cells", type=int, default=100_000)
    a = ap.parse_args()
    ctx = sr.Context.default()
    opts = F.SnnOpts(F.SNN_JACCARD, F.SNN_PAIRS_SHARED, 1, 0, a.prune)
    out = {"cells": a.cells, "prune": a.prune, "runs": []}
    ad = fitted(ctx, a, a.cells)
    for k in a.k:
        g = knn_graph(ctx, ad, k)
        info = F.SnnInfo()
        snn_once(ctx, g, opts, info)[0].free()                       # warm: scratch allocation, code-object load
        rows = []
        for _ in range(a.reps):
            s, wall = snn_once(ctx, g, opts, info)
            s.free()
            rows.append((info.ms, info.ms_lists, info.ms_count, info.ms_fill, wall))
        med = np.median(np.array(rows), axis=0)
        i = flat_info(info)
        must = a.cells * k * 4 + i["nnz"] * 12 + (a.cells + 1) * 8       # the list in, C out
        gathered = i["sum_candidates"] * 4 * 2                           # every candidate read once per pass
        run = {"k": k, "info": i,
               "ms": {"call": round(med[0], 3), "lists": round(med[1], 3), "count": round(med[2], 3), "fill": round(med[3], 3),
                      "wall": round(med[4], 3), "call_min": round(min(r[0] for r in rows), 3)},
               "bytes_must_move": must, "floor_ms": round(must / (STREAM_TBS * 1e12) * 1e3, 4),
               "bytes_gathered": gathered, "gather_TBs_in_passes": round(gathered / ((med[2] + med[3]) * 1e-3) / 1e12, 3),
               "staging_bytes_one_pass": i["sum_candidates"] * 12}
        out["runs"].append(run)
        g.free()
    del ad
    if a.scipy_cells > 0:
        import scipy.sparse as sp
        n, k = a.scipy_cells, a.k[0]
        ad2 = fitted(ctx, a, n)
        g2 = knn_graph(ctx, ad2, k)
        info = F.SnnInfo()
        snn_once(ctx, g2, opts, info)[0].free()
        s, _ = snn_once(ctx, g2, opts, info)
        t0 = time.perf_counter()
        dptr, dind, _ = g2.fetch(F.GRAPH_DISTANCES)
        fetch_ms = (time.perf_counter() - t0) * 1e3
        dev = s.fetch(F.GRAPH_CONNECTIVITIES)
        K = k + 1
        t0 = time.perf_counter()
        A = sp.csr_matrix((np.ones(dind.size, dtype=np.int64), dind, dptr.astype(np.int64)), shape=(n, n)) + sp.identity(n, dtype=np.int64, format="csr")
        S = (A @ A.T).tocsr()
        S.setdiag(0)
        S.eliminate_zeros()
        J = S.data.astype(np.float64) / (2 * K - S.data).astype(np.float64)
        S = sp.csr_matrix((J, S.indices, S.indptr), shape=(n, n))
        S.data[S.data < a.prune] = 0.0
        S.eliminate_zeros()
        S.sort_indices()
        host_ms = (time.perf_counter() - t0) * 1e3
        equal = (np.array_equal(S.indptr.astype(np.uint64), dev[0]) and np.array_equal(S.indices.astype(np.uint32), dev[1])
                 and np.array_equal(S.data.view(np.uint64), dev[2].view(np.uint64)))
        out["scipy"] = {"cells": n, "k": k, "host_ms": round(host_ms, 1), "fetch_list_ms": round(fetch_ms, 2),
                        "device_ms": round(info.ms, 3), "nnz": int(info.nnz), "equal": bool(equal)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

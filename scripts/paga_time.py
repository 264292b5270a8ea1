"""Time of PAGA over the resident neighbour graph (srx_neighbors_result after a pipeline step, srx_louvain, then srx_paga with the
labels where they lie): info.ms (hipEvent time of the device work: the label sort and the walk) and wall time, warm, median of
--reps calls; beside it the time to read D's indices once at the streaming rate k_row_sum reaches (5.8 TB/s), which
is the walk's floor, and the 12.7 ms of the graph build (profiles/graph.md).  With --scipy-cells N > 0 a second, smaller graph
is fetched and the same counts are made on the host by scipy (one-hot^T A one-hot), timed without the fetch.

    python scripts/paga_time.py [--cells 1300000] [--genes 28000] [--density 0.03] [--n-hvg 2000] [--n-pc 50] [--k 15]
                                [--reps 3] [--scipy-cells 100000]

Prints one JSON line.  The matrix is srx_synth's (the bench's c3 shape by default), f32 storage.  Per-kernel times come from
running this script under `rocprofv3 --kernel-trace --stats` (profiles/paga.md)."""
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
GRAPH_BUILD_MS = 12.7     # srx_neighbors_from_knn at the c3 shape (profiles/graph.md)


def clustered_graph(ctx, a, cells):
    """(graph, n_communities): pipeline, k-NN graph and Louvain on a synthetic matrix of `cells` rows."""
    lib = F.lib()
    p = F.SynthParams()
    lib.srx_synth_defaults(C.byref(p), 3003, cells, a.genes, a.density)
    h = C.c_void_p()
    F.check(lib.srx_synth_generate(ctx.handle, C.byref(p), 0, cells, F.F32, F.STORE_F32, C.byref(h)), ctx.handle)
    ad = sr.IMAnnData(sr.DeviceCsr(ctx, h), None, None, [], [])
    opts = F.PcaOpts(a.n_pc, -1, -1, -1, 0, 0, 0, 0.0, 12345)
    res = F.PipelineResult()
    F.check(lib.srx_pipeline(ad.x().handle, 1e4, a.n_hvg, C.byref(opts), C.byref(res)), ctx.handle)
    kopts = F.KnnOpts(a.k, 0, 0, 0)
    gh = C.c_void_p()
    F.check(lib.srx_neighbors_result(ad.x().handle, C.byref(kopts), None, C.byref(gh)), ctx.handle)
    g = Graph(ctx, gh)
    li = F.LouvainInfo()
    F.check(lib.srx_louvain(g.handle, None, None, C.byref(li)), ctx.handle)
    return g, int(li.n_communities), float(li.ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_300_000)
    ap.add_argument("--genes", type=int, default=28_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--n-hvg", type=int, default=2000)
    ap.add_argument("--n-pc", type=int, default=50)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scipy-cells", type=int, default=100_000)
    a = ap.parse_args()
    ctx = sr.Context.default()
    lib = F.lib()
    g, G, louvain_ms = clustered_graph(ctx, a, a.cells)
    info = F.PagaInfo()

    def once():
        t0 = time.perf_counter()
        F.check(lib.srx_paga(g.handle, None, G, None, C.byref(info)), ctx.handle)
        return (time.perf_counter() - t0) * 1e3

    once()                                                           # warm: scratch allocation, code-object load
    walls, dev = [], []
    for _ in range(a.reps):
        walls.append(once())
        dev.append(info.ms)
    med = float(np.median(dev))
    floor_ms = info.nnz * 4 / (STREAM_TBS * 1e12) * 1e3
    out = {"cells": a.cells, "k": a.k, "n_groups": G, "louvain_ms": round(louvain_ms, 2), "paga": flat_info(info),
           "paga_ms": {"min": round(min(dev), 4), "median": round(med, 4)},
           "wall_ms": {"min": round(min(walls), 3), "median": round(float(np.median(walls)), 3)},
           "floor_ms": round(floor_ms, 4), "ratio_to_floor": round(med / floor_ms, 1) if floor_ms else None,
           "share_of_graph_build": round(med / GRAPH_BUILD_MS, 4)}
    g.free()
    if a.scipy_cells > 0:
        import scipy.sparse as sp
        g2, G2, _ = clustered_graph(ctx, a, a.scipy_cells)
        labels = np.zeros(a.scipy_cells, dtype=np.uint32)
        F.check(lib.srx_graph_labels_fetch(g2.handle, F.ptr(labels)), ctx.handle)
        t0 = time.perf_counter()
        indptr, indices, _ = g2.fetch(F.GRAPH_DISTANCES)
        fetch_ms = (time.perf_counter() - t0) * 1e3
        i2 = F.PagaInfo()
        E_dev = np.zeros((G2, G2), dtype=np.uint64)
        t = F.PagaTables(None, None, F.ptr(E_dev), None, None, None)
        F.check(lib.srx_paga(g2.handle, None, G2, C.byref(t), C.byref(i2)), ctx.handle)
        F.check(lib.srx_paga(g2.handle, None, G2, C.byref(t), C.byref(i2)), ctx.handle)
        host = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            A = sp.csr_matrix((np.ones(indices.size, dtype=np.int64), indices, indptr.astype(np.int64)), shape=(a.scipy_cells,) * 2)
            L = sp.csr_matrix((np.ones(a.scipy_cells, dtype=np.int64), (np.arange(a.scipy_cells), labels)), shape=(a.scipy_cells, G2))
            E = (L.T @ A @ L).toarray()
            host.append((time.perf_counter() - t0) * 1e3)
        out["scipy"] = {"cells": a.scipy_cells, "n_groups": G2, "host_count_ms": round(float(np.median(host)), 2),
                        "fetch_ms": round(fetch_ms, 2), "device_ms": round(i2.ms, 4), "equal": bool(np.array_equal(E.astype(np.uint64), E_dev))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Times of the UMAP layout (srx_umap) on the c3-shaped synthetic matrix: pipeline -> neighbours (k) -> layout from the PCA
start, everything resident.  Reported (min / median of --runs calls after --warmup): info.ms of a full call of --epochs epochs,
of a call stopped after one epoch (the fixed part: start, w_max, the active count, the read-backs), the time per epoch from
their difference, the sampled (entry, epoch) pairs and the rate of the gathers they make (16 bytes per attraction or negative
sample at 2 components).  Report only: prints one JSON document.

    python scripts/umap_time.py [--cells 1300000 --genes 28000 --density 0.03 --k 15 --epochs 200 --runs 5 --warmup 1]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

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
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--components", type=int, default=2)
    ap.add_argument("--rate", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
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
    F.check(lib.srx_neighbors_result(m.handle, C.byref(F.KnnOpts(a.k, 0, 0, 0)), None, C.byref(graph)), ctx.handle)
    gi = F.GraphInfo()
    F.check(lib.srx_graph_info_get(graph, C.byref(gi)), ctx.handle)
    ab_a, ab_b = C.c_double(), C.c_double()
    F.check(lib.srx_umap_fit_ab(1.0, 0.5, C.byref(ab_a), C.byref(ab_b)), None)

    def call(stop_after):
        o = F.UmapOpts(ab_a.value, ab_b.value, 0.5, 1.0, 1.0, 1.0, 0, a.epochs, stop_after, a.components, a.rate, F.UMAP_INIT_PCA, 0)
        ms, info = [], F.UmapInfo()
        for i in range(a.warmup + a.runs):
            F.check(lib.srx_umap(graph, m.handle, C.byref(o), None, None, C.byref(info)), ctx.handle)
            if i >= a.warmup:
                ms.append(info.ms)
        return ms, info

    full, info = call(0)
    one, info1 = call(1)
    per_epoch = (min(full) - min(one)) / max(a.epochs - 1, 1)
    terms = info.samples * (1 + a.rate) - info.negatives_skipped
    out = {"cells": a.cells, "k": a.k, "nnz_connectivities": int(gi.nnz_connectivities), "max_row_nnz": int(gi.max_row_nnz),
           "components": a.components, "negative_sample_rate": a.rate, "epochs": a.epochs, "lanes_per_vertex": F.UMAP_GROUP,
           "entries_active": int(info.entries_active), "samples": int(info.samples), "negatives": int(info.negatives),
           "negatives_skipped": int(info.negatives_skipped), "call_ms": min_med(full), "one_epoch_call_ms": min_med(one),
           "ms_per_epoch": round(per_epoch, 4), "samples_per_epoch": round(info.samples / a.epochs),
           "gathered_positions_per_epoch": round(terms / a.epochs),
           "gather_GB_per_s": round(terms / a.epochs * 8 * a.components / (per_epoch * 1e-3) / 1e9, 1) if per_epoch > 0 else None,
           "csr_stream_GB_per_s": round(gi.nnz_connectivities * 12 / (per_epoch * 1e-3) / 1e9, 1) if per_epoch > 0 else None}
    print(json.dumps(out, indent=1))
    lib.srx_graph_free(graph)


if __name__ == "__main__":
    main()

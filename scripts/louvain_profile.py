"""Time of Louvain clustering over the resident neighbour graph (srx_neighbors_result after a pipeline step, then srx_louvain
on the handle): info.ms (hipEvent time of the device work) and wall time, warm, median of --reps calls; levels, sweeps, moves,
communities and Q; the share of the k-NN search's device time of the same graph build.

    python scripts/louvain_profile.py [--cells 1300000] [--genes 28000] [--density 0.03] [--n-hvg 2000] [--n-pc 50] [--k 15]
                                      [--reps 3] [--resolution 1.0]

Prints one JSON line.  The matrix is srx_synth's (the bench's c3 shape by default), f32 storage.  Per-kernel times come from
running this script under `rocprofv3 --kernel-trace --stats` (profiles/louvain.md)."""
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
from singlerust_amd.memory.processing.louvain import _info_dict     # noqa: E402
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
    ap.add_argument("--resolution", type=float, default=1.0)
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
    gh = C.c_void_p()
    ctx.prof_enable(1 << F.K_KNN)
    F.check(lib.srx_neighbors_result(ad.x().handle, C.byref(kopts), None, C.byref(gh)), ctx.handle)
    knn_ms = ctx.prof_get(F.K_KNN)[0]
    ctx.prof_enable(0)
    g = Graph(ctx, gh)
    lopts = F.LouvainOpts(a.resolution, 0.0, 0, 0)
    info = F.LouvainInfo()

    def once():
        t0 = time.perf_counter()
        F.check(lib.srx_louvain(g.handle, C.byref(lopts), None, C.byref(info)), ctx.handle)
        return (time.perf_counter() - t0) * 1e3

    once()                                                           # warm: scratch allocation, code-object load
    walls, dev = [], []
    for _ in range(a.reps):
        walls.append(once())
        dev.append(info.ms)
    med = float(np.median(dev))
    out = {"cells": a.cells, "k": a.k, "graph": g.info(), "louvain": _info_dict(info),
           "louvain_ms": {"min": round(min(dev), 2), "median": round(med, 2)},
           "wall_ms": {"min": round(min(walls), 2), "median": round(float(np.median(walls)), 2)},
           "knn_class_ms": round(knn_ms, 2), "louvain_share_of_knn": round(med / knn_ms, 4) if knn_ms else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

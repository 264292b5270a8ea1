#!/usr/bin/env python
"""Times of the doublet chain (srx_doublets_result) on the c3-shaped synthetic matrix: raw counts and a clone that went through
the pipeline (2000 HVGs, 50 components), then simulate -> project -> neighbours -> scores with r = --ratio and k = --k, everything
resident.  Reported (min / median of --runs calls after --warmup): the call's wall time and the four hipEvent stage times of its
info; the bytes the two simulation passes must move (count: the column indices of both parents of every synthetic row and one
int64 per row; fill: indices and values of both parents and of the union) with the rate they give over ms_simulate — which
also holds the parents' kernel, the scan of the row offsets and the allocation of the synthetic matrix — as a share of the
8.0 TB/s HBM peak; the wall time of srx_doublets_simulate alone.  --scipy adds the host's `X[a] + X[b]` (scipy, one thread)
on the same matrix made by the host generator with the same parents.  Report only: prints one JSON document.

    python scripts/doublets_time.py [--cells 1300000 --genes 28000 --density 0.03 --ratio 2 --k 15 --runs 3 --warmup 1 --scipy]
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

HBM_PEAK = 8.0e12


def min_med(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_300_000)
    ap.add_argument("--genes", type=int, default=28_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=3003)
    ap.add_argument("--ratio", type=float, default=2.0)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scipy", action="store_true")
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
    counts = sr.DeviceCsr(ctx, h)
    fitted = counts.clone()
    fitted.prepare()
    popts, res = F.PcaOpts(50, -1, -1, -1, 0, 0, 0, 0.0, 12345), F.PipelineResult()
    F.check(lib.srx_pipeline(fitted.handle, 1e4, 2000, C.byref(popts), C.byref(res)), ctx.handle)

    o = F.DoubletOpts(a.ratio, 0.0, 0.0, 1e4, 0.0, 0, a.k, 0, F.BACKED_NORMALIZE | F.BACKED_LOG1P, 0)
    wall, stages, info = [], {s: [] for s in ("ms_simulate", "ms_project", "ms_knn", "ms_score")}, F.DoubletInfo()
    d = C.c_void_p()
    for i in range(a.warmup + a.runs):
        if d:
            lib.srx_doublets_free(d)
        d = C.c_void_p()
        ctx.synchronize()
        t0 = time.perf_counter()
        F.check(lib.srx_doublets_result(fitted.handle, counts.handle, C.byref(o), C.byref(d), C.byref(info)), ctx.handle)
        if i >= a.warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            for s in stages:
                stages[s].append(getattr(info, s))
    n_sim = int(info.n_sim)
    parents = np.zeros((n_sim, 2), dtype=np.uint64)
    F.check(lib.srx_doublets_fetch(d, F.DOUBLETS_PARENTS, F.ptr(parents)), ctx.handle)
    lib.srx_doublets_free(d)
    lens = np.zeros(a.cells, dtype=np.uint32)
    F.check(lib.srx_compute_number(counts.handle, 0, F.ptr(lens)), ctx.handle)
    both = int(lens[parents.astype(np.int64)].astype(np.int64).sum())          # entries of both parents over all synthetic rows
    nnz_sim = int(info.nnz_sim)
    count_bytes = both * 4 + n_sim * 8
    fill_bytes = both * 8 + nnz_sim * 8                                         # f32 storage: 4 B index + 4 B value
    sim_ms = min(stages["ms_simulate"])
    sim_wall = []
    for i in range(a.warmup + a.runs):
        s = C.c_void_p()
        ctx.synchronize()
        t0 = time.perf_counter()
        F.check(lib.srx_doublets_simulate(counts.handle, n_sim, 0, None, C.byref(s), None), ctx.handle)
        if i >= a.warmup:
            sim_wall.append((time.perf_counter() - t0) * 1e3)
        lib.srx_matrix_free(s)
    out = {"cells": a.cells, "genes": a.genes, "density": a.density, "ratio": a.ratio, "k": int(info.k), "k_adj": int(info.k_adj),
           "n_sim": n_sim, "nnz_counts": int(counts.info().nnz), "nnz_sim": nnz_sim, "d": int(info.d),
           "threshold": info.threshold, "threshold_found": int(info.threshold_found), "smooth_rounds": int(info.smooth_rounds),
           "rows_recomputed": int(info.rows_recomputed), "call_wall_ms": min_med(wall),
           **{s: min_med(v) for s, v in stages.items()},
           "simulate_alone_wall_ms": min_med(sim_wall), "count_pass_bytes": count_bytes, "fill_pass_bytes": fill_bytes,
           "simulate_GBps": round((count_bytes + fill_bytes) / sim_ms / 1e6, 1),
           "simulate_share_of_hbm_peak": round((count_bytes + fill_bytes) / (sim_ms * 1e-3) / HBM_PEAK, 4)}
    if a.scipy:
        import scipy.sparse as sp
        indptr = np.zeros(a.cells + 1, dtype=np.uint64)
        F.check(lib.srx_synth_indptr(C.byref(p), 0, a.cells, F.ptr(indptr)))
        nnz = int(indptr[-1])
        idx, val = np.zeros(nnz, dtype=np.uint64), np.zeros(nnz, dtype=np.float32)
        F.check(lib.srx_synth_fill_host(C.byref(p), 0, a.cells, F.ptr(indptr), F.ptr(idx), F.ptr(val)))
        x = sp.csr_matrix((val, idx.astype(np.int32), indptr.astype(np.int64)), shape=(a.cells, a.genes))
        pa, pb = parents[:, 0].astype(np.int64), parents[:, 1].astype(np.int64)
        t0 = time.perf_counter()
        y = x[pa] + x[pb]
        y.sort_indices()
        out["scipy_host_wall_s"] = round(time.perf_counter() - t0, 3)
        out["scipy_nnz"] = int(y.nnz)                # (scipy drops sums that are 0.0; counts are positive, so the same pattern)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

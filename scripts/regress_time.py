#!/usr/bin/env python
"""Times of regress out -> scale -> clip -> PCA (srx_pca_regress) on a synthetic matrix of a benchmark shape, f32 storage, after
srx_normalize_log1p_inplace, on the genes of srx_select_hvg, with two covariates (the cells' total counts and a hashed one),
max_value 10: the five ms_* fields of srx_regress_info, beside srx_pca_pearson on the raw counts of the same shape in the same
session, the calls alternating (the yardstick: it runs the same SYRK and score kernels over the same number of chunks).  With
--host (up to --host-rows cells) also the host route the call replaces: the dense block to the host, then numpy in f64 (normal
equations, scale, clip, covariance, np.linalg.eigh).  That route is numpy, not scanpy / statsmodels, which are not installed here.

    python scripts/regress_time.py --config c2 --host        # JSON on stdout
    python scripts/regress_time.py --config c3
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"c2": (100_000, 20_000, 0.05, 2002), "c3": (1_300_000, 28_000, 0.03, 3003)}


def hashed(n, seed=7):
    """100 (splitmix64(seed 2^32 + i) >> 11) / 2^53, vectorised."""
    with np.errstate(over="ignore"):
        x = (np.uint64(seed) << np.uint64(32)) + np.arange(n, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return 100.0 * (x >> np.uint64(11)).astype(np.float64) / 2.0 ** 53


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--cells", type=int, default=0)
    ap.add_argument("--top", type=int, default=2000)
    ap.add_argument("--n-pc", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--max-value", type=float, default=10.0)
    ap.add_argument("--chunk-cells", type=int, default=0)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-rows", type=int, default=100_000)
    a = ap.parse_args()
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    cells, genes, density, seed = CONFIGS[a.config]
    cells = a.cells or cells
    lib = F.lib()
    ctx = sr.Context.default()
    p = F.SynthParams()
    lib.srx_synth_defaults(C.byref(p), seed, cells, genes, density)
    h = C.c_void_p()
    F.check(lib.srx_synth_generate(ctx.handle, C.byref(p), 0, cells, F.F32, F.STORE_F32, C.byref(h)), ctx.handle)
    raw = sr.DeviceCsr(ctx, h)
    raw.prepare()
    m = raw.clone()
    totals = np.zeros(cells)
    F.check(lib.srx_normalize_log1p_inplace(m.handle, 1e4, F.ptr(totals)), ctx.handle)
    cov = np.ascontiguousarray(np.stack([totals, hashed(cells)], axis=1))
    idx, n_out = np.zeros(a.top, np.uint64), C.c_uint64(0)
    F.check(lib.srx_select_hvg(m.handle, a.top, F.ptr(idx), C.byref(n_out)), ctx.handle)
    sel = idx[:n_out.value].copy()
    F.check(lib.srx_select_hvg_pearson(raw.handle, a.top, None, F.ptr(idx), C.byref(n_out), None, None), ctx.handle)
    sel_p = idx[:n_out.value].copy()
    k = int(sel.size)
    pca = F.PcaOpts(a.n_pc, -1, 0, -1, 0, 0, 0, 0.0, 0)
    o = F.RegressOpts(1, 0, a.max_value, a.chunk_cells, pca)
    op = F.PearsonPcaOpts(F.PearsonOpts(0.0, 0.0), F.PEARSON_TOTALS_SELECTED, 1, a.chunk_cells, pca)
    info, pinfo, rows, prow = F.RegressInfo(), F.PearsonPcaInfo(), [], []
    evr = np.zeros(a.n_pc)
    for it in range(1 + a.runs):                         # the first calls allocate the scratch buffers and capture the solver's graphs
        t0 = time.perf_counter()
        rc = lib.srx_pca_regress(m.handle, F.ptr(sel), k, F.ptr(cov), 2, C.byref(o), None, None, F.ptr(evr), None, None, C.byref(info))
        wall = (time.perf_counter() - t0) * 1e3
        if rc not in (F.OK, F.E_NOCONV):
            F.check(rc, ctx.handle)
        t0 = time.perf_counter()
        rcp = lib.srx_pca_pearson(raw.handle, F.ptr(sel_p), int(sel_p.size), C.byref(op), None, None, None, None, C.byref(pinfo))
        pwall = (time.perf_counter() - t0) * 1e3
        if rcp not in (F.OK, F.E_NOCONV):
            F.check(rcp, ctx.handle)
        if it:
            rows.append((info.ms_fit, info.ms_scale, info.ms_gram, info.ms_solve, info.ms_scores, wall))
            prow.append((pinfo.ms_gram, pinfo.ms_solve, pinfo.ms_scores, pwall))
    rows, prow = np.array(rows), np.array(prow)
    med, pmed = np.median(rows, axis=0), np.median(prow, axis=0)
    names = ("ms_fit", "ms_scale", "ms_gram", "ms_solve", "ms_scores", "ms_wall")
    out = {"config": a.config, "cells": cells, "genes": genes, "k": k, "n_cov": 2, "max_value": a.max_value, "n_pc": a.n_pc,
           "converged": rc == F.OK, "residual": info.pca.residual, "sweeps": int(info.pca.n_iter), "evr_first": float(evr[0]),
           "n_clipped": int(info.n_clipped), "n_constant_genes": int(info.n_constant_genes), "min_pivot": info.min_pivot,
           "n_chunks": int(info.n_chunks), "chunk_cells": int(info.chunk_cells),
           **{n: float(v) for n, v in zip(names, med)},
           "spread": {n: [float(rows[:, i].min()), float(rows[:, i].max())] for i, n in enumerate(names)},
           "pearson": {"k": int(sel_p.size), "converged": rcp == F.OK, "n_chunks": int(pinfo.n_chunks), "ms_gram": float(pmed[0]),
                       "ms_solve": float(pmed[1]), "ms_scores": float(pmed[2]), "ms_wall": float(pmed[3]),
                       "spread": {n: [float(prow[:, i].min()), float(prow[:, i].max())]
                                  for i, n in enumerate(("ms_gram", "ms_solve", "ms_scores", "ms_wall"))}}}
    if a.host and cells <= a.host_rows:
        t0 = time.perf_counter()
        X = np.zeros((cells, k))
        oo = F.RegressOpts(0, 0, 0.0, 0, pca)
        F.check(lib.srx_regress_residuals(m.handle, F.ptr(sel), k, None, 0, C.byref(oo), F.ptr(X), None), ctx.handle)   # x - xbar
        t1 = time.perf_counter()
        ct = cov - cov.mean(axis=0)
        beta = np.linalg.solve(ct.T @ ct, ct.T @ X)
        r = X - ct @ beta
        s = np.sqrt((r * r).sum(axis=0) / (cells - 1))
        s[s == 0] = 1.0
        Z = np.clip(r / s, -a.max_value, a.max_value)
        t2 = time.perf_counter()
        mean = Z.mean(axis=0)
        Cm = (Z.T @ Z - cells * np.outer(mean, mean)) / (cells - 1)
        t3 = time.perf_counter()
        w, V = np.linalg.eigh(Cm)
        t4 = time.perf_counter()
        S = (Z - mean) @ V[:, ::-1][:, :a.n_pc]
        t5 = time.perf_counter()
        out["host_route"] = {"note": "numpy f64 with %s threads; not scanpy / statsmodels" % os.environ.get("OMP_NUM_THREADS", "?"),
                             "s_block_to_host": t1 - t0, "s_regress_scale_clip": t2 - t1, "s_covariance": t3 - t2, "s_eigh": t4 - t3,
                             "s_scores": t5 - t4, "s_total": t5 - t0, "evr_first": float(w[-1] / np.trace(Cm)), "scores_shape": list(S.shape)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Times of the residual PCA (srx_pca_pearson) on a synthetic raw-count matrix of a benchmark shape: the Gram pass (chunks +
f64 SYRK), the eigen-solve and the score pass, the SYRK's achieved f64 rate beside the rate of a bare v_mfma_f64_16x16x4 loop
measured in the same session (bench_micro/mfma_f64_peak, if it has been built), the bytes the SYRK reads per chunk, and — up to
--host-rows cells — the host route the call replaces: srx_pearson_residuals to the host, the covariance and np.linalg.eigh.
Not compared: scanpy (not installed here) and sklearn's randomized solver.

    python scripts/pearson_pca_time.py --config c2 --host        # JSON on stdout
    python scripts/pearson_pca_time.py --config c3
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"c2": (100_000, 20_000, 0.05, 2002), "c3": (1_300_000, 28_000, 0.03, 3003)}
TILE = 64


def mfma_ceiling():
    exe = os.path.join(ROOT, "bench_micro", "mfma_f64_peak")
    if not os.path.exists(exe):
        return None
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--cells", type=int, default=0)
    ap.add_argument("--top", type=int, default=2000)
    ap.add_argument("--n-pc", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
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
    m = sr.DeviceCsr(ctx, h)
    m.prepare()
    idx, n_out = np.zeros(a.top, np.uint64), C.c_uint64(0)
    F.check(lib.srx_select_hvg_pearson(m.handle, a.top, None, F.ptr(idx), C.byref(n_out), None, None), ctx.handle)
    sel = idx[:n_out.value].copy()
    k = int(sel.size)
    pca = F.PcaOpts(a.n_pc, -1, 0, -1, 0, 0, 0, 0.0, 0)
    o = F.PearsonPcaOpts(F.PearsonOpts(0.0, 0.0), F.PEARSON_TOTALS_SELECTED, 1, a.chunk_cells, pca)
    info, rows = F.PearsonPcaInfo(), []
    evr = np.zeros(a.n_pc)
    for it in range(1 + a.runs):                         # the first call allocates the scratch buffers and captures the solver's graphs
        t0 = time.perf_counter()
        rc = lib.srx_pca_pearson(m.handle, F.ptr(sel), k, C.byref(o), None, None, F.ptr(evr), None, C.byref(info))
        wall = (time.perf_counter() - t0) * 1e3
        if rc not in (F.OK, F.E_NOCONV):
            F.check(rc, ctx.handle)
        if it:
            rows.append((info.ms_gram, info.ms_solve, info.ms_scores, wall))
    med = np.median(np.array(rows), axis=0)
    n_t = (k + TILE - 1) // TILE
    pairs = n_t * (n_t + 1) // 2
    useful = float(cells) * k * (k + 1)                   # 2 flops per multiply-add of the upper triangle
    executed = float(cells) * pairs * TILE * TILE * 2.0   # what the tiles issue (whole diagonal tiles, padded columns)
    chunk_rows = int(info.chunk_cells)
    out = {"config": a.config, "cells": cells, "genes": genes, "k": k, "n_pc": a.n_pc, "converged": rc == F.OK,
           "residual": info.pca.residual, "sweeps": int(info.pca.n_iter), "evr_first": float(evr[0]),
           "ms_gram": float(med[0]), "ms_solve": float(med[1]), "ms_scores": float(med[2]), "ms_wall": float(med[3]),
           "n_chunks": int(info.n_chunks), "chunk_cells": chunk_rows, "chunk_bytes_written": int(info.chunk_bytes),
           "syrk_bytes_read_per_chunk": int(pairs * 2 * chunk_rows * TILE * 8),
           "syrk_useful_tflops_incl_chunk_generation": useful / (med[0] * 1e-3) / 1e12,
           "syrk_executed_tflops_incl_chunk_generation": executed / (med[0] * 1e-3) / 1e12,
           "scores_tflops_incl_chunk_generation": 2.0 * cells * k * 64 / (med[2] * 1e-3) / 1e12,
           "mfma_loop": mfma_ceiling()}
    if a.host and cells <= a.host_rows:
        t0 = time.perf_counter()
        Z = np.zeros((cells, k))
        po = F.PearsonOpts(0.0, 0.0)
        F.check(lib.srx_pearson_residuals(m.handle, F.ptr(sel), k, C.byref(po), F.ptr(Z), None), ctx.handle)
        t1 = time.perf_counter()
        mean = Z.mean(axis=0)
        Cm = (Z.T @ Z - cells * np.outer(mean, mean)) / (cells - 1)
        t2 = time.perf_counter()
        w, V = np.linalg.eigh(Cm)
        t3 = time.perf_counter()
        S = (Z - mean) @ V[:, ::-1][:, :a.n_pc]
        t4 = time.perf_counter()
        out["host_route"] = {"note": "totals = all (srx_pearson_residuals), numpy with %d threads" % (os.cpu_count() or 0),
                             "s_residuals_to_host": t1 - t0, "s_covariance": t2 - t1, "s_eigh": t3 - t2, "s_scores": t4 - t3,
                             "s_total": t4 - t0, "scores_shape": list(S.shape)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Times of the Pearson-residual gene selection (srx_select_hvg_pearson) on the c3-shaped synthetic matrix (raw counts), the
dense pass's pair rate beside its instruction count, and for context a chunked numpy / scipy evaluation of the same definition
on the host over the first --host-rows cells (scanpy's method: dense chunks of 1000 rows; NOT scanpy itself, which is not
installed here).  Also: whether the device's residuals equal numpy's own f64 evaluation bit for bit on a small count matrix.

    python scripts/pearson_profile.py                       # JSON on stdout
    python scripts/pearson_profile.py --md profiles/pearson_measured.md
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# f64 vector instructions per pair in the main loop of k_pr_dense (hipcc -S: 272 in the block that evaluates 8 pairs), and the
# FMA-rate peak they are set beside: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz
F64_INSTR_PER_PAIR = 34
PEAK_F64_LANE_OPS = 256 * 4 * 16 * 2.4e9


def host_chunked(X, theta=100.0, chunk=1000):
    """(v, seconds): the definition of include/srx.h over a scipy CSR matrix in dense chunks of rows, f64."""
    n, G = X.shape
    t0 = time.perf_counter()
    r = np.asarray(X.sum(axis=1)).ravel()
    g = np.asarray(X.sum(axis=0)).ravel()
    T = r.sum()
    clip = np.sqrt(n)
    s1, s2 = np.zeros(G), np.zeros(G)
    for a in range(0, n, chunk):
        D = X[a:a + chunk].toarray()
        mu = np.outer(r[a:a + chunk], g) / T
        with np.errstate(invalid="ignore", divide="ignore"):
            z = (D - mu) / np.sqrt(mu + mu * mu / theta)
        z = np.where(mu > 0, np.clip(z, -clip, clip), 0.0)
        s1 += z.sum(axis=0)
        s2 += (z * z).sum(axis=0)
    v = s2 / n - (s1 / n) ** 2
    return v, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_300_000)
    ap.add_argument("--genes", type=int, default=28_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=3003)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--top", type=int, default=2000)
    ap.add_argument("--host-rows", type=int, default=100_000)
    ap.add_argument("--md", default=None)
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
    nnz = int(m.info().nnz)
    idx, var, n_out = np.zeros(a.top, np.uint64), np.zeros(a.genes), C.c_uint64(0)
    info, rows = F.PearsonInfo(), []
    for it in range(a.warmup + a.runs):
        t0 = time.perf_counter()
        F.check(lib.srx_select_hvg_pearson(m.handle, a.top, None, F.ptr(idx), C.byref(n_out), F.ptr(var), C.byref(info)), ctx.handle)
        wall = (time.perf_counter() - t0) * 1e3
        if it >= a.warmup:
            rows.append((info.ms_dense, info.ms_sparse, info.ms_rank, wall))
    med = np.median(np.array(rows), axis=0)
    pairs = float(a.cells) * float(a.genes)
    rate = pairs / (med[0] * 1e-3)
    out = {"cells": a.cells, "genes": a.genes, "nnz": nnz, "storage": "f32", "runs": a.runs, "selected": int(n_out.value),
           "n_expressed": int(info.n_expressed), "n_empty_cells": int(info.n_empty_cells), "theta": info.theta, "clip": info.clip,
           "sum_quantum": info.sum_quantum, "sq_quantum": info.sq_quantum,
           "ms_dense": round(float(med[0]), 3), "ms_sparse": round(float(med[1]), 3), "ms_rank": round(float(med[2]), 3),
           "ms_call_wall": round(float(med[3]), 3), "dense_pairs_per_s": rate, "dense_f64_instr_per_pair": F64_INSTR_PER_PAIR,
           "dense_share_of_f64_issue_rate": round(rate * F64_INSTR_PER_PAIR / PEAK_F64_LANE_OPS, 3)}

    # the host, for context: the first host_rows cells of the same matrix as a matrix of their own
    import scipy.sparse as sp
    nh = min(a.host_rows, a.cells)
    ip = np.zeros(nh + 1, np.uint64)
    lib.srx_synth_indptr(C.byref(p), 0, nh, F.ptr(ip))
    hidx, hval = np.zeros(int(ip[-1]), np.uint64), np.zeros(int(ip[-1]), np.float32)
    lib.srx_synth_fill_host(C.byref(p), 0, nh, F.ptr(ip), F.ptr(hidx), F.ptr(hval))
    X = sp.csr_matrix((hval.astype(np.float64), hidx.astype(np.int64), ip.astype(np.int64)), shape=(nh, a.genes))
    v_host, sec = host_chunked(X)
    sub = sr.DeviceCsr.upload(ctx, nh, a.genes, ip, hidx, hval, store=F.STORE_F32)
    v_dev, i2 = np.zeros(a.genes), F.PearsonInfo()
    t0 = time.perf_counter()
    F.check(lib.srx_pearson_gene_variance(sub.handle, None, F.ptr(v_dev), C.byref(i2)), ctx.handle)
    dev_ms = (time.perf_counter() - t0) * 1e3
    out["host_numpy_chunked"] = {"rows": nh, "seconds": round(sec, 2), "device_ms_same_rows_first_call": round(dev_ms, 2),
                                 "max_abs_variance_difference": float(np.max(np.abs(v_dev - v_host))),
                                 "note": "1000-row dense chunks in numpy on the host CPUs: scanpy's method, not scanpy itself"}

    # are the device's residuals numpy's f64 bits?
    rng = np.random.default_rng(7)
    D = rng.poisson(rng.gamma(0.5, 2.0, size=(2000, 500))).astype(np.float64)
    S = sp.csr_matrix(D)
    small = sr.DeviceCsr.upload(ctx, 2000, 500, S.indptr.astype(np.uint64), S.indices.astype(np.uint64), S.data, store=F.STORE_F64)
    genes, z = np.arange(500, dtype=np.uint64), np.zeros((2000, 500))
    F.check(lib.srx_pearson_residuals(small.handle, F.ptr(genes), 500, None, F.ptr(z), None), ctx.handle)
    r, g = D.sum(axis=1), D.sum(axis=0)
    mu = np.outer(r, g) / r.sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        zn = np.where(mu > 0, np.clip((D - mu) / np.sqrt(mu + mu * mu / 100.0), -np.sqrt(2000.0), np.sqrt(2000.0)), 0.0)
    out["elements_vs_numpy_f64"] = {"shape": [2000, 500], "differing": int((z != zn).sum()), "of": int(z.size)}
    print(json.dumps(out, indent=1))
    if a.md:
        with open(a.md, "w") as f:
            f.write("```json\n" + json.dumps(out, indent=1) + "\n```\n")


if __name__ == "__main__":
    main()

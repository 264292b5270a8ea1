#!/usr/bin/env python
"""Stage times of the Seurat v3 gene selection (srx_select_hvg_seurat_v3) on the c3-shaped synthetic matrix (raw counts) at
several batch counts, beside srx_group_moments on the same labels in the same run (the unclipped walk is the yardstick of
the clipped one: the same walk plus one table read), and for context the numpy restatement of the definition
(tests/hvg_seurat_ref.py) on the host over the first --host-rows cells as one batch.  NOT scanpy or skmisc, which are not
installed here.

    python scripts/seurat_profile.py                       # JSON on stdout
    python scripts/seurat_profile.py --md profiles/hvg_seurat_measured.md
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def hashed_batches(n, k):
    i = np.arange(n, dtype=np.uint64)
    return (((i * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(k)).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_300_000)
    ap.add_argument("--genes", type=int, default=28_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=3003)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--top", type=int, default=2000)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
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
    out = {"cells": a.cells, "genes": a.genes, "nnz": int(m.info().nnz), "storage": "f32", "runs": a.runs, "n_top": a.top, "by_batches": {}}
    idx, n_out = np.zeros(a.top, np.uint64), C.c_uint64(0)
    for nb in a.batches:
        labels = hashed_batches(a.cells, nb)
        info, rows, gm = F.SeuratV3Info(), [], []
        for it in range(a.warmup + a.runs):
            t0 = time.perf_counter()
            F.check(lib.srx_select_hvg_seurat_v3(m.handle, a.top, F.ptr(labels), nb, None, F.ptr(idx), C.byref(n_out), None, C.byref(info)), ctx.handle)
            wall = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            F.check(lib.srx_group_moments(m.handle, F.ptr(labels), nb, None, None, None, None), ctx.handle)
            wall_gm = (time.perf_counter() - t0) * 1e3
            if it >= a.warmup:
                rows.append((info.ms_moments, info.ms_loess, info.ms_clip, info.ms_rank, wall))
                gm.append(wall_gm)
        med = np.median(np.array(rows), axis=0)
        out["by_batches"][str(nb)] = {
            "ms_moments": round(float(med[0]), 3), "ms_loess": round(float(med[1]), 3), "ms_clip": round(float(med[2]), 3),
            "ms_rank": round(float(med[3]), 3), "ms_call_wall": round(float(med[4]), 3),
            "ms_group_moments_wall": round(float(np.median(gm)), 3), "clip_over_moments": round(float(med[2] / med[0]), 3),
            "min_batch_cells": int(info.min_batch_cells), "selected": int(n_out.value),
            "note": "ms_moments: value scan, label sort, walk, count walk, totals, per-(batch, gene) statistics; ms_clip: clip table, "
                    "clipped walk (no count walk), nv; ms_group_moments_wall: the whole srx_group_moments call on the host clock"}

    # the host, for context: the numpy restatement on the first host_rows cells, one batch
    import scipy.sparse as sp
    import hvg_seurat_ref as R
    nh = min(a.host_rows, a.cells)
    if nh:
        ip = np.zeros(nh + 1, np.uint64)
        lib.srx_synth_indptr(C.byref(p), 0, nh, F.ptr(ip))
        hidx, hval = np.zeros(int(ip[-1]), np.uint64), np.zeros(int(ip[-1]), np.float32)
        lib.srx_synth_fill_host(C.byref(p), 0, nh, F.ptr(ip), F.ptr(hidx), F.ptr(hval))
        X = sp.csr_matrix((hval.astype(np.float64), hidx.astype(np.int64), ip.astype(np.int64)), shape=(nh, a.genes))
        t0 = time.perf_counter()
        ref = R.run(X, None, 1, a.top)
        sec = time.perf_counter() - t0
        sub = sr.DeviceCsr.upload(ctx, nh, a.genes, ip, hidx, hval, store=F.STORE_F32)
        sel, i2 = np.zeros(a.top, np.uint64), F.SeuratV3Info()
        F.check(lib.srx_select_hvg_seurat_v3(sub.handle, a.top, None, 1, None, F.ptr(sel), C.byref(n_out), None, C.byref(i2)), ctx.handle)
        t0 = time.perf_counter()
        F.check(lib.srx_select_hvg_seurat_v3(sub.handle, a.top, None, 1, None, F.ptr(sel), C.byref(n_out), None, C.byref(i2)), ctx.handle)
        dev_ms = (time.perf_counter() - t0) * 1e3
        out["host_numpy"] = {"rows": nh, "seconds": round(sec, 2), "device_ms_same_rows": round(dev_ms, 2),
                             "selected_in_common": int(np.intersect1d(sel[:int(n_out.value)], ref["selected"]).size), "of": a.top,
                             "note": "tests/hvg_seurat_ref.py (numpy, one python loop over the fit points) on the host CPUs; not scanpy"}
    print(json.dumps(out, indent=1))
    if a.md:
        with open(a.md, "w") as f:
            f.write("```json\n" + json.dumps(out, indent=1) + "\n```\n")


if __name__ == "__main__":
    main()

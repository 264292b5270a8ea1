#!/usr/bin/env python
"""Times of the diffusion map (srx_diffmap) on the c3-shaped synthetic matrix: pipeline -> neighbours (k) -> eigenpairs of the
transition operator, everything resident.  Reported (min / median of --runs calls after --warmup): info.ms, the operator
products, restarts and breakdowns at the defaults, one srx_dpt, and with --host-eigsh the time of
scipy.sparse.linalg.eigsh(T, k, which="LM") on the downloaded operator (scanpy's own call) with its product count.
Report only: prints one JSON document.

    python scripts/diffmap_time.py [--cells 1300000 --genes 28000 --density 0.03 --k 15 --comps 15 --runs 3 --warmup 1 --host-eigsh]

Another lane-group width is another build of the library (SRX_DIFFMAP_GROUP is a compile-time constant): link one with
-DSRX_DIFFMAP_GROUP=4|16|32 on diffmap.hip's compile line and pass it with --lib.  The split between the operator product and
the reorthogonalisation is read from the per-kernel totals of a kernel trace of this script:

    rocprofv3 --kernel-trace --stats -d OUT -o dm -- python scripts/diffmap_time.py --runs 1 --warmup 0
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


def min_med(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_300_000)
    ap.add_argument("--genes", type=int, default=28_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=3003)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--comps", type=int, default=0)
    ap.add_argument("--ncv", type=int, default=0)
    ap.add_argument("--tol", type=float, default=0.0)
    ap.add_argument("--max-matvecs", type=int, default=0)
    ap.add_argument("--lib", default="", help="another build of libsrx_hip.so (e.g. one with another SRX_DIFFMAP_GROUP)")
    ap.add_argument("--lanes", type=int, default=0, help="the SRX_DIFFMAP_GROUP of --lib, for the record")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-eigsh", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    if a.lib:
        F.LIB_PATH = os.path.abspath(a.lib)
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
    o = F.DiffmapOpts(a.tol, 0, a.comps, a.ncv, a.max_matvecs, 1)

    def call():
        ms, info = [], F.DiffmapInfo()
        for i in range(a.warmup + a.runs):
            rc = lib.srx_diffmap(graph, C.byref(o), None, None, C.byref(info))
            if rc != F.OK:
                return None, info, lib.srx_last_error(ctx.handle).decode()
            if i >= a.warmup:
                ms.append(info.ms)
        return ms, info, None

    out = {"cells": a.cells, "k": a.k, "nnz_connectivities": int(gi.nnz_connectivities), "max_row_nnz": int(gi.max_row_nnz),
           "lanes_per_row": a.lanes or F.DIFFMAP_GROUP}
    evals = None
    ms, info, err = call()
    out.update({"n_comps": int(info.n_comps), "ncv": int(info.ncv), "matvecs": int(info.matvecs), "restarts": int(info.restarts),
                "breakdowns": int(info.breakdowns), "max_residual": float(info.max_residual), "max_ortho": float(info.max_ortho)})
    if err:
        out["error"] = err
    else:
        out["call_ms"] = min_med(ms)
        out["ms_per_matvec_step"] = round(min(ms) / max(info.matvecs, 1), 4)
        evals = np.zeros(int(info.n_comps))
        F.check(lib.srx_graph_diffmap_fetch(graph, F.ptr(evals), None, None), ctx.handle)
        out["evals"] = [float(x) for x in evals]
        pt = np.zeros(a.cells)
        t0 = time.perf_counter()
        F.check(lib.srx_dpt(graph, 0, 0.0, F.ptr(pt)), ctx.handle)
        out["dpt_call_ms_with_download"] = round((time.perf_counter() - t0) * 1e3, 3)
    if a.host_eigsh and evals is not None:
        import scipy.sparse as sp
        import scipy.sparse.linalg as sla
        t0 = time.perf_counter()
        indptr = np.zeros(a.cells + 1, dtype=np.uint64)
        indices = np.zeros(gi.nnz_connectivities, dtype=np.uint32)
        data = np.zeros(gi.nnz_connectivities, dtype=np.float64)
        F.check(lib.srx_graph_fetch(graph, F.GRAPH_CONNECTIVITIES, F.ptr(indptr), F.ptr(indices), F.ptr(data)), ctx.handle)
        F.check(lib.srx_graph_transitions_fetch(graph, F.ptr(data)), ctx.handle)
        T = sp.csr_matrix((data, indices.astype(np.int32), indptr.astype(np.int64)), shape=(a.cells, a.cells))
        out["host_download_s"] = round(time.perf_counter() - t0, 3)
        count = [0]

        def mv(x):
            count[0] += 1
            return T @ x
        t0 = time.perf_counter()
        w = sla.eigsh(sla.LinearOperator(T.shape, matvec=mv, dtype=np.float64), k=len(evals), which="LM", return_eigenvectors=True)[0]
        out["host_eigsh_s"] = round(time.perf_counter() - t0, 3)
        out["host_eigsh_matvecs"] = count[0]
        out["host_eigsh_max_abs_diff"] = float(np.abs(np.sort(w)[::-1] - evals).max())
        out["host_threads"] = os.environ.get("OMP_NUM_THREADS")
    print(json.dumps(out, indent=1))
    lib.srx_graph_free(graph)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Times and recall of the inverted-file k-NN index (srx_knn_index_result / srx_knn_index_search) on the scores the pipeline
leaves on the device for the c3-shaped synthetic matrix (2000 HVGs, 50 components), beside the exact search
(srx_knn_result) in the same run.  Everything stays resident: the timed calls pass NULL outputs; one more call per setting
fetches the indices for recall@k against the exact list.

Reported per --cells (min / median of --runs warm calls): the build's wall time with its ms_train and ms_assign, the exact
search's wall time, and for every n_probe of --probes the search's wall time, recall@k, rows_certified / rows_rescanned /
rows_exhaustive, pairs and points_scanned.  Prints one JSON document.  Exit status 1 when, at 1 300 000 cells or more, build
plus search at the default n_probe is not faster than the exact search.

    python scripts/knn_ivf_profile.py [--cells 100000 1300000 --k 15 --probes 1 4 16 20 64 --runs 5 --exact-runs 3]
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
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[100_000, 1_300_000])
    ap.add_argument("--genes", type=int, default=28_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=3003)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--probes", type=int, nargs="+", default=[1, 4, 16, 20, 64])
    ap.add_argument("--n-lists", type=int, default=0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--exact-runs", type=int, default=3)
    a = ap.parse_args()
    import numpy as np

    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    lib = F.lib()
    ctx = sr.Context.default()
    out, slower = [], False
    for cells in a.cells:
        p = F.SynthParams()
        lib.srx_synth_defaults(C.byref(p), a.seed, cells, a.genes, a.density)
        h = C.c_void_p()
        F.check(lib.srx_synth_generate(ctx.handle, C.byref(p), 0, cells, F.F32, F.STORE_F32, C.byref(h)), ctx.handle)
        m = sr.DeviceCsr(ctx, h)
        m.prepare()
        popts, res = F.PcaOpts(50, -1, -1, -1, 0, 0, 0, 0.0, 12345), F.PipelineResult()
        F.check(lib.srx_pipeline(m.handle, 1e4, 2000, C.byref(popts), C.byref(res)), ctx.handle)

        ko = F.KnnOpts(a.k, 0, 0, 0)
        exact_idx = np.zeros((cells, a.k), dtype=np.uint32)
        F.check(lib.srx_knn_result(m.handle, C.byref(ko), F.ptr(exact_idx), None, None), ctx.handle)      # warm, and the truth
        exact = []
        for _ in range(a.exact_runs):
            ctx.synchronize()
            t0 = time.perf_counter()
            F.check(lib.srx_knn_result(m.handle, C.byref(ko), None, None, None), ctx.handle)
            ctx.synchronize()
            exact.append((time.perf_counter() - t0) * 1e3)

        io = F.IvfOpts(a.n_lists, 10, 0, 0)
        build, train, assign, info, ix = [], [], [], F.IvfInfo(), C.c_void_p()
        for i in range(a.runs + 1):
            if ix:
                lib.srx_knn_index_free(ix)
            ix = C.c_void_p()
            ctx.synchronize()
            t0 = time.perf_counter()
            F.check(lib.srx_knn_index_result(m.handle, 0, C.byref(io), C.byref(ix)), ctx.handle)
            ctx.synchronize()
            F.check(lib.srx_knn_index_info_get(ix, C.byref(info)), ctx.handle)
            if i:
                build.append((time.perf_counter() - t0) * 1e3)
                train.append(info.ms_train)
                assign.append(info.ms_assign)
        row = {"cells": cells, "k": a.k, "d": int(info.d), "n_lists": int(info.n_lists), "n_train": int(info.n_train),
               "min_list": int(info.min_list), "max_list": int(info.max_list), "empty_lists": int(info.empty_lists),
               "exact_wall_ms": min_med(exact), "build_wall_ms": min_med(build), "ms_train": min_med(train),
               "ms_assign": min_med(assign), "search": []}
        idx = np.zeros((cells, a.k), dtype=np.uint32)
        for n_probe in a.probes:
            if n_probe > info.n_lists:
                continue
            si, wall = F.IvfSearchInfo(), []
            for i in range(a.runs + 1):
                ctx.synchronize()
                t0 = time.perf_counter()
                F.check(lib.srx_knn_index_search(ix, None, 0, C.byref(ko), n_probe, None, None, C.byref(si)), ctx.handle)
                ctx.synchronize()
                if i:
                    wall.append((time.perf_counter() - t0) * 1e3)
            F.check(lib.srx_knn_index_search(ix, None, 0, C.byref(ko), n_probe, F.ptr(idx), None, None), ctx.handle)
            # rows are ascending by distance, not by index: recall through a sorted merge of the two rows
            a_s, b_s = np.sort(idx, axis=1), np.sort(exact_idx, axis=1)
            hits = sum(int((a_s[:, j][:, None] == b_s).any(axis=1).sum()) for j in range(a.k))
            row["search"].append({"n_probe": n_probe, "wall_ms": min_med(wall), "recall": round(hits / (cells * a.k), 5),
                                  "rows_certified": int(si.rows_certified), "rows_rescanned": int(si.rows_rescanned),
                                  "rows_exhaustive": int(si.rows_exhaustive), "pairs": int(si.pairs),
                                  "points_scanned": int(si.points_scanned)})
        lib.srx_knn_index_free(ix)
        dflt = [s for s in row["search"] if s["n_probe"] == min(20, info.n_lists)]
        if dflt:
            row["build_plus_default_search_ms"] = round(row["build_wall_ms"]["median"] + dflt[0]["wall_ms"]["median"], 3)
            if cells >= 1_300_000 and row["build_plus_default_search_ms"] >= row["exact_wall_ms"]["median"]:
                slower = True
        out.append(row)
        m.free()
    print(json.dumps(out, indent=1))
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())

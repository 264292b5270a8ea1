#!/usr/bin/env python
"""Times of the gene-set score (srx_score_genes) and of the sums over gene lists (srx_gene_list_sums) on a synthetic matrix of a
benchmark shape, f32 storage, after srx_normalize_log1p_inplace: a cell-cycle-sized input (two sets of 45 and 55 hashed genes,
default ctrl_size and n_bins), the stages of srx_score_genes_info, the walk alone over the same four lists, 64 lists in one walk
and 65 lists in two, beside srx_compute_sum(m, Row) in the same session on the same handle (the yardstick: it streams the 4-byte
values where the walk streams the 2-byte column indices).  srx_compute_sum is timed as a call (its kernel and the read-back of
n_obs doubles); the kernels alone come from a kernel trace of this script (--trace-hint prints the command).  With --host also a
numpy / scipy evaluation of the same definition on --host-rows cells of the same generator (not scanpy, which is not installed).

    python scripts/score_genes_time.py --config c3 --host --out profiles/score_genes.md
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
M64 = (1 << 64) - 1


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def hashed_genes(G, count, seed):
    return np.array(sorted(sorted(range(G), key=lambda j: mix64(seed * 1000003 + j))[:count]), dtype=np.uint64)


def pack(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    return ptr, np.ascontiguousarray(np.concatenate(lists).astype(np.uint64))


def synth(sr, F, ctx, seed, cells, genes, density):
    lib = F.lib()
    p = F.SynthParams()
    lib.srx_synth_defaults(C.byref(p), seed, cells, genes, density)
    h = C.c_void_p()
    F.check(lib.srx_synth_generate(ctx.handle, C.byref(p), 0, cells, F.F32, F.STORE_F32, C.byref(h)), ctx.handle)
    m = sr.DeviceCsr(ctx, h)
    m.prepare()
    F.check(lib.srx_normalize_log1p_inplace(m.handle, 1e4, None), ctx.handle)
    return m


def median_of(fn, runs):
    rows = []
    for it in range(1 + runs):                               # the first call allocates the scratch buffers
        r = fn()
        if it:
            rows.append(r)
    rows = np.array(rows, dtype=np.float64)
    return np.median(rows, axis=0), rows.min(axis=0), rows.max(axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--cells", type=int, default=0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-wide", action="store_true", help="skip the 64- and 65-list runs")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-rows", type=int, default=100_000)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-hint", action="store_true")
    a = ap.parse_args()
    if a.trace_hint:
        print("rocprofv3 --kernel-trace --stats -d OUT -o score -- python scripts/score_genes_time.py --config %s --runs 1 --no-wide" % a.config)
        return
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    cells, genes, density, seed = CONFIGS[a.config]
    cells = a.cells or cells
    lib = F.lib()
    ctx = sr.Context.default()
    m = synth(sr, F, ctx, seed, cells, genes, density)
    nnz = int(m.info().nnz)
    order = sorted(range(genes), key=lambda j: mix64(1000003 + j))          # two disjoint sets: the first 45 and the next 55 of one order
    sets = [np.array(sorted(order[:45]), dtype=np.uint64), np.array(sorted(order[45:100]), dtype=np.uint64)]
    sp, sg = pack(sets)
    score, cptr, cg = np.zeros((cells, 2)), np.zeros(3, np.uint64), np.zeros(2 * 50 * 26, np.uint64)
    info, ginfo = F.ScoreGenesInfo(), F.GeneListInfo()
    total = np.zeros(cells)

    def run_score():
        t0 = time.perf_counter()
        F.check(lib.srx_score_genes(m.handle, F.ptr(sp), F.ptr(sg), 2, None, 0, None, F.ptr(score), F.ptr(cptr), F.ptr(cg), cg.size, C.byref(info)),
                ctx.handle)
        return info.ms_mean, info.ms_ctrl, info.ms_walk, (time.perf_counter() - t0) * 1e3

    def run_rowsum():
        t0 = time.perf_counter()
        F.check(lib.srx_compute_sum(m.handle, F.ROW, F.ptr(total)), ctx.handle)
        return ((time.perf_counter() - t0) * 1e3,)

    def sums_of(lists):
        lp, lg = pack(lists)
        out = np.zeros((cells, len(lists)))

        def run():
            t0 = time.perf_counter()
            F.check(lib.srx_gene_list_sums(m.handle, F.ptr(lp), F.ptr(lg), len(lists), F.ptr(out), None, C.byref(ginfo)), ctx.handle)
            return ginfo.ms_scan, ginfo.ms_walk, (time.perf_counter() - t0) * 1e3, ginfo.n_walks
        return run

    sc = median_of(run_score, a.runs)
    ctrl = [cg[int(cptr[s]):int(cptr[s + 1])].copy() for s in range(2)]
    rs = median_of(run_rowsum, a.runs)
    four = median_of(sums_of(sets + ctrl), a.runs)
    out = {"config": a.config, "cells": cells, "genes": genes, "nnz": nnz, "set_sizes": [45, 55], "ctrl_sizes": [int(c.size) for c in ctrl],
           "n_items": int(info.n_items), "sum_scale_log2": int(info.sum_scale_log2), "max_abs": info.max_abs, "n_walks": int(info.n_walks),
           "score": {"ms_mean": sc[0][0], "ms_ctrl": sc[0][1], "ms_walk": sc[0][2], "ms_wall": sc[0][3],
                     "spread_walk": [sc[1][2], sc[2][2]], "spread_wall": [sc[1][3], sc[2][3]]},
           "row_sum_call_ms": rs[0][0], "row_sum_call_spread": [rs[1][0], rs[2][0]],
           "four_lists": {"ms_scan": four[0][0], "ms_walk": four[0][1], "ms_wall": four[0][2], "spread_walk": [four[1][1], four[2][1]]},
           "index_bytes": 2 * nnz, "value_bytes": 4 * nnz}
    out["walk_GBps_of_indices"] = out["index_bytes"] / (four[0][1] * 1e-3) / 1e9
    out["ratio_walk_to_row_sum_call"] = four[0][1] / rs[0][0]
    if not a.no_wide:
        for n_lists in (64, 65):
            lists = [hashed_genes(genes, 50, 100 + t) for t in range(n_lists)]
            w = median_of(sums_of(lists), max(a.runs - 1, 1))
            out["lists_%d" % n_lists] = {"n_walks": int(w[0][3]), "ms_walk": w[0][1], "ms_wall": w[0][2], "spread_walk": [w[1][1], w[2][1]]}
    if a.host:
        import pandas as pd
        import scipy.sparse as sp_
        rows = min(a.host_rows, cells)
        mh = synth(sr, F, ctx, seed, rows, genes, density)
        hn = int(mh.info().nnz)
        ip, ix = np.zeros(rows + 1, np.uint64), np.zeros(hn, np.uint64)
        F.check(lib.srx_matrix_download_pattern(mh.handle, F.ptr(ip), F.ptr(ix)), ctx.handle)
        X = sp_.csr_matrix((mh.values(np.float32), ix.astype(np.int32), ip.astype(np.int64)), shape=(rows, genes))
        hs = np.zeros((rows, 2))
        F.check(lib.srx_score_genes(mh.handle, F.ptr(sp), F.ptr(sg), 2, None, 0, None, F.ptr(hs), F.ptr(cptr), F.ptr(cg), cg.size, C.byref(info)), ctx.handle)
        hctrl = [cg[int(cptr[s]):int(cptr[s + 1])].astype(np.int64) for s in range(2)]
        t0 = time.perf_counter()
        mean = np.asarray(X.sum(axis=0, dtype=np.float64)).ravel() / rows
        n_items = int(np.round(genes / 24))
        cut = (pd.Series(mean).rank(method="min").astype(np.int64) // n_items).to_numpy()
        t1 = time.perf_counter()
        Xc = X.tocsc()
        t2 = time.perf_counter()
        got = np.zeros((rows, 2))
        for s in range(2):
            a_ = np.asarray(Xc[:, sets[s].astype(np.int64)].sum(axis=1, dtype=np.float64)).ravel() / sets[s].size
            b_ = np.asarray(Xc[:, hctrl[s]].sum(axis=1, dtype=np.float64)).ravel() / hctrl[s].size
            got[:, s] = a_ - b_
        t3 = time.perf_counter()
        out["host_route"] = {"note": "numpy / scipy / pandas in f64 with the library's control lists; not scanpy", "rows": rows, "nnz": hn,
                             "s_means_and_bins": t1 - t0, "s_to_csc": t2 - t1, "s_sums": t3 - t2, "s_total": t3 - t0,
                             "max_abs_difference_from_device": float(np.abs(got - hs).max()), "bins_used": int(len(set(cut[sets[0].astype(np.int64)])))}
        mh.free()
    print(json.dumps(out))
    if a.out:
        write_md(a.out, out)


def write_md(path, o):
    s, f = o["score"], o["four_lists"]
    L = ["# Gene-set scores: times at %s" % o["config"], "",
         "`python scripts/score_genes_time.py --config %s --host`: %d cells x %d genes, %d stored entries, f32 storage, log1p values; two" % (
             o["config"], o["cells"], o["genes"], o["nnz"]),
         "hashed sets of 45 and 55 genes, ctrl_size 50, n_bins 25 (controls: %s genes, n_items %d); medians of the runs after the first." % (
             " and ".join(str(c) for c in o["ctrl_sizes"]), o["n_items"]), "",
         "| stage | ms | min .. max |", "|---|---|---|",
         "| srx_score_genes: value scan + column means (ms_mean) | %.2f | |" % s["ms_mean"],
         "| srx_score_genes: control genes, host (ms_ctrl) | %.2f | |" % s["ms_ctrl"],
         "| srx_score_genes: walk over 4 lists + score (ms_walk) | %.2f | %.2f .. %.2f |" % (s["ms_walk"], *s["spread_walk"]),
         "| srx_score_genes: the call, wall | %.2f | %.2f .. %.2f |" % (s["ms_wall"], *s["spread_wall"]),
         "| srx_gene_list_sums, the same 4 lists: value scan (ms_scan) | %.2f | |" % f["ms_scan"],
         "| srx_gene_list_sums, the same 4 lists: walk (ms_walk, with the table upload) | %.2f | %.2f .. %.2f |" % (f["ms_walk"], *f["spread_walk"]),
         "| srx_compute_sum(m, Row): the call (kernel + read-back of n_obs doubles) | %.2f | %.2f .. %.2f |" % (o["row_sum_call_ms"], *o["row_sum_call_spread"])]
    for k in ("lists_64", "lists_65"):
        if k in o:
            L.append("| srx_gene_list_sums, %s lists of 50 genes: %d walk(s) | %.2f | %.2f .. %.2f |" % (k[6:], o[k]["n_walks"], o[k]["ms_walk"], *o[k]["spread_walk"]))
    L += ["", "The walk streams %.2f GB of 16-bit indices: %.0f GB/s.  Walk / row-sum call = %.2f (the kernels alone: below)." % (
        o["index_bytes"] / 1e9, o["walk_GBps_of_indices"], o["ratio_walk_to_row_sum_call"]), ""]
    if "host_route" in o:
        h = o["host_route"]
        L += ["Host route on %d cells (%d entries), %s: means and bins %.2f s, CSR -> CSC %.2f s, the four column sums %.2f s, total %.2f s;" % (
            h["rows"], h["nnz"], h["note"], h["s_means_and_bins"], h["s_to_csc"], h["s_sums"], h["s_total"]),
            "largest difference from the device's scores on those cells %.2e." % h["max_abs_difference_from_device"], ""]
    L += ["```json", json.dumps(o), "```", ""]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(L))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Times of the marker-gene pass (srx_rank_genes_groups) on the c3-shaped synthetic matrix, log-normalised on the device:
8, 32 and 256 random groups and one Louvain labelling read where it lies.  Reported per labelling (min / median of --runs
calls after --warmup): info.ms and its stages (the library prints them under SRX_MARKERS_TRACE=1), beside the plain per-gene
moments pass (SRX_K_MOMENTS via srx_prof_get) on a handle with the same values in the same process, and a host numpy / scipy
`onehot @ X` + Welch t-test over the first --host-rows rows of the same matrix.  Report only: prints one JSON document.

With --method wilcoxon the rank-sum route (srx_rank_genes_wilcoxon[_graph]) is timed instead, on one random labelling of 32
groups and the Louvain labelling: info.ms, the three stage times, the chunks and the staging bytes of srx_wilcoxon_info, beside
the t-test call on the same input in the same process (the yardstick for everything but the staging, the sort and the ranks)
and scipy.stats.rankdata / mannwhitneyu over the first --host-rows rows.

    python scripts/markers_time.py [--cells 1300000 --genes 28000 --density 0.03 --runs 10 --warmup 2 --host-rows 130000]
    python scripts/markers_time.py --method wilcoxon [--tie-correct --scratch-bytes B]
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["SRX_MARKERS_TRACE"] = "1"

TRACE = re.compile(r"srx markers: groups (\d+) blocks (\d+) prepare ([\d.]+) moments ([\d.]+) statistics ([\d.]+) ranking ([\d.]+) ms")


class StderrCapture:
    """The library writes its stage times to the C stderr: divert file descriptor 2 into a file for the duration."""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def min_med(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4)}


def wilcoxon_report(a, lib, ctx, m, p, graph, timed, out, rng):
    """The rank-sum route on random_32 and the Louvain labelling, the t-test call beside it, scipy on a tenth of the rows."""
    from singlerust_amd import _ffi as F
    wopts = F.WilcoxonOpts(0, -1, 1 if a.tie_correct else 0, 0, a.scratch_bytes)
    ropts = F.RankGenesOpts(0, -1)
    out["method"] = "wilcoxon"
    out["tie_correct"] = bool(a.tie_correct)

    def timed_wilcoxon(call):
        ms, stages, wi = [], [], F.WilcoxonInfo()
        for i in range(a.warmup + a.runs):
            hk = C.c_void_p()
            call(hk)
            info = F.MarkersInfo()
            F.check(lib.srx_markers_info_get(hk, C.byref(info)), ctx.handle)
            F.check(lib.srx_markers_wilcoxon_info_get(hk, C.byref(wi)), ctx.handle)
            lib.srx_markers_free(hk)
            print("wilcoxon call %d: info.ms %.1f (stage %.1f sort %.1f ranks %.1f), %d chunks" % (i, info.ms, wi.ms_stage, wi.ms_sort, wi.ms_ranks,
                                                                                                  wi.n_chunks), file=sys.stderr, flush=True)
            if i >= a.warmup:
                ms.append(info.ms)
                stages.append([wi.ms_stage, wi.ms_sort, wi.ms_ranks])
        st = np.array(stages)
        r = {"n_groups": int(info.n_groups), "info_ms": min_med(ms), "n_chunks": int(wi.n_chunks), "scratch_bytes": int(wi.scratch_bytes),
             "segment_limit": int(wi.segment_limit), "segments_short": int(wi.segments_short), "segments_long": int(wi.segments_long)}
        for j, name in enumerate(("stage", "sort", "ranks")):
            r[name + "_ms"] = min_med(list(st[:, j]))
        return r

    labels = rng.integers(0, 32, a.cells).astype(np.uint32)
    calls = {"random_32": (lambda hk: F.check(lib.srx_rank_genes_wilcoxon(m.handle, F.ptr(labels), 32, C.byref(wopts), C.byref(hk)), ctx.handle),
                           lambda hk: F.check(lib.srx_rank_genes_groups(m.handle, F.ptr(labels), 32, C.byref(ropts), C.byref(hk)), ctx.handle))}
    if graph is not None:
        calls["louvain"] = (lambda hk: F.check(lib.srx_rank_genes_wilcoxon_graph(m.handle, graph, C.byref(wopts), C.byref(hk)), ctx.handle),
                            lambda hk: F.check(lib.srx_rank_genes_groups_graph(m.handle, graph, C.byref(ropts), C.byref(hk)), ctx.handle))
    for name, (wx, tt) in calls.items():
        out["labellings"][name] = {"wilcoxon": timed_wilcoxon(wx), "t_test": timed(tt)}

    # the host: scipy's ranking over the first host_rows rows of the same matrix, 200 genes, one group against the rest
    import scipy.sparse as sp
    import scipy.stats
    nh = min(a.host_rows, a.cells)
    ip = np.zeros(nh + 1, np.uint64)
    lib.srx_synth_indptr(C.byref(p), 0, nh, F.ptr(ip))
    idx, val = np.zeros(int(ip[-1]), np.uint64), np.zeros(int(ip[-1]), np.float32)
    lib.srx_synth_fill_host(C.byref(p), 0, nh, F.ptr(ip), F.ptr(idx), F.ptr(val))
    X = sp.csr_matrix((val.astype(np.float64), idx.astype(np.int64), ip.astype(np.int64)), shape=(nh, a.genes))
    X = sp.diags(1e4 / np.maximum(np.asarray(X.sum(axis=1)).ravel(), 1.0)) @ X
    X.data = np.log1p(X.data)
    D = X[:, :200].toarray()
    lab = rng.integers(0, 32, nh)
    t0 = time.perf_counter()
    ranks = scipy.stats.rankdata(D, axis=0)
    np.stack([ranks[lab == g].sum(axis=0) for g in range(32)])
    t_rank = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    scipy.stats.mannwhitneyu(D[lab == 0], D[lab != 0], axis=0, use_continuity=False, method="asymptotic")
    t_mwu = (time.perf_counter() - t0) * 1e3
    out["host_scipy"] = {"rows": nh, "genes": 200, "rankdata_and_32_group_sums_ms": round(t_rank, 1),
                         "mannwhitneyu_one_group_ms": round(t_mwu, 1),
                         "note": "dense columns, on the host CPUs; all %d genes would take %d times as long" % (a.genes, a.genes // 200)}
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_300_000)
    ap.add_argument("--genes", type=int, default=28_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=3003)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-rows", type=int, default=130_000)
    ap.add_argument("--no-louvain", action="store_true")
    ap.add_argument("--method", choices=("t-test", "wilcoxon"), default="t-test")
    ap.add_argument("--tie-correct", action="store_true")
    ap.add_argument("--scratch-bytes", type=int, default=0)
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
    out = {"cells": a.cells, "genes": a.genes, "nnz": int(m.info().nnz), "storage": "f32", "runs": a.runs, "labellings": {}}
    graph = None
    if not a.no_louvain:
        # the chain as far as the labels: pipeline (leaves X log-normalised), neighbours, Louvain
        opts, res = F.PcaOpts(50, -1, -1, -1, 0, 0, 0, 0.0, 12345), F.PipelineResult()
        F.check(lib.srx_pipeline(m.handle, 1e4, 2000, C.byref(opts), C.byref(res)), ctx.handle)
        graph = C.c_void_p()
        F.check(lib.srx_neighbors_result(m.handle, C.byref(F.KnnOpts(15, 0, 0, 0)), None, C.byref(graph)), ctx.handle)
        li = F.LouvainInfo()
        F.check(lib.srx_louvain(graph, None, None, C.byref(li)), ctx.handle)
        out["louvain"] = {"communities": int(li.n_communities), "ms": round(li.ms, 3)}
    else:
        F.check(lib.srx_normalize_log1p_inplace(m.handle, 1e4, None), ctx.handle)

    def timed(call):
        ms, stages = [], []
        for i in range(a.warmup + a.runs):
            hk = C.c_void_p()
            with StderrCapture() as cap:
                call(hk)
            info = F.MarkersInfo()
            F.check(lib.srx_markers_info_get(hk, C.byref(info)), ctx.handle)
            lib.srx_markers_free(hk)
            t = TRACE.search(cap.text)
            if i >= a.warmup:
                ms.append(info.ms)
                stages.append([float(x) for x in t.groups()[2:]])
        st = np.array(stages)
        r = {"n_groups": int(info.n_groups), "blocks": int(t.group(2)), "info_ms": min_med(ms)}
        for j, name in enumerate(("prepare_max_validate_sort", "grouped_moments", "statistics", "ranking")):
            r[name + "_ms"] = min_med(list(st[:, j]))
        return r

    ropts = F.RankGenesOpts(0, -1)
    rng = np.random.default_rng(1)
    if a.method == "wilcoxon":
        wilcoxon_report(a, lib, ctx, m, p, graph, timed, out, rng)
        return
    for k in (8, 32, 256):
        labels = rng.integers(0, k, a.cells).astype(np.uint32)
        out["labellings"]["random_%d" % k] = timed(
            lambda hk: F.check(lib.srx_rank_genes_groups(m.handle, F.ptr(labels), k, C.byref(ropts), C.byref(hk)), ctx.handle))
    if graph is not None:
        out["labellings"]["louvain"] = timed(
            lambda hk: F.check(lib.srx_rank_genes_groups_graph(m.handle, graph, C.byref(ropts), C.byref(hk)), ctx.handle))

    # the yardstick: the plain per-gene moments pass over the same values (a clone whose values are rewritten before every call,
    # so that its moments cache does not answer)
    work = m.clone()
    ctx.prof_enable(1 << F.K_MOMENTS)
    plain = []
    for i in range(a.warmup + a.runs):
        work.copy_values_from(m)
        ctx.prof_reset()
        F.check(lib.srx_gene_moments(work.handle, None, None, None), ctx.handle)
        ctx.synchronize()
        if i >= a.warmup:
            plain.append(ctx.prof_get(F.K_MOMENTS)[0])
    ctx.prof_enable(0)
    out["plain_gene_moments_ms"] = min_med(plain)
    work.free()

    # the host: the first host_rows rows of the same matrix (the generator is row-local), log-normalised with numpy
    import scipy.sparse as sp
    import scipy.stats
    nh = min(a.host_rows, a.cells)
    ip = np.zeros(nh + 1, np.uint64)
    lib.srx_synth_indptr(C.byref(p), 0, nh, F.ptr(ip))
    idx, val = np.zeros(int(ip[-1]), np.uint64), np.zeros(int(ip[-1]), np.float32)
    lib.srx_synth_fill_host(C.byref(p), 0, nh, F.ptr(ip), F.ptr(idx), F.ptr(val))
    X = sp.csr_matrix((val.astype(np.float64), idx.astype(np.int64), ip.astype(np.int64)), shape=(nh, a.genes))
    X = sp.diags(1e4 / np.maximum(np.asarray(X.sum(axis=1)).ravel(), 1.0)) @ X
    X.data = np.log1p(X.data)
    host = {}
    for k in (8, 32):
        labels = rng.integers(0, k, nh)
        t0 = time.perf_counter()
        onehot = sp.csr_matrix((np.ones(nh), (labels, np.arange(nh))), shape=(k, nh))
        X2 = X.copy()
        X2.data **= 2
        S, Q = np.asarray((onehot @ X).todense()), np.asarray((onehot @ X2).todense())
        n_g = np.bincount(labels, minlength=k)[:, None].astype(np.float64)
        n_r = nh - n_g
        mean, mean_r = S / n_g, (S.sum(0) - S) / n_r
        var = (Q / n_g - mean ** 2) * n_g / (n_g - 1)
        var_r = ((Q.sum(0) - Q) / n_r - mean_r ** 2) * n_r / (n_r - 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            score = (mean - mean_r) / np.sqrt(var / n_g + var_r / n_r)
        np.argsort(-np.nan_to_num(score), axis=1, kind="stable")
        host["random_%d" % k] = round((time.perf_counter() - t0) * 1e3, 1)
    t0 = time.perf_counter()
    scipy.stats.ttest_ind(X[labels == 0][:, :200].toarray(), X[labels != 0][:, :200].toarray(), axis=0, equal_var=False)
    host["scipy_ttest_ind_one_group_200_genes_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    out["host_numpy_scipy"] = {"rows": nh, "ms": host, "note": "moments by onehot @ X, Welch t and a stable argsort per group, on the host CPUs"}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

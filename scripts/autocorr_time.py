"""Time of Moran's I / Geary's C over the resident matrix and the resident neighbour graph (srx_pipeline, srx_neighbors_result on
its own PCA scores, then srx_autocorr with C where it lies): info.ms split into its three parts (graph sums | S, Q, A, B | the
walk for P) and per kernel, warm, median of --reps calls.  Beside it what the walk must do: the entry visits (sum over the edges j > i of the
neighbour's row length), the bytes those visits move (index + value per visit) and the time they would take at the streaming
rate k_row_sum reaches (5.8 TB/s); and the unit of comparison, srx_compute_sum(m, Row) timed in the same session on
the same handle (as a call: its kernel and the read-back of one double per cell).
With --host-cells N > 0 a second, smaller case is fetched and Moran's I of the first --host-genes genes is made on the host by
scipy (the restatement of tests/autocorr_ref.py: literal_f64's sums, sparse), timed without the fetch.

    python scripts/autocorr_time.py [--cells 1300000] [--genes 28000] [--density 0.03] [--n-hvg 2000] [--n-pc 50] [--k 15]
                                    [--reps 3] [--host-cells 100000] [--host-genes 256] [--rows-per-block 0]

Prints one JSON line.  The matrix is srx_synth's (the bench's c3 shape by default), f32 storage, log-normalised by the pipeline."""
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
from singlerust_amd.memory import statistics                        # noqa: E402
from singlerust_amd.memory.processing._common import flat_info      # noqa: E402
from singlerust_amd.memory.processing.neighbors import Graph        # noqa: E402

STREAM_TBS = 5.8          # k_row_sum's read rate (the kernel table)


def nnz_values_bytes(row_len):
    """The bytes of the matrix's f32 values, what the row-sum pass streams."""
    return float(row_len.sum()) * 4


def resident_case(ctx, a, cells):
    """(adata, graph): pipeline and k-NN graph on a synthetic matrix of `cells` rows."""
    lib = F.lib()
    p = F.SynthParams()
    lib.srx_synth_defaults(C.byref(p), 3003, cells, a.genes, a.density)
    h = C.c_void_p()
    F.check(lib.srx_synth_generate(ctx.handle, C.byref(p), 0, cells, F.F32, F.STORE_F32, C.byref(h)), ctx.handle)
    ad = sr.IMAnnData(sr.DeviceCsr(ctx, h), None, None, [], [])
    opts = F.PcaOpts(a.n_pc, -1, -1, -1, 0, 0, 0, 0.0, 12345)
    res = F.PipelineResult()
    F.check(lib.srx_pipeline(ad.x().handle, 1e4, a.n_hvg, C.byref(opts), C.byref(res)), ctx.handle)
    gh = C.c_void_p()
    F.check(lib.srx_neighbors_result(ad.x().handle, C.byref(F.KnnOpts(a.k, 0, 0, 0)), None, C.byref(gh)), ctx.handle)
    return ad, Graph(ctx, gh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_300_000)
    ap.add_argument("--genes", type=int, default=28_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--n-hvg", type=int, default=2000)
    ap.add_argument("--n-pc", type=int, default=50)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-cells", type=int, default=100_000)
    ap.add_argument("--host-genes", type=int, default=256)
    ap.add_argument("--rows-per-block", type=int, default=0)
    a = ap.parse_args()
    ctx = sr.Context.default()
    lib = F.lib()
    out = {}
    for cells in [a.cells] + ([a.host_cells] if a.host_cells > 0 and a.host_cells != a.cells else []):
        ad, g = resident_case(ctx, a, cells)
        info = F.AutocorrInfo()
        opts = F.AutocorrOpts(a.rows_per_block, 0)
        mi = np.zeros(a.genes)

        def once():
            t0 = time.perf_counter()
            F.check(lib.srx_autocorr(ad.x().handle, g.handle, C.byref(opts), C.byref(F.AutocorrOut(F.ptr(mi))), C.byref(info)), ctx.handle)
            return (time.perf_counter() - t0) * 1e3

        once()                                                       # warm: scratch allocation, code-object load, the gene tiles
        walls, parts = [], []
        for _ in range(a.reps):
            walls.append(once())
            parts.append((info.ms, info.ms_graph, info.ms_moments, info.ms_walk, info.ms_wmax, info.ms_degrees, info.ms_s2,
                          info.ms_sum_sumsq, info.ms_dsum_dsumsq))
        med = np.median(np.array(parts), axis=0)
        # the unit of comparison, in the same session on the same handle: srx_compute_sum(m, Row), timed as a call (its kernel
        # and the read-back of one double per cell)
        row_len = np.asarray(statistics.compute_number(ad, sr.Direction.Row), dtype=np.int64)
        total = np.zeros(cells)
        rs = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            F.check(lib.srx_compute_sum(ad.x().handle, F.ROW, F.ptr(total)), ctx.handle)
            rs.append((time.perf_counter() - t0) * 1e3)
        row_sum_call = float(np.median(rs[1:]))
        row_sum_rate = nnz_values_bytes(row_len) / (row_sum_call * 1e-3)          # bytes of values per second of the call
        indptr, indices, _ = g.fetch(F.GRAPH_CONNECTIVITIES)
        rows = np.repeat(np.arange(cells, dtype=np.int64), np.diff(indptr.astype(np.int64)))
        upper = indices.astype(np.int64) > rows
        visits = int(row_len[indices[upper]].sum())
        nnz = int(row_len.sum())
        visit_bytes = visits * (4 + (2 if a.genes <= 65536 else 4))
        r = {"cells": cells, "k": a.k, "autocorr": flat_info(info),
             "ms": {"total": round(float(med[0]), 3), "graph": round(float(med[1]), 3), "moments": round(float(med[2]), 3), "walk": round(float(med[3]), 3)},
             "ms_per_kernel": {"k_ac_wmax": round(float(med[4]), 3), "k_ac_degrees": round(float(med[5]), 3), "k_ac_s2": round(float(med[6]), 3),
                               "k_ac_moments_S_Q": round(float(med[7]), 3), "k_ac_moments_A_B": round(float(med[8]), 3),
                               "k_ac_walk": round(float(med[3]), 3),
                               "graph_read_backs_and_value_scan": round(float(med[1] - med[4] - med[5] - med[6]), 3)},
             "rows_per_block_opt": a.rows_per_block,
             "wall_ms": {"min": round(min(walls), 3), "median": round(float(np.median(walls)), 3)},
             "edges_upper": int(upper.sum()), "entry_visits": visits, "visit_bytes": visit_bytes,
             "visit_floor_ms": round(visit_bytes / (STREAM_TBS * 1e12) * 1e3, 3),
             "walk_rate_TBs": round(visit_bytes / (float(med[3]) * 1e-3) / 1e12, 3) if med[3] > 0 else None,
             "matrix_nnz": nnz, "row_sum_call_ms": round(row_sum_call, 3),
             "row_sum_call_TBs": round(row_sum_rate / 1e12, 3),
             "call_in_row_sum_calls": round(float(med[0]) / row_sum_call, 1),
             "visits_at_row_sum_call_rate_ms": round(visit_bytes / row_sum_rate * 1e3, 3),
             "walk_over_visits_at_row_sum_call_rate": round(float(med[3]) / (visit_bytes / row_sum_rate * 1e3), 2),
             "row_sum_at_stream_rate_ms": round(nnz * 4 / (STREAM_TBS * 1e12) * 1e3, 3),
             "genes_constant": int(info.genes_constant), "max_I": float(np.nanmax(mi)) if not np.isnan(mi).all() else None}
        if cells == a.host_cells and a.host_genes > 0:
            import scipy.sparse as sp
            mi_ = ad.x().info()
            ip, ix = np.zeros(cells + 1, dtype=np.uint64), np.zeros(mi_.nnz, dtype=np.uint64)
            F.check(lib.srx_matrix_download_pattern(ad.x().handle, F.ptr(ip), F.ptr(ix)), ctx.handle)
            vals = ad.x().values(np.float64)
            X = sp.csr_matrix((vals, ix.astype(np.int64), ip.astype(np.int64)), shape=(cells, a.genes))
            W = sp.csr_matrix((g.fetch(F.GRAPH_CONNECTIVITIES)[2], indices.astype(np.int64), indptr.astype(np.int64)), shape=(cells, cells))
            host = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                Xs = X[:, :a.host_genes].tocsc().tocsr()
                d = np.asarray(W.sum(axis=1)).ravel()
                s0 = d.sum()
                S = np.asarray(Xs.sum(axis=0)).ravel()
                Q = np.asarray(Xs.multiply(Xs).sum(axis=0)).ravel()
                A = np.asarray(Xs.T @ d).ravel()
                P2 = np.asarray(Xs.multiply(W @ Xs).sum(axis=0)).ravel()
                m = S / cells
                with np.errstate(divide="ignore", invalid="ignore"):
                    I = cells / s0 * (P2 - 2 * m * A + m * m * s0) / (Q - cells * m * m)
                host.append((time.perf_counter() - t0) * 1e3)
            ok = np.isfinite(I) & np.isfinite(mi[:a.host_genes])
            r["host"] = {"genes": a.host_genes, "scipy_ms": round(float(np.median(host)), 1),
                         "scipy_ms_scaled_to_all_genes": round(float(np.median(host)) * a.genes / a.host_genes, 0),
                         "max_abs_diff_I": float(np.abs(I[ok] - mi[:a.host_genes][ok]).max()) if ok.any() else None}
        out["c%d" % cells] = r
        g.free()
        ad.x().free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

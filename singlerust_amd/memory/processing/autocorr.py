"""Moran's I and Geary's C per gene over libsrx_hip (``srx_autocorr`` / ``srx_autocorr_csr`` /
``srx_autocorr_from_tables``): which genes vary smoothly
along the neighbour graph, what ``sc.metrics.morans_i`` / ``sc.metrics.gearys_c`` give over ``obsp["connectivities"]``.

Not in the reference.  The definition (five 64-bit fixed-point tables per gene, the statistics from them in extended
precision, z-scores under normality) is in include/srx.h.  The tables are made on the device from the resident matrix and the
resident graph; the arithmetic on the five numbers per gene is host code in the library.
NOT compared: scanpy, squidpy, esda (not installed).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import IMAnnData
from ._common import csr_triple, flat_info, graph_of

_F64 = ("morans_i", "gearys_c", "z_i", "z_c", "sum", "sumsq", "dsum", "dsumsq", "cross")
_I64 = ("sum_int", "sumsq_int", "dsum_int", "dsumsq_int", "cross_int")


class _Out:
    """The host buffers of one call and the ``srx_autocorr_out`` that points at them; ``want`` None = every array."""

    def __init__(self, n_genes: int, want=None):
        names = _F64 + _I64 if want is None else tuple(want)
        self.arrays = {k: np.zeros(n_genes, dtype=np.float64 if k in _F64 else np.int64) for k in names}
        self.c = F.AutocorrOut(*[F.ptr(self.arrays[k]) if k in self.arrays and n_genes else None for k in _F64 + _I64])
        self.info = F.AutocorrInfo()

    def result(self) -> dict:
        r = dict(self.arrays)
        r["info"] = flat_info(self.info)
        return r


def _opts(rows_per_block):
    return C.byref(F.AutocorrOpts(int(rows_per_block), 0)) if rows_per_block else None


def _on_graph(adata: IMAnnData, who: str, want, rows_per_block=None) -> dict:
    g = graph_of(adata, who)
    x = adata.x()
    o = _Out(adata.n_vars(), want)
    F.check(F.lib().srx_autocorr(x.handle, g.handle, _opts(rows_per_block), C.byref(o.c), C.byref(o.info)), x.ctx.handle)
    return o.result()


def _subset(values: np.ndarray, genes):
    return values if genes is None else values[np.asarray(genes, dtype=np.int64)]


def morans_i(adata: IMAnnData, genes=None) -> np.ndarray:
    """Moran's I of every gene (or of the gene indices ``genes``) on the graph that ``neighbors(adata, connectivities=True)``
    left on the device; NaN for a constant gene."""
    return _subset(_on_graph(adata, "morans_i", ("morans_i",))["morans_i"], genes)


def gearys_c(adata: IMAnnData, genes=None) -> np.ndarray:
    """Geary's C of every gene (or of the gene indices ``genes``) on the resident graph; NaN for a constant gene."""
    return _subset(_on_graph(adata, "gearys_c", ("gearys_c",))["gearys_c"], genes)


def gene_autocorr(adata: IMAnnData, rows_per_block=None) -> dict:
    """Both statistics, their z-scores under normality, the five tables (as f64 and as the integers themselves) and ``info``
    as a dict; also written to ``adata.uns["autocorr"]``."""
    r = _on_graph(adata, "gene_autocorr", None, rows_per_block)
    adata.uns["autocorr"] = r
    return r


def autocorr_csr(mat, graph, rows_per_block=None) -> dict:
    """The same for a caller-supplied symmetric graph: a scipy sparse matrix or an (indptr, indices, data) triple with zero
    diagonal, strictly ascending rows and the same bits both ways.  ``mat``: an ``IMAnnData`` or its device matrix."""
    x = mat.x() if hasattr(mat, "x") else mat
    indptr, indices, data = csr_triple(graph, "autocorr_csr")
    o = _Out(int(x.info().n_cols))
    F.check(F.lib().srx_autocorr_csr(x.handle, F.ptr(indptr), F.ptr(indices) if indices.size else None,
                                     F.ptr(data) if data.size else None, indptr.size - 1, _opts(rows_per_block), C.byref(o.c),
                                     C.byref(o.info)), x.ctx.handle)
    return o.result()


def autocorr_from_tables(tables: dict, info: dict) -> dict:
    """The statistics from the five integer tables (``sum_int`` ... ``cross_int``) and an ``info`` dict holding ``n``, the eight
    scales and ``w_int``, ``s1_int``, ``s2_int``: host code in the library, no GPU."""
    t = [np.ascontiguousarray(tables[k], dtype=np.int64) for k in _I64]
    G = t[0].size
    if any(a.shape != (G,) for a in t):
        raise ValueError("autocorr_from_tables: five tables of one length expected")
    o = _Out(G, _F64)
    for k in ("n", "s_sum", "s_sumsq", "s_dsum", "s_dsumsq", "s_cross", "s_w", "s_1", "s_2", "w_int", "s1_int", "s2_int"):
        setattr(o.info, k, int(info[k]))
    F.check(F.lib().srx_autocorr_from_tables(*[F.ptr(a) if G else None for a in t], G, C.byref(o.info), C.byref(o.c)), None)
    r = o.result()
    r.update({k: a for k, a in zip(_I64, t)})
    return r


def autocorr_scales(n: int, nnz: int, max_abs: float, max_weight: float, max_degree: float) -> dict:
    """The eight fixed-point scales of the header's rule (``srx_autocorr_scales``): host code in the library, no GPU."""
    i = F.AutocorrInfo()
    i.n, i.nnz, i.max_abs, i.max_weight, i.max_degree = int(n), int(nnz), float(max_abs), float(max_weight), float(max_degree)
    F.check(F.lib().srx_autocorr_scales(C.byref(i)), None)
    return {k: getattr(i, k) for k in ("s_sum", "s_sumsq", "s_dsum", "s_dsumsq", "s_cross", "s_w", "s_1", "s_2")}

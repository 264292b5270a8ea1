"""Highly variable genes by analytic Pearson residuals over libsrx_hip (``srx_select_hvg_pearson``, ``srx_pearson_residuals``):
what ``sc.experimental.pp.highly_variable_genes(flavor="pearson_residuals")`` and ``normalize_pearson_residuals`` give, on
the RAW counts, before ``normalize_total`` / ``log1p``.

Not in the reference.  The definition (include/srx.h) is scanpy's closed form; every residual is evaluated on the device, the
matrix never leaves it.  Departures from scanpy: an empty cell has residual 0 (scanpy: NaN), equal variances are ordered by gene
index (scanpy: an unstable argsort), no ``batch_key``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import DeviceCsr, IMAnnData
from ._common import flat_info


def _matrix(x) -> DeviceCsr:
    return x.x() if isinstance(x, IMAnnData) else x


def _opts(theta, clip) -> F.PearsonOpts:
    # the option struct reads 0 as "the default" (theta 100, clip sqrt(n_obs)); None means the same here
    return F.PearsonOpts(0.0 if theta is None else float(theta), 0.0 if clip is None else float(clip))


def pearson_gene_variance(adata, theta=100.0, clip=None):
    """(residual variance of every gene, info dict): ``srx_pearson_gene_variance``."""
    m = _matrix(adata)
    var = np.zeros(int(m.info().n_cols), dtype=np.float64)
    o, i = _opts(theta, clip), F.PearsonInfo()
    F.check(F.lib().srx_pearson_gene_variance(m.handle, C.byref(o), F.ptr(var), C.byref(i)), m.ctx.handle)
    return var, flat_info(i)


def highly_variable_genes_pearson(adata, n_top_genes=2000, theta=100.0, clip=None) -> np.ndarray:
    """The ``n_top_genes`` genes with the largest residual variance, in rank order (uint64).  An ``IMAnnData`` receives
    ``var["highly_variable"]`` (bool: what ``FeatureSelection.HighlyVariableCol("highly_variable")`` reads),
    ``var["highly_variable_rank"]`` (NaN where not selected), ``var["residual_variances"]``, ``var["means"]`` and
    ``var["variances"]`` (over all cells, from the handle's cached moments; CSR storage only, NaN on a CSC handle) and
    ``uns["hvg"]``."""
    m = _matrix(adata)
    mi = m.info()
    n_vars, n_obs = int(mi.n_cols), int(mi.n_rows)
    want = min(int(n_top_genes), n_vars)
    idx = np.zeros(max(want, 1), dtype=np.uint64)
    n_out = C.c_uint64(0)
    var = np.zeros(n_vars, dtype=np.float64)
    o, i = _opts(theta, clip), F.PearsonInfo()
    F.check(F.lib().srx_select_hvg_pearson(m.handle, want, C.byref(o), F.ptr(idx), C.byref(n_out), F.ptr(var) if n_vars else None,
                                           C.byref(i)), m.ctx.handle)
    sel = idx[:int(n_out.value)].copy()
    if isinstance(adata, IMAnnData):
        mask = np.zeros(n_vars, dtype=bool)
        mask[sel.astype(np.int64)] = True
        rank = np.full(n_vars, np.nan)
        rank[sel.astype(np.int64)] = np.arange(sel.size, dtype=np.float64)
        means, variances = np.full(n_vars, np.nan), np.full(n_vars, np.nan)
        if not m.is_csc() and n_obs:
            s, sq = np.zeros(n_vars), np.zeros(n_vars)
            F.check(F.lib().srx_gene_moments(m.handle, None, F.ptr(s), F.ptr(sq)), m.ctx.handle)
            means = s / n_obs
            variances = sq / n_obs - means * means
        adata.var["highly_variable"] = mask
        adata.var["highly_variable_rank"] = rank
        adata.var["residual_variances"] = var
        adata.var["means"] = means
        adata.var["variances"] = variances
        adata.uns["hvg"] = dict(flat_info(i), flavor="pearson_residuals", n_top_genes=int(n_top_genes))
    return sel


def pearson_residuals(adata, genes, theta=100.0, clip=None) -> np.ndarray:
    """The clipped residuals (n_obs x len(genes), f64) of the listed genes, zeros included: ``srx_pearson_residuals``.  Genes may
    come in any order and may repeat."""
    m = _matrix(adata)
    g = np.ascontiguousarray(genes, dtype=np.uint64).ravel()
    out = np.zeros((int(m.info().n_rows), g.size), dtype=np.float64)
    o = _opts(theta, clip)
    dst = out if out.size else np.zeros(1)           # (the C call refuses a NULL output also where nothing is written)
    F.check(F.lib().srx_pearson_residuals(m.handle, F.ptr(g) if g.size else None, g.size, C.byref(o), F.ptr(dst), None), m.ctx.handle)
    return out

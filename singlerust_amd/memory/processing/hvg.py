"""Highly variable genes by analytic Pearson residuals over libsrx_hip (``srx_select_hvg_pearson``, ``srx_pearson_residuals``):
what ``sc.experimental.pp.highly_variable_genes(flavor="pearson_residuals")`` and ``normalize_pearson_residuals`` give, on
the RAW counts, before ``normalize_total`` / ``log1p``; and the PCA of the residuals of the chosen genes
(``srx_pca_pearson``: ``sc.experimental.pp.normalize_pearson_residuals_pca``), whose scores stay on the device.

Not in the reference.  The definition (include/srx.h) is scanpy's closed form; every residual is evaluated on the device, the
matrix never leaves it.  Departures from scanpy: an empty cell has residual 0 (scanpy: NaN), equal variances are ordered by gene
index (scanpy: an unstable argsort), no ``batch_key``.

Also here: ``highly_variable_genes_seurat_v3`` (``srx_select_hvg_seurat_v3``), scanpy's ``flavor="seurat_v3"`` with
``batch_key`` on the raw counts: per batch a direct loess fit of the mean / variance trend and the variance of the clipped
counts, then median ranks over the batches.  Departures: skmisc's "direct" surface in place of the interpolated default, ties by
gene index, integer ranks.
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


TOTALS = {"all": F.PEARSON_TOTALS_ALL, "selected": F.PEARSON_TOTALS_SELECTED}


def _pca_opts(theta, clip, totals, center, chunk_cells, n_components, max_iter=0, tol=0.0, seed=0, solver=0) -> F.PearsonPcaOpts:
    if totals not in TOTALS:
        raise ValueError("totals must be 'all' or 'selected', not %r" % (totals,))
    pca = F.PcaOpts(int(n_components), -1, 0, -1, 0, int(max_iter), int(solver), float(tol), int(seed))
    return F.PearsonPcaOpts(_opts(theta, clip), TOTALS[totals], int(bool(center)), int(chunk_cells), pca)


def _pca_info(i) -> dict:
    out = {n: getattr(i, n) for n, _ in i._fields_ if n != "pca"}
    out.update(flat_info(i.pca))
    return out


def pearson_gram(adata, genes, theta=100.0, clip=None, totals="selected", chunk_cells=0):
    """(Z^T Z (k x k), column sums of Z (k), info dict) of the clipped residuals Z of the listed genes: ``srx_pearson_gram``,
    the kernel-level entry of ``pca_pearson_residuals``.  An empty list is refused (``SrxError``, ``E_ARG``)."""
    m = _matrix(adata)
    g = np.ascontiguousarray(genes, dtype=np.uint64).ravel()
    gram, colsum = np.zeros((g.size, g.size), dtype=np.float64), np.zeros(g.size, dtype=np.float64)
    o, i = _pca_opts(theta, clip, totals, True, chunk_cells, -1), F.PearsonPcaInfo()
    F.check(F.lib().srx_pearson_gram(m.handle, F.ptr(g) if g.size else None, g.size, C.byref(o), F.ptr(gram), F.ptr(colsum), C.byref(i)),
            m.ctx.handle)
    return gram, colsum, _pca_info(i)


def pca_pearson_residuals(adata, genes=None, n_top_genes=2000, n_components=50, theta=100.0, clip=None, totals="selected",
                          center=True, chunk_cells=0, max_iter=0, tol=0.0, seed=0, solver=0) -> dict:
    """PCA of the clipped Pearson residuals of ``genes`` on the RAW counts (``srx_pca_pearson``).  ``genes`` None: the
    ``n_top_genes`` of ``highly_variable_genes_pearson`` (same theta and clip) are selected first.  ``totals``: "selected" takes the
    cell sums and the total over the listed genes (scanpy, which subsets before it normalises), "all" over the whole matrix
    (``pearson_residuals``).  The scores stay resident as the handle's PCA result (``neighbors``, ``harmony_integrate``, ... read
    them there); an ``IMAnnData`` also receives ``obsm["X_pca"]`` and ``uns["pca"]`` (``std`` is ones: no scaling).  Returns the
    info dict.  No ``PcaModel`` can be made of this result."""
    m = _matrix(adata)
    if genes is None:
        genes = highly_variable_genes_pearson(adata, n_top_genes, theta, clip)
    g = np.ascontiguousarray(genes, dtype=np.uint64).ravel()
    k, n = g.size, int(m.info().n_rows)
    n_pc = max(min(2 if int(n_components) < 0 else int(n_components), k), 0)
    scores, comps = np.zeros((n, n_pc), dtype=np.float64), np.zeros((k, n_pc), dtype=np.float64)
    evr, mean = np.zeros(n_pc, dtype=np.float64), np.zeros(k, dtype=np.float64)
    o, i = _pca_opts(theta, clip, totals, center, chunk_cells, n_components, max_iter, tol, seed, solver), F.PearsonPcaInfo()
    F.check(F.lib().srx_pca_pearson(m.handle, F.ptr(g) if k else None, k, C.byref(o), F.ptr(scores) if scores.size else None,
                                    F.ptr(comps) if comps.size else None, F.ptr(evr) if n_pc else None, F.ptr(mean) if k else None,
                                    C.byref(i)), m.ctx.handle)
    info = _pca_info(i)
    if isinstance(adata, IMAnnData):
        adata.obsm["X_pca"] = scores
        adata.uns["pca"] = {"components": comps, "explained_variance_ratio": evr, "mean": mean, "std": np.ones(k),
                            "selected_features": g, "n_iter": info["n_iter"], "residual": info["residual"], "solver": info["solver"],
                            "center": bool(center), "scale": False, "residuals": "pearson", "totals": totals}
    return dict(info, scores=scores, components=comps, explained_variance_ratio=evr, mean=mean, selected_features=g)


# ---- Seurat v3 ----------------------------------------------------------------------------------------------------------------------
_SEURAT_GENE = ("means", "variances", "variances_norm", "median", "nbatches")
_SEURAT_BATCH = ("mean", "var", "fitted", "reg_var", "clip", "clip_sum", "clip_sumsq", "nv", "rank")
_SEURAT_FLAVORS = {"seurat_v3": 0, "seurat_v3_paper": 1}


def seurat_v3_tables(adata, n_top_genes=2000, batch=None, n_batches=None, span=0.3, flavor="seurat_v3"):
    """(selection uint64 in rank order, dict of every table of ``srx_seurat_v3_tables``, info dict):
    ``srx_select_hvg_seurat_v3`` with everything fetched.  ``batch``: uint32 codes below ``n_batches`` (None: one batch)."""
    if flavor not in _SEURAT_FLAVORS:
        raise ValueError("flavor must be 'seurat_v3' or 'seurat_v3_paper', not %r" % (flavor,))
    m = _matrix(adata)
    mi = m.info()
    n_vars, n_obs = int(mi.n_cols), int(mi.n_rows)
    codes = None
    if batch is not None:
        codes = np.ascontiguousarray(batch, dtype=np.uint32).ravel()
        if codes.size != n_obs:
            raise ValueError("batch holds %d labels for %d cells" % (codes.size, n_obs))
        if n_batches is None:
            n_batches = int(codes.max()) + 1 if codes.size else 1
    nb = 1 if n_batches is None else int(n_batches)
    T = {k: np.zeros(n_vars, dtype=np.uint32 if k == "nbatches" else np.float64) for k in _SEURAT_GENE}
    T.update({k: np.zeros((nb, n_vars), dtype=np.uint32 if k == "rank" else np.float64) for k in _SEURAT_BATCH})
    tables = F.SeuratV3Tables(*[F.ptr(T[k]) if T[k].size else None for k in _SEURAT_GENE + _SEURAT_BATCH])
    idx = np.zeros(max(min(int(n_top_genes), n_vars), 1), dtype=np.uint64)
    n_out = C.c_uint64(0)
    o, i = F.SeuratV3Opts(float(span), _SEURAT_FLAVORS[flavor], 0), F.SeuratV3Info()
    F.check(F.lib().srx_select_hvg_seurat_v3(m.handle, int(n_top_genes), F.ptr(codes) if codes is not None else None, nb, C.byref(o),
                                             F.ptr(idx), C.byref(n_out), C.byref(tables), C.byref(i)), m.ctx.handle)
    return idx[:int(n_out.value)].copy(), T, flat_info(i)


def highly_variable_genes_seurat_v3(adata, n_top_genes=2000, batch=None, span=0.3, flavor="seurat_v3"):
    """``sc.pp.highly_variable_genes(flavor="seurat_v3", batch_key=...)`` on the RAW counts, on the device
    (``srx_select_hvg_seurat_v3``; the definition is in include/srx.h, with a direct loess surface where scanpy's is
    interpolated).  ``batch``: one label per cell of any type (None: one batch); ``flavor="seurat_v3_paper"`` orders by the number
    of batches first.  Returns (the selection in rank order, uint64; a dict of the per-gene columns under scanpy's names:
    ``means``, ``variances``, ``variances_norm``, ``highly_variable_rank`` (the median rank, NaN where the gene is in no batch's
    top), ``highly_variable_nbatches``, ``highly_variable``).  An ``IMAnnData`` receives the columns in ``var`` and ``uns["hvg"]``."""
    codes, cats = (None, None)
    if batch is not None:
        cats, inv = np.unique(np.asarray(batch), return_inverse=True)
        codes = np.ascontiguousarray(inv, dtype=np.uint32)
    sel, T, info = seurat_v3_tables(adata, n_top_genes, codes, None if cats is None else max(int(cats.size), 1), span, flavor)
    mask = np.zeros(T["means"].size, dtype=bool)
    mask[sel.astype(np.int64)] = True
    cols = {"means": T["means"], "variances": T["variances"], "variances_norm": T["variances_norm"],
            "highly_variable_rank": T["median"], "highly_variable_nbatches": T["nbatches"], "highly_variable": mask}
    if isinstance(adata, IMAnnData):
        for k, v in cols.items():
            adata.var[k] = v
        adata.uns["hvg"] = dict(info, flavor=flavor, n_top_genes=int(n_top_genes))
    return sel, cols

"""Covariates regressed out, the residuals scaled and clipped, and the PCA of the result over libsrx_hip (``srx_regress_fit``,
``srx_regress_residuals``, ``srx_regress_gram``, ``srx_pca_regress``): what ``sc.pp.regress_out`` -> ``sc.pp.scale(max_value)`` ->
``sc.tl.pca`` give for continuous covariates, on the values as stored (typically after ``normalize_log1p_inplace``).

Not in the reference.  The definition is in include/srx.h: an ordinary least-squares fit with an intercept per gene, the residuals
divided by their standard deviation (``ddof 1``), clipped on both sides.  The dense n x k matrix exists a chunk of cells at a time
on the device; the scores stay resident as the handle's PCA result.  Departures from scanpy: no categorical regressor, no
``zero_center=False``, a constant or collinear covariate is refused where statsmodels takes a pseudo-inverse.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import DeviceCsr, IMAnnData
from ._common import flat_info


def _matrix(x) -> DeviceCsr:
    return x.x() if isinstance(x, IMAnnData) else x


def _covariates(adata, covariates, n_obs: int) -> np.ndarray:
    """n_obs x p f64, C order: None (p = 0), an array (n_obs or n_obs x p), or the names of ``adata.obs`` columns."""
    if covariates is None:
        return np.zeros((n_obs, 0), dtype=np.float64)
    if isinstance(covariates, str):
        covariates = [covariates]
    if isinstance(covariates, (list, tuple)) and covariates and all(isinstance(c, str) for c in covariates):
        if not isinstance(adata, IMAnnData):
            raise ValueError("covariates named by obs key need an IMAnnData")
        covariates = np.stack([np.asarray(adata.obs[c], dtype=np.float64) for c in covariates], axis=1)
    c = np.asarray(covariates, dtype=np.float64)
    if c.ndim == 1:
        c = c.reshape(-1, 1) if c.size else c.reshape(n_obs, 0)
    if c.ndim != 2 or c.shape[0] != n_obs:
        raise ValueError("covariates must hold one row per cell (%d), not %r" % (n_obs, c.shape))
    return np.ascontiguousarray(c)


def _genes(m, genes) -> np.ndarray:
    if genes is None:
        return np.arange(int(m.info().n_cols), dtype=np.uint64)
    return np.ascontiguousarray(genes, dtype=np.uint64).ravel()


def _opts(scale, max_value, chunk_cells=0, n_components=-1, max_iter=0, tol=0.0, seed=0, solver=0) -> F.RegressOpts:
    # the option struct reads max_value 0 as "no clip"; None means the same here
    pca = F.PcaOpts(int(n_components), -1, 0, -1, 0, int(max_iter), int(solver), float(tol), int(seed))
    return F.RegressOpts(int(bool(scale)), 0, 0.0 if max_value is None else float(max_value), int(chunk_cells), pca)


def _info(i) -> dict:
    out = {n: getattr(i, n) for n, _ in i._fields_ if n != "pca"}
    out.update(flat_info(i.pca))
    return out


def _cov_ptr(c):
    return F.ptr(c) if c.size else None


def regress_fit(adata, covariates, genes=None, scale=True, max_value=None, chunk_cells=0):
    """(beta p x k, xbar k, s k, info dict): the per-gene least-squares coefficients on the CENTRED covariates, the gene means
    and the standard deviation of the residuals (ones with ``scale=False``): ``srx_regress_fit``."""
    m = _matrix(adata)
    g = _genes(m, genes)
    c = _covariates(adata, covariates, int(m.info().n_rows))
    p, k = c.shape[1], g.size
    beta, xbar, sd = np.zeros((p, k), dtype=np.float64), np.zeros(k, dtype=np.float64), np.zeros(k, dtype=np.float64)
    o, i = _opts(scale, max_value, chunk_cells), F.RegressInfo()
    F.check(F.lib().srx_regress_fit(m.handle, F.ptr(g) if k else None, k, _cov_ptr(c), p, C.byref(o), F.ptr(beta) if beta.size else None,
                                    F.ptr(xbar) if k else None, F.ptr(sd) if k else None, C.byref(i)), m.ctx.handle)
    return beta, xbar, sd, _info(i)


def regress_out(adata, covariates, genes=None, scale=False, max_value=None, chunk_cells=0) -> np.ndarray:
    """The residuals (n_obs x len(genes), f64) of the listed genes after the covariates are regressed out, optionally scaled and
    clipped: ``srx_regress_residuals``.  A gene whose values are all equal gives a column of zeros."""
    m = _matrix(adata)
    g = _genes(m, genes)
    n = int(m.info().n_rows)
    c = _covariates(adata, covariates, n)
    out = np.zeros((n, g.size), dtype=np.float64)
    dst = out if out.size else np.zeros(1)
    o = _opts(scale, max_value, chunk_cells)
    F.check(F.lib().srx_regress_residuals(m.handle, F.ptr(g) if g.size else None, g.size, _cov_ptr(c), c.shape[1], C.byref(o), F.ptr(dst),
                                          None), m.ctx.handle)
    return out


def scale(adata, genes=None, max_value=None, chunk_cells=0) -> np.ndarray:
    """``sc.pp.scale(adata, max_value=...)`` of the listed genes as a dense block: ``regress_out`` without covariates."""
    return regress_out(adata, None, genes, True, max_value, chunk_cells)


def regress_gram(adata, covariates, genes=None, scale=True, max_value=None, chunk_cells=0):
    """(Z^T Z (k x k), column sums of Z (k), info dict) of the regressed, scaled and clipped values Z: ``srx_regress_gram``, the
    kernel-level entry of ``pca_regress_scale``."""
    m = _matrix(adata)
    g = _genes(m, genes)
    c = _covariates(adata, covariates, int(m.info().n_rows))
    gram, colsum = np.zeros((g.size, g.size), dtype=np.float64), np.zeros(g.size, dtype=np.float64)
    o, i = _opts(scale, max_value, chunk_cells), F.RegressInfo()
    F.check(F.lib().srx_regress_gram(m.handle, F.ptr(g) if g.size else None, g.size, _cov_ptr(c), c.shape[1], C.byref(o),
                                     F.ptr(gram) if gram.size else None, F.ptr(colsum) if g.size else None, C.byref(i)), m.ctx.handle)
    return gram, colsum, _info(i)


def pca_regress_scale(adata, covariates=None, genes=None, n_top_genes=2000, n_components=50, scale=True, max_value=10.0, chunk_cells=0,
                      max_iter=0, tol=0.0, seed=0, solver=0) -> dict:
    """``regress_out`` -> ``scale(max_value)`` -> ``pca`` of ``genes`` on the values as stored (``srx_pca_regress``).  ``genes``
    None: the ``n_top_genes`` of ``srx_select_hvg`` are selected first.  ``covariates``: None (plain scale + clip), an
    ``n_obs x p`` array, or names of ``adata.obs`` columns.  The scores stay resident as the handle's PCA result (``neighbors``,
    ``harmony_integrate``, ... read them there); an ``IMAnnData`` also receives ``obsm["X_pca"]`` and ``uns["pca"]``.  Returns
    the info dict with the arrays.  No ``PcaModel`` can be made of this result."""
    m = _matrix(adata)
    mi = m.info()
    n = int(mi.n_rows)
    if genes is None:
        want = min(int(n_top_genes), int(mi.n_cols))
        idx, n_out = np.zeros(max(want, 1), dtype=np.uint64), C.c_uint64(0)
        F.check(F.lib().srx_select_hvg(m.handle, want, F.ptr(idx), C.byref(n_out)), m.ctx.handle)
        genes = idx[:int(n_out.value)].copy()
    g = np.ascontiguousarray(genes, dtype=np.uint64).ravel()
    c = _covariates(adata, covariates, n)
    k = g.size
    n_pc = max(min(2 if int(n_components) < 0 else int(n_components), k), 0)
    scores, comps = np.zeros((n, n_pc), dtype=np.float64), np.zeros((k, n_pc), dtype=np.float64)
    evr, mean, sd = np.zeros(n_pc, dtype=np.float64), np.zeros(k, dtype=np.float64), np.zeros(k, dtype=np.float64)
    o, i = _opts(scale, max_value, chunk_cells, n_components, max_iter, tol, seed, solver), F.RegressInfo()
    F.check(F.lib().srx_pca_regress(m.handle, F.ptr(g) if k else None, k, _cov_ptr(c), c.shape[1], C.byref(o),
                                    F.ptr(scores) if scores.size else None, F.ptr(comps) if comps.size else None, F.ptr(evr) if n_pc else None,
                                    F.ptr(mean) if k else None, F.ptr(sd) if k else None, C.byref(i)), m.ctx.handle)
    info = _info(i)
    if isinstance(adata, IMAnnData):
        adata.obsm["X_pca"] = scores
        adata.uns["pca"] = {"components": comps, "explained_variance_ratio": evr, "mean": mean, "std": sd, "selected_features": g,
                            "n_iter": info["n_iter"], "residual": info["residual"], "solver": info["solver"], "center": True,
                            "scale": bool(scale), "residuals": "regress", "max_value": max_value, "n_covariates": int(c.shape[1])}
    return dict(info, scores=scores, components=comps, explained_variance_ratio=evr, mean=mean, std=sd, selected_features=g)

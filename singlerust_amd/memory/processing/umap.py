"""UMAP layout of the neighbour graph over libsrx_hip (``srx_umap`` / ``srx_umap_csr``): what fills ``obsm["X_umap"]``.

Not in the reference.  The method (umap-learn's ``optimize_layout_euclidean`` restated as a synchronous, vertex-owned
iteration that is bit-identical from call to call) is defined in include/srx.h; every epoch runs on the device and nothing
computes on the CPU except the two-parameter curve fit ``fit_ab``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import IMAnnData
from ._common import csr_triple, flat_info, graph_of

_INITS = {"pca": F.UMAP_INIT_PCA, "random": F.UMAP_INIT_RANDOM}


def fit_ab(spread: float = 1.0, min_dist: float = 0.5):
    """(a, b) of the curve 1 / (1 + a x^(2b)) fitted to the membership of (spread, min_dist): ``srx_umap_fit_ab``, host only."""
    a, b = C.c_double(), C.c_double()
    F.check(F.lib().srx_umap_fit_ab(float(spread), float(min_dist), C.byref(a), C.byref(b)), None)
    return a.value, b.value


def _start(init, n: int, dim: int):
    """(init code, the start as an n x dim f64 array or None)."""
    if isinstance(init, str):
        if init not in _INITS:
            raise ValueError("umap: init is 'pca', 'random' or an n x n_components array")
        return _INITS[init], None
    y0 = np.ascontiguousarray(init, dtype=np.float64)
    if y0.shape != (n, dim):
        raise ValueError("umap: the start must be n x n_components = %d x %d" % (n, dim))
    return F.UMAP_INIT_GIVEN, y0


def _opts(min_dist, spread, n_components, n_epochs, alpha, gamma, negative_sample_rate, init_code, seed, a, b, stop_after) -> F.UmapOpts:
    return F.UmapOpts(float(a), float(b), float(min_dist), float(spread), float(gamma), float(alpha), int(seed) & (2 ** 64 - 1),
                      int(n_epochs), int(stop_after), int(n_components), int(negative_sample_rate), int(init_code), 0)


def umap(adata: IMAnnData, min_dist: float = 0.5, spread: float = 1.0, n_components: int = 2, n_epochs: int = 0, alpha: float = 1.0,
         gamma: float = 1.0, negative_sample_rate: int = 5, init="pca", seed: int = 0, key_added: str = "X_umap",
         a: float = 0.0, b: float = 0.0, stop_after: int = 0) -> dict:
    """Layout of the connectivities that ``neighbors(adata, connectivities=True)`` left on the device (no host round trip).
    ``init``: "pca" (the scores the last fit left on the device, scaled to +-10), "random" (hashed from ``seed``) or an
    n x n_components array.  ``n_epochs=0``: 500 for n <= 10 000, else 200; ``a = b = 0``: fitted from (spread, min_dist).
    Writes ``adata.obsm[key_added]`` (n x n_components f64) and ``adata.uns["umap"]`` (``params`` and the call's
    ``srx_umap_info`` under ``info``); returns the info."""
    g = graph_of(adata, "umap")
    n, dim = adata.n_obs(), int(n_components)
    code, y0 = _start(init, n, dim)
    emb = np.zeros((n, max(dim, 0)), dtype=np.float64)
    info = F.UmapInfo()
    opts = _opts(min_dist, spread, dim, n_epochs, alpha, gamma, negative_sample_rate, code, seed, a, b, stop_after)
    F.check(F.lib().srx_umap(g.handle, adata.x().handle if code == F.UMAP_INIT_PCA else None, C.byref(opts),
                             F.ptr(y0) if y0 is not None and y0.size else None, F.ptr(emb) if emb.size else None, C.byref(info)),
            g.ctx.handle)
    adata.obsm[key_added] = emb
    d = flat_info(info)
    adata.uns["umap"] = {"params": {"a": d["a"], "b": d["b"], "min_dist": float(min_dist), "spread": float(spread),
                                    "n_components": dim, "n_epochs": d["n_epochs"], "alpha": float(alpha), "gamma": float(gamma),
                                    "negative_sample_rate": int(negative_sample_rate),
                                    "init": init if isinstance(init, str) else "given", "seed": int(seed)}, "info": d}
    return d


def graph_embedding(graph) -> np.ndarray:
    """The embedding the last ``srx_umap`` left with a ``Graph`` handle (``srx_graph_embedding_fetch``)."""
    dim = C.c_uint32()
    F.check(F.lib().srx_graph_embedding_fetch(graph.handle, None, C.byref(dim)), graph.ctx.handle)
    out = np.zeros((graph.info()["n"], dim.value), dtype=np.float64)
    F.check(F.lib().srx_graph_embedding_fetch(graph.handle, F.ptr(out) if out.size else None, None), graph.ctx.handle)
    return out


def umap_csr(ctx, matrix, min_dist: float = 0.5, spread: float = 1.0, n_components: int = 2, n_epochs: int = 0, alpha: float = 1.0,
             gamma: float = 1.0, negative_sample_rate: int = 5, init="random", seed: int = 0, a: float = 0.0, b: float = 0.0,
             stop_after: int = 0):
    """Layout of any symmetric weighted graph: a scipy sparse matrix or an (indptr, indices, data) CSR triple with ascending
    columns, positive weights and no diagonal (``srx_umap_csr`` validates on the device as ``srx_louvain_csr`` does).
    ``init``: "random" or an n x n_components array.  Returns (embedding n x n_components f64, info dict)."""
    indptr, indices, data = csr_triple(matrix, "umap_csr")
    n, dim = indptr.size - 1, int(n_components)
    code, y0 = _start(init, n, dim)
    emb = np.zeros((n, max(dim, 0)), dtype=np.float64)
    info = F.UmapInfo()
    opts = _opts(min_dist, spread, dim, n_epochs, alpha, gamma, negative_sample_rate, code, seed, a, b, stop_after)
    F.check(F.lib().srx_umap_csr(ctx.handle, F.ptr(indptr), F.ptr(indices) if indices.size else None,
                                 F.ptr(data) if data.size else None, n, C.byref(opts),
                                 F.ptr(y0) if y0 is not None and y0.size else None, F.ptr(emb) if emb.size else None,
                                 C.byref(info)), ctx.handle)
    return emb, flat_info(info)

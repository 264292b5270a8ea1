"""Exact k-nearest-neighbour graph of the cells over libsrx_hip (``srx_knn_result`` / ``srx_knn_points``).

Not in the reference: it is the step that consumes ``obsm["X_pca"]`` and stands in front of what the reference's
commented-out ``tsne`` / ``tsne_inplace`` (dim_red/mod.rs:159-227) would build from the scores.  Euclidean distance in
f64, every row ascending by (distance, index); nothing computes on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import IMAnnData


def _info_dict(info: F.KnnInfo) -> dict:
    return {"n_ref": int(info.n_ref), "n_query": int(info.n_query), "d": int(info.d), "k": int(info.k),
            "n_candidates": int(info.n_candidates), "rows_certified": int(info.rows_certified),
            "rows_recomputed": int(info.rows_recomputed)}


def neighbors(adata: IMAnnData, n_neighbors: int = 15, n_pcs=None, include_self: bool = False) -> dict:
    """Self graph of the cells in the space of the scores the last ``pca_inplace`` left on the device (no host round trip).
    Stores ``obsm["knn_indices"]`` (uint32, n_obs x k), ``obsm["knn_distances"]`` (f64) and ``uns["neighbors"]``
    (the parameters and the call's ``srx_knn_info``); returns the latter.  ``n_pcs``: use the leading PCs only."""
    n = adata.n_obs()
    k = int(n_neighbors)
    opts = F.KnnOpts(k, int(n_pcs or 0), int(bool(include_self)), 0)
    info = F.KnnInfo()
    idx = np.zeros((n, max(k, 0)), dtype=np.uint32)
    dist = np.zeros((n, max(k, 0)), dtype=np.float64)
    F.check(F.lib().srx_knn_result(adata.x().handle, C.byref(opts), F.ptr(idx) if idx.size else None,
                                   F.ptr(dist) if dist.size else None, C.byref(info)), adata.x().ctx.handle)
    adata.obsm["knn_indices"] = idx
    adata.obsm["knn_distances"] = dist
    adata.uns["neighbors"] = {"params": {"n_neighbors": k, "n_pcs": None if n_pcs is None else int(n_pcs),
                                         "include_self": bool(include_self), "metric": "euclidean"},
                              "info": _info_dict(info)}
    return adata.uns["neighbors"]


def knn_points(ctx, ref, query=None, k: int = 15, n_dims=None, include_self: bool = False):
    """Neighbours of every row of ``query`` among the rows of ``ref`` (n x d f64 arrays; ``query`` None: the self graph of
    ``ref``).  Returns (indices uint32 n_query x k, distances f64, info dict)."""
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    if ref.ndim != 2:
        raise ValueError("ref must be n x d")
    if query is not None:
        query = np.ascontiguousarray(query, dtype=np.float64)
        if query.ndim != 2 or query.shape[1] != ref.shape[1]:
            raise ValueError("query must be n_query x d with the d of ref")
    nq = ref.shape[0] if query is None else query.shape[0]
    k = int(k)
    opts = F.KnnOpts(k, int(n_dims or 0), int(bool(include_self)), 0)
    info = F.KnnInfo()
    idx = np.zeros((nq, max(k, 0)), dtype=np.uint32)
    dist = np.zeros((nq, max(k, 0)), dtype=np.float64)
    F.check(F.lib().srx_knn_points(ctx.handle, F.ptr(ref) if ref.size else None, ref.shape[0],
                                   None if query is None else C.c_void_p(query.ctypes.data if nq else ref.ctypes.data or 1), nq, ref.shape[1], C.byref(opts),
                                   F.ptr(idx) if idx.size else None, F.ptr(dist) if dist.size else None, C.byref(info)),
            ctx.handle)
    return idx, dist, _info_dict(info)

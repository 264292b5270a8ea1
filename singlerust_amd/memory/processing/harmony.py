"""Harmony batch integration over libsrx_hip (``srx_harmony_result`` / ``srx_harmony_points``): what fills
``obsm["X_pca_harmony"]`` between the PCA and the neighbour graph.

Not in the reference.  The method (soft k-means on the cosine-normalised scores with a batch-diversity penalty, then a ridge
correction per cluster, repeated) is defined in include/srx.h; nothing computes on the CPU except the bookkeeping of the
labels and the stopping rules.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import IMAnnData
from ._common import OwnedHandle

_TABLES = {"corrected": F.HARMONY_CORRECTED, "R": F.HARMONY_R, "centroids": F.HARMONY_CENTROIDS,
           "observed": F.HARMONY_OBSERVED, "expected": F.HARMONY_EXPECTED}


def _info_dict(i: F.HarmonyInfo) -> dict:
    r = int(i.rounds)
    return {"n": int(i.n), "d": int(i.d), "n_batches": int(i.n_batches), "n_clusters": int(i.n_clusters),
            "n_blocks": int(i.n_blocks), "rounds": r, "converged": int(i.converged), "cluster_iters": int(i.cluster_iters),
            "round_iters": [int(i.round_iters[k]) for k in range(r)],
            "round_objective": [float(i.round_objective[k]) for k in range(r)], "ms": float(i.ms)}


def _opts(theta=2.0, sigma=0.1, lambda_=1.0, epsilon_cluster=1e-5, epsilon_harmony=1e-4, seed=0, n_clusters=0, n_blocks=0,
          max_rounds=0, max_cluster_iters=0, init_iters=0, n_dims=0) -> F.HarmonyOpts:
    return F.HarmonyOpts(float(theta), float(sigma), float(lambda_), float(epsilon_cluster), float(epsilon_harmony),
                         int(seed) & (2 ** 64 - 1), int(n_clusters), int(n_blocks), int(max_rounds), int(max_cluster_iters),
                         int(init_iters), int(n_dims or 0))


def encode_batches(labels):
    """(codes uint32, categories) of any label array: the categories in sorted order, as ``np.unique`` gives them."""
    cats, codes = np.unique(np.asarray(labels), return_inverse=True)
    return np.ascontiguousarray(codes, dtype=np.uint32), cats


class Harmony(OwnedHandle):
    """Owning wrapper of an ``srx_harmony``: the corrected block, R, the centroids, O and E on the device."""

    _free = "srx_harmony_free"

    def info(self) -> dict:
        i = F.HarmonyInfo()
        F.check(F.lib().srx_harmony_info_get(self._h, C.byref(i)), self.ctx.handle)
        return _info_dict(i)

    def fetch(self, which: str = "corrected") -> np.ndarray:
        """One table as f64: "corrected" (n x d), "R" (n x K), "centroids" (K x d), "observed" / "expected" (K x B)."""
        i = self.info()
        shape = {"corrected": (i["n"], i["d"]), "R": (i["n"], i["n_clusters"]), "centroids": (i["n_clusters"], i["d"]),
                 "observed": (i["n_clusters"], i["n_batches"]), "expected": (i["n_clusters"], i["n_batches"])}[which]
        if i["n"] == 0:
            shape = (0, shape[1]) if which in ("corrected", "R") else shape
        out = np.zeros(shape, dtype=np.float64)
        F.check(F.lib().srx_harmony_fetch(self._h, _TABLES[which], F.ptr(out) if out.size else None), self.ctx.handle)
        return out

    def knn(self, k: int = 15, n_dims=None, include_self: bool = False):
        """(indices uint32 n x k, distances f64, info dict) of the corrected block (``srx_knn_harmony``)."""
        from .neighbors import _info_dict as knn_info
        n = self.info()["n"]
        opts = F.KnnOpts(int(k), int(n_dims or 0), int(bool(include_self)), 0)
        info = F.KnnInfo()
        idx = np.zeros((n, max(int(k), 0)), dtype=np.uint32)
        dist = np.zeros((n, max(int(k), 0)), dtype=np.float64)
        F.check(F.lib().srx_knn_harmony(self._h, C.byref(opts), F.ptr(idx) if idx.size else None,
                                        F.ptr(dist) if dist.size else None, C.byref(info)), self.ctx.handle)
        return idx, dist, knn_info(info)

    def neighbors(self, k: int = 15, n_dims=None):
        """(Graph, knn info dict) of the corrected block (``srx_neighbors_harmony``)."""
        from .neighbors import Graph, _info_dict as knn_info
        opts = F.KnnOpts(int(k), int(n_dims or 0), 0, 0)
        info = F.KnnInfo()
        h = C.c_void_p()
        F.check(F.lib().srx_neighbors_harmony(self._h, C.byref(opts), C.byref(info), C.byref(h)), self.ctx.handle)
        return Graph(self.ctx, h), knn_info(info)


def harmony_points(ctx, points, batch, n_batches=None, **kw) -> Harmony:
    """Harmony on caller-supplied points (n x d f64) with integer labels ``batch`` (``n_batches``: the largest label + 1
    unless given).  Keyword arguments: the fields of ``srx_harmony_opts`` (``lambda_`` for lambda)."""
    points = np.ascontiguousarray(points, dtype=np.float64)
    batch = np.ascontiguousarray(batch, dtype=np.uint32)
    if points.ndim != 2 or batch.shape != (points.shape[0],):
        raise ValueError("harmony_points: points (n x d) and batch (n) expected")
    n, d = points.shape
    if n_batches is None:
        n_batches = int(batch.max()) + 1 if n else 1
    opts = _opts(**kw)
    h = C.c_void_p()
    F.check(F.lib().srx_harmony_points(ctx.handle, F.ptr(points) if points.size else None, n, d, F.ptr(batch) if n else None,
                                       int(n_batches), C.byref(opts), C.byref(h), None), ctx.handle)
    return Harmony(ctx, h)


def harmony_integrate(adata: IMAnnData, batch, adjusted_basis: str = "X_pca_harmony", **kw) -> dict:
    """Harmony on the scores the last ``pca_inplace`` left on the device (no host round trip).  ``batch``: one label per cell
    (any type; the sorted distinct values are the batches), or the name of a column of ``adata.obs``.  Writes
    ``adata.obsm[adjusted_basis]`` and ``adata.uns["harmony"]`` (the call's ``srx_harmony_info``), keeps the handle on the
    adata for ``neighbors(adata, use_rep=adjusted_basis)``, and returns the info."""
    if isinstance(batch, str):
        batch = adata.obs[batch]
    codes, cats = encode_batches(batch)
    if codes.shape != (adata.n_obs(),):
        raise ValueError("harmony_integrate: one batch label per cell expected")
    ctx = adata.x().ctx
    opts = _opts(**kw)
    h = C.c_void_p()
    F.check(F.lib().srx_harmony_result(adata.x().handle, F.ptr(codes) if codes.size else None, max(len(cats), 1),
                                       C.byref(opts), C.byref(h), None), ctx.handle)
    hm = Harmony(ctx, h)
    old = getattr(adata, "_harmony", None)
    if old is not None:
        old[1].free()
    adata._harmony = (adjusted_basis, hm)              # stays on the device for neighbors(use_rep=...)
    adata.obsm[adjusted_basis] = hm.fetch("corrected")
    adata.uns["harmony"] = dict(hm.info(), batches=list(cats))
    return adata.uns["harmony"]

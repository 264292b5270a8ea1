"""The shared-nearest-neighbour (SNN) graph of a k-NN list over libsrx_hip (``srx_snn_from_knn`` / ``srx_snn_graph``): what
Seurat's ``FindNeighbors``, PhenoGraph and scran's ``buildSNNGraph`` cluster.  Two cells are joined when their neighbour sets
overlap, the weight is the Jaccard index of the two sets (or the shared count), weak pairs are pruned; include/srx.h has the
definition.  Not in the reference, and not compared with Seurat, PhenoGraph or scran.

The result is an ordinary ``Graph``: ``louvain``, ``umap``, ``paga``, ``diffmap`` and ``gene_autocorr`` read its connectivities
where they lie, so nothing leaves the device between the PCA and the labels.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import IMAnnData
from ._common import flat_info
from .neighbors import Graph

_WEIGHTS = {"jaccard": F.SNN_JACCARD, "number": F.SNN_NUMBER}
_PAIRS = {"shared": F.SNN_PAIRS_SHARED, "knn": F.SNN_PAIRS_KNN}


def _opts(prune, weight, pairs, include_self) -> F.SnnOpts:
    w = _WEIGHTS.get(weight, weight) if isinstance(weight, str) else weight
    p = _PAIRS.get(pairs, pairs) if isinstance(pairs, str) else pairs
    if isinstance(w, str):
        raise ValueError(f"weight = {weight!r} is neither 'jaccard' nor 'number'")
    if isinstance(p, str):
        raise ValueError(f"pairs = {pairs!r} is neither 'shared' nor 'knn'")
    return F.SnnOpts(int(w), int(p), int(bool(include_self)), 0, float(prune))


def snn_min_shared(k: int, include_self: bool = True, prune: float = 1.0 / 15.0) -> int:
    """The smallest shared count whose Jaccard index reaches ``prune`` (``srx_snn_min_shared``; host code, no GPU)."""
    out = C.c_uint32(0)
    F.check(F.lib().srx_snn_min_shared(int(k), int(bool(include_self)), float(prune), C.byref(out)), None)
    return int(out.value)


def snn_graph(graph_or_knn, prune: float = 1.0 / 15.0, weight="jaccard", pairs="shared", include_self: bool = True,
              ctx=None, distances=None) -> Graph:
    """The SNN graph as a new ``Graph``; its ``snn_info`` attribute holds the call's ``srx_snn_info`` as a dict.

    ``graph_or_knn``: a ``Graph`` (the list it holds on the device is read where it lies: ``srx_snn_graph``), or an n x k
    array of neighbour indices with ``ctx`` (``srx_snn_from_knn``; ``distances``, n x k, only ride along into the result's
    distances).  ``weight``: ``"jaccard"`` or ``"number"``; ``pairs``: ``"shared"`` (Seurat) or ``"knn"`` (PhenoGraph: only
    pairs joined by the list)."""
    opts = _opts(prune, weight, pairs, include_self)
    info = F.SnnInfo()
    h = C.c_void_p()
    if isinstance(graph_or_knn, Graph):
        ctx = graph_or_knn.ctx
        F.check(F.lib().srx_snn_graph(graph_or_knn.handle, C.byref(opts), C.byref(info), C.byref(h)), ctx.handle)
    else:
        if ctx is None:
            raise ValueError("snn_graph: a k-NN list needs ctx")
        idx = np.ascontiguousarray(graph_or_knn, dtype=np.uint32)
        if idx.ndim != 2:
            raise ValueError("the k-NN list must be n x k")
        dist = None
        if distances is not None:
            dist = np.ascontiguousarray(distances, dtype=np.float64)
            if dist.shape != idx.shape:
                raise ValueError("indices and distances must both be n x k")
        n, k = idx.shape
        F.check(F.lib().srx_snn_from_knn(ctx.handle, F.ptr(idx) if idx.size else None,
                                         F.ptr(dist) if dist is not None and dist.size else None, n, k, C.byref(opts),
                                         C.byref(info), C.byref(h)), ctx.handle)
    g = Graph(ctx, h)
    g.snn_info = flat_info(info)
    return g


def neighbors_snn(adata: IMAnnData, n_neighbors: int = 20, n_pcs=None, prune: float = 1.0 / 15.0, weight="jaccard",
                  pairs="shared", include_self: bool = True, use_rep=None) -> dict:
    """Seurat's ``FindNeighbors`` on the scores the last ``pca_inplace`` left on the device: the exact k-NN list, then its SNN
    graph, with no host round trip in between.  ``n_neighbors`` is Seurat's ``k.param``, which counts the cell itself, so the
    list has ``k = n_neighbors - 1`` entries per row.  The handle kept on the adata (what ``louvain``, ``umap``, ``paga`` read)
    is the SNN graph; ``obsp["connectivities"]`` is its matrix, ``obsp["distances"]`` the k-NN list's."""
    from .neighbors import _harmony_handle

    k = int(n_neighbors) - 1
    ctx = adata.x().ctx
    kopts = F.KnnOpts(k, int(n_pcs or 0), 0, 0)
    kinfo = F.KnnInfo()
    h = C.c_void_p()
    if use_rep is None:
        F.check(F.lib().srx_neighbors_result(adata.x().handle, C.byref(kopts), C.byref(kinfo), C.byref(h)), ctx.handle)
    else:
        F.check(F.lib().srx_neighbors_harmony(_harmony_handle(adata, use_rep).handle, C.byref(kopts), C.byref(kinfo), C.byref(h)),
                ctx.handle)
    src = Graph(ctx, h)
    try:
        g = snn_graph(src, prune, weight, pairs, include_self)
    finally:
        src.free()
    old = getattr(adata, "_graph", None)
    if old is not None:
        old.free()
    adata._graph = g
    adata.obsp["distances"] = g.matrix(F.GRAPH_DISTANCES)
    adata.obsp["connectivities"] = g.matrix(F.GRAPH_CONNECTIVITIES)
    adata.uns["neighbors"] = {"params": {"n_neighbors": int(n_neighbors), "n_pcs": None if n_pcs is None else int(n_pcs),
                                         "include_self": False, "metric": "euclidean", "method": "snn", "prune": float(prune),
                                         "weight": weight, "pairs": pairs, "snn_include_self": bool(include_self)},
                              "info": flat_info(kinfo), "graph": g.info(), "snn": g.snn_info}
    if use_rep is not None:
        adata.uns["neighbors"]["params"]["use_rep"] = use_rep
    return adata.uns["neighbors"]

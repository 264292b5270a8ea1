"""Exact k-nearest-neighbour graph of the cells over libsrx_hip (``srx_knn_result`` / ``srx_knn_points``) and the weighted
graph built from it (``srx_neighbors_result`` / ``srx_neighbors_from_knn``: ``obsp["distances"]``, ``obsp["connectivities"]``);
the batch-balanced form of both (``bbknn`` / ``bbknn_points``: ``srx_bbknn_*``) and the trimming of a graph (``Graph.trim``).

Not in the reference: it is the step that consumes ``obsm["X_pca"]`` and stands in front of what the reference's
commented-out ``tsne`` / ``tsne_inplace`` (dim_red/mod.rs:159-227) would build from the scores.  Euclidean distance in
f64, every row ascending by (distance, index); nothing computes on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import IMAnnData
from ._common import OwnedHandle, flat_info


def _info_dict(info: F.KnnInfo) -> dict:
    return {"n_ref": int(info.n_ref), "n_query": int(info.n_query), "d": int(info.d), "k": int(info.k),
            "n_candidates": int(info.n_candidates), "rows_certified": int(info.rows_certified),
            "rows_recomputed": int(info.rows_recomputed)}


def _trim_dict(info: F.TrimInfo) -> dict:
    return {name: getattr(info, name) for name, _ in info._fields_ if name != "reserved_"}


def _bbknn_dict(info: F.BbknnInfo) -> dict:
    d = {name: getattr(info, name) for name, _ in info._fields_ if name not in ("reserved_", "trim")}
    d["trim"] = _trim_dict(info.trim)
    return d


class Graph(OwnedHandle):
    """Owning wrapper of an ``srx_graph``: distances and connectivities as CSR on the device, with rho and sigma."""

    _free = "srx_graph_free"

    def info(self) -> dict:
        i = F.GraphInfo()
        F.check(F.lib().srx_graph_info_get(self._h, C.byref(i)), self.ctx.handle)
        return flat_info(i)

    def fetch(self, which: int):
        """(indptr uint64 n + 1, indices uint32, data f64) of ``F.GRAPH_DISTANCES`` or ``F.GRAPH_CONNECTIVITIES``."""
        i = self.info()
        nnz = i["nnz_connectivities"] if which == F.GRAPH_CONNECTIVITIES else i["nnz_distances"]
        indptr = np.zeros(i["n"] + 1, dtype=np.uint64)
        indices = np.zeros(nnz, dtype=np.uint32)
        data = np.zeros(nnz, dtype=np.float64)
        F.check(F.lib().srx_graph_fetch(self._h, int(which), F.ptr(indptr), F.ptr(indices) if nnz else None,
                                        F.ptr(data) if nnz else None), self.ctx.handle)
        return indptr, indices, data

    def scales(self):
        """(rho, sigma), one f64 per cell."""
        n = self.info()["n"]
        rho, sigma = np.zeros(n), np.zeros(n)
        F.check(F.lib().srx_graph_fetch_scales(self._h, F.ptr(rho) if n else None, F.ptr(sigma) if n else None), self.ctx.handle)
        return rho, sigma

    def matrix(self, which: int):
        """The matrix as ``scipy.sparse.csr_matrix`` where scipy imports, else the CSR triple of ``fetch``."""
        indptr, indices, data = self.fetch(which)
        try:
            import scipy.sparse as sp
        except ImportError:
            return indptr, indices, data
        n = len(indptr) - 1
        return sp.csr_matrix((data, indices.astype(np.int64 if n >= 2 ** 31 else np.int32), indptr.astype(np.int64)), shape=(n, n))

    def trim(self, trim: int) -> "Graph":
        """BBKNN's trimming of the connectivities (``srx_graph_trim``) as a new ``Graph``; this one stays as it is.  Per row
        the ``trim``-th largest value is the row's threshold (0 for a row of at most ``trim`` entries); an entry stays when it
        reaches the thresholds of both its row and its column.  ``trim_info`` on the result holds the ``srx_trim_info``."""
        info = F.TrimInfo()
        h = C.c_void_p()
        F.check(F.lib().srx_graph_trim(self._h, int(trim), C.byref(info), C.byref(h)), self.ctx.handle)
        g = Graph(self.ctx, h)
        g.trim_info = _trim_dict(info)
        return g


def connectivities_from_knn(ctx, indices, distances) -> Graph:
    """The graph of a k-NN list (n x k; no row names itself): see ``srx_neighbors_from_knn``."""
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    distances = np.ascontiguousarray(distances, dtype=np.float64)
    if indices.ndim != 2 or indices.shape != distances.shape:
        raise ValueError("indices and distances must both be n x k")
    n, k = indices.shape
    h = C.c_void_p()
    F.check(F.lib().srx_neighbors_from_knn(ctx.handle, F.ptr(indices) if indices.size else None,
                                           F.ptr(distances) if distances.size else None, n, k, C.byref(h)), ctx.handle)
    return Graph(ctx, h)


def _harmony_handle(adata: IMAnnData, use_rep: str):
    """The ``Harmony`` handle that ``harmony_integrate`` kept on the adata under the basis ``use_rep``."""
    kept = getattr(adata, "_harmony", None)
    if kept is None or kept[0] != use_rep or not kept[1].handle:
        raise F.SrxError(F.E_ARG, f"neighbors: use_rep={use_rep!r} names no representation on the device; run "
                                  f"harmony_integrate(adata, batch, adjusted_basis={use_rep!r}) first")
    return kept[1]


def _neighbors_graph(adata: IMAnnData, k: int, n_pcs, knn_lists: bool, use_rep=None) -> dict:
    ctx = adata.x().ctx
    opts = F.KnnOpts(k, int(n_pcs or 0), 0, 0)
    info = F.KnnInfo()
    h = C.c_void_p()
    if use_rep is None:
        F.check(F.lib().srx_neighbors_result(adata.x().handle, C.byref(opts), C.byref(info), C.byref(h)), ctx.handle)
    else:
        F.check(F.lib().srx_neighbors_harmony(_harmony_handle(adata, use_rep).handle, C.byref(opts), C.byref(info), C.byref(h)),
                ctx.handle)
    g = Graph(ctx, h)
    old = getattr(adata, "_graph", None)
    if old is not None:
        old.free()
    adata._graph = g                     # stays on the device for the consumers of the graph
    adata.obsp["distances"] = g.matrix(F.GRAPH_DISTANCES)
    adata.obsp["connectivities"] = g.matrix(F.GRAPH_CONNECTIVITIES)
    if knn_lists:                        # the rows of D, ascending by (distance, index) as srx_knn_result orders them
        indptr, indices, data = g.fetch(F.GRAPH_DISTANCES)
        idx, dist = indices.reshape(-1, k), data.reshape(-1, k)
        order = np.lexsort((idx, dist), axis=1)
        adata.obsm["knn_indices"] = np.take_along_axis(idx, order, axis=1)
        adata.obsm["knn_distances"] = np.take_along_axis(dist, order, axis=1)
    adata.uns["neighbors"] = {"params": {"n_neighbors": k, "n_pcs": None if n_pcs is None else int(n_pcs),
                                         "include_self": False, "metric": "euclidean", "method": "umap"},
                              "info": _info_dict(info), "graph": g.info()}
    if use_rep is not None:
        adata.uns["neighbors"]["params"]["use_rep"] = use_rep
    return adata.uns["neighbors"]


def neighbors(adata: IMAnnData, n_neighbors: int = 15, n_pcs=None, include_self: bool = False,
              connectivities: bool = False, knn_lists: bool = False, use_rep=None) -> dict:
    """Self graph of the cells in the space of the scores the last ``pca_inplace`` left on the device (no host round trip).
    Stores ``obsm["knn_indices"]`` (uint32, n_obs x k), ``obsm["knn_distances"]`` (f64) and ``uns["neighbors"]``
    (the parameters and the call's ``srx_knn_info``); returns the latter.  ``n_pcs``: use the leading PCs only.

    ``connectivities=True`` builds the weighted graph on the device instead (``srx_neighbors_result``; ``include_self`` must
    be False): ``obsp["distances"]`` and ``obsp["connectivities"]`` (scipy CSR, or (indptr, indices, data) without scipy),
    ``uns["neighbors"]["graph"]`` (the ``srx_graph_info``), the device handle kept on the adata; ``obsm["knn_*"]`` are
    filled from the rows of the distances only with ``knn_lists=True``.

    ``use_rep``: the ``adjusted_basis`` of a ``harmony_integrate`` on this adata (``"X_pca_harmony"``): the search reads the
    corrected scores that call left on the device (``srx_knn_harmony`` / ``srx_neighbors_harmony``) instead of the PCA's."""
    n = adata.n_obs()
    k = int(n_neighbors)
    if connectivities:
        if include_self:
            raise F.SrxError(F.E_ARG, "neighbors: the graph is built from a list that excludes self (include_self=False)")
        return _neighbors_graph(adata, k, n_pcs, knn_lists, use_rep)
    opts = F.KnnOpts(k, int(n_pcs or 0), int(bool(include_self)), 0)
    info = F.KnnInfo()
    idx = np.zeros((n, max(k, 0)), dtype=np.uint32)
    dist = np.zeros((n, max(k, 0)), dtype=np.float64)
    if use_rep is None:
        F.check(F.lib().srx_knn_result(adata.x().handle, C.byref(opts), F.ptr(idx) if idx.size else None,
                                       F.ptr(dist) if dist.size else None, C.byref(info)), adata.x().ctx.handle)
    else:
        F.check(F.lib().srx_knn_harmony(_harmony_handle(adata, use_rep).handle, C.byref(opts), F.ptr(idx) if idx.size else None,
                                        F.ptr(dist) if dist.size else None, C.byref(info)), adata.x().ctx.handle)
    adata.obsm["knn_indices"] = idx
    adata.obsm["knn_distances"] = dist
    adata.uns["neighbors"] = {"params": {"n_neighbors": k, "n_pcs": None if n_pcs is None else int(n_pcs),
                                         "include_self": bool(include_self), "metric": "euclidean"},
                              "info": _info_dict(info)}
    if use_rep is not None:
        adata.uns["neighbors"]["params"]["use_rep"] = use_rep
    return adata.uns["neighbors"]


def _bbknn_opts(neighbors_within_batch, n_pcs, trim) -> F.BbknnOpts:
    return F.BbknnOpts(int(neighbors_within_batch), int(n_pcs or 0), -1 if trim is None else int(trim))


def _batch_labels(batch, n: int):
    """(labels uint32 n, n_batches) of integer labels 0 .. B - 1 (``None``: one batch)."""
    if batch is None:
        return None, 1
    b = np.asarray(batch)
    if b.ndim != 1 or b.shape[0] != n or b.dtype.kind not in "iu":
        raise ValueError("batch must be one integer label per point")
    if n and int(b.min()) < 0:
        raise ValueError("batch labels must not be negative")
    return np.ascontiguousarray(b, dtype=np.uint32), int(b.max()) + 1 if n else 1


def bbknn_points(ctx, points, batch, neighbors_within_batch: int = 3, n_dims=None, trim=None, n_batches=None, graph: bool = True):
    """Batch-balanced neighbours of caller-supplied points (n x d f64; ``srx_bbknn_points``): every row takes
    ``neighbors_within_batch`` neighbours from each batch (one fewer from its own, the point itself being left out).
    ``batch``: integer labels 0 .. B - 1; ``trim``: None = 10 * neighbors_within_batch * B, 0 = none.
    Returns (indices uint32 n x K, distances f64 n x K, ``Graph`` or None, info dict) with K = neighbors_within_batch * B - 1."""
    points = np.ascontiguousarray(points, dtype=np.float64)
    if points.ndim != 2:
        raise ValueError("points must be n x d")
    n, d = points.shape
    labels, B = _batch_labels(batch, n)
    if n_batches is not None:
        B = int(n_batches)
    opts = _bbknn_opts(neighbors_within_batch, n_dims, trim)
    kw = int(neighbors_within_batch) or 3
    K = max(kw * B - 1, 0)
    idx = np.zeros((n, K), dtype=np.uint32)
    dist = np.zeros((n, K), dtype=np.float64)
    info = F.BbknnInfo()
    h = C.c_void_p()
    F.check(F.lib().srx_bbknn_points(ctx.handle, F.ptr(points) if points.size else None, n, d, None if labels is None else F.ptr(labels), B,
                                     C.byref(opts), F.ptr(idx) if idx.size else None, F.ptr(dist) if dist.size else None,
                                     C.byref(info), C.byref(h) if graph else None), ctx.handle)
    return idx, dist, Graph(ctx, h) if graph else None, _bbknn_dict(info)


def bbknn(adata: IMAnnData, batch, neighbors_within_batch: int = 3, n_pcs=None, trim=None, use_rep=None) -> dict:
    """BBKNN on the scores the last ``pca_inplace`` left on the device (``srx_bbknn_result``; no host round trip), or with
    ``use_rep`` on the corrected scores of a ``harmony_integrate`` (``srx_bbknn_harmony``).  ``batch``: one integer label
    0 .. B - 1 per cell, or the name of such a column of ``adata.obs``.  Writes ``obsp["distances"]``, ``obsp["connectivities"]``
    and ``uns["neighbors"]`` the way ``neighbors(connectivities=True)`` does, with ``n_neighbors = neighbors_within_batch * B``
    (bbknn counts the cell); the handle kept on the adata is what ``louvain``, ``umap``, ``paga``, ... read."""
    ctx = adata.x().ctx
    if isinstance(batch, str):
        batch = adata.obs[batch]
    labels, B = _batch_labels(batch, adata.n_obs())
    opts = _bbknn_opts(neighbors_within_batch, n_pcs, trim)
    info = F.BbknnInfo()
    h = C.c_void_p()
    lp = None if labels is None else F.ptr(labels)
    if use_rep is None:
        F.check(F.lib().srx_bbknn_result(adata.x().handle, lp, B, C.byref(opts), C.byref(info), C.byref(h)), ctx.handle)
    else:
        F.check(F.lib().srx_bbknn_harmony(_harmony_handle(adata, use_rep).handle, lp, B, C.byref(opts), C.byref(info), C.byref(h)),
                ctx.handle)
    g = Graph(ctx, h)
    old = getattr(adata, "_graph", None)
    if old is not None:
        old.free()
    adata._graph = g
    adata.obsp["distances"] = g.matrix(F.GRAPH_DISTANCES)
    adata.obsp["connectivities"] = g.matrix(F.GRAPH_CONNECTIVITIES)
    kw = int(info.neighbors_within_batch)
    adata.uns["neighbors"] = {"params": {"n_neighbors": kw * B, "n_pcs": None if n_pcs is None else int(n_pcs), "include_self": False,
                                         "metric": "euclidean", "method": "bbknn", "neighbors_within_batch": kw,
                                         "n_batches": B, "trim": int(info.trim.trim)},
                              "info": _bbknn_dict(info), "graph": g.info()}
    if use_rep is not None:
        adata.uns["neighbors"]["params"]["use_rep"] = use_rep
    return adata.uns["neighbors"]


class KnnIndex(OwnedHandle):
    """Owning wrapper of an ``srx_knn_index``: the inverted-file index of the approximate search (centroids, lists, the
    index's own copy of the points), all on the device."""

    _free = "srx_knn_index_free"

    def info(self) -> dict:
        i = F.IvfInfo()
        F.check(F.lib().srx_knn_index_info_get(self._h, C.byref(i)), self.ctx.handle)
        return flat_info(i)

    def fetch(self):
        """(centroids f64 n_lists x d, list offsets uint64 n_lists + 1, list members uint32 n_ref)."""
        i = self.info()
        cent = np.zeros((i["n_lists"], i["d"]), dtype=np.float64)
        off = np.zeros(i["n_lists"] + 1, dtype=np.uint64)
        mem = np.zeros(i["n_ref"], dtype=np.uint32)
        F.check(F.lib().srx_knn_index_fetch(self._h, F.ptr(cent), F.ptr(off), F.ptr(mem)), self.ctx.handle)
        return cent, off, mem

    def search(self, query=None, k: int = 15, n_probe: int = 0, include_self: bool = False, n_dims=None):
        """Neighbours of every row of ``query`` (None: the self form) among the indexed points, from the ``n_probe`` nearest
        lists (0: min(20, n_lists)).  Returns (indices uint32 n_query x k, distances f64, the ``srx_ivf_search_info`` dict)."""
        i = self.info()
        if query is not None:
            query = np.ascontiguousarray(query, dtype=np.float64)
            if query.ndim != 2 or query.shape[1] != i["d"]:
                raise ValueError("query must be n_query x d with the d of the index")
        nq = i["n_ref"] if query is None else query.shape[0]
        k = int(k)
        opts = F.KnnOpts(k, int(n_dims or 0), int(bool(include_self)), 0)
        info = F.IvfSearchInfo()
        idx = np.zeros((nq, max(k, 0)), dtype=np.uint32)
        dist = np.zeros((nq, max(k, 0)), dtype=np.float64)
        F.check(F.lib().srx_knn_index_search(self._h, None if query is None else C.c_void_p(query.ctypes.data or 1), nq,
                                             C.byref(opts), int(n_probe), F.ptr(idx) if idx.size else None,
                                             F.ptr(dist) if dist.size else None, C.byref(info)), self.ctx.handle)
        return idx, dist, flat_info(info)

    def graph(self, k: int = 15, n_probe: int = 0):
        """The weighted graph of the self search (``srx_neighbors_index``): (``Graph``, search info dict)."""
        opts = F.KnnOpts(int(k), 0, 0, 0)
        info = F.IvfSearchInfo()
        h = C.c_void_p()
        F.check(F.lib().srx_neighbors_index(self._h, C.byref(opts), int(n_probe), C.byref(info), C.byref(h)), self.ctx.handle)
        return Graph(self.ctx, h), flat_info(info)


def _ivf_opts(n_lists, train_iters, seed, max_train_points):
    return F.IvfOpts(int(n_lists), int(train_iters), int(seed), int(max_train_points))


def knn_index_points(ctx, ref, centroids=None, n_lists: int = 0, train_iters: int = 10, seed: int = 0,
                     max_train_points: int = 0) -> KnnIndex:
    """The index over the rows of ``ref`` (n x d f64).  ``centroids`` (n_lists x d): taken as they are; None: trained
    (``srx_knn_index_points``)."""
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    if ref.ndim != 2:
        raise ValueError("ref must be n x d")
    if centroids is not None:
        centroids = np.ascontiguousarray(centroids, dtype=np.float64)
        if centroids.ndim != 2 or centroids.shape[1] != ref.shape[1]:
            raise ValueError("centroids must be n_lists x d with the d of ref")
        n_lists = centroids.shape[0]
    opts = _ivf_opts(n_lists, train_iters, seed, max_train_points)
    h = C.c_void_p()
    F.check(F.lib().srx_knn_index_points(ctx.handle, F.ptr(ref) if ref.size else None, ref.shape[0], ref.shape[1], C.byref(opts),
                                         None if centroids is None else C.c_void_p(centroids.ctypes.data or 1), C.byref(h)),
            ctx.handle)
    return KnnIndex(ctx, h)


def knn_index(adata: IMAnnData, n_pcs=None, n_lists: int = 0, train_iters: int = 10, seed: int = 0,
              max_train_points: int = 0) -> KnnIndex:
    """The index over the scores the last ``pca_inplace`` left on the device (``srx_knn_index_result``)."""
    opts = _ivf_opts(n_lists, train_iters, seed, max_train_points)
    h = C.c_void_p()
    ctx = adata.x().ctx
    F.check(F.lib().srx_knn_index_result(adata.x().handle, int(n_pcs or 0), C.byref(opts), C.byref(h)), ctx.handle)
    return KnnIndex(ctx, h)


def neighbors_approx(adata: IMAnnData, n_neighbors: int = 15, n_pcs=None, n_lists: int = 0, n_probe: int = 0,
                     connectivities: bool = False, knn_lists: bool = False, train_iters: int = 10, seed: int = 0,
                     max_train_points: int = 0) -> dict:
    """``neighbors`` through an inverted-file index of the scores (``srx_knn_index_result`` + ``srx_knn_index_search`` /
    ``srx_neighbors_index``): the k nearest among the members of the ``n_probe`` nearest of ``n_lists`` lists, exact within
    them.  Fills the keys ``neighbors`` fills, with ``"method": "ivf"`` and the index and search counters in
    ``uns["neighbors"]``; the index is freed before returning."""
    k = int(n_neighbors)
    ix = knn_index(adata, n_pcs, n_lists, train_iters, seed, max_train_points)
    try:
        params = {"n_neighbors": k, "n_pcs": None if n_pcs is None else int(n_pcs), "include_self": False,
                  "metric": "euclidean", "method": "ivf", "n_lists": ix.info()["n_lists"]}
        if connectivities:
            g, info = ix.graph(k, n_probe)
            old = getattr(adata, "_graph", None)
            if old is not None:
                old.free()
            adata._graph = g
            adata.obsp["distances"] = g.matrix(F.GRAPH_DISTANCES)
            adata.obsp["connectivities"] = g.matrix(F.GRAPH_CONNECTIVITIES)
            if knn_lists:
                _, indices, data = g.fetch(F.GRAPH_DISTANCES)
                idx, dist = indices.reshape(-1, k), data.reshape(-1, k)
                order = np.lexsort((idx, dist), axis=1)
                adata.obsm["knn_indices"] = np.take_along_axis(idx, order, axis=1)
                adata.obsm["knn_distances"] = np.take_along_axis(dist, order, axis=1)
            adata.uns["neighbors"] = {"params": params, "info": info, "index": ix.info(), "graph": g.info()}
        else:
            idx, dist, info = ix.search(None, k, n_probe)
            adata.obsm["knn_indices"] = idx
            adata.obsm["knn_distances"] = dist
            adata.uns["neighbors"] = {"params": params, "info": info, "index": ix.info()}
        params["n_probe"] = info["n_probe"]
    finally:
        ix.free()
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

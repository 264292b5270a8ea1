"""New cells on a fitted data set over libsrx_hip: the label vote (``srx_knn_vote`` / ``srx_knn_vote_graph``), the UMAP transform
(``srx_umap_transform_knn`` / ``srx_umap_transform_graph``) and ``ingest``, which composes them with ``pca_transform`` and the
neighbour search: what ``sc.tl.ingest`` gives the query's ``obs`` and ``obsm["X_umap"]``.

Not in the reference.  The method (umap-learn's ``UMAP.transform`` restated so that it is bit-identical from call to call, and
pandas' ``mode`` for the labels) is defined in include/srx.h; nothing is refitted and every stage runs on the device.
NOT compared: umap-learn, scanpy (not installed).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import IMAnnData
from ._common import flat_info, graph_of
from .dim_red import PcaModel, pca_transform
from .neighbors import Graph, knn_points

_PARTS = ("embedding", "start", "weights", "columns", "sigma")


def _list(indices, distances, who: str):
    idx = np.ascontiguousarray(indices, dtype=np.uint32)
    if idx.ndim != 2:
        raise ValueError("%s: indices must be n_query x k" % who)
    if distances is None:
        return idx, None
    dist = np.ascontiguousarray(distances, dtype=np.float64)
    if dist.shape != idx.shape:
        raise ValueError("%s: distances must have the shape of indices" % who)
    return idx, dist


def umap_transform(ctx, indices, distances, ref, min_dist: float = 0.5, spread: float = 1.0, n_epochs: int = 0, alpha: float = 0.25,
                   gamma: float = 1.0, negative_sample_rate: int = 5, seed: int = 0, a: float = 0.0, b: float = 0.0,
                   stop_after: int = 0, chunk_epochs: int = 0, n_components=None, parts: bool = False):
    """Place query cells in a fitted UMAP.  ``indices`` / ``distances``: the query's k-NN list among the reference points
    (n_query x kq, 3 <= kq <= 64, e.g. from ``knn_points(ctx, ref_scores, query_scores)``).  ``ref``: the reference embedding as an
    n_ref x dim array (dim 2 or 3), or the ``Graph`` on which ``umap`` ran, whose embedding is then read where it lies on the
    device (``n_components``: what the caller expects it to have; None = whatever it has).  ``n_epochs=0``: 100 for
    n_query <= 10 000, else 30; ``a = b = 0``: fitted from (spread, min_dist).  Returns (embedding n_query x dim f64, info dict);
    with ``parts=True`` the info also holds ``start``, ``weights``, ``columns`` and ``sigma`` of the membership stage."""
    idx, dist = _list(indices, distances, "umap_transform")
    nq, kq = idx.shape
    on_graph = isinstance(ref, Graph)
    if on_graph:
        dim = C.c_uint32(0)
        F.check(F.lib().srx_graph_embedding_fetch(ref.handle, None, C.byref(dim)), ref.ctx.handle)
        dim = int(dim.value) if n_components is None else int(n_components)
    else:
        yref = np.ascontiguousarray(ref, dtype=np.float64)
        if yref.ndim != 2:
            raise ValueError("umap_transform: the reference embedding must be n_ref x dim")
        dim = yref.shape[1]
    shapes = {"embedding": ((nq, dim), np.float64), "start": ((nq, dim), np.float64), "weights": ((nq, kq), np.float64),
              "columns": ((nq, kq), np.uint32), "sigma": ((nq,), np.float64)}
    arrays = {k: np.zeros(*shapes[k]) for k in (_PARTS if parts else ("embedding",))}
    out = F.UmapTransformOut(*[F.ptr(arrays[k]) if k in arrays and arrays[k].size else None for k in _PARTS])
    opts = F.UmapTransformOpts(float(a), float(b), float(min_dist), float(spread), float(gamma), float(alpha), int(seed) & (2 ** 64 - 1),
                               int(n_epochs), int(stop_after), int(negative_sample_rate), int(chunk_epochs))
    info = F.UmapTransformInfo()
    pi, pd = (F.ptr(idx) if idx.size else None), (F.ptr(dist) if dist is not None and dist.size else None)
    if on_graph:
        F.check(F.lib().srx_umap_transform_graph(ref.handle, pi, pd, nq, kq, dim, C.byref(opts), C.byref(out), C.byref(info)),
                ref.ctx.handle)
    else:
        F.check(F.lib().srx_umap_transform_knn(ctx.handle, pi, pd, nq, kq, F.ptr(yref) if yref.size else None, yref.shape[0], dim,
                                               C.byref(opts), C.byref(out), C.byref(info)), ctx.handle)
    d = flat_info(info)
    if parts:
        d.update({k: arrays[k] for k in _PARTS[1:]})
    return arrays["embedding"], d


def knn_vote(ctx, indices, ref, n_groups=None):
    """The label of every query row from its neighbours' labels: the most frequent one, ties to the lowest (pandas' ``mode``, as
    scanpy's ``ingest`` maps labels).  ``ref``: the reference labels (n_ref integers below ``n_groups``; None = max + 1), or the
    ``Graph`` on which ``louvain`` ran, whose labels are then read where they lie.  Returns (labels uint32, confidence f64 =
    the winning label's share of the k neighbours)."""
    idx, _ = _list(indices, None, "knn_vote")
    nq, k = idx.shape
    labels, counts = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
    pi = F.ptr(idx) if idx.size else None
    po, pc = (F.ptr(labels), F.ptr(counts)) if nq else (None, None)
    if isinstance(ref, Graph):
        F.check(F.lib().srx_knn_vote_graph(ref.handle, pi, nq, k, po, pc), ref.ctx.handle)
    else:
        lab = np.asarray(ref)
        if lab.ndim != 1 or (lab.size and (lab.min() < 0 or lab.max() > 0xFFFFFFFF)):
            raise ValueError("knn_vote: the reference labels must be n_ref integers in 0 .. 2^32 - 1")
        lab = np.ascontiguousarray(lab, dtype=np.uint32)
        groups = int(n_groups) if n_groups is not None else (int(lab.max()) + 1 if lab.size else 1)
        F.check(F.lib().srx_knn_vote(ctx.handle, pi, nq, k, F.ptr(lab) if lab.size else None, lab.size, groups, po, pc), ctx.handle)
    return labels, counts.astype(np.float64) / max(k, 1)


def ingest(query: IMAnnData, ref: IMAnnData, model: PcaModel = None, obs: str = "louvain", embedding: str = "X_umap",
           n_neighbors=None, n_pcs=None, index=None, n_probe: int = 0, feature_map=None, target_sum=None, log1p: bool = False,
           **umap_opts) -> dict:
    """Map the cells of ``query`` onto the fitted ``ref`` (``pca_inplace`` -> ``neighbors(connectivities=True)`` -> ``louvain``
    -> ``umap`` have run on it): ``sc.tl.ingest``.  The query is projected with the reference's PCA (``model``: None = the one
    the last fit left on ``ref``; ``feature_map`` / ``target_sum`` / ``log1p`` as ``pca_transform`` takes them), its
    ``n_neighbors`` nearest reference cells are found in the first ``n_pcs`` scores (``index``: a ``KnnIndex`` over the
    reference scores for the approximate search with ``n_probe``; None = the exact ``knn_points``), the labels are voted and the
    cells placed in the reference's UMAP, both against what lies on the device with the reference's graph.
    ``n_neighbors``: None = the reference graph's k + 1 (scanpy's n_neighbors counts the cell itself, as the graph section of
    include/srx.h says), at most 64.  Writes ``query.obsm["X_pca"]``, ``query.obs[obs]``, ``query.obs[obs + "_confidence"]``,
    ``query.obsm[embedding]`` and ``query.uns["ingest"]`` (params and the transform's info); returns the latter."""
    g = graph_of(ref, "ingest")
    ctx = ref.x().ctx
    own = model is None
    if own:
        model = PcaModel.from_result(ref)
    try:
        scores = pca_transform(query, model, feature_map, target_sum=target_sum, log1p=log1p)
    finally:
        if own:
            model.free()
    k = int(n_neighbors) if n_neighbors is not None else min(int(g.info()["k"]) + 1, 64)
    if index is not None:
        idx, dist, _ = index.search(scores, k=k, n_probe=n_probe, n_dims=n_pcs)
    else:
        idx, dist, _ = knn_points(ctx, ref.obsm["X_pca"], scores, k=k, n_dims=n_pcs)
    labels, conf = knn_vote(ctx, idx, g)
    emb, info = umap_transform(ctx, idx, dist, g, **umap_opts)
    query.obsm["X_pca"] = scores
    query.obs[obs] = labels
    query.obs[obs + "_confidence"] = conf
    query.obsm[embedding] = emb
    query.uns["ingest"] = {"params": {"obs": obs, "embedding": embedding, "n_neighbors": k, "n_pcs": None if n_pcs is None else int(n_pcs),
                                      "approximate": index is not None, **umap_opts}, "info": info}
    return query.uns["ingest"]

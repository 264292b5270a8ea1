"""t-SNE over libsrx_hip (``srx_tsne_*``): what fills ``obsm["X_tsne"]``.

The reference's commented-out ``tsne`` / ``tsne_inplace`` (dim_red/mod.rs:159-227).  The method (perplexity affinities of
the k-NN list, a Barnes-Hut repulsion over a uniform pyramid, scikit-learn's gains and momenta, bit-identical from call to
call) is defined in include/srx.h; every step runs on the device and nothing computes on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import IMAnnData
from ._common import OwnedHandle, flat_info, graph_of

_INITS = {"pca": F.TSNE_INIT_PCA, "random": F.TSNE_INIT_RANDOM}


class Tsne(OwnedHandle):
    """Owning wrapper of an ``srx_tsne``: the joint affinities P (CSR), beta and the last embedding on the device."""

    _free = "srx_tsne_free"

    def info(self) -> dict:
        i = F.TsneInfo()
        F.check(F.lib().srx_tsne_info_get(self._h, C.byref(i)), self.ctx.handle)
        return flat_info(i)

    def affinities(self):
        """(indptr uint64 n + 1, indices uint32, data f64, beta f64 n)."""
        i = self.info()
        indptr = np.zeros(i["n"] + 1, dtype=np.uint64)
        indices = np.zeros(i["nnz"], dtype=np.uint32)
        data = np.zeros(i["nnz"], dtype=np.float64)
        beta = np.zeros(i["n"], dtype=np.float64)
        F.check(F.lib().srx_tsne_fetch_affinities(self._h, F.ptr(indptr), F.ptr(indices) if indices.size else None,
                                                  F.ptr(data) if data.size else None, F.ptr(beta) if beta.size else None),
                self.ctx.handle)
        return indptr, indices, data, beta


def tsne_affinities(ctx, indices, distances, perplexity: float = 0.0) -> Tsne:
    """The affinities of a k-NN list (n x k; no row names itself): ``srx_tsne_affinities_knn``.  ``perplexity=0``:
    min(30, k / 3)."""
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    distances = np.ascontiguousarray(distances, dtype=np.float64)
    if indices.ndim != 2 or indices.shape != distances.shape:
        raise ValueError("indices and distances must both be n x k")
    n, k = indices.shape
    h = C.c_void_p()
    F.check(F.lib().srx_tsne_affinities_knn(ctx.handle, F.ptr(indices) if indices.size else None,
                                            F.ptr(distances) if distances.size else None, n, k, float(perplexity), C.byref(h)),
            ctx.handle)
    return Tsne(ctx, h)


def tsne_affinities_graph(graph, perplexity: float = 0.0) -> Tsne:
    """The same from the distances a ``Graph`` holds on the device (``srx_tsne_affinities_graph``); the graph is untouched."""
    h = C.c_void_p()
    F.check(F.lib().srx_tsne_affinities_graph(graph.handle, float(perplexity), C.byref(h)), graph.ctx.handle)
    return Tsne(graph.ctx, h)


def tsne_forces(t: Tsne, y, theta: float = 0.5, levels: int = 0):
    """The diagnostic ``srx_tsne_forces``: (attr n x 2, rep n x 2, z n, info dict) at the positions ``y`` (n x 2)."""
    n = t.info()["n"]
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.shape != (n, 2):
        raise ValueError("tsne_forces: the positions must be n x 2 = %d x 2" % n)
    attr, rep, z = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros(n)
    fi = F.TsneForceInfo()
    F.check(F.lib().srx_tsne_forces(t.handle, F.ptr(y) if n else None, float(theta), int(levels), F.ptr(attr) if n else None,
                                    F.ptr(rep) if n else None, F.ptr(z) if n else None, C.byref(fi)), t.ctx.handle)
    info = {"levels": fi.levels, "side": fi.side, "lo": (fi.lo[0], fi.lo[1]), "cells_accepted": fi.cells_accepted,
            "cells_exact": fi.cells_exact, "pairs_exact": fi.pairs_exact}
    return attr, rep, z, info


def _start(init, n: int):
    if isinstance(init, str):
        if init not in _INITS:
            raise ValueError("tsne: init is 'pca', 'random' or an n x 2 array")
        return _INITS[init], None
    y0 = np.ascontiguousarray(init, dtype=np.float64)
    if y0.shape != (n, 2):
        raise ValueError("tsne: the start must be n x 2 = %d x 2" % n)
    return F.TSNE_INIT_GIVEN, y0


def tsne_run(t: Tsne, matrix=None, init="random", theta: float = 0.5, exaggeration: float = 12.0, learning_rate: float = 0.0,
             seed: int = 0, n_iter: int = 1000, exaggeration_iters: int = 250, stop_after: int = 0, levels: int = 0):
    """``srx_tsne_run`` on a ``Tsne`` handle.  ``matrix``: the ``DeviceCsr`` whose scores start the layout (``init="pca"``).
    Returns (embedding n x 2 f64, info dict)."""
    n = t.info()["n"]
    code, y0 = _start(init, n)
    emb = np.zeros((n, 2), dtype=np.float64)
    info = F.TsneRunInfo()
    opts = F.TsneOpts(float(theta), float(exaggeration), float(learning_rate), int(seed) & (2 ** 64 - 1), int(n_iter),
                      int(exaggeration_iters), int(stop_after), int(levels), int(code), 0)
    F.check(F.lib().srx_tsne_run(t.handle, matrix.handle if code == F.TSNE_INIT_PCA and matrix is not None else None, C.byref(opts),
                                 F.ptr(y0) if y0 is not None and y0.size else None, F.ptr(emb) if emb.size else None, C.byref(info)),
            t.ctx.handle)
    return emb, flat_info(info)


def tsne(adata: IMAnnData, perplexity: float = 0.0, theta: float = 0.5, exaggeration: float = 12.0, learning_rate: float = 0.0,
         n_iter: int = 1000, exaggeration_iters: int = 250, init="pca", seed: int = 0, key_added: str = "X_tsne", stop_after: int = 0,
         levels: int = 0) -> dict:
    """Layout of the cells from the distances that ``neighbors(adata, connectivities=True)`` left on the device (no host
    round trip).  ``perplexity=0``: min(30, k / 3) for the graph's k.  ``init``: "pca" (the scores the last fit left on the
    device, scaled to 1e-4), "random" (hashed from ``seed``) or an n x 2 array.  Writes ``adata.obsm[key_added]`` (n x 2 f64)
    and ``adata.uns["tsne"]`` (``params``, the affinities' ``srx_tsne_info`` and the run's ``srx_tsne_run_info``); keeps the
    handle on the adata; returns the run's info."""
    g = graph_of(adata, "tsne")
    t = tsne_affinities_graph(g, perplexity)
    old = getattr(adata, "_tsne", None)
    if old is not None:
        old.free()
    adata._tsne = t
    emb, d = tsne_run(t, adata.x(), init, theta, exaggeration, learning_rate, seed, n_iter, exaggeration_iters, stop_after, levels)
    adata.obsm[key_added] = emb
    a = t.info()
    adata.uns["tsne"] = {"params": {"perplexity": a["perplexity"], "theta": float(theta), "exaggeration": float(exaggeration),
                                    "learning_rate": d["eta"], "n_iter": d["n_iter"], "exaggeration_iters": int(exaggeration_iters),
                                    "init": init if isinstance(init, str) else "given", "seed": int(seed)},
                         "affinities": a, "info": d}
    return d


def tsne_embedding(t: Tsne) -> np.ndarray:
    """The embedding the last ``srx_tsne_run`` left with a ``Tsne`` handle (``srx_tsne_embedding_fetch``)."""
    out = np.zeros((t.info()["n"], 2), dtype=np.float64)
    F.check(F.lib().srx_tsne_embedding_fetch(t.handle, F.ptr(out) if out.size else None), t.ctx.handle)
    return out

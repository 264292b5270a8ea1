"""Louvain communities of the neighbour graph over libsrx_hip (``srx_louvain`` / ``srx_louvain_csr``): what fills
``obs["louvain"]``.

Not in the reference.  The method (a parallel Louvain with synchronous sweeps) is defined in include/srx.h; every level
runs on the device and nothing computes on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import IMAnnData
from ._common import csr_triple, graph_of


def _opts(resolution, min_gain, max_levels, max_sweeps) -> F.LouvainOpts:
    return F.LouvainOpts(float(resolution), float(min_gain), int(max_levels), int(max_sweeps))


def _info_dict(i: F.LouvainInfo) -> dict:
    nl = int(i.n_levels)
    return {"n": int(i.n), "n_communities": int(i.n_communities), "n_levels": nl, "sweeps": int(i.sweeps), "moves": int(i.moves),
            "modularity": float(i.modularity), "ms": float(i.ms), "level_communities": [int(v) for v in i.level_communities[:nl]],
            "level_modularity": [float(v) for v in i.level_modularity[:nl]]}


def louvain(adata: IMAnnData, resolution: float = 1.0, key_added: str = "louvain", min_gain: float = 0.0,
            max_levels: int = 0, max_sweeps: int = 0) -> dict:
    """Communities of the connectivities that ``neighbors(adata, connectivities=True)`` left on the device (no host round
    trip).  Writes ``adata.obs[key_added]`` (uint32, communities numbered by descending size) and ``adata.uns[key_added]``
    (``params`` and the call's ``srx_louvain_info`` under ``info``); returns the info."""
    g = graph_of(adata, "louvain")
    labels = np.zeros(adata.n_obs(), dtype=np.uint32)
    info = F.LouvainInfo()
    opts = _opts(resolution, min_gain, max_levels, max_sweeps)
    F.check(F.lib().srx_louvain(g.handle, C.byref(opts), F.ptr(labels) if labels.size else None, C.byref(info)), g.ctx.handle)
    adata.obs[key_added] = labels
    g.labels_key = key_added          # whose labels the handle holds now (rank_genes_groups reads them where they lie)
    adata.uns[key_added] = {"params": {"resolution": float(resolution), "min_gain": float(min_gain), "max_levels": int(max_levels),
                                       "max_sweeps": int(max_sweeps)}, "info": _info_dict(info)}
    return adata.uns[key_added]["info"]


def graph_labels(graph) -> np.ndarray:
    """The labels the last ``srx_louvain`` left with a ``Graph`` handle (``srx_graph_labels_fetch``)."""
    labels = np.zeros(graph.info()["n"], dtype=np.uint32)
    F.check(F.lib().srx_graph_labels_fetch(graph.handle, F.ptr(labels) if labels.size else None), graph.ctx.handle)
    return labels


def louvain_csr(ctx, matrix, resolution: float = 1.0, min_gain: float = 0.0, max_levels: int = 0, max_sweeps: int = 0):
    """Communities of any symmetric weighted graph: a scipy sparse matrix or an (indptr, indices, data) CSR triple with
    ascending columns, positive weights and no diagonal (``srx_louvain_csr`` validates on the device).  Returns
    (labels uint32, info dict)."""
    indptr, indices, data = csr_triple(matrix, "louvain_csr")
    n = indptr.size - 1
    labels = np.zeros(n, dtype=np.uint32)
    info = F.LouvainInfo()
    opts = _opts(resolution, min_gain, max_levels, max_sweeps)
    F.check(F.lib().srx_louvain_csr(ctx.handle, F.ptr(indptr), F.ptr(indices) if indices.size else None,
                                    F.ptr(data) if data.size else None, n, C.byref(opts), F.ptr(labels) if n else None,
                                    C.byref(info)), ctx.handle)
    return labels, _info_dict(info)

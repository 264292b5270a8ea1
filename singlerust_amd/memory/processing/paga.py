"""PAGA over libsrx_hip (``srx_paga`` / ``srx_paga_csr`` / ``srx_paga_from_counts`` / ``srx_paga_init_positions``): the
neighbour graph coarse-grained over the groups, what fills ``uns["paga"]``.

Not in the reference.  The definition (scanpy's ``model="v1.2"``, restated so that the result is exact) is in include/srx.h.
The walk over the graph runs on the device, where D and the labels already lie; the arithmetic on the
``n_groups x n_groups`` table is host code in the library (``srx_paga_from_counts`` needs no GPU).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import IMAnnData
from ._common import flat_info, graph_of


class _Tables:
    """The host buffers of one call and the ``srx_paga_tables`` that points at them."""

    def __init__(self, G: int):
        self.sizes = np.zeros(G, dtype=np.uint64)
        self.out_edges = np.zeros(G, dtype=np.uint64)
        self.counts = np.zeros((G, G), dtype=np.uint64)
        self.connectivities = np.zeros((G, G), dtype=np.float64)
        self.expected = np.zeros((G, G), dtype=np.float64)
        self.tree = np.zeros((G, G), dtype=np.float64)
        self.c = F.PagaTables(F.ptr(self.sizes), F.ptr(self.out_edges), F.ptr(self.counts), F.ptr(self.connectivities), F.ptr(self.expected),
                              F.ptr(self.tree))
        self.info = F.PagaInfo()

    def result(self) -> dict:
        return {"sizes": self.sizes, "out_edges": self.out_edges, "counts": self.counts, "connectivities": self.connectivities,
                "expected": self.expected, "tree": self.tree, "info": flat_info(self.info)}


def _n_groups(labels: np.ndarray, n_groups) -> int:
    if n_groups is not None:
        return int(n_groups)
    return int(labels.max()) + 1 if labels.size else 1


def _sparse(a: np.ndarray):
    try:
        import scipy.sparse as sp
    except ImportError:
        return a
    return sp.csr_matrix(a)


def _dense(a) -> np.ndarray:
    return np.ascontiguousarray(a.toarray() if hasattr(a, "toarray") else a, dtype=np.float64)


def _group_labels(adata: IMAnnData, g, groups: str, who: str):
    """(host labels or None for those on the handle, n_groups)."""
    if getattr(g, "labels_key", None) == groups and groups in adata.uns and "info" in adata.uns[groups]:
        return None, max(1, int(adata.uns[groups]["info"]["n_communities"]))
    if groups not in adata.obs:
        raise F.SrxError(F.E_ARG, "%s: adata.obs holds no %r" % (who, groups))
    labels = np.ascontiguousarray(adata.obs[groups], dtype=np.uint32)
    return labels, _n_groups(labels, None)


def paga(adata: IMAnnData, groups: str = "louvain") -> dict:
    """PAGA of the graph that ``neighbors(adata, connectivities=True)`` left on the device, over ``adata.obs[groups]`` (read
    where they lie when the handle's labels are that clustering's: no host round trip).  Writes ``adata.uns["paga"]``:
    ``connectivities``, ``connectivities_tree`` and ``expected_n_edges_random`` (scipy CSR where scipy imports, else dense),
    ``groups``, ``sizes`` and ``info``; returns the info."""
    g = graph_of(adata, "paga")
    labels, G = _group_labels(adata, g, groups, "paga")
    t = _Tables(G)
    F.check(F.lib().srx_paga(g.handle, None if labels is None else F.ptr(labels), G, C.byref(t.c), C.byref(t.info)), g.ctx.handle)
    r = t.result()
    adata.uns["paga"] = {"connectivities": _sparse(r["connectivities"]), "connectivities_tree": _sparse(r["tree"]),
                         "expected_n_edges_random": _sparse(r["expected"]), "groups": groups, "sizes": r["sizes"], "info": r["info"]}
    return r["info"]


def paga_csr(ctx, pattern, labels, n_groups=None) -> dict:
    """PAGA of any directed pattern: a scipy sparse matrix or an (indptr, indices) pair; every stored entry counts once.
    ``n_groups`` None = the largest label + 1.  Returns the six tables and ``info`` as a dict."""
    if isinstance(pattern, (tuple, list)):
        indptr, indices = pattern[0], pattern[1]
    else:
        m = pattern.tocsr()
        indptr, indices = m.indptr, m.indices
    indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    if indptr.ndim != 1 or indptr.size < 1 or indices.ndim != 1 or labels.shape != (indptr.size - 1,):
        raise ValueError("paga_csr: indptr (n + 1), indices (nnz) and labels (n) expected")
    if int(indptr[-1]) != indices.size:
        raise ValueError("paga_csr: indptr[n] does not equal the number of stored entries")
    G = _n_groups(labels, n_groups)
    t = _Tables(G if 1 <= G <= F.GROUPS_MAX else 1)
    F.check(F.lib().srx_paga_csr(ctx.handle, F.ptr(indptr), F.ptr(indices) if indices.size else None, indptr.size - 1,
                                 F.ptr(labels) if labels.size else None, G, C.byref(t.c), C.byref(t.info)), ctx.handle)
    return t.result()


def paga_from_counts(counts, sizes) -> dict:
    """Everything after the walk from the ``n_groups x n_groups`` counts E and the group sizes; host code, no GPU."""
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    G = sizes.size
    if counts.shape != (G, G):
        raise ValueError("paga_from_counts: counts (n_groups x n_groups) and sizes (n_groups) expected")
    t = _Tables(G if 1 <= G <= F.GROUPS_MAX else 1)
    F.check(F.lib().srx_paga_from_counts(F.ptr(counts), F.ptr(sizes), G, C.byref(t.c), C.byref(t.info)), None)
    return t.result()


def paga_init_positions(adata: IMAnnData, pos, groups: str = "louvain", seed: int = 0) -> np.ndarray:
    """Start positions for ``umap(adata, init=...)`` from ``adata.uns["paga"]`` and ``pos``, the caller's coarse layout
    (``n_groups x 2`` or ``x 3``): every cell near its group's position, spread towards the group's strongest neighbour."""
    g = graph_of(adata, "paga_init_positions")
    if "paga" not in adata.uns:
        raise F.SrxError(F.E_ARG, "paga_init_positions: run paga(adata) first")
    conn = _dense(adata.uns["paga"]["connectivities"])
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    G = conn.shape[0]
    if pos.ndim != 2 or pos.shape[0] != G:
        raise ValueError("paga_init_positions: pos is n_groups x 2 or n_groups x 3")
    labels, _ = _group_labels(adata, g, groups, "paga_init_positions")
    n = adata.n_obs()
    out = np.zeros((n, pos.shape[1]), dtype=np.float64)
    F.check(F.lib().srx_paga_init_positions(g.handle, g.ctx.handle, None if labels is None else F.ptr(labels), n, G, F.ptr(conn),
                                            F.ptr(pos), pos.shape[1], int(seed) & 0xFFFFFFFFFFFFFFFF, F.ptr(out) if n else None),
            g.ctx.handle)
    return out

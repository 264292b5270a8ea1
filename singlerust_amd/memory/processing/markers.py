"""Marker genes per group over libsrx_hip (``srx_group_moments`` / ``srx_rank_genes_groups[_graph]``): what fills
``uns["rank_genes_groups"]``.

Not in the reference.  The statistics (Welch's t from 64-bit fixed-point grouped moments; the Wilcoxon rank-sum z from exact
grouped rank sums, ``srx_rank_genes_wilcoxon[_graph]``), group against rest, are defined in include/srx.h; everything runs on
the device over the resident matrix and nothing computes on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import IMAnnData
from ._common import OwnedHandle, flat_info

TABLES = {"cnt": F.MARKERS_CNT, "sum": F.MARKERS_SUM, "sumsq": F.MARKERS_SUMSQ, "mean": F.MARKERS_MEAN, "var": F.MARKERS_VAR,
          "mean_rest": F.MARKERS_MEAN_REST, "var_rest": F.MARKERS_VAR_REST, "score": F.MARKERS_SCORE, "lfc": F.MARKERS_LFC,
          "pct": F.MARKERS_PCT, "pct_rest": F.MARKERS_PCT_REST, "ranksum2": F.MARKERS_RANKSUM2}
_U64_TABLES = (F.MARKERS_CNT, F.MARKERS_RANKSUM2)


def _labels(labels, n_obs: int):
    labels = np.ascontiguousarray(labels)
    if labels.shape != (n_obs,) or labels.dtype.kind not in "iu":
        raise ValueError("labels: one integer per cell expected")
    if labels.size and int(labels.min()) < 0:
        raise ValueError("labels: negative label")
    n_groups = int(labels.max()) + 1 if labels.size else 1
    return labels.astype(np.uint32), n_groups


class Markers(OwnedHandle):
    """Owning wrapper of an ``srx_markers`` (the device tables of one ``rank_genes_groups`` call)."""

    _free = "srx_markers_free"

    def info(self) -> dict:
        i = F.MarkersInfo()
        F.check(F.lib().srx_markers_info_get(self._h, C.byref(i)), self.ctx.handle)
        return flat_info(i)

    def top(self):
        """(genes uint32, scores, logfoldchanges), n_groups x n_top each."""
        i = self.info()
        shape = (i["n_groups"], i["n_top"])
        genes, scores, lfc = np.zeros(shape, np.uint32), np.zeros(shape), np.zeros(shape)
        F.check(F.lib().srx_markers_fetch_top(self._h, F.ptr(genes), F.ptr(scores), F.ptr(lfc)), self.ctx.handle)
        return genes, scores, lfc

    def table(self, which) -> np.ndarray:
        """One full n_groups x n_genes table: a ``TABLES`` name or an ``SRX_MARKERS_*`` value."""
        which = TABLES[which] if isinstance(which, str) else int(which)
        i = self.info()
        out = np.zeros((i["n_groups"], i["n_cols"]), np.uint64 if which in _U64_TABLES else np.float64)
        F.check(F.lib().srx_markers_fetch_table(self._h, which, F.ptr(out)), self.ctx.handle)
        return out

    def ties(self) -> np.ndarray:
        """The tie term T per gene (uint64): a handle of the Wilcoxon route made with ``tie_correct`` only."""
        out = np.zeros(self.info()["n_cols"], np.uint64)
        F.check(F.lib().srx_markers_fetch_ties(self._h, F.ptr(out)), self.ctx.handle)
        return out

    def wilcoxon_info(self) -> dict:
        """Chunks, staging bytes, segment routes and stage times of the Wilcoxon route (refused on a t-test handle)."""
        i = F.WilcoxonInfo()
        F.check(F.lib().srx_markers_wilcoxon_info_get(self._h, C.byref(i)), self.ctx.handle)
        return flat_info(i)

    def sizes(self) -> np.ndarray:
        out = np.zeros(self.info()["n_groups"], np.uint64)
        F.check(F.lib().srx_markers_fetch_sizes(self._h, F.ptr(out)), self.ctx.handle)
        return out


def group_moments(adata: IMAnnData, labels) -> dict:
    """Per-(group, gene) count, sum and sum of squares of the stored values (pseudobulk sums, dot-plot fractions):
    ``{"n_cells": (n_groups,), "cnt", "sum", "sumsq": (n_groups, n_vars)}`` for integer labels 0 .. n_groups - 1."""
    x = adata.x()
    labels, n_groups = _labels(labels, adata.n_obs())
    n_vars = adata.n_vars()
    out = {"n_cells": np.zeros(n_groups, np.uint64), "cnt": np.zeros((n_groups, n_vars), np.uint64),
           "sum": np.zeros((n_groups, n_vars)), "sumsq": np.zeros((n_groups, n_vars))}
    F.check(F.lib().srx_group_moments(x.handle, F.ptr(labels) if labels.size else None, n_groups, F.ptr(out["n_cells"]),
                                      F.ptr(out["cnt"]), F.ptr(out["sum"]), F.ptr(out["sumsq"])), x.ctx.handle)
    return out


def rank_genes_groups(adata: IMAnnData, groupby: str = "louvain", n_genes: int = 100, logged: bool = True,
                      key_added: str = "rank_genes_groups", method: str = "t-test", tie_correct: bool = False) -> dict:
    """Welch's t-test of every group against the rest, scanpy's ``tl.rank_genes_groups`` default, or with
    ``method="wilcoxon"`` the Wilcoxon rank-sum z (``tie_correct`` as scanpy's flag of that name).  Where the graph on the
    device still holds the labels of ``obs[groupby]`` (the last ``louvain`` wrote them) they are read there, with no host round
    trip; otherwise ``obs[groupby]`` (integers 0 .. n_groups - 1) is uploaded.  Writes ``adata.uns[key_added]``: ``names``,
    ``scores``, ``logfoldchanges`` (n_groups x n_genes, best first), ``pts`` / ``pts_rest`` (n_groups x n_vars), ``params``,
    ``info``; the device tables stay reachable as ``adata._markers``.  Returns the info."""
    x = adata.x()
    if method not in ("t-test", "wilcoxon"):
        raise F.SrxError(F.E_ARG, f"rank_genes_groups: method '{method}' is neither 't-test' nor 'wilcoxon'")
    if tie_correct and method != "wilcoxon":
        raise F.SrxError(F.E_ARG, "rank_genes_groups: tie_correct belongs to method='wilcoxon'")
    if groupby not in adata.obs:
        raise F.SrxError(F.E_ARG, f"rank_genes_groups: obs has no '{groupby}'")
    n_top = min(int(n_genes), adata.n_vars())
    wilcoxon = method == "wilcoxon"
    opts = F.WilcoxonOpts(n_top, 1 if logged else 0, 1 if tie_correct else 0, 0, 0) if wilcoxon else F.RankGenesOpts(n_top, 1 if logged else 0)
    lib = F.lib()
    on_graph, on_labels = ((lib.srx_rank_genes_wilcoxon_graph, lib.srx_rank_genes_wilcoxon) if wilcoxon
                           else (lib.srx_rank_genes_groups_graph, lib.srx_rank_genes_groups))
    h = C.c_void_p()
    g = getattr(adata, "_graph", None)
    resident = bool(g is not None and g.handle and getattr(g, "labels_key", None) == groupby)
    if resident:
        F.check(on_graph(x.handle, g.handle, C.byref(opts), C.byref(h)), x.ctx.handle)
    else:
        labels, n_groups = _labels(adata.obs[groupby], adata.n_obs())
        F.check(on_labels(x.handle, F.ptr(labels) if labels.size else None, n_groups, C.byref(opts), C.byref(h)), x.ctx.handle)
    old = getattr(adata, "_markers", None)
    if old is not None:
        old.free()
    mk = adata._markers = Markers(x.ctx, h)
    genes, scores, lfc = mk.top()
    names = np.asarray(adata.var_names, dtype=object)[genes] if genes.size else np.zeros(genes.shape, dtype=object)
    info = mk.info()
    adata.uns[key_added] = {"names": names, "scores": scores, "logfoldchanges": lfc, "pts": mk.table("pct"),
                            "pts_rest": mk.table("pct_rest"),
                            "params": {"groupby": groupby, "method": method, "reference": "rest", "n_genes": n_top,
                                       "logged": bool(logged), "resident_labels": resident,
                                       "tie_correct": bool(tie_correct)},
                            "info": info}
    return info

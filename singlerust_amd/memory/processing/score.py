"""Gene-set scores and per-cell sums over gene lists over libsrx_hip (``srx_gene_list_sums``, ``srx_score_genes_controls``,
``srx_score_genes``): what ``sc.tl.score_genes``, ``sc.tl.score_genes_cell_cycle`` and the ``qc_vars`` part of
``sc.pp.calculate_qc_metrics`` give, on the values as stored.

Not in the reference.  The definition is in include/srx.h: one walk over the column indices sums up to 64 gene lists per cell
in fixed point; a score is the mean over the set minus the mean over control genes drawn from the same expression bins.
Departure from scanpy: the control genes of a bin are chosen by a hash of (seed, gene), not by numpy's generator, so scores
agree with scanpy's in distribution, not value for value; nothing here has been compared with scanpy.  Out of scope: ``use_raw``,
layers, weighted signatures, CSC handles, sharded and backed contexts.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import DeviceCsr, IMAnnData

LISTS_MAX = F.GENE_LISTS_MAX


def _matrix(x) -> DeviceCsr:
    return x.x() if isinstance(x, IMAnnData) else x


def _info(i) -> dict:
    return {n: getattr(i, n) for n, _ in i._fields_}


def resolve_genes(var_names, genes, n_vars: int):
    """(indices u64, dropped names): ``genes`` as indices, a boolean mask over the genes, or names looked up in ``var_names``
    (an ``IMAnnData``'s).  Names that are not found are dropped and returned, as scanpy drops them; a name listed twice is kept
    once."""
    g = np.asarray(genes)
    if g.dtype == bool:
        if g.shape != (n_vars,):
            raise ValueError("a gene mask must hold one entry per gene (%d), not %r" % (n_vars, g.shape))
        return np.flatnonzero(g).astype(np.uint64), []
    if g.size and g.dtype.kind in "USO" and all(isinstance(v, str) for v in g.ravel().tolist()):
        if var_names is None:
            raise ValueError("genes given by name need an IMAnnData (var_names)")
        where = {}
        for j, name in enumerate(var_names):
            where.setdefault(name, j)
        found, dropped, seen = [], [], set()
        for name in g.ravel().tolist():
            if name not in where:
                dropped.append(name)
            elif name not in seen:
                seen.add(name)
                found.append(where[name])
        return np.asarray(found, dtype=np.uint64), dropped
    return np.ascontiguousarray(g, dtype=np.uint64).ravel(), []


def _pack(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    flat = np.concatenate([np.asarray(l, dtype=np.uint64) for l in lists]) if lists else np.zeros(0, dtype=np.uint64)
    return ptr, np.ascontiguousarray(flat if flat.size else np.zeros(1, dtype=np.uint64))


def _named_sets(adata, sets):
    """names, index lists and dropped names of one list or a dict of lists"""
    m = _matrix(adata)
    n_vars = int(m.info().n_cols)
    var_names = adata.var_names if isinstance(adata, IMAnnData) else None
    named = sets if isinstance(sets, dict) else {"score": sets}
    names, lists, dropped = [], [], {}
    for k, v in named.items():
        idx, gone = resolve_genes(var_names, v, n_vars)
        names.append(k)
        lists.append(idx)
        if gone:
            dropped[k] = gone
    return names, lists, dropped


def gene_list_sums(adata, lists, want_info=False):
    """(sum f64, cnt u32), each n_obs x len(lists): per cell and list the sum and the number of the STORED entries whose gene is
    in the list (a stored 0 counts): ``srx_gene_list_sums``.  ``lists``: a sequence of index arrays (or masks, or names)."""
    m = _matrix(adata)
    n, n_vars = int(m.info().n_rows), int(m.info().n_cols)
    var_names = adata.var_names if isinstance(adata, IMAnnData) else None
    idx = [resolve_genes(var_names, l, n_vars)[0] for l in lists]
    ptr, flat = _pack(idx)
    s, c = np.zeros((n, len(idx)), dtype=np.float64), np.zeros((n, len(idx)), dtype=np.uint32)
    i = F.GeneListInfo()
    F.check(F.lib().srx_gene_list_sums(m.handle, F.ptr(ptr), F.ptr(flat), len(idx), F.ptr(s) if s.size else F.ptr(np.zeros(1)),
                                       F.ptr(c) if c.size else F.ptr(np.zeros(1, dtype=np.uint32)), C.byref(i)), m.ctx.handle)
    return (s, c, _info(i)) if want_info else (s, c)


def _opts(ctrl_size, n_bins, seed, ctrl_as_ref) -> F.ScoreGenesOpts:
    return F.ScoreGenesOpts(int(ctrl_size), int(n_bins), int(seed) & (2 ** 64 - 1), int(bool(ctrl_as_ref)), 0)


def control_capacity(lists, ctrl_size: int, n_bins: int, n_pool: int) -> int:
    """the bound of srx.h: per set ctrl_size * min(|set|, P / n_items + 1)"""
    ctrl_size, n_bins = int(ctrl_size) or 50, int(n_bins) or 25
    n_items = max(int(np.round(n_pool / max(n_bins - 1, 1))), 1)
    return max(sum(ctrl_size * min(len(l), n_pool // n_items + 1) for l in lists), 1)


def score_genes_controls(gene_mean, sets, ctrl_size=50, n_bins=25, gene_pool=None, seed=0, ctrl_as_ref=True):
    """(control lists, cut per gene): the control genes of each set from the gene means alone; host code, no device:
    ``srx_score_genes_controls``.  ``cut`` is UINT32_MAX outside the pool."""
    mean = np.ascontiguousarray(gene_mean, dtype=np.float64)
    lists = [np.ascontiguousarray(s, dtype=np.uint64).ravel() for s in sets]
    ptr, flat = _pack(lists)
    pool = None if gene_pool is None else np.ascontiguousarray(gene_pool, dtype=np.uint64).ravel()
    n_pool = mean.size if pool is None else pool.size
    cap = control_capacity(lists, ctrl_size, n_bins, n_pool)
    cptr, cgenes, cut = np.zeros(len(lists) + 1, dtype=np.uint64), np.zeros(cap, dtype=np.uint64), np.zeros(max(mean.size, 1), dtype=np.uint32)
    o = _opts(ctrl_size, n_bins, seed, ctrl_as_ref)
    F.check(F.lib().srx_score_genes_controls(F.ptr(mean) if mean.size else None, mean.size, None if pool is None else F.ptr(pool),
                                             0 if pool is None else pool.size, F.ptr(ptr), F.ptr(flat), len(lists), C.byref(o), F.ptr(cptr),
                                             F.ptr(cgenes), cap, F.ptr(cut)))
    return [cgenes[int(cptr[s]):int(cptr[s + 1])].copy() for s in range(len(lists))], cut[:mean.size]


def score_genes(adata, gene_list, ctrl_size=50, n_bins=25, gene_pool=None, seed=0, ctrl_as_ref=True, return_controls=False, want_info=False):
    """``sc.tl.score_genes``: per cell the mean of the set minus the mean of its control genes (``srx_score_genes``).
    ``gene_list``: one list (indices, a mask, or names resolved through ``adata.var_names``) or a dict of lists scored in one
    call.  Returns an ``n_obs`` array for one list, a dict of arrays for a dict; with ``return_controls`` also the control
    lists, with ``want_info`` the info dict (``dropped``: the names that were not found).  An ``IMAnnData`` receives the scores
    in ``obs`` (key ``"score"`` for a single list)."""
    m = _matrix(adata)
    n, n_vars = int(m.info().n_rows), int(m.info().n_cols)
    names, lists, dropped = _named_sets(adata, gene_list)
    pool = None
    if gene_pool is not None:
        pool = resolve_genes(adata.var_names if isinstance(adata, IMAnnData) else None, gene_pool, n_vars)[0]
    ptr, flat = _pack(lists)
    cap = control_capacity(lists, ctrl_size, n_bins, n_vars if pool is None else pool.size)
    score = np.zeros((n, len(lists)), dtype=np.float64)
    cptr, cgenes = np.zeros(len(lists) + 1, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
    o, i = _opts(ctrl_size, n_bins, seed, ctrl_as_ref), F.ScoreGenesInfo()
    F.check(F.lib().srx_score_genes(m.handle, F.ptr(ptr), F.ptr(flat), len(lists), None if pool is None else F.ptr(pool),
                                    0 if pool is None else pool.size, C.byref(o), F.ptr(score) if score.size else F.ptr(np.zeros(1)),
                                    F.ptr(cptr), F.ptr(cgenes), cap, C.byref(i)), m.ctx.handle)
    cols = {k: np.ascontiguousarray(score[:, s]) for s, k in enumerate(names)}
    if isinstance(adata, IMAnnData):
        adata.obs.update(cols)
    out = [cols if isinstance(gene_list, dict) else cols["score"]]
    if return_controls:
        ctrl = {k: cgenes[int(cptr[s]):int(cptr[s + 1])].copy() for s, k in enumerate(names)}
        out.append(ctrl if isinstance(gene_list, dict) else ctrl["score"])
    if want_info:
        out.append(dict(_info(i), dropped=dropped))
    return out[0] if len(out) == 1 else tuple(out)


def cell_cycle_phase(s_score, g2m_score) -> np.ndarray:
    """scanpy's rule and order: "S" by default, "G2M" where G2M > S, "G1" where both are < 0."""
    s, g = np.asarray(s_score, dtype=np.float64), np.asarray(g2m_score, dtype=np.float64)
    phase = np.full(s.shape, "S", dtype=object)
    phase[g > s] = "G2M"
    phase[(s < 0) & (g < 0)] = "G1"
    return phase


def score_genes_cell_cycle(adata, s_genes, g2m_genes, n_bins=25, gene_pool=None, seed=0, want_info=False) -> dict:
    """``sc.tl.score_genes_cell_cycle``: both sets scored in ONE call with ``ctrl_size = min(len(s), len(g2m))`` (the sizes after
    names that are not found were dropped), then the phase by ``cell_cycle_phase`` on the host.  Returns ``S_score``,
    ``G2M_score`` and ``phase``; an ``IMAnnData`` receives the three in ``obs``."""
    names, lists, dropped = _named_sets(adata, {"S_score": s_genes, "G2M_score": g2m_genes})
    ctrl_size = min(len(lists[0]), len(lists[1]))
    if ctrl_size == 0:
        raise ValueError("score_genes_cell_cycle: a gene set is empty (not found: %r)" % (dropped,))
    scores, info = score_genes(adata, dict(zip(names, lists)), ctrl_size=ctrl_size, n_bins=n_bins, gene_pool=gene_pool, seed=seed,
                               want_info=True)
    out = dict(scores, phase=cell_cycle_phase(scores["S_score"], scores["G2M_score"]))
    if isinstance(adata, IMAnnData):
        adata.obs["phase"] = out["phase"]
    if want_info:
        out["info"] = dict(info, dropped=dropped)
    return out


def qc_gene_fractions(adata, qc_vars: dict) -> dict:
    """Per gene subset k of ``qc_vars`` (a mask over the genes, indices, or names): ``total_counts_<k>`` (the sum),
    ``pct_counts_<k>`` = 100 * sum / the cell's total (``srx_compute_sum(Row)``; 0 / 0 stays NaN) and ``n_genes_by_counts_<k>``,
    as ``sc.pp.calculate_qc_metrics(qc_vars=[k])`` names them.  ``n_genes_by_counts_<k>`` is the number of STORED entries of the
    cell in the subset: it differs from scanpy's count of values > 0 exactly where the matrix stores an explicit zero (or a
    negative value); a count matrix in canonical form has none.  An ``IMAnnData`` receives the columns in ``obs``."""
    m = _matrix(adata)
    keys = list(qc_vars)
    s, c = gene_list_sums(adata, [qc_vars[k] for k in keys])
    total = np.zeros(int(m.info().n_rows), dtype=np.float64)
    F.check(F.lib().srx_compute_sum(m.handle, F.ROW, F.ptr(total) if total.size else None), m.ctx.handle)
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for t, k in enumerate(keys):
            out["total_counts_" + k] = np.ascontiguousarray(s[:, t])
            out["pct_counts_" + k] = 100.0 * s[:, t] / total
            out["n_genes_by_counts_" + k] = np.ascontiguousarray(c[:, t])
    if isinstance(adata, IMAnnData):
        adata.obs.update(out)
    return out

"""ForceAtlas2 layout of the neighbour graph over libsrx_hip (``srx_draw_graph`` / ``srx_draw_graph_csr``): what
``sc.tl.draw_graph(layout="fa")`` gives ``obsm["X_draw_graph_fa"]``.

Not in the reference.  The method (Jacomy et al. 2014 with the defaults scanpy passes to the fa2 package: a Barnes-Hut
repulsion with integer masses over t-SNE's uniform pyramid, linear attraction and gravity, the adaptive speed of Gephi,
bit-identical from call to call) is defined in include/srx.h; every iteration runs on the device and nothing computes on
the CPU except ``fa2_speed``, the speed rule as host code.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import IMAnnData
from ._common import csr_triple, flat_info, graph_of
from .paga import paga_init_positions


def _opts(theta, scaling_ratio, gravity, jitter_tolerance, seed, n_iter, stop_after, levels, init_code, strong_gravity, linlog) -> F.Fa2Opts:
    return F.Fa2Opts(float(theta), float(scaling_ratio), float(gravity), float(jitter_tolerance), int(seed) & (2 ** 64 - 1), int(n_iter),
                     int(stop_after), int(levels), int(init_code), int(bool(strong_gravity)), int(bool(linlog)))


def _start(init, n: int):
    """(init code, the start as an n x 2 f64 array or None)."""
    if init is None:
        return F.FA2_INIT_RANDOM, None
    y0 = np.ascontiguousarray(init, dtype=np.float64)
    if y0.shape != (n, 2):
        raise ValueError("draw_graph: the start must be n x 2 = %d x 2" % n)
    return F.FA2_INIT_GIVEN, y0


def _init_pos(adata: IMAnnData, init_pos, seed: int):
    """``init_pos`` of ``draw_graph`` as (the start for ``_start``, its name for the params)."""
    if init_pos is None:
        return None, "random"
    if isinstance(init_pos, str) and init_pos == "paga":
        paga = adata.uns.get("paga")
        if paga is None:
            raise ValueError("draw_graph: init_pos='paga' needs adata.uns['paga']; run paga(adata) first")
        if "pos" not in paga:
            raise ValueError("draw_graph: init_pos='paga' needs adata.uns['paga']['pos'], the n_groups x 2 layout of the groups")
        return paga_init_positions(adata, np.asarray(paga["pos"], dtype=np.float64)[:, :2], paga.get("groups", "louvain"), seed), "paga"
    if isinstance(init_pos, str):
        if init_pos not in adata.obsm:
            raise ValueError("draw_graph: init_pos=%r is neither 'paga' nor a key of adata.obsm" % init_pos)
        return np.asarray(adata.obsm[init_pos], dtype=np.float64)[:, :2], init_pos
    return init_pos, "given"


def draw_graph(adata: IMAnnData, layout: str = "fa", init_pos=None, n_iter: int = 500, seed: int = 0, theta: float = 1.2,
               scaling_ratio: float = 2.0, gravity: float = 1.0, jitter_tolerance: float = 1.0, strong_gravity: bool = False,
               linlog: bool = False, levels: int = 0, stop_after: int = 0, key_added_ext=None) -> dict:
    """ForceAtlas2 layout of the connectivities that ``neighbors(adata, connectivities=True)`` left on the device (no host
    round trip).  ``init_pos``: None (hashed from ``seed``, in [0, 1)), an n x 2 array, a key of ``adata.obsm``, or "paga"
    (``paga_init_positions`` from ``adata.uns["paga"]["pos"]``).  Writes ``adata.obsm["X_draw_graph_" + (key_added_ext or
    layout)]`` (n x 2 f64) and ``adata.uns["draw_graph"]`` (``params`` and the call's ``srx_fa2_info`` under ``info``);
    returns the info."""
    if layout != "fa":
        raise ValueError("draw_graph: layout=%r is not supported; only 'fa' (ForceAtlas2) is" % (layout,))
    g = graph_of(adata, "draw_graph")
    n = adata.n_obs()
    start, name = _init_pos(adata, init_pos, seed)
    code, y0 = _start(start, n)
    out = np.zeros((n, 2), dtype=np.float64)
    info = F.Fa2Info()
    opts = _opts(theta, scaling_ratio, gravity, jitter_tolerance, seed, n_iter, stop_after, levels, code, strong_gravity, linlog)
    F.check(F.lib().srx_draw_graph(g.handle, C.byref(opts), F.ptr(y0) if y0 is not None and y0.size else None,
                                   F.ptr(out) if out.size else None, C.byref(info)), g.ctx.handle)
    adata.obsm["X_draw_graph_" + (key_added_ext or layout)] = out
    d = flat_info(info)
    adata.uns["draw_graph"] = {"params": {"layout": layout, "init_pos": name, "n_iter": d["n_iter"], "seed": int(seed), "theta": float(theta),
                                          "scaling_ratio": float(scaling_ratio), "gravity": float(gravity),
                                          "jitter_tolerance": float(jitter_tolerance), "strong_gravity": bool(strong_gravity),
                                          "linlog": bool(linlog)}, "info": d}
    return d


def draw_graph_csr(ctx, matrix, init_pos=None, n_iter: int = 500, seed: int = 0, theta: float = 1.2, scaling_ratio: float = 2.0,
                   gravity: float = 1.0, jitter_tolerance: float = 1.0, strong_gravity: bool = False, linlog: bool = False, levels: int = 0,
                   stop_after: int = 0):
    """Layout of any symmetric weighted graph: a scipy sparse matrix or an (indptr, indices, data) CSR triple with ascending
    columns, positive weights and no diagonal (``srx_draw_graph_csr`` validates on the device as ``srx_louvain_csr`` does).
    ``init_pos``: None or an n x 2 array.  Returns (layout n x 2 f64, info dict)."""
    indptr, indices, data = csr_triple(matrix, "draw_graph_csr")
    n = indptr.size - 1
    code, y0 = _start(init_pos, n)
    out = np.zeros((n, 2), dtype=np.float64)
    info = F.Fa2Info()
    opts = _opts(theta, scaling_ratio, gravity, jitter_tolerance, seed, n_iter, stop_after, levels, code, strong_gravity, linlog)
    F.check(F.lib().srx_draw_graph_csr(ctx.handle, F.ptr(indptr), F.ptr(indices) if indices.size else None,
                                       F.ptr(data) if data.size else None, n, C.byref(opts),
                                       F.ptr(y0) if y0 is not None and y0.size else None, F.ptr(out) if out.size else None,
                                       C.byref(info)), ctx.handle)
    return out, flat_info(info)


def draw_graph_forces(ctx, matrix, y, theta: float = 1.2, levels: int = 0, scaling_ratio: float = 2.0, gravity: float = 1.0,
                      strong_gravity: bool = False, linlog: bool = False):
    """The diagnostic ``srx_draw_graph_forces``: (rep n x 2, grav n x 2, attr n x 2, masses n uint32, info dict) at the
    positions ``y`` (n x 2) of the graph ``matrix`` (as for ``draw_graph_csr``)."""
    indptr, indices, data = csr_triple(matrix, "draw_graph_forces")
    n = indptr.size - 1
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.shape != (n, 2):
        raise ValueError("draw_graph_forces: the positions must be n x 2 = %d x 2" % n)
    rep, grav, attr, mass = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2)), np.zeros(n, dtype=np.uint32)
    fi = F.Fa2ForceInfo()
    opts = _opts(theta, scaling_ratio, gravity, 1.0, 0, 0, 0, levels, F.FA2_INIT_GIVEN, strong_gravity, linlog)
    F.check(F.lib().srx_draw_graph_forces(ctx.handle, F.ptr(indptr), F.ptr(indices) if indices.size else None,
                                          F.ptr(data) if data.size else None, n, F.ptr(y) if n else None, C.byref(opts),
                                          F.ptr(rep) if n else None, F.ptr(grav) if n else None, F.ptr(attr) if n else None,
                                          F.ptr(mass) if n else None, C.byref(fi)), ctx.handle)
    info = {"levels": fi.levels, "side": fi.side, "lo": (fi.lo[0], fi.lo[1]), "total_mass": fi.total_mass,
            "cells_accepted": fi.cells_accepted, "cells_exact": fi.cells_exact, "pairs_exact": fi.pairs_exact,
            "pairs_coincident": fi.pairs_coincident}
    return rep, grav, attr, mass, info


def graph_layout(graph) -> np.ndarray:
    """The layout the last ``srx_draw_graph`` left with a ``Graph`` handle (``srx_graph_layout_fetch``)."""
    out = np.zeros((graph.info()["n"], 2), dtype=np.float64)
    F.check(F.lib().srx_graph_layout_fetch(graph.handle, F.ptr(out) if out.size else None), graph.ctx.handle)
    return out


def fa2_speed(n: int, swing: float, traction: float, jitter_tolerance: float = 1.0, speed: float = 1.0, speed_efficiency: float = 1.0):
    """The speed rule of an iteration (``srx_fa2_speed``, host only): the new (speed, speed_efficiency)."""
    s, e = C.c_double(float(speed)), C.c_double(float(speed_efficiency))
    F.check(F.lib().srx_fa2_speed(int(n), float(swing), float(traction), float(jitter_tolerance), C.byref(s), C.byref(e)), None)
    return s.value, e.value

"""Diffusion maps and pseudotime over libsrx_hip (``srx_diffmap`` / ``srx_diffmap_csr`` / ``srx_dpt`` / ``srx_dpt_from``): what
fills ``obsm["X_diffmap"]``, ``uns["diffmap_evals"]`` and ``obs["dpt_pseudotime"]``.

Not in the reference.  The method (scanpy's symmetric transition operator, its ``n_comps`` algebraically largest eigenpairs by
a thick-restart Lanczos iteration on the device, DPT's distance from a root without branchings) is defined in include/srx.h;
nothing computes on the CPU except the projected eigen-problem of at most 129 x 129 once per restart.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import IMAnnData
from ._common import csr_triple, flat_info, graph_of


_info_dict = flat_info          # the name this module had for it


def _opts(n_comps, ncv, tol, max_matvecs, seed, density_normalize) -> F.DiffmapOpts:
    return F.DiffmapOpts(float(tol), int(seed) & (2 ** 64 - 1), int(n_comps), int(ncv), int(max_matvecs), int(bool(density_normalize)))


def _room(n: int, n_comps: int):
    """Output arrays for a call that may clamp n_comps to n - 1."""
    m = max(min(int(n_comps) or 15, F.DIFFMAP_MAX_COMPS), 1)
    return np.zeros(m, dtype=np.float64), np.zeros(max(n, 1) * m, dtype=np.float64)


def diffmap(adata: IMAnnData, n_comps: int = 15, ncv: int = 0, tol: float = 0.0, max_matvecs: int = 0, seed: int = 0,
            density_normalize: bool = True, key_added: str = "X_diffmap") -> dict:
    """Eigenpairs of the transition operator of the connectivities that ``neighbors(adata, connectivities=True)`` left on the
    device (no host round trip).  Writes ``adata.obsm[key_added]`` (n x n_comps f64, descending eigenvalues),
    ``adata.uns["diffmap_evals"]`` and ``adata.uns["diffmap"]`` (the call's ``srx_diffmap_info``); returns the info.
    ``SrxError`` with code ``E_NOCONV`` when ``max_matvecs`` products did not reach ``tol``."""
    g = graph_of(adata, "diffmap")
    n = adata.n_obs()
    evals, evecs = _room(n, n_comps)
    info = F.DiffmapInfo()
    opts = _opts(n_comps, ncv, tol, max_matvecs, seed, density_normalize)
    F.check(F.lib().srx_diffmap(g.handle, C.byref(opts), F.ptr(evals), F.ptr(evecs), C.byref(info)), g.ctx.handle)
    m = int(info.n_comps)
    adata.obsm[key_added] = evecs[:n * m].reshape(n, m).copy()
    adata.uns["diffmap_evals"] = evals[:m].copy()
    adata.uns["diffmap"] = flat_info(info)
    return adata.uns["diffmap"]


def graph_diffmap(graph):
    """(eigenvalues, eigenvectors n x n_comps) the last successful ``srx_diffmap`` left with a ``Graph`` handle."""
    m = C.c_uint32()
    F.check(F.lib().srx_graph_diffmap_fetch(graph.handle, None, None, C.byref(m)), graph.ctx.handle)
    n = graph.info()["n"]
    evals, evecs = np.zeros(m.value), np.zeros((n, m.value))
    F.check(F.lib().srx_graph_diffmap_fetch(graph.handle, F.ptr(evals), F.ptr(evecs), None), graph.ctx.handle)
    return evals, evecs


def graph_transitions(graph) -> np.ndarray:
    """The values of the transition operator T in the order of the connectivities' CSR (``srx_graph_transitions_fetch``)."""
    out = np.zeros(graph.info()["nnz_connectivities"], dtype=np.float64)
    F.check(F.lib().srx_graph_transitions_fetch(graph.handle, F.ptr(out) if out.size else None), graph.ctx.handle)
    return out


def dpt(adata: IMAnnData, root: int, cap: float = 0.0, key_added: str = "dpt_pseudotime") -> np.ndarray:
    """Pseudotime from ``root`` out of the eigenpairs the graph handle holds (``srx_dpt``; ``cap=0``: 0.9994).  Writes
    ``adata.obs[key_added]`` and returns it."""
    g = graph_of(adata, "diffmap")
    out = np.zeros(adata.n_obs(), dtype=np.float64)
    F.check(F.lib().srx_dpt(g.handle, int(root), float(cap), F.ptr(out)), g.ctx.handle)
    adata.obs[key_added] = out
    return out


def dpt_from(ctx, evals, evecs, root: int, cap: float = 0.0) -> np.ndarray:
    """Pseudotime from eigenpairs on the host (``srx_dpt_from``), e.g. what ``diffmap_csr`` returned."""
    evals = np.ascontiguousarray(evals, dtype=np.float64)
    evecs = np.ascontiguousarray(evecs, dtype=np.float64)
    if evecs.ndim != 2 or evals.shape != (evecs.shape[1],):
        raise ValueError("dpt_from: evals (m) and evecs (n x m) expected")
    n, m = evecs.shape
    out = np.zeros(n, dtype=np.float64)
    F.check(F.lib().srx_dpt_from(ctx.handle, F.ptr(evals), F.ptr(evecs), n, m, int(root), float(cap), F.ptr(out)), ctx.handle)
    return out


def diffmap_csr(ctx, matrix, n_comps: int = 15, ncv: int = 0, tol: float = 0.0, max_matvecs: int = 0, seed: int = 0,
                density_normalize: bool = True):
    """Eigenpairs for any symmetric weighted graph: a scipy sparse matrix or an (indptr, indices, data) CSR triple with
    ascending columns, positive weights, no diagonal and no empty row (``srx_diffmap_csr`` validates on the device as
    ``srx_louvain_csr`` does).  Returns (eigenvalues, eigenvectors n x n_comps f64, info dict)."""
    indptr, indices, data = csr_triple(matrix, "diffmap_csr")
    n = indptr.size - 1
    evals, evecs = _room(n, n_comps)
    info = F.DiffmapInfo()
    opts = _opts(n_comps, ncv, tol, max_matvecs, seed, density_normalize)
    F.check(F.lib().srx_diffmap_csr(ctx.handle, F.ptr(indptr), F.ptr(indices) if indices.size else None,
                                    F.ptr(data) if data.size else None, n, C.byref(opts), F.ptr(evals), F.ptr(evecs), C.byref(info)),
            ctx.handle)
    k = int(info.n_comps)
    return evals[:k].copy(), evecs[:n * k].reshape(n, k).copy(), flat_info(info)

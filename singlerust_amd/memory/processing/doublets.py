"""Doublet detection over libsrx_hip (``srx_doublets_*``): what ``sc.pp.scrublet`` gives ``obs["doublet_score"]`` and
``obs["predicted_doublet"]``, between the filters and everything else.

Not in the reference.  The method (synthetic doublets as sums of cell pairs, projected onto the fitted PCA, scored by the
share of synthetic rows among their neighbours, called by a histogram threshold) is restated in include/srx.h; every
intermediate stays in HBM, only the simulated scores come to the host for the threshold.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import DeviceCsr, IMAnnData
from ._common import OwnedHandle, flat_info

_TABLES = {"scores_obs": (F.DOUBLETS_SCORES_OBS, np.float64), "scores_sim": (F.DOUBLETS_SCORES_SIM, np.float64),
           "se_obs": (F.DOUBLETS_SE_OBS, np.float64), "se_sim": (F.DOUBLETS_SE_SIM, np.float64), "z": (F.DOUBLETS_Z, np.float64),
           "predicted": (F.DOUBLETS_PREDICTED, np.uint8), "points": (F.DOUBLETS_POINTS, np.float64),
           "parents": (F.DOUBLETS_PARENTS, np.uint64), "knn": (F.DOUBLETS_KNN, np.uint32)}


def _opts(sim_ratio=0.0, expected_rate=0.0, stdev_rate=0.0, target_sum=None, log1p=False, threshold=0.0, seed=0, k=0,
          n_dims=0) -> F.DoubletOpts:
    bits = (F.BACKED_NORMALIZE if target_sum is not None else 0) | (F.BACKED_LOG1P if log1p else 0)
    return F.DoubletOpts(float(sim_ratio), float(expected_rate), float(stdev_rate), float(target_sum or 0.0), float(threshold),
                         int(seed) & (2 ** 64 - 1), int(k), int(n_dims or 0), bits, 0)


class Doublets(OwnedHandle):
    """Owning wrapper of an ``srx_doublets``: the point block, the neighbour list, the parents and the scores on the device."""

    _free = "srx_doublets_free"

    def info(self) -> dict:
        i = F.DoubletInfo()
        F.check(F.lib().srx_doublets_info_get(self._h, C.byref(i)), self.ctx.handle)
        return flat_info(i)

    def fetch(self, which: str) -> np.ndarray:
        """One table: "scores_obs" / "se_obs" / "z" (n f64), "scores_sim" / "se_sim" (n_sim f64), "predicted" (n bool),
        "points" ((n + n_sim) x d f64), "parents" (n_sim x 2 uint64), "knn" ((n + n_sim) x k_adj uint32)."""
        i = self.info()
        n, n_sim = i["n_obs"], i["n_sim"]
        code, dtype = _TABLES[which]
        shape = {"scores_obs": (n,), "se_obs": (n,), "z": (n,), "predicted": (n,), "scores_sim": (n_sim,), "se_sim": (n_sim,),
                 "points": (n + n_sim, i["d"]), "parents": (n_sim, 2), "knn": (n + n_sim, i["k_adj"])}[which]
        out = np.zeros(shape, dtype=dtype)
        F.check(F.lib().srx_doublets_fetch(self._h, code, F.ptr(out)), self.ctx.handle)
        return out.astype(bool) if which == "predicted" else out

    def call(self, threshold: float = 0.0) -> dict:
        """Scrublet's ``call_doublets(threshold=...)`` on the resident scores; 0 = the automatic threshold again."""
        i = F.DoubletInfo()
        F.check(F.lib().srx_doublets_call(self._h, float(threshold), C.byref(i)), self.ctx.handle)
        return flat_info(i)


def _matrix(x) -> DeviceCsr:
    return x.x() if isinstance(x, IMAnnData) else x


def simulate_doublets(counts, n_sim=None, seed=0, parents=None):
    """(DeviceCsr of the synthetic rows, parents n_sim x 2 uint64): ``srx_doublets_simulate``.  ``counts``: an ``IMAnnData`` or a
    ``DeviceCsr`` in CSR storage; ``parents`` (n_sim x 2) given, or hashed from ``seed``; ``n_sim`` defaults to the rows of
    ``parents``, or to twice the cells."""
    m = _matrix(counts)
    if parents is not None:
        parents = np.ascontiguousarray(parents, dtype=np.uint64).reshape(-1, 2)
        if n_sim is None:
            n_sim = parents.shape[0]
        if parents.shape[0] != int(n_sim):
            raise ValueError("simulate_doublets: parents must be n_sim x 2")
    elif n_sim is None:
        n_sim = 2 * int(m.info().n_rows)
    used = np.zeros((int(n_sim), 2), dtype=np.uint64)
    h = C.c_void_p()
    F.check(F.lib().srx_doublets_simulate(m.handle, int(n_sim), int(seed) & (2 ** 64 - 1), F.ptr(parents) if parents is not None and parents.size else None,
                                          C.byref(h), F.ptr(used) if used.size else None), m.ctx.handle)
    return DeviceCsr(m.ctx, h), used


def doublet_scores_knn(ctx, indices, n_obs, expected_rate=0.05, stdev_rate=0.02):
    """(scores, standard errors) of every row of a neighbour list ((n_obs + n_sim) x k_adj): ``srx_doublet_scores_knn``."""
    idx = np.ascontiguousarray(indices, dtype=np.uint32)
    if idx.ndim != 2:
        raise ValueError("doublet_scores_knn: indices ((n_obs + n_sim) x k_adj) expected")
    n_tot, k_adj = idx.shape
    score, se = np.zeros(n_tot), np.zeros(n_tot)
    F.check(F.lib().srx_doublet_scores_knn(ctx.handle, F.ptr(idx) if idx.size else None, int(n_obs), n_tot - int(n_obs), k_adj,
                                           float(expected_rate), float(stdev_rate), F.ptr(score), F.ptr(se)), ctx.handle)
    return score, se


def doublets_threshold(scores):
    """(threshold, found, smoothing rounds) of simulated scores: ``srx_doublets_threshold`` (host code, no device)."""
    x = np.ascontiguousarray(scores, dtype=np.float64).ravel()
    t, found, rounds = C.c_double(), C.c_int32(), C.c_uint32()
    F.check(F.lib().srx_doublets_threshold(F.ptr(x) if x.size else None, x.size, C.byref(t), C.byref(found), C.byref(rounds)))
    return t.value, bool(found.value), int(rounds.value)


def scrublet(fitted, counts, **opts) -> Doublets:
    """The whole chain (``srx_doublets_result``).  ``fitted``: the matrix that holds the PCA result (a clone of the counts after
    the pipeline); ``counts``: the raw counts of the same cells and genes, CSR.  Keyword arguments: ``sim_ratio``,
    ``expected_rate``, ``stdev_rate``, ``threshold``, ``seed``, ``k``, ``n_dims``, and what was applied to ``fitted`` before its
    fit: ``target_sum`` (normalize_total) and ``log1p``.  Where ``counts`` is an ``IMAnnData`` it receives
    ``obs["doublet_score"]``, ``obs["predicted_doublet"]`` and ``uns["scrublet"]``."""
    f, c = _matrix(fitted), _matrix(counts)
    o = _opts(**opts)
    h = C.c_void_p()
    F.check(F.lib().srx_doublets_result(f.handle, c.handle, C.byref(o), C.byref(h), None), c.ctx.handle)
    d = Doublets(c.ctx, h)
    for a in (counts, fitted):
        if isinstance(a, IMAnnData):
            a.obs["doublet_score"] = d.fetch("scores_obs")
            a.obs["predicted_doublet"] = d.fetch("predicted")
            a.uns["scrublet"] = d.info()
    return d

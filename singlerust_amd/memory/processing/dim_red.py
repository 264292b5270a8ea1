"""``single_rust::memory::processing::dim_red`` (src/memory/processing/dim_red/mod.rs)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F
from ...anndata import FeatureSelection, IMAnnData
from .. import statistics
from ._common import OwnedHandle


def select_features(adata: IMAnnData, feature_selection) -> np.ndarray:
    """dim_red/mod.rs:123-156: feature indices in selection order (Vec<usize>)."""
    fs = feature_selection
    if isinstance(fs, FeatureSelection.HighlyVariable):            # :135-140
        g = adata.n_vars()
        out = np.zeros(min(int(fs.n), g), dtype=np.uint64)
        n_out = C.c_uint64(0)
        F.check(F.lib().srx_select_hvg(adata.x().handle, int(fs.n), F.ptr(out) if out.size else None,
                                       C.byref(n_out)), adata.x().ctx.handle)
        return out[: n_out.value]
    if isinstance(fs, FeatureSelection.HighlyVariableCol):         # :125-134
        if fs.col not in adata.var:
            raise KeyError(f"Error accessing column '{fs.col}'")
        mask = np.asarray(adata.var[fs.col])
        if mask.dtype != np.bool_:
            raise TypeError(f"Column '{fs.col}' is not boolean")
        return np.nonzero(mask)[0].astype(np.uint64)
    if isinstance(fs, FeatureSelection.Randomized):                # :141-146 (thread_rng: unseeded)
        idx = np.random.default_rng().permutation(adata.n_vars()).astype(np.uint64)
        return idx[: int(fs.n)]
    if isinstance(fs, FeatureSelection.VarianceThreshold):         # :147-153
        from ...anndata import Direction
        var = statistics.compute_variance(adata, Direction.Column)
        return np.nonzero(var > fs.threshold)[0].astype(np.uint64)
    if isinstance(fs, FeatureSelection.NoSelection) or fs is None:  # :154
        return np.arange(adata.n_vars(), dtype=np.uint64)
    raise TypeError(f"unknown FeatureSelection {fs!r}")


def pca_inplace(adata: IMAnnData, n_components=None, center=None, scale=None, n_threads=None,
                feature_selection=FeatureSelection.None_, svd_mode=None, *, block=0, max_iter=0, tol=0.0,
                seed=0, store_loadings=False, solver=0) -> F.PcaInfo:
    """dim_red/mod.rs:24-94.  Stores obsm["X_pca"] (n_obs x n_pc f64), the only output the
    reference keeps (:105-106); with store_loadings also varm["PCA_loadings"] in the layout
    of :108-118.  ``svd_mode`` (FaerSVD / LapackSVD marker) is accepted and ignored: the GPU
    path is a randomized subspace iteration on CSR x dense-panel SpMMs."""
    sel = select_features(adata, feature_selection)
    k = int(sel.shape[0])
    n_pc = min(2 if n_components is None else int(n_components), k)             # :52
    opts = F.PcaOpts(-1 if n_components is None else int(n_components),
                     -1 if center is None else int(bool(center)),
                     -1 if scale is None else int(bool(scale)),
                     -1 if n_threads is None else int(n_threads),
                     int(block), int(max_iter), int(solver), float(tol), int(seed))
    n = adata.n_obs()
    scores = np.zeros((n, n_pc), dtype=np.float64)
    comps = np.zeros((k, n_pc), dtype=np.float64)
    evr = np.zeros(n_pc, dtype=np.float64)
    mean = np.zeros(k, dtype=np.float64)
    std = np.zeros(k, dtype=np.float64)
    info = F.PcaInfo()
    F.check(F.lib().srx_pca(adata.x().handle, F.ptr(sel), k, C.byref(opts), F.ptr(scores), F.ptr(comps),
                            F.ptr(evr), F.ptr(mean), F.ptr(std), C.byref(info)), adata.x().ctx.handle)
    adata.obsm["X_pca"] = scores                                                # :105-106
    adata.uns["pca"] = {"components": comps, "explained_variance_ratio": evr, "mean": mean, "std": std,
                        "selected_features": sel, "n_iter": info.n_iter, "residual": info.residual,
                        "solver": info.solver, "center": True if center is None else bool(center),
                        "scale": True if scale is None else bool(scale)}
    if store_loadings:                                                          # :108-118
        full = np.zeros((adata.n_vars(), n_pc), dtype=np.float64)
        F.check(F.lib().srx_pca_loadings(F.ptr(comps), F.ptr(std), F.ptr(sel), k, n_pc, adata.n_vars(),
                                         F.ptr(full)))
        adata.varm["PCA_loadings"] = full
    return info


ABSENT = np.iinfo(np.uint64).max          # feature-map entry of a model gene the query does not have


class PcaModel(OwnedHandle):
    """A fitted PCA held on the device (``srx_pca_model``): the reference's ``Pca`` after ``fit``, whose
    ``transform`` (src/shared/processing/pca/mod.rs:156-185) projects other cells into the same PC space."""

    _free = "srx_pca_model_free"

    @classmethod
    def from_result(cls, adata: IMAnnData) -> "PcaModel":
        """The model the last PCA on ``adata`` left in HBM (``pca_inplace`` / the pipeline), copied on the device."""
        h = C.c_void_p()
        F.check(F.lib().srx_pca_model_from_result(adata.x().handle, C.byref(h)), adata.x().ctx.handle)
        return cls(adata.x().ctx, h)

    @classmethod
    def from_parts(cls, ctx, components, mean=None, std=None, selected_features=None, center=True,
                   scale=True) -> "PcaModel":
        """A model from host arrays: components k x n_pc, mean / std k (as ``pca_inplace`` stores them)."""
        comps = np.ascontiguousarray(components, dtype=np.float64)
        if comps.ndim != 2:
            raise ValueError("components must be k x n_pc")
        k, n_pc = comps.shape
        mean = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
        std = None if std is None else np.ascontiguousarray(std, dtype=np.float64)
        sel = None if selected_features is None else np.ascontiguousarray(selected_features, dtype=np.uint64)
        for name, a in (("mean", mean), ("std", std), ("selected_features", sel)):
            if a is not None and a.shape != (k,):
                raise ValueError(f"{name} must have k = {k} entries")
        h = C.c_void_p()
        F.check(F.lib().srx_pca_model_create(ctx.handle, k, n_pc, F.ptr(comps), F.ptr(mean), F.ptr(std), F.ptr(sel),
                                             int(bool(center)), int(bool(scale)), C.byref(h)), ctx.handle)
        return cls(ctx, h)

    @classmethod
    def from_uns(cls, adata: IMAnnData) -> "PcaModel":
        """The model ``pca_inplace`` stored in ``uns["pca"]`` (host arrays; center / scale default to the reference's true)."""
        u = adata.uns["pca"]
        return cls.from_parts(adata.x().ctx, u["components"], u["mean"], u["std"], u["selected_features"],
                              u.get("center", True), u.get("scale", True))

    def info(self):
        """(k, n_pc, selected features or None)."""
        k, n_pc = C.c_uint64(0), C.c_uint64(0)
        F.check(F.lib().srx_pca_model_info(self._h, C.byref(k), C.byref(n_pc), None), self.ctx.handle)
        sel = np.zeros(k.value, dtype=np.uint64)
        rc = F.lib().srx_pca_model_info(self._h, None, None, F.ptr(sel))
        return int(k.value), int(n_pc.value), (sel if rc == F.OK else None)


def feature_map_by_names(model_names, query_names) -> np.ndarray:
    """Feature map of ``pca_transform``: for every model gene (by name) its column in the query, ``ABSENT`` where the
    query does not have it."""
    where = {n: i for i, n in enumerate(query_names)}
    return np.array([where.get(n, ABSENT) for n in model_names], dtype=np.uint64)


def pca_transform(query: IMAnnData, model: PcaModel, feature_map=None, *, target_sum=None,
                  log1p=False) -> np.ndarray:
    """Pca::transform (pca/mod.rs:156-185) of the cells of ``query``: n_obs x n_pc f64 scores.  ``feature_map``: the query
    column of each model gene (``ABSENT`` for a missing one; None = the model's own selected features, the query has the
    fitted matrix's gene axis).  ``target_sum`` applies normalize_total(target_sum, Row) and ``log1p`` ln_1p to the raw values
    on the fly; the query's values are left as they are."""
    fm = None if feature_map is None else np.ascontiguousarray(feature_map, dtype=np.uint64)
    bits = (F.BACKED_NORMALIZE if target_sum is not None else 0) | (F.BACKED_LOG1P if log1p else 0)
    k, n_pc, _ = model.info()
    if fm is not None and fm.shape != (k,):
        raise ValueError(f"feature_map must have k = {k} entries")
    out = np.zeros((query.n_obs(), n_pc), dtype=np.float64)
    F.check(F.lib().srx_pca_transform(model.handle, query.x().handle, F.ptr(fm), float(target_sum or 0.0), bits,
                                      F.ptr(out) if out.size else None), query.x().ctx.handle)
    return out


def pca_transform_inplace(query: IMAnnData, model: PcaModel, feature_map=None, *, target_sum=None,
                          log1p=False) -> None:
    """``pca_transform`` stored as obsm["X_pca"]."""
    query.obsm["X_pca"] = pca_transform(query, model, feature_map, target_sum=target_sum, log1p=log1p)

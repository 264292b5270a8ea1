"""srx_umap / srx_umap_csr / srx_graph_embedding_fetch on the device against the definition of include/srx.h (tests/umap_ref.py):
exact counters and element-wise positions after 1 and 3 epochs on every graph family, determinism and stop_after, quality over
a full run against the reference's own seed-to-seed range (tests/golden/umap_kat.json), the resident path and the refusals.

Tolerance of the element-wise comparison.  For each case D = max |f64 numpy - longdouble numpy| of the final positions is
computed here on the CPU, and the device gets 32 D: its pow and its summation order differ from numpy's by a few ulp per term
and a row sums up to 6 x its length terms.  Measured on the planted 800-point graph (dim 2, R = 5, |y| <= 12.2): D_PLANTED_1
after one epoch, D_PLANTED_3 after three epochs of the 3-epoch schedule and D_PLANTED_3_OF_200 after three of the 200-epoch
schedule, where nearly every entry acts in every epoch (profiles/umap.md has every case).  After 10 epochs D is already 9e-8
(the map is chaotic), so the element-wise comparison stops at 3 epochs; an f32 evaluation is 5.6e-6 away after ONE epoch,
which is why the arithmetic is f64."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import umap_ref as ref

pytestmark = pytest.mark.gpu

A, B = 1.577, 0.895
# max |f64 - longdouble| of the reference on the planted graph, dim 2, R = 5 (this file's docstring), rounded up; the device gets
# TOL_FACTOR times the D of each case
D_PLANTED_1 = 1.5e-15
D_PLANTED_3 = 4.5e-14
D_PLANTED_3_OF_200 = 1.8e-12
TOL_FACTOR = 32
DIMS = (2, 3)
RATES = (0, 1, 5)
SCHEDULES = ((1, 0), (3, 0), (200, 1), (200, 3))


def G():
    from singlerust_amd import _ffi
    return getattr(_ffi, "UMAP_GROUP", None)


def run(ctx, W, **kw):
    from singlerust_amd.memory.processing import umap_csr
    kw.setdefault("a", A)
    kw.setdefault("b", B)
    return umap_csr(ctx, W, **kw)


_GRAPHS = {}


def graph(name):
    """(W, Y0 n x 3) of a named case, built once."""
    if name not in _GRAPHS:
        if name == "planted":
            W = ref.planted()[2]
        elif name == "graph12":
            _GRAPHS[name] = ref.graph12()
            return _GRAPHS[name]
        elif name == "rows":
            W = ref.star_rows(G()) if G() else ref.every_length(130)
        elif name == "no_entries":
            W = sp.csr_matrix((5, 5))
        else:
            W = ref.ring(int(name[1:]))
        _GRAPHS[name] = (W, ref.random_start(W.shape[0], 3, 4242))
    return _GRAPHS[name]


_REF = {}


def reference(name, dim, rate, E, stop):
    """(Y f64, info, D) of the definition, computed once per case and left unchanged."""
    key = (name, dim, rate, E, stop)
    if key not in _REF:
        W, Y0 = graph(name)
        y0 = np.ascontiguousarray(Y0[:, :dim])
        Y, info, _ = ref.layout(W, y0, A, B, E, rate=rate, seed=11, stop_after=stop)
        Yl, infol, _ = ref.layout(W, y0, A, B, E, rate=rate, seed=11, stop_after=stop, dtype=np.longdouble)
        assert all(info[k] == infol[k] for k in ref.COUNTERS)
        D = float(np.abs(Y.astype(np.longdouble) - Yl).max()) if Y.size else 0.0
        _REF[key] = (Y, info, D)
    return _REF[key]


# ---- 4. exact counters, element-wise positions --------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("name", ["planted", "graph12", "rows", "n1", "n2", "n257", "n0", "no_entries"])
def test_counters_and_positions(ctx, name, dim):
    W, Y0 = graph(name)
    n = W.shape[0]
    y0 = np.ascontiguousarray(Y0[:, :dim])
    if name == "rows":
        lens = np.diff(W.indptr)
        g = G()
        assert lens.max() == 300 and ({g - 1, g, g + 1, 2 * g + 1} <= set(lens.tolist()) if g else set(range(1, 131)) <= set(lens.tolist()))
    for rate in RATES:
        for E, stop in SCHEDULES:
            Y, want, D = reference(name, dim, rate, E, stop)
            emb, info = run(ctx, W, n_components=dim, n_epochs=E, stop_after=stop, negative_sample_rate=rate, seed=11, init=y0)
            err = float(np.abs(emb - Y).max()) if Y.size else 0.0
            print("%s dim %d R %d E %d stop %d: samples %d negatives %d skipped %d active %d | D %.3e 32D %.3e device %.3e max|y| %.2f"
                  % (name, dim, rate, E, stop, info["samples"], info["negatives"], info["negatives_skipped"], info["entries_active"],
                     D, TOL_FACTOR * D, err, float(np.abs(Y).max()) if Y.size else 0.0))
            assert emb.shape == (n, dim) and emb.dtype == np.float64
            for k in ref.COUNTERS + ("n", "nnz", "n_epochs", "epochs_run", "dim"):
                assert info[k] == want[k], (k, info[k], want[k])
            assert info["a"] == A and info["b"] == B
            assert info["w_max"] == want["w_max"]
            assert np.isfinite(emb).all()
            assert err <= TOL_FACTOR * D
            if W.nnz == 0:
                assert np.array_equal(emb, y0) and info["samples"] == 0
    if name == "planted" and dim == 2:
        assert reference(name, 2, 5, 1, 0)[2] <= D_PLANTED_1 and reference(name, 2, 5, 3, 0)[2] <= D_PLANTED_3
        assert reference(name, 2, 5, 200, 3)[2] <= D_PLANTED_3_OF_200
    if name == "n2":
        assert reference(name, dim, 5, 3, 0)[1]["negatives_skipped"] > 0             # every other negative hits the vertex itself


def test_random_start_is_the_stated_hash(ctx):
    W = ref.ring(257)
    for dim in DIMS:
        y0 = ref.random_start(257, dim, 5)
        emb, info = run(ctx, W, n_components=dim, n_epochs=3, seed=5, init="random")
        emb2, info2 = run(ctx, W, n_components=dim, n_epochs=3, seed=5, init=y0)
        assert np.array_equal(emb.view(np.uint64), emb2.view(np.uint64))
        assert {k: v for k, v in info.items() if k != "ms"} == {k: v for k, v in info2.items() if k != "ms"}


# ---- 5. determinism and independence ------------------------------------------------------------------------------------------
def test_determinism_seed_and_stop_after(ctx):
    W, Y0 = graph("planted")
    y0 = np.ascontiguousarray(Y0[:, :2])
    full, info = run(ctx, W, n_epochs=6, seed=3, init=y0)
    again, info2 = run(ctx, W, n_epochs=6, seed=3, init=y0)
    assert np.array_equal(full.view(np.uint64), again.view(np.uint64))
    assert {k: v for k, v in info.items() if k != "ms"} == {k: v for k, v in info2.items() if k != "ms"}
    other, _ = run(ctx, W, n_epochs=6, seed=4, init=y0)
    assert not np.array_equal(full, other)
    assert np.isfinite(full).all() and np.isfinite(other).all()
    # stop_after = 3 is the first three epochs of the six-epoch schedule ...
    half, ih = run(ctx, W, n_epochs=6, stop_after=3, seed=3, init=y0)
    Y3, want3, _ = ref.layout(W, y0, A, B, 6, seed=3, stop_after=3)
    Y3l = ref.layout(W, y0, A, B, 6, seed=3, stop_after=3, dtype=np.longdouble)[0]
    D3 = float(np.abs(Y3 - Y3l).max())
    print("stop_after 3 of 6: D %.3e device %.3e" % (D3, np.abs(half - Y3).max()))
    assert ih["epochs_run"] == 3 and ih["n_epochs"] == 6 and all(ih[k] == want3[k] for k in ref.COUNTERS)
    assert np.abs(half - Y3).max() <= TOL_FACTOR * D3
    # ... and epochs 4..6 continued by hand in the reference from the device's Y^3 give the full run
    Y6, want6, _ = ref.layout(W, half, A, B, 6, seed=3, first_epoch=4)
    Y6l = ref.layout(W, half, A, B, 6, seed=3, first_epoch=4, dtype=np.longdouble)[0]
    D6 = float(np.abs(Y6 - Y6l).max())
    print("epochs 4..6 by hand: D %.3e device %.3e" % (D6, np.abs(full - Y6).max()))
    assert info["samples"] == want3["samples"] + want6["samples"]
    assert info["negatives_skipped"] == want3["negatives_skipped"] + want6["negatives_skipped"]
    assert np.abs(full - Y6).max() <= TOL_FACTOR * D6


# ---- 6. quality over a full run -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planted_800", "separated_20011"])
def test_quality_over_a_full_run(ctx, name):
    gold = ref.golden()["quality"][name]
    if name == "planted_800":
        x, lab, W = ref.planted()
        sub = None
    else:
        import louvain_ref
        W, lab = louvain_ref.fixture_graph(name)
        x = louvain_ref.FIXTURES[name]()[0]
        sub = np.sort(np.random.default_rng(gold["subsample_seed"]).choice(len(x), gold["subsample"], replace=False))
    assert gold["n"] == W.shape[0] and gold["nnz"] == W.nnz
    emb, info = run(ctx, W, n_epochs=200, seed=1, init="random")
    assert np.isfinite(emb).all() and info["epochs_run"] == 200
    tw, sil = ref.quality(x, emb, lab, sub)
    print(name, "trustworthiness", tw, "floor", gold["floor_trustworthiness"], "start", gold["start_trustworthiness"], "| silhouette", sil,
          "floor", gold["floor_silhouette"], "| max|y|", np.abs(emb).max(), "samples", info["samples"], "ms", info["ms"])
    assert info["samples"] == gold["seeds"][0]["samples"]                             # the schedule does not depend on the seed
    assert tw >= gold["floor_trustworthiness"] and sil >= gold["floor_silhouette"]
    assert tw > gold["start_trustworthiness"]


# ---- 7. the resident path -------------------------------------------------------------------------------------------------------
def test_resident_path(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import dim_red, graph_embedding, graph_labels, louvain, neighbors, umap
    from test_knn_gpu import _planted, _upload
    a = _upload(ctx, _planted())
    with pytest.raises(sr.SrxError):
        umap(a)                                                                      # no graph yet
    dim_red.pca_inplace(a, 20, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    neighbors(a, n_neighbors=15, connectivities=True)
    with pytest.raises(sr.SrxError):
        graph_embedding(a._graph)                                                    # no umap yet
    louvain(a)
    labels0 = a.obs["louvain"].copy()
    before = a._graph.fetch(F.GRAPH_CONNECTIVITIES)
    values = a.x_values().copy()
    scores = a.obsm["X_pca"].copy()
    info = umap(a, init="pca", n_epochs=50, seed=2)
    assert a.uns["umap"]["info"] == info and a.uns["umap"]["params"]["init"] == "pca"
    emb = a.obsm["X_umap"]
    assert emb.shape == (a.n_obs(), 2) and np.isfinite(emb).all()
    # the same bits going in (the start computed on the host from the fetched scores), the same bits coming out
    y0 = ref.pca_start(scores, 2)
    e2, i2 = run(ctx, before, a=0.0, b=0.0, n_epochs=50, seed=2, init=y0)
    assert np.array_equal(emb.view(np.uint64), e2.view(np.uint64))
    assert {k: v for k, v in info.items() if k != "ms"} == {k: v for k, v in i2.items() if k != "ms"}
    assert np.array_equal(graph_embedding(a._graph).view(np.uint64), emb.view(np.uint64))
    # labels, C, the matrix's values and its resident result (a touched matrix loses it) are as they were
    after = a._graph.fetch(F.GRAPH_CONNECTIVITIES)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(before, after))
    assert np.array_equal(graph_labels(a._graph), labels0)
    assert np.array_equal(a.x_values().view(np.uint8), values.view(np.uint8))
    fetched = np.zeros_like(scores)
    F.check(F.lib().srx_result_fetch(a.x().handle, F.ptr(fetched), None, None, None, None, None), ctx.handle)
    assert np.array_equal(fetched.view(np.uint64), scores.view(np.uint64))
    louvain(a, key_added="again")
    assert np.array_equal(a.obs["again"], labels0)
    # NULL opts: every default (500 epochs at this size, the fitted curve of (1.0, 0.5), R = 5, seed 0) with the PCA start
    dflt, di = np.zeros((a.n_obs(), 2)), F.UmapInfo()
    F.check(F.lib().srx_umap(a._graph.handle, a.x().handle, None, None, F.ptr(dflt), C.byref(di)), ctx.handle)
    info0 = umap(a, key_added="X_default")
    assert di.n_epochs == di.epochs_run == 500 and di.dim == 2 and (di.a, di.b) == (info0["a"], info0["b"])
    assert np.array_equal(dflt.view(np.uint64), a.obsm["X_default"].view(np.uint64)) and di.samples == info0["samples"]
    # three components on the same handle replace the embedding
    umap(a, init="pca", n_components=3, n_epochs=5, key_added="X_umap3")
    assert graph_embedding(a._graph).shape == (a.n_obs(), 3)
    assert np.array_equal(graph_embedding(a._graph).view(np.uint64), a.obsm["X_umap3"].view(np.uint64))


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import dim_red, neighbors
    from test_knn_gpu import _planted, _upload
    lib = F.lib()
    W = ref.ring(12)
    ip, ix, w = W.indptr.astype(np.uint64), W.indices.astype(np.uint32), W.data.astype(np.float64)
    y0 = ref.random_start(12, 3, 1)
    SENT = 12345.0

    def opts(**kw):
        d = dict(a=A, b=B, min_dist=0.5, spread=1.0, gamma=1.0, alpha0=1.0, seed=0, n_epochs=3, stop_after=0, n_components=2,
                 negative_sample_rate=5, init=F.UMAP_INIT_GIVEN, reserved_=0)
        d.update(kw)
        return F.UmapOpts(*[d[name] for name, _ in F.UmapOpts._fields_])

    def refused(o, init=y0, c=None, graph=None, mat=None, arrays=(ip, ix, w)):
        out = np.full((600 if graph is not None else 12, 3), SENT)
        info = F.UmapInfo()
        info.samples = 777
        h = (c or ctx).handle
        if graph is not None:
            rc = lib.srx_umap(graph, mat, C.byref(o), None if init is None else F.ptr(init), F.ptr(out), C.byref(info))
        else:
            rc = lib.srx_umap_csr(h, F.ptr(arrays[0]), F.ptr(arrays[1]), F.ptr(arrays[2]), 12, C.byref(o),
                                  None if init is None else F.ptr(init), F.ptr(out), C.byref(info))
        msg = lib.srx_last_error(h)
        assert rc == F.E_ARG and msg, (rc, msg)
        assert (out == SENT).all() and info.samples == 777                           # nothing written
        return msg.decode()

    for d in (0, 1, 4, -2):
        assert "n_components" in refused(opts(n_components=d))
    for r in (-1, 33):
        assert "negative_sample_rate" in refused(opts(negative_sample_rate=r))
    for v in (0.0, -1.0, np.nan, np.inf):
        assert "a and b" in refused(opts(a=v))
        assert "a and b" in refused(opts(b=v))
        assert "gamma" in refused(opts(gamma=v))
        assert "alpha0" in refused(opts(alpha0=v))
        assert "spread" in refused(opts(spread=v))
    for v in (-0.1, 1.5, np.nan):
        assert "min_dist" in refused(opts(min_dist=v))
    for e in (-1, 2 ** 20 + 1):
        assert "n_epochs" in refused(opts(n_epochs=e))
    assert "stop_after" in refused(opts(n_epochs=3, stop_after=4))
    assert "stop_after" in refused(opts(stop_after=-1))
    for v in (np.nan, np.inf, -np.inf):
        bad = y0.copy()
        bad[7, 1] = v
        assert "NaN or Inf" in refused(opts(), init=bad)
    assert "start positions" in refused(opts(), init=None)
    assert "start" in refused(opts(init=7))
    assert "PCA start" in refused(opts(init=F.UMAP_INIT_PCA))                       # srx_umap_csr has no matrix
    bw = w.copy()
    bw[0] = np.nextafter(bw[0], 2.0)
    assert "symmetric" in refused(opts(), arrays=(ip, ix, bw))                       # the validation of srx_louvain_csr
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    assert "sharded" in refused(opts(), c=c2)
    # the PCA start on a handle: no matrix, no result, too few components, another size, another context
    a = _upload(ctx, _planted())
    dim_red.pca_inplace(a, 20, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    neighbors(a, n_neighbors=15, connectivities=True)
    gh = a._graph.handle
    pca = opts(init=F.UMAP_INIT_PCA)
    assert "matrix" in refused(pca, init=None, graph=gh, mat=None)
    fresh = _upload(ctx, _planted())
    assert "no PCA result" in refused(pca, init=None, graph=gh, mat=fresh.x().handle)
    dim_red.pca_inplace(fresh, 2, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    assert "components" in refused(opts(init=F.UMAP_INIT_PCA, n_components=3), init=None, graph=gh, mat=fresh.x().handle)
    fewer = _upload(ctx, _planted()[:300])
    dim_red.pca_inplace(fewer, 5, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    assert "cells" in refused(pca, init=None, graph=gh, mat=fewer.x().handle)
    other = _upload(sr.Context(0), _planted())
    dim_red.pca_inplace(other, 5, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    assert "contexts" in refused(pca, init=None, graph=gh, mat=other.x().handle)
    assert "start positions" in refused(opts(), init=None, graph=gh)
    with pytest.raises(sr.SrxError):
        from singlerust_amd.memory.processing import graph_embedding
        graph_embedding(a._graph)                                                    # every call above left the handle as it was
    # the context is still usable
    emb, info = run(ctx, W, n_epochs=3, init=np.ascontiguousarray(y0[:, :2]))
    assert info["epochs_run"] == 3 and np.isfinite(emb).all()

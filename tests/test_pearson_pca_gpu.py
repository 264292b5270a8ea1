"""PCA of the Pearson residuals on the device (srx_pearson_gram / srx_pca_pearson) against the numpy restatement of its definition
(pearson_pca_ref.py: pearson_ref's long-double residuals, np.linalg.eigh in f64).

Bounds, u = 2^-53, against the long-double reference Z_ref:
  Gram         |G - Z_ref^T Z_ref|_ij <= (n + 32) u (|Z_ref|^T |Z_ref|)_ij   (the dot-product bound for n terms plus the 8-ulp
               element bound of test_pearson_gpu.py, doubled for a product)
  column sums  |s - sum_i z_ij| <= (n + 8) u sum_i |z_ij|
  mean         |mean - m_ref| <= (n + 8) u mean_i |z_ij|
  PCA          evr to 1e-5 relative; every requested component and its scores to 1e-5, Frobenius-normalised per component (the
               project's PCA gate), after the sign rule; asserted only after the REFERENCE has shown a relative
               eigenvalue gap >= 1e-3 for every requested component.
Every test prints the largest ratio it reached before it asserts.  The Gram shapes walk the tile edges (k 2 .. 130: one tile
with one, many and padded columns, two and three tiles per side), the rows an MFMA K-step of 4 and a slab of 64 (n 5 .. 257), and
chunk_cells = 64 / 100 put a chunk edge on and off a K-step."""
import ctypes as C
import functools

import numpy as np
import pytest

import pearson_pca_ref as P
import pearson_ref as R

pytestmark = pytest.mark.gpu
INF = float("inf")
TOT = {"all": 0, "selected": 1}


def F():
    from singlerust_amd import _ffi
    return _ffi


def upload(ctx, X, dtype=np.uint32, csc=False):
    import singlerust_amd as sr
    n, G, indptr, indices, values = (R.to_csc if csc else R.to_csr)(X, dtype)
    return sr.DeviceCsr.upload(ctx, n, G, indptr, indices, values, csc=csc)


def make_opts(theta=None, clip=None, totals="selected", center=1, chunk=0, n_pc=2, solver=0, scale=0):
    f = F()
    pca = f.PcaOpts(n_pc, -1, scale, -1, 0, 0, solver, 0.0, 0)
    return f.PearsonPcaOpts(f.PearsonOpts(0.0 if theta is None else theta, 0.0 if clip is None else clip), TOT[totals], center, chunk, pca)


def dev_gram(m, genes, **kw):
    g = np.ascontiguousarray(genes, dtype=np.uint64)
    gram, colsum, info, o = np.full((g.size, g.size), -7.0), np.full(g.size, -7.0), F().PearsonPcaInfo(), make_opts(**kw)
    F().check(F().lib().srx_pearson_gram(m.handle, F().ptr(g), g.size, C.byref(o), F().ptr(gram), F().ptr(colsum), C.byref(info)), m.ctx.handle)
    return gram, colsum, info


def dev_pca(m, genes, n_pc, **kw):
    g = np.ascontiguousarray(genes, dtype=np.uint64)
    n, k = int(m.info().n_rows), g.size
    scores, comps, evr, mean = np.full((n, n_pc), -7.0), np.full((k, n_pc), -7.0), np.full(n_pc, -7.0), np.full(k, -7.0)
    info, o = F().PearsonPcaInfo(), make_opts(n_pc=n_pc, **kw)
    F().check(F().lib().srx_pca_pearson(m.handle, F().ptr(g), k, C.byref(o), F().ptr(scores), F().ptr(comps), F().ptr(evr), F().ptr(mean),
                                        C.byref(info)), m.ctx.handle)
    return scores, comps, evr, mean, info


@functools.lru_cache(maxsize=None)
def gram_reference(n, k, theta, clip, totals):
    """The long-double reference of one Gram case: computed once, shared, read-only."""
    X, genes = P.gram_case(n, k)
    Z = P.residuals(X, genes, theta, clip, totals)
    out = P.gram(Z)
    for a in out:
        a.setflags(write=False)
    return out


def check_gram(gram, colsum, n, ref, what):
    g_ref, g_abs, s_ref, s_abs = ref
    gb, sb = P.gram_bound(n, g_abs), P.colsum_bound(n, s_abs)
    ge = np.abs(gram.astype(np.longdouble) - g_ref).astype(np.float64)
    se = np.abs(colsum.astype(np.longdouble) - s_ref).astype(np.float64)
    rg = float(np.max(ge / np.maximum(gb, 1e-300)))
    rs = float(np.max(se / np.maximum(sb, 1e-300)))
    print("pearson gram %s: max ratio %.3f (Gram) %.3f (column sums) of the bounds" % (what, rg, rs))
    assert np.array_equal(gram, gram.T), what                   # symmetric bit for bit
    assert np.all(ge <= gb), (what, rg)
    assert np.all(se <= sb), (what, rs)


# ---- the Gram alone -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 63, 64, 257])
@pytest.mark.parametrize("k", [2, 15, 16, 17, 33, 130])
def test_gram_at_every_tile_and_chunk_edge(ctx, k, n):
    X, genes = P.gram_case(n, k)
    m = upload(ctx, X)
    ref = gram_reference(n, k, None, None, "selected")
    for chunk in (0, 64, 100):
        gram, colsum, info = dev_gram(m, genes, chunk=chunk)
        assert info.n_cells == n and info.n_chunks == (1 if chunk == 0 else -(-n // min(chunk, n)))
        check_gram(gram, colsum, n, ref, "k=%d n=%d chunk=%d" % (k, n, chunk))
        gram2, colsum2, _ = dev_gram(m, genes, chunk=chunk)
        assert np.array_equal(gram, gram2) and np.array_equal(colsum, colsum2)          # two calls are bit-identical
        if n >= R.FEATURES_FROM:
            z = int(np.nonzero(genes == 0)[0][0])                                         # the listed all-zero gene: a column of zeros
            assert np.all(gram[z] == 0.0) and np.all(gram[:, z] == 0.0) and colsum[z] == 0.0
    m.free()


@pytest.mark.parametrize("totals", P.TOTALS)
@pytest.mark.parametrize("theta", [100.0, INF], ids=["nb", "poisson"])
@pytest.mark.parametrize("clip", [1.0, None, INF], ids=["clip1", "default", "noclip"])
def test_gram_options_formats_and_storages(ctx, clip, theta, totals):
    n, k = 257, 33
    X, genes = P.gram_case(n, k)
    assert X[0].sum() == 0 and X[:, 0].sum() == 0 and 0 in genes                        # an empty cell, a listed all-zero gene
    ref = gram_reference(n, k, theta, clip, totals)
    if clip == 1.0:
        Z = P.residuals(X, genes, theta, clip, totals)
        assert (Z == 1).any() and (Z == -1).any()                                        # the clip is active on both sides
    for csc in (False, True):
        for dtype in (np.uint32, np.float64):
            m = upload(ctx, X, dtype, csc)
            for chunk in (0, 100):
                gram, colsum, info = dev_gram(m, genes, theta=theta, clip=clip, totals=totals, chunk=chunk)
                check_gram(gram, colsum, n, ref, "clip=%s theta=%s %s csc=%d %s chunk=%d" % (clip, theta, totals, csc, dtype.__name__, chunk))
                assert info.theta == theta and info.clip == (np.sqrt(float(n)) if clip is None else clip)
            m.free()


def test_the_two_totals_give_different_gram_matrices(ctx):
    n, k = 64, 17
    X, genes = P.gram_case(n, k)
    m = upload(ctx, X)
    a, _, ia = dev_gram(m, genes, totals="all")
    s, _, is_ = dev_gram(m, genes, totals="selected")
    assert ia.total == float(X.sum()) and is_.total == float(X[:, genes.astype(np.int64)].sum()) and ia.total > is_.total
    assert np.abs(a - s).max() > 1e-6 * np.abs(a).max()
    m.free()


# ---- the PCA -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted():
    X = P.planted_counts()
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def pca_reference(k, totals, center):
    Z = P.residuals(planted(), P.planted_genes(k), None, None, totals)
    ref = P.pca(np.asarray(Z, dtype=np.float64), 50, bool(center))
    ref["m_ld"] = (Z.sum(axis=0) / Z.shape[0]) if center else np.zeros(k, dtype=np.longdouble)
    ref["mean_abs"] = np.abs(Z).mean(axis=0).astype(np.float64)
    return ref


def per_component(got, ref):
    return float(np.max(np.linalg.norm(got - ref, axis=0) / np.linalg.norm(ref, axis=0)))


@pytest.mark.parametrize("center", [1, 0], ids=["centred", "uncentred"])
@pytest.mark.parametrize("totals", P.TOTALS)
@pytest.mark.parametrize("k", [64, 240])
@pytest.mark.parametrize("n_pc", [2, 50])
def test_pca_of_the_planted_counts(ctx, n_pc, k, totals, center):
    n = P.PLANTED_SHAPE[0]
    genes, ref = P.planted_genes(k), pca_reference(k, totals, center)
    gap = P.min_relative_gap(ref["values"], n_pc)
    assert gap >= 1e-3, gap                                                              # on the reference, before anything is compared
    m = upload(ctx, planted())
    scores, comps, evr, mean, info = dev_pca(m, genes, n_pc, totals=totals, center=center)
    e_evr = float(np.max(np.abs(evr - ref["evr"][:n_pc]) / ref["evr"][:n_pc]))
    e_v, e_s = per_component(comps, ref["components"][:, :n_pc]), per_component(scores, ref["scores"][:, :n_pc])
    mb = (n + 8) * P.U * ref["mean_abs"]
    e_m = np.abs(mean.astype(np.longdouble) - ref["m_ld"]).astype(np.float64)
    print("pearson pca k=%d n_pc=%d %s center=%d: evr %.2e components %.2e scores %.2e (gate 1e-5), mean %.3f of its bound, gap %.2e, "
          "residual %.1e, %d sweeps" % (k, n_pc, totals, center, e_evr, e_v, e_s, float(np.max(e_m / np.maximum(mb, 1e-300))), gap,
                                       info.pca.residual, info.pca.n_iter))
    assert info.pca.k == k and info.pca.n_pc == n_pc and info.pca.solver == F().SOLVER_GRAM and info.n_chunks == 1
    assert e_evr <= 1e-5 and e_v <= 1e-5 and e_s <= 1e-5
    assert np.all(e_m <= mb) and (center or np.all(mean == 0.0))
    # the sign rule: the largest-|.| entry of every component is positive
    assert all(comps[int(np.argmax(np.abs(comps[:, c]))), c] > 0 for c in range(n_pc))
    m.free()


def test_the_totals_flag_is_not_ignored(ctx):
    genes = P.planted_genes(64)
    m = upload(ctx, planted())
    _, _, evr_a, _, _ = dev_pca(m, genes, 2, totals="all")
    _, _, evr_s, _, _ = dev_pca(m, genes, 2, totals="selected")
    ra, rs = pca_reference(64, "all", 1)["evr"][:2], pca_reference(64, "selected", 1)["evr"][:2]
    assert np.abs(ra - rs).max() > 1e-3 * ra.max()                                       # they differ on this matrix ...
    assert np.abs(evr_a - evr_s).max() > 1e-3 * ra.max()                                 # ... and on the device
    m.free()


def test_chunks_csc_and_storage_give_the_same_pca(ctx):
    """The chunked route (a chunk edge every 100 cells) and a CSC handle at f64 storage against the same reference."""
    genes, ref = P.planted_genes(240), pca_reference(240, "selected", 1)
    for csc, dtype, chunk in ((False, np.uint32, 100), (True, np.float64, 0)):
        m = upload(ctx, planted(), dtype, csc)
        scores, comps, evr, _, info = dev_pca(m, genes, 10, chunk=chunk)
        assert info.n_chunks == (6 if chunk else 1)
        assert per_component(comps, ref["components"][:, :10]) <= 1e-5 and per_component(scores, ref["scores"][:, :10]) <= 1e-5
        assert np.allclose(evr, ref["evr"][:10], rtol=1e-5, atol=0)
        m.free()


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
def test_the_resident_scores_feed_the_neighbour_search(ctx):
    from singlerust_amd.memory.processing import knn_points
    f = F()
    genes = P.planted_genes(64)
    m = upload(ctx, planted())
    n = P.PLANTED_SHAPE[0]
    scores, _, _, _, _ = dev_pca(m, genes, 10)
    opts, info = f.KnnOpts(), f.KnnInfo()
    opts.k = 15
    idx, dist = np.zeros((n, 15), dtype=np.uint32), np.zeros((n, 15), dtype=np.float64)
    f.check(f.lib().srx_knn_result(m.handle, C.byref(opts), f.ptr(idx), f.ptr(dist), C.byref(info)), ctx.handle)
    idx_p, dist_p, _ = knn_points(ctx, scores, k=15)
    assert np.array_equal(idx, idx_p)                                                    # index for index
    m.free()


def test_no_model_of_a_residual_pca_and_no_state_left_behind(ctx):
    f = F()
    X = planted()
    genes = P.planted_genes(64)
    m = upload(ctx, X)
    fresh = m.clone()

    def ordinary(h):
        sel = np.sort(genes)
        o = f.PcaOpts(5, -1, -1, -1, 0, 0, 0, 0.0, 0)
        sc, co, ev = np.zeros((X.shape[0], 5)), np.zeros((64, 5)), np.zeros(5)
        f.check(f.lib().srx_pca(h.handle, f.ptr(sel), 64, C.byref(o), f.ptr(sc), f.ptr(co), f.ptr(ev), None, None, None), ctx.handle)
        return sc, co, ev
    want = ordinary(fresh)
    dev_pca(m, genes, 10)
    h = C.c_void_p()
    assert f.lib().srx_pca_model_from_result(m.handle, C.byref(h)) == f.E_ARG and not h.value
    assert b"residual" in f.lib().srx_last_error(ctx.handle)
    got = ordinary(m)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    h2 = C.c_void_p()                                                                    # an ordinary result makes a model again
    f.check(f.lib().srx_pca_model_from_result(m.handle, C.byref(h2)), ctx.handle)
    f.lib().srx_pca_model_free(h2)
    fresh.free()
    m.free()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    f = F()
    lib = f.lib()
    X = planted()[:40, :30]
    m = upload(ctx, X)
    out, info = np.full((40, 2), -7.0), f.PearsonPcaInfo()

    def pca(genes, o):
        g = np.array(genes, dtype=np.uint64)
        return lib.srx_pca_pearson(m.handle, f.ptr(g), g.size, C.byref(o), f.ptr(out), None, None, None, C.byref(info))
    ok = [3, 1, 2]
    assert pca([1, 2, 1], make_opts()) == f.E_ARG and b"twice" in lib.srx_last_error(ctx.handle)
    assert pca([1, 30], make_opts()) == f.E_ARG
    assert pca([1], make_opts()) == f.E_SHAPE
    assert pca(ok, make_opts(scale=1)) == f.E_ARG
    assert pca(ok, make_opts(solver=f.SOLVER_SPMM)) == f.E_ARG
    assert pca(ok, make_opts(theta=-1.0)) == f.E_ARG and pca(ok, make_opts(clip=float("nan"))) == f.E_ARG
    bad = make_opts()
    bad.totals = 2
    assert pca(ok, bad) == f.E_ARG
    assert np.all(out == -7.0)
    few = upload(ctx, planted()[:4, :30])
    g = np.array(ok, dtype=np.uint64)
    o = make_opts()
    assert lib.srx_pca_pearson(few.handle, f.ptr(g), 3, C.byref(o), None, None, None, None, None) == f.E_SHAPE
    few.free()
    assert pca(ok, make_opts()) == f.OK                                                  # and the handle still works
    m.free()


def test_an_empty_list_is_refused_not_divided_by(ctx):
    """k == 0 at the C entries and through the Python wrapper: SRX_E_ARG with a message, nothing written."""
    import singlerust_amd as sr
    from singlerust_amd.memory.processing import pearson_gram
    f = F()
    lib = f.lib()
    m = upload(ctx, planted()[:40, :30])
    g, out, cs, info, o = np.zeros(1, dtype=np.uint64), np.full(4, -7.0), np.full(4, -7.0), f.PearsonPcaInfo(), make_opts()
    info.total = -7.0
    assert lib.srx_pearson_gram(m.handle, f.ptr(g), 0, C.byref(o), f.ptr(out), f.ptr(cs), C.byref(info)) == f.E_ARG
    assert b"empty" in lib.srx_last_error(ctx.handle)
    assert lib.srx_pearson_gram(m.handle, None, 0, C.byref(o), f.ptr(out), f.ptr(cs), C.byref(info)) == f.E_ARG
    assert lib.srx_pca_pearson(m.handle, f.ptr(g), 0, C.byref(o), f.ptr(out), None, None, None, C.byref(info)) == f.E_ARG
    assert np.all(out == -7.0) and np.all(cs == -7.0) and info.total == -7.0
    a = sr.IMAnnData.new_basic(R.to_csr(planted()[:40, :30], np.float32), ctx=ctx)
    for wrapped in (a, m):
        with pytest.raises(sr.SrxError) as e:
            pearson_gram(wrapped, [])
        assert e.value.code == f.E_ARG
    gram, colsum, _ = pearson_gram(a, [4], totals="all")                                 # k = 1 is a Gram matrix (under the
    assert gram.shape == (1, 1) and gram[0, 0] > 0                                       # selected totals mu == x: all zeros)
    zero, _, _ = pearson_gram(a, [4])
    assert zero[0, 0] == 0.0
    m.free()


def test_sharded_and_backed_contexts_are_refused_first(ctx):
    """Both entries refuse a context with more than one rank and one with an open backed session, as the Pearson section does,
    and before the shape of the list is judged (k = 1 with such a context is SRX_E_ARG, not SRX_E_SHAPE)."""
    import singlerust_amd as sr
    f = F()
    lib = f.lib()
    X = planted()[:40, :30]

    def both(m, c, word):
        o, out = make_opts(), np.full((40, 2), -7.0)
        for genes in ([3, 1, 2], [3]):
            g = np.array(genes, dtype=np.uint64)
            gram = np.full((g.size, g.size), -7.0)
            assert lib.srx_pearson_gram(m.handle, f.ptr(g), g.size, C.byref(o), f.ptr(gram), None, None) == f.E_ARG
            assert word in lib.srx_last_error(c.handle)
            assert lib.srx_pca_pearson(m.handle, f.ptr(g), g.size, C.byref(o), f.ptr(out), None, None, None, None) == f.E_ARG
            assert word in lib.srx_last_error(c.handle)
            assert np.all(gram == -7.0) and np.all(out == -7.0)
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    m2 = upload(c2, X)
    both(m2, c2, b"rank")
    m2.free()
    c2.close()
    c3 = sr.Context(0)
    m3 = upload(c3, X)
    b = C.c_void_p()
    f.check(lib.srx_backed_create(c3.handle, X.shape[1], f.STORE_F32, C.byref(b)), c3.handle)
    both(m3, c3, b"backed")
    lib.srx_backed_destroy(b)
    dev_pca(m3, [3, 1, 2], 2)                                                            # accepted again once the session is gone
    # a bad theta with a list that is too short is an argument error too: the Pearson refusals come first
    g, o = np.array([3], dtype=np.uint64), make_opts(theta=-1.0)
    assert lib.srx_pca_pearson(m3.handle, f.ptr(g), 1, C.byref(o), None, None, None, None, None) == f.E_ARG
    m3.free()
    c3.close()


def test_doublets_refuse_a_residual_pca_by_name(ctx):
    from singlerust_amd.memory.processing import scrublet
    import singlerust_amd as sr
    counts = upload(ctx, planted(), np.float32)
    fitted = counts.clone()
    dev_pca(fitted, P.planted_genes(64), 10)
    with pytest.raises(sr.SrxError) as e:
        scrublet(fitted, counts)
    assert e.value.code == F().E_ARG and "residual" in str(e.value)
    fitted.free()
    counts.free()


def test_python_wrapper(ctx):
    import singlerust_amd as sr
    from singlerust_amd.memory.processing import pca_pearson_residuals
    X = planted()
    a = sr.IMAnnData.new_basic(R.to_csr(X, np.float32), ctx=ctx)
    res = pca_pearson_residuals(a, n_top_genes=64, n_components=5)
    assert a.obsm["X_pca"].shape == (600, 5) and res["selected_features"].size == 64 and res["k"] == 64
    ref = P.pca(np.asarray(P.residuals(X, res["selected_features"], totals="selected"), dtype=np.float64), 5)
    assert P.min_relative_gap(ref["values"], 5) >= 1e-3
    assert per_component(a.obsm["X_pca"], ref["scores"]) <= 1e-5
    assert a.uns["pca"]["scale"] is False and np.all(a.uns["pca"]["std"] == 1.0)

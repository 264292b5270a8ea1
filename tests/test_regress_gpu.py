"""Regress out / scale / clip / PCA on the device (srx_regress_fit / _sums / _residuals / _gram, srx_pca_regress) against the
numpy restatement of the definition (regress_ref.py: long double, the p x p system by elimination).

Bounds, u = 2^-53, against the long-double reference:
  xbar         bit-equal to srx_compute_sum(Column) / n
  cbar, A, W   |.| <= (n + 8) u sum |terms| (the dot-product bound; for A and W the terms carry (|ct| + mean |c|) so that the
               rounding of cbar is covered)
  beta, r, s   behind a solve whose error depends on A: K u x magnitude, K = 8 x the largest ratio the reference's OWN f64
               evaluation reaches against its long-double evaluation on the same case over the three (floor 8), one factor per
               case, measured and printed, never against the device.  Magnitudes: r: |x| + |xbar| + sum_q |ct||beta|;  s: relative;  beta: |A^-1| W_abs;
               z = r / s: K_r u mag_r / s + (K_s + 2) u |z|.
               The normal equations on the device's own output, |Ct^T r_j| <= K u |Ct|^T |r_j|, take the larger of K_r and
               8 x the ratio the f64 evaluation's own residuals reach in that unit: at n = p + 2 the fit is nearly exact,
               |r| is far below the terms it is made of and K_r alone, measured against those terms, does not carry over
               (n = 5, p = 3 reached 7.9 K_r u |Ct|^T |r| on the device).
  clip         the clipped set equals the reference's, those entries are exactly +-max_value, info.n_clipped is the count
  Gram         against the long-double Z^T Z of the block srx_regress_residuals returned in the same test:
               (n + 2) u (|Z|^T |Z|)_ij, column sums (n + 8) u sum |z|, symmetric bit for bit
  PCA          evr, every component and its scores to 1e-5, Frobenius-normalised per component, after the sign
               rule, asserted only after the reference's gap condition
Every test prints the largest ratio it reached before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest

import pearson_pca_ref as P
import pearson_ref as R
import regress_ref as G

pytestmark = pytest.mark.gpu
U = G.U


def F():
    from singlerust_amd import _ffi
    return _ffi


def upload(ctx, X, dtype=np.float64, csc=False):
    import singlerust_amd as sr
    n, Gn, indptr, indices, values = (R.to_csc if csc else R.to_csr)(X, dtype)
    return sr.DeviceCsr.upload(ctx, n, Gn, indptr, indices, values, csc=csc)


def make_opts(scale=1, mv=0.0, chunk=0, n_pc=2, solver=0, pca_scale=0):
    f = F()
    return f.RegressOpts(scale, 0, mv, chunk, f.PcaOpts(n_pc, -1, pca_scale, -1, 0, 0, solver, 0.0, 0))


def _args(m, genes, cov):
    g = np.ascontiguousarray(genes, dtype=np.uint64)
    c = np.ascontiguousarray(cov, dtype=np.float64)
    return g, c, (m.handle, F().ptr(g), g.size, F().ptr(c) if c.size else None, c.shape[1])


def dev_fit(m, genes, cov, **kw):
    g, c, a = _args(m, genes, cov)
    beta, xbar, sd, info, o = np.full((c.shape[1], g.size), -7.0), np.full(g.size, -7.0), np.full(g.size, -7.0), F().RegressInfo(), make_opts(**kw)
    F().check(F().lib().srx_regress_fit(*a, C.byref(o), F().ptr(beta) if beta.size else None, F().ptr(xbar), F().ptr(sd), C.byref(info)), m.ctx.handle)
    return beta, xbar, sd, info


def dev_sums(m, genes, cov, **kw):
    g, c, a = _args(m, genes, cov)
    p = c.shape[1]
    cbar, A, W, o = np.full(p, -7.0), np.full((p, p), -7.0), np.full((p, g.size), -7.0), make_opts(**kw)
    F().check(F().lib().srx_regress_sums(*a, C.byref(o), F().ptr(cbar), F().ptr(A), F().ptr(W), None), m.ctx.handle)
    return cbar, A, W


def dev_block(m, genes, cov, **kw):
    g, c, a = _args(m, genes, cov)
    out, info, o = np.full((int(m.info().n_rows), g.size), -7.0), F().RegressInfo(), make_opts(**kw)
    F().check(F().lib().srx_regress_residuals(*a, C.byref(o), F().ptr(out), C.byref(info)), m.ctx.handle)
    return out, info


def dev_gram(m, genes, cov, **kw):
    g, c, a = _args(m, genes, cov)
    gram, colsum, info, o = np.full((g.size, g.size), -7.0), np.full(g.size, -7.0), F().RegressInfo(), make_opts(**kw)
    F().check(F().lib().srx_regress_gram(*a, C.byref(o), F().ptr(gram), F().ptr(colsum), C.byref(info)), m.ctx.handle)
    return gram, colsum, info


def dev_pca(m, genes, cov, n_pc, **kw):
    g, c, a = _args(m, genes, cov)
    n, k = int(m.info().n_rows), g.size
    scores, comps, evr = np.full((n, n_pc), -7.0), np.full((k, n_pc), -7.0), np.full(n_pc, -7.0)
    mean, sd, info, o = np.full(k, -7.0), np.full(k, -7.0), F().RegressInfo(), make_opts(n_pc=n_pc, **kw)
    F().check(F().lib().srx_pca_regress(*a, C.byref(o), F().ptr(scores), F().ptr(comps), F().ptr(evr), F().ptr(mean), F().ptr(sd), C.byref(info)),
              m.ctx.handle)
    return scores, comps, evr, mean, sd, info


def f64(x):
    return np.asarray(x, dtype=np.float64)


def ratio(err, bound):
    return float(np.max(f64(err) / np.maximum(f64(bound), 1e-300), initial=0.0))


def column_sum(m):
    out = np.zeros(int(m.info().n_cols))
    F().check(F().lib().srx_compute_sum(m.handle, F().COLUMN, F().ptr(out)), m.ctx.handle)
    return out


# ---- the shape walk: every sum, the fit, r, s and z ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0, 1, 3, 16])
@pytest.mark.parametrize("k", [2, 16, 17, 130])
@pytest.mark.parametrize("n", [5, 63, 64, 257])
def test_shape_walk(ctx, n, k, p):
    f = F()
    if n < p + 2:
        X, genes, _ = G.walk_case(n, k)
        m = upload(ctx, X)
        g, c, a = _args(m, genes, np.ones((n, p)))
        out = np.full((n, k), -7.0)
        assert f.lib().srx_regress_residuals(*a, None, f.ptr(out), None) == f.E_SHAPE and np.all(out == -7.0)
        m.free()
        return
    worst = {}
    for dtype in (np.float32, np.float64):
        X, genes, const_pos = G.walk_case(n, k, dtype)
        gi = genes.astype(np.int64)
        assert not np.all(np.diff(gi) > 0)                                               # the list is not ascending
        if n >= R.FEATURES_FROM:
            assert (X[:, gi] == 0).all(axis=0).any() and ((const_pos is not None) or not X[0].any())
        Xl, cov = X[:, gi], G.walk_covariates(X, p)
        ref = G.evaluate(Xl, cov, True, 0.0)
        K, raw = G.measured_factor(Xl, cov)
        print("n=%d k=%d p=%d %s: K %.1f (f64 evaluation: r %.1f s %.1f beta %.1f), normal equations %.1f (min pivot %.3e)"
              % (n, k, p, dtype.__name__, K["r"], raw["r"], raw["s"], raw["beta"], K["ctr"], float(np.min(ref["piv"], initial=1.0))))
        mag_r, s_ref, z_ref, flat = f64(ref["mag_r"]), f64(ref["s"]), ref["z"], ref["const"]
        for csc in (False, True):
            m = upload(ctx, X, dtype, csc)
            want_xbar = column_sum(m)[gi] / n
            for chunk in (0, 64, 100):
                tag = "n=%d k=%d p=%d %s csc=%d chunk=%d" % (n, k, p, dtype.__name__, csc, chunk)
                beta, xbar, sd, info = dev_fit(m, genes, cov, chunk=chunk)
                assert np.array_equal(xbar, want_xbar), tag                              # bit for bit
                assert info.n_cells == n and info.n_genes == k and info.n_cov == p and info.n_constant_genes == int(flat.sum())
                assert info.n_chunks == (1 if chunk == 0 else -(-n // min(chunk, n))), tag
                res = {}
                if p:
                    cbar, A, W = dev_sums(m, genes, cov, chunk=chunk)
                    res["cbar"] = ratio(np.abs(cbar - ref["cbar"]), (n + 8) * U * f64(ref["cbar_abs"]))
                    res["A"] = ratio(np.abs(A - ref["A"]), (n + 8) * U * f64(ref["A_abs"]))
                    res["W"] = ratio(np.abs(W - ref["W"]), (n + 8) * U * f64(ref["W_abs"]))
                    assert np.array_equal(A, A.T), tag
                    res["beta"] = ratio(np.abs(beta - ref["beta"]), K["beta"] * U * G.beta_magnitude(ref))
                    assert abs(info.min_pivot - float(np.min(ref["piv"]))) <= 1e-9, tag
                res["s"] = ratio(np.abs(sd - ref["s"]) / s_ref, K["s"] * U)
                r, _ = dev_block(m, genes, cov, scale=0, chunk=chunk)
                res["r"] = ratio(np.abs(r - ref["r"]), K["r"] * U * mag_r)
                z, _ = dev_block(m, genes, cov, chunk=chunk)
                res["z"] = ratio(np.abs(z - z_ref), K["r"] * U * mag_r / s_ref + (K["s"] + 2) * U * np.abs(f64(z_ref)))
                if p:                                                                    # the normal equations, on the device's own output
                    ct = f64(ref["ct"])
                    res["Ct^T r"] = ratio(np.abs(ct.astype(np.longdouble).T @ r), K["ctr"] * U * (np.abs(ct).T @ np.abs(r)))
                for key, v in res.items():
                    worst[key] = max(worst.get(key, 0.0), v)
                    assert v <= 1.0, (tag, key, v)
                assert np.all(np.isfinite(r)) and np.all(np.isfinite(z)), tag
                assert np.all(r[:, flat] == 0.0) and np.all(z[:, flat] == 0.0) and np.all(sd[flat] == 1.0), tag   # exact zero columns
            m.free()
    print("n=%d k=%d p=%d: largest ratios of the bounds %s" % (n, k, p, {a: round(b, 3) for a, b in worst.items()}))


# ---- the clip -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted():
    pl = G.planted()
    pl["X"].setflags(write=False)
    return pl["X"]


@functools.lru_cache(maxsize=None)
def pca_genes(k):
    """The first k columns of the fixture in a fixed, unsorted order."""
    return np.random.default_rng(77).permutation(k).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def planted_reference(k, p, mv, dtype=np.float64):
    X = planted().astype(dtype).astype(np.float64)[:, pca_genes(k).astype(np.int64)]
    ref = G.evaluate(X, G.planted_covariates(p, G.PCA_SEED), True, mv)
    ref["pca"] = P.pca(f64(ref["z"]), 50)
    ref["K"], _ = G.measured_factor(X, G.planted_covariates(p, G.PCA_SEED))
    return ref


@pytest.mark.parametrize("mv", [0.25, 2.0, 3.0])
def test_clip_set_is_the_references(ctx, mv):
    m = upload(ctx, planted())
    for k, p in ((64, 2), (240, 0)):
        ref, genes, cov = planted_reference(k, p, mv), pca_genes(k), G.planted_covariates(p, G.PCA_SEED)
        assert float(np.min(np.abs(np.abs(f64(ref["z_raw"])) - mv))) >= 1e-9                  # the input condition (test_regress_cpu.py)
        z, info = dev_block(m, genes, cov, mv=mv, chunk=100)
        clipped = np.abs(z) == mv
        zero_clipped = int((ref["clipped"] & (planted()[:, genes.astype(np.int64)] == 0)).sum())
        print("max_value=%g k=%d p=%d: %d clipped (%d zero entries), device count %d" % (mv, k, p, int(ref["clipped"].sum()), zero_clipped,
                                                                                         info.n_clipped))
        assert ref["clipped"].any() and (mv != 0.25 or zero_clipped > 0)
        assert np.array_equal(clipped, ref["clipped"])
        assert np.all(z[clipped] == np.sign(f64(ref["z_raw"]))[clipped] * mv)
        assert info.n_clipped == int(clipped.sum())
        _, _, ginfo = dev_gram(m, genes, cov, mv=mv)
        assert ginfo.n_clipped == info.n_clipped
    m.free()


# ---- the Gram and the column sums against the block they are made of ---------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 16, 17, 130])
@pytest.mark.parametrize("n", [5, 63, 64, 257])
def test_gram_is_the_product_of_the_block(ctx, n, k):
    X, genes, _ = G.walk_case(n, k)
    cov = G.walk_covariates(X, min(3, n - 2))
    for csc in (False, True):
        m = upload(ctx, X, np.float64, csc)
        for chunk in (0, 64, 100):
            tag = "n=%d k=%d csc=%d chunk=%d" % (n, k, csc, chunk)
            z, binfo = dev_block(m, genes, cov, mv=0.25, chunk=chunk)
            gram, colsum, info = dev_gram(m, genes, cov, mv=0.25, chunk=chunk)
            Z = z.astype(np.longdouble)
            g_ref, g_abs, s_ref, s_abs = P.gram(Z)
            rg = ratio(np.abs(gram - g_ref), (n + 2) * U * f64(g_abs))
            rs = ratio(np.abs(colsum - s_ref), (n + 8) * U * f64(s_abs))
            print("regress gram %s: max ratio %.3f (Gram) %.3f (column sums) of the bounds, %d clipped" % (tag, rg, rs, info.n_clipped))
            assert (np.abs(z) == 0.25).any() and info.n_clipped == binfo.n_clipped == int((np.abs(z) == 0.25).sum()), tag
            assert np.array_equal(gram, gram.T), tag                                     # symmetric bit for bit
            assert rg <= 1.0 and rs <= 1.0, tag
            gram2, colsum2, _ = dev_gram(m, genes, cov, mv=0.25, chunk=chunk)
            assert np.array_equal(gram, gram2) and np.array_equal(colsum, colsum2), tag  # two calls are bit-identical
        m.free()


# ---- the PCA ---------------------------------------------------------------------------------------------------------------------------------
def per_component(got, ref):
    return float(np.max(np.linalg.norm(got - ref, axis=0) / np.linalg.norm(ref, axis=0)))


def check_pca(out, ref, n_pc, tag):
    scores, comps, evr, mean, sd, info = out
    pr, K = ref["pca"], ref["K"]
    gap = P.min_relative_gap(pr["values"], n_pc)
    assert gap >= 1e-3, (tag, gap)                                                       # on the reference, before anything is compared
    n = scores.shape[0]
    e_evr = float(np.max(np.abs(evr - pr["evr"][:n_pc]) / pr["evr"][:n_pc]))
    e_v, e_s = per_component(comps, pr["components"][:, :n_pc]), per_component(scores, pr["scores"][:, :n_pc])
    s_ref, z_ref = f64(ref["s"]), f64(ref["z"])
    zb = K["r"] * U * f64(ref["mag_r"]) / s_ref + (K["s"] + 2) * U * np.abs(z_ref)
    r_m = ratio(np.abs(mean - ref["z"].sum(axis=0) / n), (n + 8) * U * np.abs(z_ref).mean(axis=0) + zb.mean(axis=0))
    r_s = ratio(np.abs(sd - ref["s"]) / s_ref, K["s"] * U)
    print("regress pca %s n_pc=%d: evr %.2e components %.2e scores %.2e (gate 1e-5), mean %.3f sd %.3f of their bounds, gap %.2e, "
          "residual %.1e, %d sweeps, %d clipped" % (tag, n_pc, e_evr, e_v, e_s, r_m, r_s, gap, info.pca.residual, info.pca.n_iter, info.n_clipped))
    assert info.pca.k == comps.shape[0] and info.pca.n_pc == n_pc and info.pca.solver == F().SOLVER_GRAM
    assert e_evr <= 1e-5 and e_v <= 1e-5 and e_s <= 1e-5, tag
    assert r_m <= 1.0 and r_s <= 1.0, tag                                                # the caller's order
    assert info.n_clipped == int(ref["clipped"].sum()), tag
    assert all(comps[int(np.argmax(np.abs(comps[:, c]))), c] > 0 for c in range(n_pc))   # the sign rule


@pytest.mark.parametrize("mv", [0.0, 3.0])
@pytest.mark.parametrize("p", [0, 2])
@pytest.mark.parametrize("n_pc", [2, 5, 50])
@pytest.mark.parametrize("k", [64, 240])
def test_pca_of_the_fixture(ctx, k, n_pc, p, mv):
    ref = planted_reference(k, p, mv)
    m = upload(ctx, planted())
    out = dev_pca(m, pca_genes(k), G.planted_covariates(p, G.PCA_SEED), n_pc, mv=mv)
    check_pca(out, ref, n_pc, "k=%d p=%d max_value=%g" % (k, p, mv))
    assert out[5].n_chunks == 1 and out[5].n_cov == p
    m.free()


def test_formats_storages_and_chunks_give_the_same_pca(ctx):
    k, p, mv, n_pc = 64, 2, 3.0, 5
    cov = G.planted_covariates(p, G.PCA_SEED)
    for dtype in (np.float32, np.float64):
        ref = planted_reference(k, p, mv, dtype)
        for csc in (False, True):
            m = upload(ctx, planted(), dtype, csc)
            for chunk in (0, 64, 100):
                out = dev_pca(m, pca_genes(k), cov, n_pc, mv=mv, chunk=chunk)
                check_pca(out, ref, n_pc, "%s csc=%d chunk=%d" % (dtype.__name__, csc, chunk))
                assert out[5].n_chunks == (1 if chunk == 0 else -(-600 // chunk))
            m.free()


def test_two_calls_are_bit_identical_and_the_handle_is_untouched(ctx):
    f = F()
    genes, cov = pca_genes(64), G.planted_covariates(2, G.PCA_SEED)
    m = upload(ctx, planted(), np.float32)
    vals, sums, dt = m.values().copy(), column_sum(m), m.info().dtype
    a = dev_pca(m, genes, cov, 5, mv=3.0, chunk=100)
    b = dev_pca(m, genes, cov, 5, mv=3.0, chunk=100)
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(x, y)
    dev_fit(m, genes, cov)
    dev_block(m, genes, cov, mv=2.0)
    assert np.array_equal(m.values(), vals) and np.array_equal(column_sum(m), sums) and m.info().dtype == dt
    cnt, s1, s2 = np.zeros(240, dtype=np.uint64), np.zeros(240), np.zeros(240)
    f.check(f.lib().srx_gene_moments(m.handle, f.ptr(cnt), f.ptr(s1), f.ptr(s2)), ctx.handle)
    X32 = planted().astype(np.float32).astype(np.float64)
    assert np.array_equal(cnt, (X32 != 0).sum(axis=0).astype(np.uint64)) and np.allclose(s2, (X32 ** 2).sum(axis=0), rtol=1e-12)
    m.free()


def test_plain_scale_agrees_with_the_sparse_gram_route(ctx):
    """p = 0, scale on, no clip against srx_pca(center = 1, scale = 1) on the same handle and list: the sparse Gram route shares
    none of this code.  Scores differ by sqrt((n - 1) / n): ddof 1 here, ddof 0 there."""
    f = F()
    k, n_pc, n = 64, 5, 600
    genes = np.arange(k, dtype=np.uint64)
    assert not G.constant_genes(planted()[:, :k]).any()
    assert P.min_relative_gap(P.pca(f64(G.evaluate(planted()[:, :k], np.zeros((n, 0)))["z"]), n_pc)["values"], n_pc) >= 1e-3
    m = upload(ctx, planted())
    scores, comps, evr, _, sd, _ = dev_pca(m, genes, np.zeros((n, 0)), n_pc)
    o = f.PcaOpts(n_pc, 1, 1, -1, 0, 0, 0, 0.0, 0)
    sc, co, ev, sd0 = np.zeros((n, n_pc)), np.zeros((k, n_pc)), np.zeros(n_pc), np.zeros(k)
    f.check(f.lib().srx_pca(m.handle, f.ptr(genes), k, C.byref(o), f.ptr(sc), f.ptr(co), f.ptr(ev), None, f.ptr(sd0), None), ctx.handle)
    e = (float(np.max(np.abs(evr - ev) / ev)), per_component(comps, co), per_component(scores, sc * np.sqrt((n - 1) / n)))
    print("plain scale against srx_pca: evr %.2e components %.2e scores %.2e (gate 1e-5)" % e)
    assert max(e) <= 1e-5
    assert np.allclose(sd, sd0 * np.sqrt(n / (n - 1)), rtol=1e-9)           # (ddof 0 there, from the moments: mean^2 cancels)
    m.free()


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
def test_the_resident_scores_feed_the_neighbour_search(ctx):
    from singlerust_amd.memory.processing import knn_points
    f = F()
    m = upload(ctx, planted())
    n = 600
    scores = dev_pca(m, pca_genes(64), G.planted_covariates(2, G.PCA_SEED), 10, mv=3.0)[0]
    opts, info = f.KnnOpts(), f.KnnInfo()
    opts.k = 15
    idx, dist = np.zeros((n, 15), dtype=np.uint32), np.zeros((n, 15), dtype=np.float64)
    f.check(f.lib().srx_knn_result(m.handle, C.byref(opts), f.ptr(idx), f.ptr(dist), C.byref(info)), ctx.handle)
    idx_p, _, _ = knn_points(ctx, scores, k=15)
    assert np.array_equal(idx, idx_p)
    m.free()


def test_no_model_of_this_result_and_the_refusals_name_the_call(ctx):
    import singlerust_amd as sr
    from singlerust_amd.memory.processing import scrublet
    f = F()
    counts = upload(ctx, planted(), np.float32)
    fitted = counts.clone()
    dev_pca(fitted, pca_genes(64), G.planted_covariates(2, G.PCA_SEED), 10)
    h = C.c_void_p()
    assert f.lib().srx_pca_model_from_result(fitted.handle, C.byref(h)) == f.E_ARG and not h.value
    msg = f.lib().srx_last_error(ctx.handle)
    assert b"srx_pca_regress" in msg and b"Pearson" not in msg
    with pytest.raises(sr.SrxError) as e:
        scrublet(fitted, counts)
    assert e.value.code == f.E_ARG and "srx_pca_regress" in str(e.value) and "Pearson" not in str(e.value)
    sel = np.arange(64, dtype=np.uint64)                                                 # an ordinary result makes a model again
    o = f.PcaOpts(5, -1, -1, -1, 0, 0, 0, 0.0, 0)
    f.check(f.lib().srx_pca(fitted.handle, f.ptr(sel), 64, C.byref(o), None, None, None, None, None, None), ctx.handle)
    f.check(f.lib().srx_pca_model_from_result(fitted.handle, C.byref(h)), ctx.handle)
    f.lib().srx_pca_model_free(h)
    fitted.free()
    counts.free()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order(ctx):
    """Each refusal of the header with every LATER one provoked in the same call: the earlier one must answer."""
    import singlerust_amd as sr
    f = F()
    lib = f.lib()
    n = 40
    X = planted()[:n, :30].copy()
    X[3, 5] = np.inf                                                                     # (10) a non-finite stored value
    m = upload(ctx, X)
    out, info = np.full((n, 3), -7.0), f.RegressInfo()
    info.min_pivot = -7.0
    good = np.stack([G.hashed_covariate(n, 7), G.hashed_covariate(n, 8)], axis=1)
    collinear = np.stack([good[:, 0], 2 * good[:, 0] + 1], axis=1)                       # (9)
    constant = np.stack([good[:, 0], np.full(n, 3.0)], axis=1)                           # (9)
    nonfinite = collinear.copy()                                                         # (8)
    nonfinite[7, 1] = np.nan

    def call(h, genes, cov, p, o, c=ctx):
        g = np.array(genes, dtype=np.uint64)
        cv = np.ascontiguousarray(cov, dtype=np.float64) if cov is not None else None
        rc = lib.srx_pca_regress(h.handle, f.ptr(g) if g.size else None, g.size, f.ptr(cv) if cv is not None else None, p, C.byref(o), f.ptr(out),
                                 None, None, None, None, C.byref(info))
        rc2 = lib.srx_regress_residuals(h.handle, f.ptr(g) if g.size else None, g.size, f.ptr(cv) if cv is not None else None, p, C.byref(o),
                                        f.ptr(out), C.byref(info))
        assert rc == rc2 or (rc2 == f.E_ARG and rc == f.E_SHAPE) or (rc == f.E_SHAPE and g.size == 1), (rc, rc2)
        return rc, lib.srx_last_error(c.handle), rc2
    ok = [3, 1, 2]
    wide = np.ones((n, 17))
    # (1) null list / null covariates with p > 0, everything else wrong too
    assert call(m, [], nonfinite, 2, make_opts(mv=-1.0))[0] == f.E_ARG and b"null" in lib.srx_last_error(ctx.handle)
    assert call(m, [1, 1], None, 17, make_opts(mv=-1.0))[0] == f.E_ARG and b"null" in lib.srx_last_error(ctx.handle)
    # (2) ranks and (3) a backed session, before max_value
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    m2 = upload(c2, X)
    rc, msg, _ = call(m2, [1, 1], wide, 17, make_opts(mv=-1.0), c2)
    assert rc == f.E_ARG and b"rank" in msg
    m2.free()
    c2.close()
    c3 = sr.Context(0)
    m3 = upload(c3, X)
    b = C.c_void_p()
    f.check(lib.srx_backed_create(c3.handle, X.shape[1], f.STORE_F32, C.byref(b)), c3.handle)
    rc, msg, _ = call(m3, [1, 1], wide, 17, make_opts(mv=-1.0), c3)
    assert rc == f.E_ARG and b"backed" in msg
    lib.srx_backed_destroy(b)
    m3.free()
    c3.close()
    # (4) max_value, (5) p, (6) the list, (7) the solver's options
    for mv in (-1.0, float("nan")):
        rc, msg, _ = call(m, [1, 1], wide, 17, make_opts(mv=mv, pca_scale=1))
        assert rc == f.E_ARG and b"max_value" in msg
    rc, msg, _ = call(m, [1, 1], wide, 17, make_opts(pca_scale=1))
    assert rc == f.E_ARG and b"covariates" in msg
    for genes, word in (([1, 2, 1], b"twice"), ([1, 30], b"out of bounds"), (list(range(16385)), b"listed genes")):
        rc, msg, _ = call(m, genes, nonfinite, 2, make_opts(pca_scale=1))
        assert rc == f.E_ARG and word in msg, (genes[:3], msg)
    g0 = np.zeros(1, dtype=np.uint64)
    assert lib.srx_regress_gram(m.handle, f.ptr(g0), 0, f.ptr(good), 2, None, f.ptr(out), None, None) == f.E_ARG
    assert b"empty" in lib.srx_last_error(ctx.handle)
    rc, msg, _ = call(m, ok, nonfinite, 2, make_opts(pca_scale=1, solver=f.SOLVER_SPMM))
    assert rc == f.E_ARG and b"pca.scale" in msg
    rc, msg, _ = call(m, ok, nonfinite, 2, make_opts(solver=f.SOLVER_SPMM))
    assert rc == f.E_ARG and b"matrix-free" in msg
    # the shape, before the covariates and the values are read
    rc, msg, rc2 = call(m, [1], nonfinite, 2, make_opts())
    assert rc == f.E_SHAPE and rc2 == f.E_ARG                                            # k = 1 is a PCA's refusal only: the block call goes on to (8)
    few = upload(ctx, X[:3])
    assert call(few, ok, nonfinite[:3], 2, make_opts())[0] == f.E_SHAPE                 # n < p + 2
    few.free()
    # (8), (9), (10)
    rc, msg, _ = call(m, ok, nonfinite, 2, make_opts())
    assert rc == f.E_ARG and b"not finite" in msg and b"covariate 1 of cell 7" in msg
    rc, msg, _ = call(m, ok, constant, 2, make_opts())
    assert rc == f.E_ARG and b"covariate 1 is constant" in msg
    rc, msg, _ = call(m, ok, collinear, 2, make_opts())
    assert rc == f.E_ARG and b"covariate 1 is collinear" in msg
    rc, msg, _ = call(m, ok, good, 2, make_opts())
    assert rc == f.E_ARG and b"NaN or infinite value" in msg
    assert np.all(out == -7.0) and info.min_pivot == -7.0                                # nothing written by any of them
    m.free()
    clean = upload(ctx, planted()[:n, :30])
    assert call(clean, ok, good, 2, make_opts())[0] == f.OK                              # and a clean call works
    clean.free()


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------------------
def test_python_wrappers(ctx):
    import singlerust_amd as sr
    from singlerust_amd.memory.processing import pca_regress_scale, regress_fit, regress_gram, regress_out, scale
    X = planted().astype(np.float32).astype(np.float64)
    a = sr.IMAnnData.new_basic(R.to_csr(planted(), np.float32), ctx=ctx)
    cov = G.planted_covariates(2, G.PCA_SEED)
    a.obs["total_counts"], a.obs["hashed"] = cov[:, 0], cov[:, 1]
    genes = pca_genes(64)
    ref = G.evaluate(X[:, genes.astype(np.int64)], cov, True, 3.0)
    K, _ = G.measured_factor(X[:, genes.astype(np.int64)], cov)
    zb = K["r"] * U * f64(ref["mag_r"]) / f64(ref["s"]) + (K["s"] + 2) * U * np.abs(f64(ref["z"]))
    z = regress_out(a, ["total_counts", "hashed"], genes, scale=True, max_value=3.0)
    assert np.all(np.abs(z - ref["z"]) <= zb)
    assert np.array_equal(z, regress_out(a.x(), cov, genes, scale=True, max_value=3.0))
    beta, xbar, sd, info = regress_fit(a, cov, genes)
    assert beta.shape == (2, 64) and info["n_cov"] == 2 and ratio(np.abs(sd - ref["s"]) / f64(ref["s"]), K["s"] * U) <= 1.0
    plain = scale(a, genes, max_value=3.0)
    ref0 = G.evaluate(X[:, genes.astype(np.int64)], np.zeros((600, 0)), True, 3.0)
    assert np.allclose(plain, f64(ref0["z"]), rtol=0, atol=1e-12) and np.array_equal(np.abs(plain) == 3.0, ref0["clipped"])
    gram, colsum, ginfo = regress_gram(a, cov, genes, max_value=3.0)
    assert np.allclose(gram, z.T @ z, rtol=1e-12, atol=1e-9) and ginfo["n_clipped"] == int(ref["clipped"].sum())
    res = pca_regress_scale(a, ["total_counts", "hashed"], genes, n_components=5, max_value=3.0)
    pr = P.pca(f64(ref["z"]), 5)
    assert P.min_relative_gap(pr["values"], 5) >= 1e-3
    assert a.obsm["X_pca"].shape == (600, 5) and per_component(a.obsm["X_pca"], pr["scores"]) <= 1e-5
    assert a.uns["pca"]["scale"] is True and a.uns["pca"]["residuals"] == "regress" and np.allclose(a.uns["pca"]["std"], f64(ref["s"]), rtol=1e-12)
    sel = pca_regress_scale(a, None, None, n_top_genes=40, n_components=3)                # the default route: srx_select_hvg, plain scale
    assert sel["selected_features"].size == 40 and sel["k"] == 40 and sel["n_cov"] == 0

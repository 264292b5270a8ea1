"""GPU parity tests (-m gpu) on BASELINE.json's configs[0] and configs[1] shapes, end to end against the oracle.

configs[0]: 2.7k cells x 32k genes, ~7 % (the reference's CPU-runnable case): every stage against the C oracle and the
            exact-SVD oracle.
configs[1]: 100k cells x 20k genes, 5 % (1.0e8 non-zeros): normalise / log1p / gene variance / HVG against the C oracle
            (serial loops, a few seconds); the PCA against an f64 covariance-eigendecomposition restatement
            (scipy sparse Z^T Z of the 2000 selected genes + numpy eigh — mathematically the oracle's SVD, and the only
            exact reference that fits a test at this size)."""
import ctypes as C

import numpy as np
import pytest

import oracle
from oracle import COLUMN, ROW, pca_oracle
from test_pca_gpu import TOL, adata_of, assert_components_within_conditioning, col_err, synth_host
from util import rel_err

pytestmark = pytest.mark.gpu


def pipeline(ctx, m, store, n_hvg, n_pc):
    from singlerust_amd import _ffi as F
    a = adata_of(m, ctx, store)
    opts = F.PcaOpts(n_pc, -1, -1, -1, 0, 0, 0, 0.0, 0)
    res = F.PipelineResult()
    F.check(F.lib().srx_pipeline(a.x().handle, 1e4, n_hvg, C.byref(opts), C.byref(res)), ctx.handle)
    k = int(res.pca.k)
    scores, comps = np.zeros((m.n_rows, n_pc)), np.zeros((k, n_pc))
    evr, mean, std, hv = np.zeros(n_pc), np.zeros(k), np.zeros(k), np.zeros(k, np.uint64)
    F.check(F.lib().srx_result_fetch(a.x().handle, F.ptr(scores), F.ptr(comps), F.ptr(evr), F.ptr(mean), F.ptr(std), F.ptr(hv)),
            ctx.handle)
    return a, scores, comps, evr, mean, std, hv


@pytest.mark.parametrize("store,vtol", [(1, 1e-6), (2, 4e-16)])
def test_config0_shape_every_stage_against_the_oracle(ctx, store, vtol):
    import singlerust_amd as sr
    from singlerust_amd.memory import statistics as st
    m, _ = synth_host(1001, 2700, 32000, 0.07)
    raw = adata_of(m, ctx, store)
    assert np.array_equal(st.compute_number(raw, sr.Direction.Row), oracle.compute_number(m, ROW))        # bit-exact
    assert np.array_equal(st.compute_number(raw, sr.Direction.Column), oracle.compute_number(m, COLUMN))
    assert np.array_equal(st.compute_sum(raw, sr.Direction.Row), oracle.compute_sum(m, ROW))              # integer counts
    assert np.array_equal(st.compute_sum(raw, sr.Direction.Column), oracle.compute_sum(m, COLUMN))
    a, scores, comps, evr, mean, std, hv = pipeline(ctx, m, store, 2000, 50)
    lg = oracle.log1p_transform(oracle.normalize_total(m, 1e4, ROW))
    assert rel_err(a.x_values(np.float64), lg.values.astype(np.float64)) <= vtol
    want_var = oracle.compute_variance(lg, COLUMN)
    got_var = st.compute_variance(a, sr.Direction.Column)
    assert np.allclose(got_var, want_var, rtol=1e-4 if store == 1 else 1e-11, atol=1e-12)
    # identical set and order at BOTH storages: the pipeline ranks on the f64 moments of the transformed values
    assert np.array_equal(hv, oracle.select_hvg(want_var, 2000))
    want, wc, wevr, wmean, wstd = pca_oracle.pca_inplace(lg, 50, None, None, hv)
    assert np.allclose(evr, wevr, rtol=1e-5) and np.allclose(mean, wmean, rtol=1e-5, atol=1e-7) and np.allclose(std, wstd, rtol=1e-5)
    # 1e-5 per component wherever the eigengap supports it (N = 2700: the tail eigenvalues crowd), the perturbation bound
    # of the storage precision elsewhere — no blanket factor
    # asserted slack budget 0 at BOTH storages: every one of the 50 components meets the plain 1e-5 (measured: worst 8.6e-7 at
    # f32 storage, 2.8e-10 at f64), the conditioning argument is not drawn on
    gaps = assert_components_within_conditioning(scores, want, wevr, store, "c1-shape score", max_slack=0)
    used = assert_components_within_conditioning.last
    assert_components_within_conditioning(comps, wc, wevr, store, "c1-shape loading", max_slack=0)
    assert (gaps[:10] > 1e-3).all()
    # the leading ten components (gaps > 1e-3) meet the plain 1e-5 at EITHER storage: the conditioning slack is for the tail
    assert col_err(scores[:, :10], want[:, :10]) < TOL and col_err(comps[:, :10], wc[:, :10]) < TOL
    if store == 2:
        assert used["n_slack"] == 0                 # f64 storage: every one of the 50 components at the plain bar
    assert np.abs(wc @ (wc.T @ comps) - comps).max() < 1e-4


def config1_shape_against_the_oracle(ctx, store, vtol, skew, label):
    import scipy.sparse as sp
    import singlerust_amd as sr
    from singlerust_amd.memory import statistics as st
    n, g = 100_000, 20_000
    m, _ = synth_host(2002, n, g, 0.05, skew=skew)
    assert 0.9e8 < len(m.values) < 1.1e8
    a, scores, comps, evr, mean, std, hv = pipeline(ctx, m, store, 2000, 50)
    lg = oracle.log1p_transform(oracle.normalize_total(m, 1e4, ROW))            # serial C loops over 1e8 non-zeros
    assert rel_err(a.x_values(np.float64), lg.values.astype(np.float64)) <= vtol
    want_var = oracle.compute_variance(lg, COLUMN)
    assert np.allclose(st.compute_variance(a, sr.Direction.Column), want_var, rtol=1e-4 if store == 1 else 1e-11, atol=1e-12)
    want_sel = oracle.select_hvg(want_var, 2000)
    # either storage, f64 moments: HighlyVariable(2000) is the reference's, index for index
    assert np.array_equal(hv, want_sel)
    # PCA of the GPU's own selection: covariance eigendecomposition in f64
    x = sp.csr_matrix((lg.values.astype(np.float64), lg.indices.astype(np.int64), lg.indptr.astype(np.int64)), shape=(n, g))
    xs = x[:, hv.astype(np.int64)].tocsc()
    mu = np.asarray(xs.mean(axis=0)).ravel()
    ex2 = np.asarray(xs.multiply(xs).mean(axis=0)).ravel()
    sd = np.sqrt(ex2 - mu * mu)
    gram = (xs.T @ xs).toarray()
    cov = (gram - n * np.outer(mu, mu)) / np.outer(sd, sd)                      # Z^T Z
    w, v = np.linalg.eigh(cov)
    order = np.argsort(w)[::-1][:50]
    wv, vv = w[order], v[:, order]
    assert np.allclose(mean, mu, rtol=1e-5, atol=1e-7) and np.allclose(std, sd, rtol=1e-5)
    assert np.allclose(evr, wv / np.trace(cov), rtol=1e-5)
    # slack budget 0: all 50 components at the plain 1e-5 at either storage (measured at f32: loadings 1.0e-7, scores 2.8e-7)
    assert_components_within_conditioning(comps, vv, wv, store, label + " loading", max_slack=0)
    want_scores = (xs @ (vv / sd[:, None])) - (mu / sd) @ vv
    assert_components_within_conditioning(scores, np.asarray(want_scores), wv, store, label + " score", max_slack=0)
    return xs


@pytest.mark.parametrize("store,vtol", [(1, 1e-6), (2, 4e-16)])
def test_config1_shape_against_the_oracle(ctx, store, vtol):
    config1_shape_against_the_oracle(ctx, store, vtol, 0, "c2-shape")


@pytest.mark.parametrize("store,vtol", [(1, 1e-6), (2, 4e-16)])
def test_config1_shape_skewed_gene_densities_against_the_oracle(ctx, store, vtol):
    """The SKEWED generator (gene density ~ 1 / sqrt(index): the selected genes are the dense ones, about twice the kept
    entries per cell, suffixes longer than one 64-entry record piece, Gram owners of very different weight) through the
    same checks as the uniform matrix: HighlyVariable(2000) index for index, all 50 components at the plain 1e-5."""
    xs = config1_shape_against_the_oracle(ctx, store, vtol, 1, "c2-shape skewed")
    per_cell = xs.nnz / xs.shape[0]
    assert per_cell > 1.5 * 0.05 * 2000          # the kept entries per cell really are well above the uniform matrix's 100


def test_wide_matrix_without_the_16bit_index_mirror(ctx, tmp_path):
    """More than 65 536 genes: no 16-bit index mirror (the 32-bit paths of the moments and compaction passes), HVG
    selection on the host; resident pipeline, backed session and CSC handle against the oracle."""
    import scipy.sparse as sp
    import singlerust_amd as sr
    from oracle import csc_oracle
    from singlerust_amd import backed
    from singlerust_amd.memory import statistics as st
    n, g = 3000, 70_000
    m, _ = synth_host(606, n, g, 0.01)
    a, scores, comps, evr, mean, std, hv = pipeline(ctx, m, 2, 500, 10)
    lg = oracle.log1p_transform(oracle.normalize_total(m, 1e4, ROW))
    assert rel_err(a.x_values(np.float64), lg.values.astype(np.float64)) <= 4e-16
    want_var = oracle.compute_variance(lg, COLUMN)
    assert np.allclose(st.compute_variance(a, sr.Direction.Column), want_var, rtol=1e-11, atol=1e-13)
    assert np.array_equal(st.compute_number(a, sr.Direction.Column), oracle.compute_number(m, COLUMN))
    assert np.array_equal(hv, oracle.select_hvg(want_var, 500))
    want, wc, wevr, *_ = pca_oracle.pca_inplace(lg, 10, None, None, hv)
    assert np.allclose(evr, wevr, rtol=1e-6) and col_err(scores, want) < 1e-6 and col_err(comps, wc) < 1e-6
    # backed session over 7 row tiles
    p = str(tmp_path / "wide")
    backed.BackedCsr.write(p, m.indptr, m.indices, m.values, g)
    r = backed.processing.pca_pipeline(backed.BackedAnnData.open(p, ctx), 450, 1e4, 500, 10, store=2)
    assert np.array_equal(r.selected, hv) and col_err(r.x_pca, want) < 1e-6
    # the same X as a CSC handle: statistics and the transpose with 70k stored rows
    x = sp.csr_matrix((m.values, m.indices.astype(np.int64), m.indptr.astype(np.int64)), shape=(n, g)).tocsc()
    x.sort_indices()
    c = sr.IMAnnData.new_basic(x, ctx=ctx, store=2)
    mc = csc_oracle.Csc.from_scipy(x)
    assert np.array_equal(st.compute_number(c, sr.Direction.Column), csc_oracle.compute_number(mc, COLUMN))
    assert np.array_equal(st.compute_sum(c, sr.Direction.Row), csc_oracle.compute_sum(mc, ROW))
    back = c.x().to_csr()
    assert np.array_equal(back.values(np.float64), m.values.astype(np.float64))


@pytest.mark.parametrize("solver", [0, 2])
def test_more_than_8192_selected_features(ctx, solver):
    """FeatureSelection::None on 9000 genes: an explicit selection wider than the device selection's 8192 (row-major
    compaction, then, for the matrix-free SpMM solver, the tile-major view cut from it), with the Gram solver (auto up to
    k = 16384) and the matrix-free solver."""
    import singlerust_amd as sr
    from singlerust_amd.memory import processing
    from singlerust_amd.memory.processing import dim_red
    m, _ = synth_host(909, 1500, 9000, 0.02)
    a = adata_of(m, ctx, 2)
    processing.normalize_total_inplace(a, 1e4, sr.Direction.Row)
    processing.log1p_transform_inplace(a)
    # VarianceThreshold(0): the genes whose non-zeros differ (std > 0 — the reference divides by the std) — still > 8192
    lg = oracle.log1p_transform(oracle.normalize_total(m, 1e4, ROW))
    info = dim_red.pca_inplace(a, 6, None, None, None, sr.FeatureSelection.VarianceThreshold(0.0), None, solver=solver)
    sel = a.uns["pca"]["selected_features"]
    assert np.array_equal(sel, np.flatnonzero(oracle.compute_variance(lg, COLUMN) > 0.0))
    assert info.k == len(sel) > 8192 and info.solver == (1 if solver == 0 else 2)
    want, wc, wevr, *_ = pca_oracle.pca_inplace(lg, 6, None, None, sel)
    assert np.allclose(a.uns["pca"]["explained_variance_ratio"], wevr, rtol=1e-6)
    assert col_err(a.obsm["X_pca"], want) < 1e-6 and col_err(a.uns["pca"]["components"], wc) < 1e-6


@pytest.mark.parametrize("k", [9000, 100])
def test_explicit_selection_on_a_300k_column_matrix(ctx, k):
    """An explicit selection of 9000 and of 100 features on a 300 000-column matrix: no 16-bit index mirror, and a
    selection table (bits + prefix counts, 75 KB) too large for the LDS — the compaction reads it from global memory.
    Gram solver, against the exact-SVD oracle."""
    import singlerust_amd as sr
    from singlerust_amd.memory import processing
    from singlerust_amd.memory.processing import dim_red
    m, _ = synth_host(3003, 400, 300000, 0.01)
    a = adata_of(m, ctx, 2)
    processing.normalize_total_inplace(a, 1e4, sr.Direction.Row)
    processing.log1p_transform_inplace(a)
    lg = oracle.log1p_transform(oracle.normalize_total(m, 1e4, ROW))
    # genes whose values differ (std > 0: the reference divides by the std), k of them spread over the whole width; five
    # components: the sixth lies within 0.1 % of the seventh at k = 9000
    cand = np.flatnonzero(oracle.compute_variance(lg, COLUMN) > 0.0)
    sel = np.sort(np.random.default_rng(k).choice(cand, k, replace=False)).astype(np.uint64)
    assert sel[-1] > 65536
    a.var["pick"] = np.isin(np.arange(m.n_cols), sel)
    info = dim_red.pca_inplace(a, 5, None, None, None, sr.FeatureSelection.HighlyVariableCol("pick"), None, solver=0)
    assert np.array_equal(a.uns["pca"]["selected_features"], sel)
    assert info.k == k and info.solver == 1
    want, wc, wevr, *_ = pca_oracle.pca_inplace(lg, 5, None, None, sel)
    assert np.allclose(a.uns["pca"]["explained_variance_ratio"], wevr, rtol=1e-6)
    assert col_err(a.obsm["X_pca"], want) < 1e-6 and col_err(a.uns["pca"]["components"], wc) < 1e-6


@pytest.mark.parametrize("seed,n,g,density,n_hvg", [(9501, 1500, 9500, 0.02, 9000), (7001, 400, 70000, 0.01, 100)])
def test_pipeline_hvg_ranked_on_the_host(ctx, seed, n, g, density, n_hvg):
    """HighlyVariable(n) outside the device ranking's envelope (more than 8192 selected; more than 65536 columns): ranked on
    the host and passed on as a list, whose selection table, mean / std and trace k_sel_finish makes.  Selection (set and
    order), mean / std, explained variance ratio, scores and components against the oracle."""
    m, _ = synth_host(seed, n, g, density)
    _, scores, comps, evr, mean, std, hv = pipeline(ctx, m, 2, n_hvg, 5)
    lg = oracle.log1p_transform(oracle.normalize_total(m, 1e4, ROW))
    assert np.array_equal(hv, oracle.select_hvg(oracle.compute_variance(lg, COLUMN), n_hvg))
    want, wc, wevr, wmean, wstd = pca_oracle.pca_inplace(lg, 5, None, None, hv)
    assert np.allclose(mean, wmean, rtol=1e-9, atol=1e-12) and np.allclose(std, wstd, rtol=1e-9, atol=1e-12)
    assert np.allclose(evr, wevr, rtol=1e-6)
    assert col_err(scores, want) < 1e-6 and col_err(comps, wc) < 1e-6


def test_reference_integration_flow(ctx):
    """tests/test_basic_load.rs:108-230 of the reference (load_file_with_test_plot_small_faer / _lapack), on a synthetic
    matrix instead of the h5ad file it reads: filter_cells_inplace(Absolute(200), None) -> filter_genes_inplace(
    Absolute(3), None) -> pca_inplace(Some(5), None, Some(true), Some(32), HighlyVariable(25), FaerSVD) — on RAW counts,
    as the reference's test does — against the oracle's filters and exact SVD."""
    import singlerust_amd as sr
    from oracle import filter_oracle as fo
    from singlerust_amd.memory import processing
    from singlerust_amd.memory.processing import dim_red
    m, _ = synth_host(4242, 3000, 2500, 0.1)
    a = adata_of(m, ctx, 0)
    n_cells_before, n_genes_before = a.n_obs(), a.n_vars()
    processing.filter_cells_inplace(a, sr.FlexValue.Absolute(200), sr.FlexValue.NoLimit())
    processing.filter_genes_inplace(a, sr.FlexValue.Absolute(3), sr.FlexValue.NoLimit())
    want, _ = fo.filter_cells(m, fo.absolute(200), fo.NONE)
    want, _ = fo.filter_genes(want, fo.absolute(3), fo.NONE)
    assert (a.n_obs(), a.n_vars()) == (want.n_rows, want.n_cols)
    assert 0 < a.n_obs() < n_cells_before and 0 < a.n_vars() <= n_genes_before
    assert np.array_equal(a.x_values(np.float64), want.values.astype(np.float64))
    info = dim_red.pca_inplace(a, 5, None, True, 32, sr.FeatureSelection.HighlyVariable(25), None)
    assert info.n_pc == 5 and info.k == 25 and a.obsm["X_pca"].shape == (want.n_rows, 5)
    sel = a.uns["pca"]["selected_features"]
    assert np.array_equal(sel, oracle.select_hvg(oracle.compute_variance(want, COLUMN), 25))
    ws, wc, wevr, *_ = pca_oracle.pca_inplace(want, 5, None, True, sel)
    assert np.allclose(a.uns["pca"]["explained_variance_ratio"], wevr, rtol=1e-6)
    assert col_err(a.obsm["X_pca"], ws) < TOL and col_err(a.uns["pca"]["components"], wc) < TOL

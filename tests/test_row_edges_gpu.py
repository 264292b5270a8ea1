"""The row kernels of singlerust_amd/csrc/rows.hip against their definitions at every loop edge (-m gpu).

row_edges.py places a row of every edge length (the unrolled trips of k_row_sum, the 2048-entry register cache of k_row_pass
and k_row_qc, the scalar tail behind it) at every alignment of its first entry, back to back with neighbours that share its
first and last 16-byte vector, and gives 40 000 short rows to the grid-stride loops.  Every comparison covers all rows, the
filler rows included: a neighbour corrupted by a boundary write fails.  Bars: exact; the derived variance bound
(row_edges.variance_bound); or the bar tests/test_log1p_gpu.py asserts for the same logarithm.  test_row_edges_cpu.py holds
the fixture and the references to the same bars without a device.  Every test prints its largest error in units of its bar."""
import ctypes as C

import numpy as np
import pytest

import row_edges as R

pytestmark = pytest.mark.gpu

STORES = [1, 2]
BOTH = sorted(R.FIXTURES)


def _adata(ctx, fx, store, values=None):
    import singlerust_amd as sr
    v = fx.typed(fx.values if values is None else values, store)
    return sr.IMAnnData.new_basic((fx.n_rows, fx.n_cols, fx.indptr, fx.indices, v), ctx=ctx, store=store)


def _stored(a, store):
    return a.x_values(np.float32 if store == 1 else np.float64)


def _report(check, fx, store, units, what="of the bar"):
    print(f"row_edges {check} [{fx.name}, store {store}]: largest error {units:.3g} {what}")


def _assert_rows_equal(fx, got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    msg = fx.first_bad_row(got != want)
    assert msg is None, f"{what}: {msg}"


def _assert_values_equal(fx, got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape
    msg = fx.first_bad_value(got != want)
    assert msg is None, f"{what}: {msg}"


def _assert_log(fx, got, arg, kind, what, store):
    units = R.log_err_in_bars(got, arg, kind)
    _report(what, fx, store, float(units.max(initial=0.0)))
    msg = fx.first_bad_value(~(units <= 1.0))
    assert msg is None, f"{what} ({kind} bar): {msg}"


def _assert_pattern_unchanged(ctx, a, fx):
    from singlerust_amd import _ffi as F
    ip, ix = np.zeros(fx.n_rows + 1, np.uint64), np.zeros(fx.nnz, np.uint64)
    F.check(F.lib().srx_matrix_download_pattern(a.x().handle, F.ptr(ip), F.ptr(ix)), ctx.handle)
    assert np.array_equal(ip, fx.indptr) and np.array_equal(ix, fx.indices)


@pytest.mark.parametrize("name", BOTH)
@pytest.mark.parametrize("store", STORES)
def test_row_sum_and_number(ctx, store, name):
    """k_row_sum (two 16-byte loads a trip, one more, a remainder of L mod 4 at f32; four values a trip at f64) and
    k_row_number: integer sums bit for bit, 0.0 for an empty row."""
    import singlerust_amd as sr
    from singlerust_amd.memory import statistics
    fx = R.FIXTURES[name]()
    a = _adata(ctx, fx, store)
    _assert_rows_equal(fx, statistics.compute_sum(a, sr.Direction.Row), R.row_sums(name), "compute_sum(Row)")
    _assert_rows_equal(fx, statistics.compute_number(a, sr.Direction.Row), fx.lens.astype(np.uint32), "compute_number(Row)")


@pytest.mark.parametrize("name", BOTH)
@pytest.mark.parametrize("store", STORES)
def test_row_variance(ctx, store, name):
    """k_row_var: NaN exactly on the empty rows, the constant row exactly 0.0, every other row within 2 (L + 4) 2^-53."""
    import singlerust_amd as sr
    from singlerust_amd.memory import statistics
    fx = R.FIXTURES[name]()
    msg, units = R.variance_in_bounds(fx, statistics.compute_variance(_adata(ctx, fx, store), sr.Direction.Row))
    _report("compute_variance(Row)", fx, store, units, "of the bound")
    assert msg is None, msg


@pytest.mark.parametrize("name", BOTH)
@pytest.mark.parametrize("store", STORES)
def test_row_min_max_of_planted_values(ctx, store, name):
    """k_row_minmax: 0.5 / 100 planted at the two ends of every edge row, 0.25 / 200 in the fillers around it."""
    import singlerust_amd as sr
    from singlerust_amd.memory import statistics
    fx = R.FIXTURES[name]()
    mn, mx = statistics.compute_min_max(_adata(ctx, fx, store, fx.minmax_values), sr.Direction.Row)
    want_mn, want_mx = R.min_max(name)
    _assert_rows_equal(fx, mn, want_mn, "compute_min_max(Row), minimum")
    _assert_rows_equal(fx, mx, want_mx, "compute_min_max(Row), maximum")
    if name == "edges":
        e = fx.is_edge & (fx.lens >= 2)
        f = ~fx.is_edge & (fx.lens >= 2)
        assert np.all(mn[e] == 0.5) and np.all(mx[e] == 100.0) and np.all(mn[f] == 0.25) and np.all(mx[f] == 200.0)
        assert np.all(np.isposinf(mn[fx.lens == 0])) and np.all(np.isneginf(mx[fx.lens == 0]))


@pytest.mark.parametrize("name", BOTH)
@pytest.mark.parametrize("store", STORES)
def test_qc_variables_per_cell(ctx, store, name):
    """k_row_qc (the row cached in registers between the two reductions, the tail re-read): number and sum exact, the variance
    as k_row_var's, the standard deviation its square root."""
    from singlerust_amd.memory import statistics
    fx = R.FIXTURES[name]()
    got = statistics.compute_qc_variables(_adata(ctx, fx, store))
    _assert_rows_equal(fx, got.num_per_cell, fx.lens.astype(np.uint32), "num_per_cell")
    _assert_rows_equal(fx, got.expr_per_cell, R.row_sums(name), "expr_per_cell")
    msg, units = R.variance_in_bounds(fx, got.variance_per_cell)
    _report("compute_qc_variables, variance_per_cell", fx, store, units, "of the bound")
    assert msg is None, msg
    ok = fx.lens > 0
    assert np.array_equal(got.std_dev_per_cell[ok], np.sqrt(got.variance_per_cell[ok]))
    assert np.all(np.isnan(got.std_dev_per_cell[~ok]))


@pytest.mark.parametrize("name", BOTH)
@pytest.mark.parametrize("store", STORES)
def test_normalize_total_every_stored_value(ctx, store, name):
    """k_row_pass<NORM>: every stored value, the fillers' too, is storage_type(fl64(v * fl64(1e4 / sum))); the pattern stays."""
    import singlerust_amd as sr
    from singlerust_amd.memory import processing
    fx = R.FIXTURES[name]()
    a = _adata(ctx, fx, store)
    processing.normalize_total_inplace(a, R.TARGET, sr.Direction.Row)
    assert a.x_dtype() == np.float64
    _assert_values_equal(fx, _stored(a, store), fx.typed(R.normalized(name), store), "normalize_total_inplace(1e4, Row)")
    _assert_pattern_unchanged(ctx, a, fx)


@pytest.mark.parametrize("name", BOTH)
@pytest.mark.parametrize("store", STORES)
def test_log1p_of_the_raw_counts(ctx, store, name):
    """k_row_pass<LOG> (no reduction; the cache, the shared vectors and the tail as in the other instantiations): f32 within
    3e-7 relative, f64 within one ulp of the longdouble log1p."""
    from singlerust_amd.memory import processing
    fx = R.FIXTURES[name]()
    a = _adata(ctx, fx, store)
    processing.log1p_transform_inplace(a)
    assert a.x_dtype() == (np.float32 if store == 1 else np.float64)
    _assert_log(fx, _stored(a, store), fx.typed(fx.values, store), "f32" if store == 1 else "f64", "log1p_transform_inplace", store)
    _assert_pattern_unchanged(ctx, a, fx)


@pytest.mark.parametrize("name", BOTH)
@pytest.mark.parametrize("store", STORES)
def test_fused_normalize_log1p(ctx, store, name):
    """k_row_pass<NORM, LOG>: the returned row sums are the integers; the values are, bit for bit, what the two separate calls
    leave on a second handle, and the logarithm of the exact normalised value at the storage's bar."""
    import singlerust_amd as sr
    from singlerust_amd.memory import processing
    fx = R.FIXTURES[name]()
    a, b = _adata(ctx, fx, store), _adata(ctx, fx, store)
    sums = processing.normalize_log1p_inplace(a, R.TARGET)
    _assert_rows_equal(fx, sums, R.row_sums(name), "normalize_log1p_inplace, row sums")
    processing.normalize_total_inplace(b, R.TARGET, sr.Direction.Row)
    processing.log1p_transform_inplace(b)
    got = _stored(a, store)
    _assert_values_equal(fx, got, _stored(b, store), "normalize_log1p_inplace against the two calls")
    _assert_log(fx, got, fx.typed(R.normalized(name), store), "f32" if store == 1 else "f64", "normalize_log1p_inplace", store)
    _assert_pattern_unchanged(ctx, a, fx)


@pytest.mark.parametrize("store", STORES)
def test_pipeline_stored_values(ctx, store):
    """srx_pipeline(1e4, 200 HVGs, 5 PCs) on the edge fixture: k_row_sum, then the moments pass stores ln_1p(v * 1e4 / sum) in
    place.  X against the longdouble log1p of the exact argument at the bars of
    test_log1p_gpu.py::test_pipeline_stored_logarithm_against_longdouble: f64 storage 2.7e-16 relative; f32 storage within one
    f32 ulp of the correctly rounded value, and correctly rounded but for 1e-5 of the values.  The PCA is not judged here."""
    from singlerust_amd import _ffi as F
    fx = R.edges()
    a = _adata(ctx, fx, store)
    opts = F.PcaOpts(5, 1, 1, -1, 0, 0, 0, 0.0, 1)
    res = F.PipelineResult()
    F.check(F.lib().srx_pipeline(a.x().handle, R.TARGET, 200, C.byref(opts), C.byref(res)), ctx.handle)
    assert int(res.pca.k) == 200
    got = _stored(a, store)
    arg = R.normalized("edges")
    if store == 2:
        _assert_log(fx, got, arg, "fast", "srx_pipeline, stored X", store)
    else:
        _assert_log(fx, got, arg, "f32_of_f64", "srx_pipeline, stored X", store)
        n_wrong = int(np.count_nonzero(got != R.ld_log1p(arg).astype(np.float32)))
        print(f"row_edges srx_pipeline [edges, store 1]: {n_wrong} of {fx.nnz} values not correctly rounded")
        assert n_wrong <= 1e-5 * fx.nnz, n_wrong
    _assert_pattern_unchanged(ctx, a, fx)

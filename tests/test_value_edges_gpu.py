"""Signed and extreme values through every entry point, against the oracle (-m gpu).

The rest of the suite feeds small non-negative counts.  Here each of the eight dtypes gets a seeded fixture with its min and
max, mixed-sign rows, a row of one negative entry, a row of non-zero entries that sum to exactly 0, empty rows and columns,
and for floats subnormals, magnitudes across the whole range, -0.0 / +0.0 and a row and a column holding NaN, +inf and -inf.
Each runs as CSR and as CSC, at AUTO and F64 storage and at F32 where the dtype is exact in f32.  The oracle (oracle,
oracle/csc_oracle.py, oracle/filter_oracle.py) is the judge of the reference's semantics; the tolerances are error bounds
of the summation orders, which the device is free to choose.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from oracle import COLUMN, ROW, csc_oracle
from oracle import filter_oracle as fo

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
INT_DTYPES = [np.int8, np.int16, np.int32, np.uint8, np.uint16, np.uint32]
ALL_DTYPES = INT_DTYPES + [np.float32, np.float64]
F32_EXACT = {np.int8, np.int16, np.uint8, np.uint16, np.float32}
N_ROWS, N_COLS = 300, 240
EMPTY_ROWS, EMPTY_COLS = (3, 150, 299), (N_COLS - 2, N_COLS - 1)


def _values(rng, dtype, k):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        lo, hi = (-30, 30) if dt == np.float32 else (-300, 280)      # (f64: sums of a column stay below max + ulp(max) / 2)
        v = np.where(rng.random(k) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(lo, hi, k)
        return v.astype(dtype)
    info = np.iinfo(dtype)
    if dt.itemsize == 4:               # half of them beyond 2^24 (AUTO storage keeps these at f64)
        big = rng.integers(2 ** 24, info.max, k, dtype=np.int64, endpoint=True)
        small = rng.integers(1, 1000, k)
        v = np.where(rng.random(k) < 0.5, big, small)
        if info.min < 0:
            v = v * np.where(rng.random(k) < 0.5, -1, 1)
        return v.astype(dtype)
    v = rng.integers(max(info.min, -info.max), info.max, k, endpoint=True)
    v[v == 0] = 1
    return v.astype(dtype)


def edge_matrix(dtype, seed=0):
    """The fixture as an oracle.Csr (no stored value is 0 but the explicit +-0.0 of the float fixtures)."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    info = np.finfo(dtype) if dt.kind == "f" else np.iinfo(dtype)
    signed = dt.kind != "u"
    live_cols = np.arange(N_COLS - len(EMPTY_COLS))
    rows = []
    for r in range(N_ROWS):
        if r in EMPTY_ROWS:
            rows.append((np.zeros(0, np.int64), np.zeros(0, dtype)))
            continue
        k = int(rng.integers(6, 40))
        cols = np.sort(rng.choice(live_cols[live_cols != 7], k, replace=False))
        v = _values(rng, dtype, k)
        if r == 0:
            if dt.kind == "f":                 # the rest of the row small: -max + max + rest cannot overflow in any order
                v = (v / np.abs(v)).astype(dtype)
                v[0], v[1] = -info.max, info.max
            else:
                v[0], v[1] = info.min if signed else 1, info.max
        if r == 1 and signed:                  # one negative entry
            cols, v = cols[:1], np.array([-37 if dt.kind != "f" else -3.5], dtype)
        if r == 2:                             # non-zero entries summing to exactly 0 (unsigned: the dtype's max alone)
            if signed:
                a, b = (100, 27) if dt.kind != "f" else (1.5, 0.25)
                cols, v = cols[:4], np.array([a, -a, b, -b], dtype)
            else:
                cols, v = cols[:1], np.array([info.max], dtype)
        if r == 4 and dt.kind == "f":          # subnormals and signed zeros
            sub = info.smallest_subnormal
            v[:6] = np.array([sub, -sub, 3 * sub, info.tiny / 2, 0.0, -0.0], dtype)
        if r == 5 and dt.kind == "f":          # the non-finite row
            v[:3] = np.array([np.nan, np.inf, -np.inf], dtype)
        if r in (10, 11, 12) and dt.kind == "f":   # the non-finite column (7)
            cols = np.sort(np.concatenate([cols, [7]]))
            v = np.insert(v, int(np.searchsorted(cols, 7)), np.array([np.nan, np.inf, -np.inf][r - 10], dtype))
        rows.append((cols, v))
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.uint64)
    idx = np.concatenate([c for c, _ in rows]).astype(np.uint64)
    val = np.concatenate([v for _, v in rows]).astype(dtype)
    return oracle.Csr(N_ROWS, N_COLS, indptr, idx, val)


def to_csc(m):
    rows = np.repeat(np.arange(m.n_rows), np.diff(m.indptr.astype(np.int64)))
    order = np.lexsort((rows, m.indices.astype(np.int64)))
    cnt = np.bincount(m.indices.astype(np.int64), minlength=m.n_cols)
    return csc_oracle.Csc(m.n_rows, m.n_cols, np.concatenate([[0], np.cumsum(cnt)]), rows[order], m.values[order])


class Ref:
    """The oracle of one format: CSR through liborc, CSC through csc_oracle."""

    def __init__(self, m, csc):
        self.m, self.csc = (to_csc(m) if csc else m), csc
        self.mod = csc_oracle if csc else oracle

    def __getattr__(self, name):
        f = getattr(self.mod, name)
        return lambda *a: f(self.m, *a)


def upload(ctx, m, csc, store):
    import singlerust_amd as sr
    if csc:
        c = to_csc(m)
        return sr.IMAnnData.new_basic((m.n_rows, m.n_cols, c.col_offsets, c.row_indices, c.values), ctx=ctx, store=store,
                                      csc=True)
    return sr.IMAnnData.new_basic((m.n_rows, m.n_cols, m.indptr, m.indices, m.values), ctx=ctx, store=store)


def stored_keys(m, csc, direction):
    rows = np.repeat(np.arange(m.n_rows), np.diff(m.indptr.astype(np.int64)))
    if not csc:
        return rows if direction == ROW else m.indices.astype(np.int64)
    c = to_csc(m)
    return c.row_indices.astype(np.int64) if direction == ROW else np.repeat(np.arange(m.n_cols), np.diff(c.col_offsets.astype(np.int64)))


def host_moments(m, direction):
    """Per row / column: count, sum |v|, sum v^2 (longdouble; non-finite where the values are)."""
    v = m.values.astype(np.longdouble)
    key = np.repeat(np.arange(m.n_rows), np.diff(m.indptr.astype(np.int64))) if direction == ROW else m.indices.astype(np.int64)
    n = m.n_rows if direction == ROW else m.n_cols
    cnt = np.bincount(key, minlength=n)
    sa, sq = np.zeros(n, np.longdouble), np.zeros(n, np.longdouble)
    with np.errstate(all="ignore"):
        np.add.at(sa, key, np.abs(v))
        np.add.at(sq, key, v * v)
        return cnt, sa.astype(np.float64), sq.astype(np.float64)


def assert_close(got, want, bound, what):
    """NaN exactly where the oracle has it, infinities equal, finite values within `bound` (a NaN / inf bound: no limit)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.flatnonzero(np.isnan(got) != np.isnan(want))[:10])
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), what
    fin = np.isfinite(want)
    b = np.where(np.isfinite(bound), bound, np.inf)[fin]
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got[fin] - want[fin]) <= b)
    assert not bad.any(), (what, got[fin][bad][:5], want[fin][bad][:5], b[bad][:5])


def storages(dtype):
    return [0, 2] + ([1] if dtype in F32_EXACT else [])


CASES = [(d, csc, s) for d in ALL_DTYPES for csc in (False, True) for s in storages(d)]
IDS = [f"{np.dtype(d).name}-{'csc' if csc else 'csr'}-{['auto', 'f32', 'f64'][s]}" for d, csc, s in CASES]


def _variance_bound(cnt, sq, want, one_pass):
    c = cnt.astype(np.float64)
    ms = np.where(c > 0, sq / np.maximum(c, 1), 0.0)
    if one_pass:
        # sq / c - mean^2 (csr.rs:179-185 / csc.rs Row): the rounding of both terms is relative to E[v^2], not to the
        # variance — a difference of two nearly equal numbers can lose every digit
        return (3 * c + 4) * EPS * ms
    # two-pass sum((v - mean)^2) / c: relative to the variance, plus the square of the mean's error
    return (c + 4) * EPS * np.abs(want) + ((c + 2) * EPS) ** 2 * ms * c


@pytest.mark.parametrize("dtype,csc,store", CASES, ids=IDS)
def test_statistics_on_edge_values(ctx, dtype, csc, store):
    import singlerust_amd as sr
    from singlerust_amd.memory import statistics as st
    D = sr.Direction
    m = edge_matrix(dtype, seed=ALL_DTYPES.index(dtype))
    ref = Ref(m, csc)
    a = upload(ctx, m, csc, store)
    exact = np.dtype(dtype).kind != "f"
    qc = st.compute_qc_variables(a)
    for d, od in ((D.Row, ROW), (D.Column, COLUMN)):
        cnt, sa, sq = host_moments(m, od)
        wn = ref.compute_number(od)
        assert np.array_equal(st.compute_number(a, d), wn) and np.array_equal(wn, cnt)
        ws = ref.compute_sum(od)
        got_s = st.compute_sum(a, d)
        if exact:
            assert np.array_equal(got_s, ws), (d, np.flatnonzero(got_s != ws)[:10])     # integers below 2^53: exact
        else:
            assert_close(got_s, ws, cnt * EPS * sa, f"sum {d}")
        # CSR: rows two-pass, columns one-pass; CSC the other way round
        one_pass = (od == COLUMN) != csc
        wv = ref.compute_variance(od)
        vb = _variance_bound(cnt, sq, wv, one_pass)
        assert_close(st.compute_variance(a, d), wv, vb, f"variance {d}")
        wsd = ref.compute_std_dev(od)
        with np.errstate(all="ignore"):
            sdb = np.where(wsd > 0, vb / (2 * wsd), np.sqrt(vb)) + 2 * EPS * np.abs(wsd)
        assert_close(st.compute_std_dev(a, d), wsd, sdb, f"std {d}")
        (gmn, gmx), (wmn, wmx) = st.compute_min_max(a, d), ref.compute_min_max(od)
        assert np.array_equal(gmn, wmn) and np.array_equal(gmx, wmx), d               # NaN ignored, values exact
        # compute_qc_variables: the same rules
        num, s_, var, sd = ((qc.num_per_cell, qc.expr_per_cell, qc.variance_per_cell, qc.std_dev_per_cell) if od == ROW else
                            (qc.num_per_gene, qc.expr_per_gene, qc.variance_per_gene, qc.std_dev_per_gene))
        assert np.array_equal(num, wn)
        if exact:
            assert np.array_equal(s_, ws)
        else:
            assert_close(s_, ws, cnt * EPS * sa, f"qc sum {d}")
        assert_close(var, wv, vb, f"qc variance {d}")
        assert_close(sd, wsd, sdb, f"qc std {d}")


def _log1p_f64_ref(x):
    with np.errstate(all="ignore"):
        return np.log1p(x.astype(np.float64))


@pytest.mark.parametrize("dtype,csc,store", CASES, ids=IDS)
def test_normalize_and_log1p_on_edge_values(ctx, dtype, csc, store):
    """normalize_total_inplace (Row, Column) then log1p_transform_inplace: the scale is target / sum (0 for a zero sum), so
    the normalised values carry the sum's rounding (exact for integer data); the log1p step is compared on the values the
    device normalised.  The zero-sum row becomes exact zeros; arguments below -1 give NaN where the oracle has it."""
    import singlerust_amd as sr
    from singlerust_amd.memory import processing
    D = sr.Direction
    m = edge_matrix(dtype, seed=ALL_DTYPES.index(dtype))
    ref = Ref(m, csc)
    exact = np.dtype(dtype).kind != "f"
    f32 = store == 1 or (store == 0 and np.dtype(dtype) == np.float32)
    for d, od in ((D.Row, ROW), (D.Column, COLUMN)):
        a = upload(ctx, m, csc, store)
        processing.normalize_total_inplace(a, 1e4, d)
        got = a.x_values(np.float64)
        want = ref.normalize_total(1e4, od).values.astype(np.float64)
        if store == 1:                         # f32 storage holds them rounded to f32 (beyond its range: inf / 0)
            with np.errstate(all="ignore"):
                want = want.astype(np.float32).astype(np.float64)
        cnt, sa, _ = host_moments(m, od)
        s = oracle.compute_sum(m, od)
        key = stored_keys(m, csc, od)          # the row / column of every value in stored order
        with np.errstate(all="ignore"):
            rel_sum = np.where(s != 0, (0.0 if exact else 1.0) * cnt * EPS * sa / np.abs(s), 0.0)
        # a float sum that cancels to below its rounding (-max + max + small values) depends on the order: its scale, and
        # whether the scaled values overflow, are not defined by the reference's semantics alone — those rows / columns are
        # left out here (their sums are checked against the bound in test_statistics_on_edge_values)
        with np.errstate(all="ignore"):
            small_dyadic = (sa < 2.0 ** 40) & (sa * 1024 == np.floor(sa * 1024))     # e.g. 1.5 - 1.5 + 0.25 - 0.25: exact
            ordered = np.where(s == 0, exact | small_dyadic, rel_sum <= 1e-3)
        sel = ordered[key]
        assert sel.mean() > 0.9
        tol = (1e-6 if f32 else 4e-16) + 2 * rel_sum[key]
        with np.errstate(all="ignore"):
            assert_close(got[sel], want[sel], (tol * np.abs(want) + (2.0 ** -149 if store == 1 else 0.0))[sel], f"normalize {d}")
        if od == ROW:
            zr = np.flatnonzero((s == 0) & ordered)
            zero_rows = np.isin(key, zr)
            assert np.all(got[zero_rows] == 0.0)
        norm = got.copy()
        processing.log1p_transform_inplace(a)
        got = a.x_values(np.float64)
        want = _log1p_f64_ref(norm)
        with np.errstate(all="ignore"):
            lb = np.spacing(np.abs(want)) * 2 if not f32 else 1e-6 * np.abs(want)
        assert_close(got, want, lb, f"log1p {d}")
        if od == ROW:
            assert np.all(got[zero_rows] == 0.0)
        below = norm < -1
        assert np.all(np.isnan(got[below]))
        if exact:                              # integer data: the normalised values are the oracle's, so are the NaN positions
            assert np.array_equal(np.isnan(got), np.isnan(_log1p_f64_ref(ref.normalize_total(1e4, od).values)))


@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.int32, np.uint32])
def test_filters_on_mixed_sign_sums(ctx, dtype):
    """filter_cells / filter_genes: Absolute limits on the counts, Relative ones on the (mixed-sign) sums' quantiles."""
    import singlerust_amd as sr
    from singlerust_amd.memory import processing
    # (integer data: the sums are exact, so no row sits on the other side of a quantile by a rounding)
    m = edge_matrix(dtype, seed=40 + ALL_DTYPES.index(dtype))
    flex = lambda t: None if t is None else (sr.FlexValue.Absolute(t[1]) if t[0] == "abs" else sr.FlexValue.Relative(t[1]))
    for lower, upper in ((fo.absolute(8), fo.absolute(30)), (fo.relative(0.1), fo.relative(0.9)),
                         (fo.relative(0.25), None), (None, fo.relative(0.6)), (fo.absolute(10), fo.relative(0.7))):
        for genes in (False, True):
            a = upload(ctx, m, False, 0)
            want, wmask = (fo.filter_genes if genes else fo.filter_cells)(m, lower, upper)
            got = (processing.filter_genes if genes else processing.filter_cells)(a, flex(lower), flex(upper))
            assert np.array_equal(got.uns["filter_mask"], wmask), (genes, lower, upper)
            assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
            assert np.array_equal(got.x_values(np.float64), want.values.astype(np.float64))


def mixed_sign_pipeline_matrix(dtype, seed, below_minus_one=False):
    """Counts with a few negative entries per row, each smaller in magnitude than its row's sum: with target 1.0 the
    arguments fall in (-1, 0) as well as above 0.  A row of entries summing to 0, a row of ONE negative entry (argument 1),
    empty rows and columns; planted columns give the PCA variance.  `below_minus_one`: one argument below -1."""
    rng = np.random.default_rng(seed)
    n, g = 600, 300
    rows = []
    for r in range(n):
        if r in (5, 333):
            rows.append((np.zeros(0, np.int64), np.zeros(0)))
            continue
        k = int(rng.integers(15, 50))
        cols = np.sort(rng.choice(np.arange(g - 3), k, replace=False))
        v = rng.integers(1, 60, k).astype(np.float64)
        v[:4] = (r * np.arange(3, 7)) % 41 + 1           # leading columns vary by row
        s = v.sum()
        neg = 4 + rng.choice(k - 4, 3, replace=False)
        v[neg] = -rng.integers(1, int(s // 16), 3, endpoint=True)     # |v| <= s / 16 < the row's new sum
        if r == 7:
            cols, v = cols[:4], np.array([9.0, -9.0, 4.0, -4.0])
        if r == 8:
            cols, v = cols[:1], np.array([-12.0])
        if r == 9 and below_minus_one:
            cols, v = cols[:3], np.array([10.0, 10.0, -11.0])       # sum 9: -11 / 9 < -1
        rows.append((cols, v))
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.uint64)
    return oracle.Csr(n, g, indptr, np.concatenate([c for c, _ in rows]).astype(np.uint64),
                      np.concatenate([v for _, v in rows]).astype(dtype))


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.float32, np.float64])
@pytest.mark.parametrize("store", [1, 2])
def test_pipeline_on_mixed_sign_data(ctx, tmp_path, dtype, store):
    """srx_pipeline at target 1.0 on mixed-sign data (arguments in (-1, 0) and above 0, a zero-sum row): the HVG list is
    oracle.select_hvg's, the stored values and column variances the oracle's; a backed session over two tiles (its compaction
    takes xf_stored on negative arguments) gives the same list and scores."""
    from singlerust_amd import _ffi as F, backed
    from test_backed_gpu import store_of
    from test_pca_gpu import TOL, col_err
    m = mixed_sign_pipeline_matrix(dtype, seed=10 * store + ALL_DTYPES.index(dtype))
    lg = oracle.log1p_transform(oracle.normalize_total(m, 1.0, ROW))
    wv = oracle.compute_variance(lg, COLUMN)
    lgv = lg.values.astype(np.float64)
    assert (lgv < 0).sum() > 100 and (lgv > 0).sum() > 1000 and not np.isnan(lgv).any()
    n_hvg, n_pc = 40, 4
    want_sel = oracle.select_hvg(wv, n_hvg)
    import singlerust_amd as sr
    from singlerust_amd.memory import statistics as st
    a = sr.IMAnnData.new_basic((m.n_rows, m.n_cols, m.indptr, m.indices, m.values), ctx=ctx, store=store)
    opts = F.PcaOpts(n_pc, -1, -1, -1, 0, 0, 0, 0.0, 0)
    res = F.PipelineResult()
    F.check(F.lib().srx_pipeline(a.x().handle, 1.0, n_hvg, C.byref(opts), C.byref(res)), ctx.handle)
    k = int(res.pca.k)
    scores, hv = np.zeros((m.n_rows, n_pc)), np.zeros(k, np.uint64)
    F.check(F.lib().srx_result_fetch(a.x().handle, F.ptr(scores), None, None, None, None, F.ptr(hv)), ctx.handle)
    assert np.array_equal(hv, want_sel)
    got = a.x_values(np.float64)
    # f64: 4e-16 relative, or 2 ulp where the library log1p of both sides decides (arguments in (-1, 0))
    bound = 1e-6 * np.abs(lgv) if store == 1 else np.maximum(4e-16 * np.abs(lgv), 2 * np.spacing(np.abs(lgv)))
    assert np.all(np.abs(got - lgv) <= bound), float(np.max(np.abs(got - lgv) / np.maximum(bound, 1e-300)))
    assert np.all(got[lgv == 0] == 0.0)
    assert np.allclose(st.compute_variance(a, sr.Direction.Column), wv, rtol=1e-5 if store == 1 else 1e-11, atol=1e-12)
    # the same matrix through a backed session, two row tiles
    ad = backed.BackedAnnData.open(store_of(m, tmp_path), ctx)
    r = backed.processing.pca_pipeline(ad, 301, 1.0, n_hvg, n_pc, center=True, scale=True, store=store)
    assert np.array_equal(r.selected, want_sel)
    assert col_err(r.x_pca, scores) < TOL


@pytest.mark.parametrize("store", [1, 2])
def test_pipeline_argument_below_minus_one_is_nan(ctx, store):
    """An argument below -1 makes its gene's moments NaN: the reference panics in partial_cmp().unwrap(); srx_pipeline
    returns SRX_E_NAN."""
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    m = mixed_sign_pipeline_matrix(np.float64, seed=5, below_minus_one=True)
    lg = oracle.log1p_transform(oracle.normalize_total(m, 1.0, ROW))
    assert np.isnan(lg.values).sum() == 1
    with pytest.raises(ValueError):
        oracle.select_hvg(oracle.compute_variance(lg, COLUMN), 40)
    a = sr.IMAnnData.new_basic((m.n_rows, m.n_cols, m.indptr, m.indices, m.values), ctx=ctx, store=store)
    opts = F.PcaOpts(4, -1, -1, -1, 0, 0, 0, 0.0, 0)
    res = F.PipelineResult()
    with pytest.raises(sr.SrxError) as e:
        F.check(F.lib().srx_pipeline(a.x().handle, 1.0, 40, C.byref(opts), C.byref(res)), ctx.handle)
    assert e.value.code == F.E_NAN

"""GPU tests (-m gpu) of the data-movement kernels in front of the hot path: the subset (filter.hip: k_subset_count, the
exclusive scan, k_subset_fill), the QC filters at their edges, and the device transpose (csc.hip: k_hist, the scan,
k_scatter, the LDS-bitmap k_row_order), against scipy.  A gather and a transpose move values without arithmetic, so every
comparison of a moved matrix is bit-exact: indptr, indices, values, shape, nnz, dtype, storage and format.

Storage follows the variant: a matrix uploaded with SRX_STORE_AUTO and held in f32 (u8 / u16 / i8 / i16 / f32 data) widens
to f64 at normalize_total, like the reference's DynCsrMatrix::F64 — also after a filter, a subset or a format conversion."""
import ctypes as C

import numpy as np
import pytest

import oracle
from oracle import ROW, filter_oracle as fo, pca_oracle
from test_pca_gpu import assert_components_within_conditioning, synth_host

pytestmark = pytest.mark.gpu

STORE_AUTO, STORE_F32, STORE_F64 = 0, 1, 2
AUTO_F32 = (np.uint8, np.uint16, np.int16, np.float32)        # SRX_STORE_AUTO holds these in f32
AUTO_F64 = (np.int32, np.float64)                             # ... and these in f64 (controls)


# ---- helpers ------------------------------------------------------------------------------------------------------

def _code(dtype):
    from singlerust_amd.anndata import DTYPE_OF_NP
    return DTYPE_OF_NP[np.dtype(dtype)]


def _canon(x, fmt="csr"):
    """scipy matrix in `fmt` with sorted indices (a copy)."""
    y = x.asformat(fmt).copy()
    y.sort_indices()
    return y


def _upload(ctx, x, store):
    """scipy CSR -> ArrayData::CsrMatrix, scipy CSC -> ArrayData::CscMatrix."""
    import singlerust_amd as sr
    return sr.IMAnnData.new_basic(x, ctx=ctx, store=store)


def _subset(ctx, dev, row_mask, col_mask):
    """srx_subset with masks over the cells / genes of X (None = keep all)."""
    from singlerust_amd import _ffi
    from singlerust_amd.anndata import DeviceCsr
    rm = None if row_mask is None else np.ascontiguousarray(row_mask, dtype=np.uint8)
    cm = None if col_mask is None else np.ascontiguousarray(col_mask, dtype=np.uint8)
    h = C.c_void_p()
    _ffi.check(_ffi.lib().srx_subset(dev.handle, _ffi.ptr(rm), _ffi.ptr(cm), C.byref(h)), ctx.handle)
    return DeviceCsr(ctx, h)


def _scipy_subset(x, row_mask, col_mask):
    y = x.tocsr()
    if row_mask is not None:
        y = y[np.asarray(row_mask, bool)]
    if col_mask is not None:
        y = y[:, np.asarray(col_mask, bool)]
    return y


def _download(ctx, dev):
    from singlerust_amd import _ffi
    i = dev.info()
    n_major = i.n_cols if dev.is_csc() else i.n_rows
    ip = np.zeros(n_major + 1, np.uint64)
    ix = np.zeros(i.nnz, np.uint64)
    _ffi.check(_ffi.lib().srx_matrix_download_pattern(dev.handle, _ffi.ptr(ip), _ffi.ptr(ix)), ctx.handle)
    return i, ip, ix, dev.values(np.float64)


def assert_holds(ctx, dev, want, dtype, store):
    """`dev` holds exactly `want` (a scipy matrix; its format is the one `dev` must have), as `dtype` in `store`."""
    fmt = "csc" if dev.is_csc() else "csr"
    assert fmt == want.format
    want = _canon(want, fmt)
    i, ip, ix, v = _download(ctx, dev)
    assert (i.n_rows, i.n_cols, i.nnz) == (want.shape[0], want.shape[1], want.nnz)
    assert (i.dtype, i.store) == (_code(dtype), store)
    assert np.array_equal(ip, want.indptr) and np.array_equal(ix, want.indices)
    assert np.array_equal(v, want.data.astype(np.float64))


def _ocsr(x):
    """scipy CSR (sorted) -> oracle.Csr."""
    x = _canon(x)
    return oracle.Csr(x.shape[0], x.shape[1], x.indptr, x.indices, x.data)


def _normalize_log1p(ctx, dev):
    from singlerust_amd import _ffi
    _ffi.check(_ffi.lib().srx_normalize_total_inplace(dev.handle, 1e4, _ffi.ROW), ctx.handle)
    _ffi.check(_ffi.lib().srx_log1p_inplace(dev.handle), ctx.handle)


def _oracle_normalize_log1p(x, fmt):
    """log1p(normalize_total(Row)) of the scipy matrix `x`, values in the order of its `fmt` arrays."""
    import scipy.sparse as sp
    x = _canon(x)
    w = oracle.log1p_transform(oracle.normalize_total(_ocsr(x), 1e4, ROW)).values.astype(np.float64)
    if fmt == "csr":
        return w
    return _canon(sp.csr_matrix((w, x.indices, x.indptr), shape=x.shape), "csc").data


def _counts(n, g, seed, dtype, density=0.08, hi=100):
    """Integer-valued counts in [1, hi), no empty row (so that every row sum is exact and positive)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    nnz = int(n * g * density)
    r = np.concatenate([np.arange(n), rng.integers(0, n, nnz)])
    c = np.concatenate([rng.integers(0, g, n), rng.integers(0, g, nnz)])
    x = sp.csr_matrix((np.ones(r.shape[0]), (r, c)), shape=(n, g))
    x.sum_duplicates()
    x.sort_indices()
    return sp.csr_matrix((rng.integers(1, hi, x.nnz).astype(dtype), x.indices, x.indptr), shape=(n, g))


# ---- a. storage follows the variant through every route that makes a new matrix ----------------------------------

ROUTES = ("filter_cells", "filter_genes", "filter_cells_inplace", "filter_genes_inplace", "subset", "to_csc", "csc_to_csr")


def _route(ctx, route, x, store):
    """Run `route` on an upload of `x`; returns (the device matrix it produced, the scipy matrix that must hold)."""
    import singlerust_amd as sr
    from singlerust_amd.memory import processing
    FV = sr.FlexValue
    if route == "csc_to_csr":
        return _upload(ctx, _canon(x, "csc"), store).x().to_csr(), x
    a = _upload(ctx, x, store)
    if route == "to_csc":
        return a.x().to_csc(), _canon(x, "csc")
    n, g = x.shape
    rng = np.random.default_rng(n + g)
    if route == "subset":
        rm, cm = rng.random(n) < 0.7, rng.random(g) < 0.7
        return _subset(ctx, a.x(), rm, cm), _scipy_subset(x, rm, cm)
    genes = route.startswith("filter_genes")
    counts = np.bincount(x.indices, minlength=g) if genes else np.diff(x.indptr)
    lo = int(np.quantile(counts, 0.25))
    keep = counts >= lo
    assert 0 < keep.sum() < keep.size
    fn = getattr(processing, route)
    if route.endswith("_inplace"):
        fn(a, FV.Absolute(lo), FV.None_)
        out = a
    else:
        out = fn(a, FV.Absolute(lo), FV.None_)
        assert np.array_equal(out.uns["filter_mask"], keep)
    return out.x(), _scipy_subset(x, None, keep) if genes else _scipy_subset(x, keep, None)


@pytest.mark.parametrize("dtype", AUTO_F32 + AUTO_F64, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("route", ROUTES)
def test_auto_storage_follows_the_variant_after_the_route(ctx, route, dtype):
    """An SRX_STORE_AUTO upload keeps its automatic storage through filters, subsets and format conversions: the moved
    matrix is bit-exact in its input storage, and normalize_total(Row) + log1p then widen f32 storage to f64 and equal
    the oracle on the scipy matrix to the f64 bar."""
    from singlerust_amd import _ffi
    x = _counts(500, 240, 11, dtype)
    dev, want = _route(ctx, route, x, STORE_AUTO)
    assert_holds(ctx, dev, want, dtype, STORE_F32 if dtype in AUTO_F32 else STORE_F64)
    _normalize_log1p(ctx, dev)
    i = dev.info()
    assert (i.dtype, i.store) == (_ffi.F64, STORE_F64)
    got = dev.values(np.float64)
    np.testing.assert_allclose(got, _oracle_normalize_log1p(want, want.format), rtol=5e-16, atol=0)


@pytest.mark.parametrize("route", ROUTES)
def test_explicit_f32_storage_stays_f32_after_the_route(ctx, route):
    """The negative control: an explicit SRX_STORE_F32 upload stays in f32 storage through the same routes and the
    transform (the values are the oracle's rounded to f32)."""
    from singlerust_amd import _ffi
    x = _counts(500, 240, 12, np.uint16)
    dev, want = _route(ctx, route, x, STORE_F32)
    assert_holds(ctx, dev, want, np.uint16, STORE_F32)
    _normalize_log1p(ctx, dev)
    i = dev.info()
    assert (i.dtype, i.store) == (_ffi.F64, STORE_F32)
    w = _oracle_normalize_log1p(want, want.format)
    got = dev.values(np.float64)
    assert np.array_equal(got, got.astype(np.float32).astype(np.float64))        # held in f32
    np.testing.assert_allclose(got, w, rtol=3e-7, atol=0)


# ---- b. srx_subset at its shapes ----------------------------------------------------------------------------------

LENGTHS = (0, 1, 63, 64, 65, 128, 129)             # + one row holding every column: row r has LENGTHS[r % 8] entries


def _shaped(n, g, seed, dtype):
    """Rows of 0, 1, 63, 64, 65, 128, 129 and g entries in turn (at most g; random columns), fractional values."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    lens = np.minimum(np.array(LENGTHS + (g,))[np.arange(n) % 8], g)
    order = np.argsort(rng.random((n, g)), axis=1)
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(g)[None, :], axis=1)
    r, c = np.nonzero(rank < lens[:, None])                     # row-major: columns ascending within a row
    indptr = np.concatenate([[0], np.cumsum(lens)])
    vals = rng.uniform(0.5, 50.0, r.shape[0]).astype(dtype)
    return sp.csr_matrix((vals, c, indptr), shape=(n, g))


def _masks(kind, n, g, seed):
    rng = np.random.default_rng(seed)
    if kind == "rows":
        return rng.random(n) < 0.6, None
    if kind == "cols":
        return None, rng.random(g) < 0.6
    if kind == "both":
        return rng.random(n) < 0.6, rng.random(g) < 0.6
    if kind == "none":
        return None, None
    if kind == "no_rows":
        return np.zeros(n, bool), rng.random(g) < 0.6
    if kind == "no_cols":
        return rng.random(n) < 0.6, np.zeros(g, bool)
    if kind == "ends":                                          # first and last row / column dropped
        rm, cm = np.ones(n, bool), np.ones(g, bool)
        rm[[0, -1]] = False
        cm[[0, -1]] = False
        return rm, cm
    if kind == "alternating":
        return np.arange(n) % 2 == 0, np.arange(g) % 2 == 1
    raise ValueError(kind)


STORES = [(STORE_F32, np.float32), (STORE_F64, np.float64)]


@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("store,dtype", STORES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["rows", "cols", "both", "none", "no_rows", "no_cols", "ends", "alternating"])
def test_subset_masks_and_row_lengths(ctx, kind, store, dtype, fmt):
    """srx_subset == scipy x[rows][:, cols] for rows of 0 .. every column (the ballot / popcount compaction over more than
    one 64-entry chunk) and every mask form; a CSC input keeps CSC (the masks swap to the stored orientation)."""
    x = _shaped(600, 300, 3, dtype)
    rm, cm = _masks(kind, 600, 300, 4)
    a = _upload(ctx, _canon(x, fmt), store)
    got = _subset(ctx, a.x(), rm, cm)
    assert_holds(ctx, got, _canon(_scipy_subset(x, rm, cm), fmt), dtype, store)


@pytest.mark.parametrize("store,dtype", STORES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [4095, 4096, 4097, 20000])
def test_subset_scan_blocks_and_striding_waves(ctx, n, store, dtype):
    """N around the scan's 1024 x 4 block, and N > 8192 where the count / fill grids (n_cus * 8 workgroups of 4 waves)
    are capped and waves stride over rows."""
    x = _shaped(n, 300, n, dtype)
    rm, cm = _masks("both", n, 300, n + 1)
    got = _subset(ctx, _upload(ctx, x, store).x(), rm, cm)
    assert_holds(ctx, got, _scipy_subset(x, rm, cm), dtype, store)


@pytest.mark.parametrize("store,dtype", STORES, ids=["f32", "f64"])
def test_subset_beyond_4m_rows(ctx, store, dtype):
    """More than 1024 x 4 x 1024 rows (about 2 entries each): the serial pass of the scan walks more than one block sum
    per thread, for the kept-entry offsets and for the new row ids."""
    import scipy.sparse as sp
    n, g = 4_200_000, 8
    rng = np.random.default_rng(8)
    bits = np.unpackbits((rng.integers(0, 256, n, dtype=np.uint8) & rng.integers(0, 256, n, dtype=np.uint8))[:, None], axis=1)
    r, c = np.nonzero(bits)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))])
    x = sp.csr_matrix((rng.uniform(0.5, 50.0, r.shape[0]).astype(dtype), c, indptr), shape=(n, g))
    rm, cm = rng.random(n) < 0.7, np.arange(g) != 3
    got = _subset(ctx, _upload(ctx, x, store).x(), rm, cm)
    assert_holds(ctx, got, _scipy_subset(x, rm, cm), dtype, store)
    got = _subset(ctx, _upload(ctx, x, store).x(), rm, None)
    assert_holds(ctx, got, _scipy_subset(x, rm, None), dtype, store)


@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 8193, 4096 * 1024 + 1])
def test_subset_scan_lengths(ctx, n):
    """The device-wide scan at its own edges, through the row mask it scans: one element, one short of / exactly / one past
    a 4096-element block, past two blocks, and the first length at which the one-workgroup pass over the block sums walks
    more than one of them per thread.  One entry per row, about half of the rows kept."""
    import scipy.sparse as sp
    rng = np.random.default_rng(n)
    x = sp.csr_matrix((rng.uniform(0.5, 50.0, n).astype(np.float32), rng.integers(0, 8, n), np.arange(n + 1)), shape=(n, 8))
    rm = rng.random(n) < 0.5
    got = _subset(ctx, _upload(ctx, x, STORE_F32).x(), rm, None)
    assert_holds(ctx, got, _scipy_subset(x, rm, None), np.float32, STORE_F32)


# ---- c. the filters at their edges --------------------------------------------------------------------------------

def _assert_filter(ctx, got, want, wmask, store=STORE_F32):
    """A filter's result (IMAnnData) == the oracle's (mask, oracle.Csr); u16 counts under SRX_STORE_AUTO sit in f32."""
    assert np.array_equal(got.uns["filter_mask"], wmask)
    assert_holds(ctx, got.x(), _scipy_of(want), want.values.dtype, store)


def _scipy_of(m):
    import scipy.sparse as sp
    return sp.csr_matrix((m.values, m.indices.astype(np.int64), m.indptr.astype(np.int64)), shape=(m.n_rows, m.n_cols))


def _flex(sr, v):
    if v is None:
        return sr.FlexValue.None_
    return sr.FlexValue.Absolute(v[1]) if v[0] == "abs" else sr.FlexValue.Relative(v[1])


@pytest.mark.parametrize("axis", ["cells", "genes"])
def test_absolute_limits_at_counts_that_occur(ctx, axis):
    """Absolute(lo) / Absolute(hi) equal to counts that occur: both ends are inclusive."""
    import singlerust_amd as sr
    from singlerust_amd.memory import processing
    x = _counts(1500, 200, 21, np.uint16, density=0.03, hi=3)
    m = _ocsr(x)
    counts = np.bincount(x.indices, minlength=200) if axis == "genes" else np.diff(x.indptr)
    uniq = np.unique(counts)
    lo, hi = int(uniq[len(uniq) // 4]), int(uniq[3 * len(uniq) // 4])
    assert lo < hi and (counts == lo).any() and (counts == hi).any()
    fn, ofn = (processing.filter_genes, fo.filter_genes) if axis == "genes" else (processing.filter_cells, fo.filter_cells)
    want, wmask = ofn(m, fo.absolute(lo), fo.absolute(hi))
    assert wmask[counts == lo].all() and wmask[counts == hi].all() and not wmask.all()
    got = fn(_upload(ctx, x, STORE_AUTO), sr.FlexValue.Absolute(lo), sr.FlexValue.Absolute(hi))
    _assert_filter(ctx, got, want, wmask)


RELATIVE = [(fo.relative(0.0), None), (None, fo.relative(1.0)), (fo.relative(1.0), None), (None, fo.relative(0.0)),
            (fo.relative(0.0), fo.relative(1.0)), (fo.relative(0.37), fo.relative(0.83)), (fo.absolute(3), fo.relative(0.61))]


@pytest.mark.parametrize("lower,upper", RELATIVE, ids=lambda v: "none" if v is None else f"{v[0]}{v[1]}")
@pytest.mark.parametrize("axis", ["cells", "genes"])
def test_relative_limits_with_tied_sums(ctx, axis, lower, upper):
    """Relative q = 0, q = 1 and q with a fractional index (0.37 (n - 1)) on integer counts whose sums tie a lot: the
    quantile lands on tied sums and the mask keeps all of them; mask and subset bit-exact."""
    import scipy.sparse as sp
    import singlerust_amd as sr
    from singlerust_amd.memory import processing
    base = _counts(500, 70, 22, np.uint16, density=0.1, hi=3)
    x = _canon(sp.hstack([sp.vstack([base] * 3)] * 3))             # 1500 x 210: every cell and gene sum occurs 3+ times
    m = _ocsr(x)
    fn, ofn = (processing.filter_genes, fo.filter_genes) if axis == "genes" else (processing.filter_cells, fo.filter_cells)
    sums = np.asarray(x.sum(axis=0 if axis == "genes" else 1)).ravel()
    assert np.unique(sums, return_counts=True)[1].min() >= 3
    want, wmask = ofn(m, lower, upper)
    got = fn(_upload(ctx, x, STORE_AUTO), _flex(sr, lower), _flex(sr, upper))
    _assert_filter(ctx, got, want, wmask)


def _wide_counts(n, g, seed):
    """n rows of about 100 integer counts over g columns; column 0 and the last column are occupied."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    r = np.concatenate([np.repeat(np.arange(n), 100), [0, n - 1, n // 2]])
    c = np.concatenate([rng.integers(0, g, n * 100), [g - 1, 0, g - 1]])
    x = sp.csr_matrix((np.ones(r.shape[0]), (r, c)), shape=(n, g))
    x.sum_duplicates()
    x.sort_indices()
    return sp.csr_matrix((rng.integers(1, 6, x.nnz).astype(np.uint16), x.indices, x.indptr), shape=(n, g))


@pytest.mark.parametrize("g", [38_912, 38_913, 65_536, 65_537])
def test_gene_counts_and_filter_genes_at_the_count_routes(ctx, g):
    """compute_number(Column) and filter_genes at the column counts where the per-gene count route changes (a counter per
    gene in LDS up to 38,912 columns, the 16-bit mirror up to 65,536), on a fresh upload (counts made under the upload)
    and on a handle that came out of filter_cells (mirror, tile cuts and counts made lazily): counts == np.bincount."""
    import singlerust_amd as sr
    from singlerust_amd.memory import processing, statistics
    FV = sr.FlexValue
    x = _wide_counts(2000, g, g)
    cnt = np.bincount(x.indices, minlength=g)
    assert cnt[0] > 0 and cnt[-1] > 0
    a = _upload(ctx, x, STORE_AUTO)
    assert np.array_equal(statistics.compute_number(a, sr.Direction.Column), cnt)
    uniq = np.unique(cnt)
    lo, hi = int(uniq[1]), int(uniq[-2])
    want, wmask = fo.filter_genes(_ocsr(x), fo.absolute(lo), fo.absolute(hi))
    _assert_filter(ctx, processing.filter_genes(_upload(ctx, x, STORE_AUTO), FV.Absolute(lo), FV.Absolute(hi)), want, wmask)

    rows = np.diff(x.indptr)
    lo_c = int(np.quantile(rows, 0.3))
    b = processing.filter_cells(_upload(ctx, x, STORE_AUTO), FV.Absolute(lo_c), FV.None_)
    keep = rows >= lo_c
    assert np.array_equal(b.uns["filter_mask"], keep) and 0 < keep.sum() < keep.size
    xs = _scipy_subset(x, keep, None)
    assert np.array_equal(statistics.compute_number(b, sr.Direction.Column), np.bincount(xs.indices, minlength=g))
    # a second filtered handle, on which filter_genes is the first per-gene pass
    b2 = processing.filter_cells(_upload(ctx, x, STORE_AUTO), FV.Absolute(lo_c), FV.None_)
    want, wmask = fo.filter_genes(_ocsr(xs), fo.absolute(lo), fo.absolute(hi))
    _assert_filter(ctx, processing.filter_genes(b2, FV.Absolute(lo), FV.Absolute(hi)), want, wmask)


# ---- d. a filtered handle into the fused pipeline -----------------------------------------------------------------

def test_filtered_auto_u16_counts_through_the_fused_pipeline(ctx):
    """AUTO u16 counts -> filter_cells -> filter_genes -> srx_pipeline (HVG + PCA): more than 8192 cells and rows longer than
    64 entries after the filters.  The pipeline widens the AUTO handle to f64, so the result meets the f64-storage bar
    against the oracle on the oracle-filtered matrix."""
    import scipy.sparse as sp
    import singlerust_amd as sr
    from singlerust_amd import _ffi
    from singlerust_amd.memory import processing
    FV = sr.FlexValue
    m32, _ = synth_host(51, 12000, 3000, 0.04)
    assert m32.values.max() < 65536 and np.array_equal(m32.values, np.rint(m32.values))
    m = m32.with_values(m32.values.astype(np.uint16))
    rows = np.diff(m.indptr.astype(np.int64))
    lo_c = int(np.quantile(rows, 0.2))
    w1, _ = fo.filter_cells(m, fo.absolute(lo_c), None)
    gcnt = oracle.compute_number(w1, oracle.COLUMN)
    lo_g = int(np.quantile(gcnt, 0.1))
    w2, gmask = fo.filter_genes(w1, fo.absolute(lo_g), None)
    n, g = w2.n_rows, w2.n_cols
    assert n > 8192 and g <= 65536 and not gmask.all() and np.diff(w2.indptr.astype(np.int64)).max() > 64

    x = sp.csr_matrix((m.values, m.indices.astype(np.int64), m.indptr.astype(np.int64)), shape=(m.n_rows, m.n_cols))
    a = _upload(ctx, x, STORE_AUTO)
    processing.filter_cells_inplace(a, FV.Absolute(lo_c), FV.None_)
    processing.filter_genes_inplace(a, FV.Absolute(lo_g), FV.None_)
    assert_holds(ctx, a.x(), _scipy_of(w2), np.uint16, STORE_F32)

    n_hvg, n_pc = 300, 10
    opts = _ffi.PcaOpts(n_pc, -1, -1, -1, 0, 0, 0, 1e-9, 0)
    res = _ffi.PipelineResult()
    _ffi.check(_ffi.lib().srx_pipeline(a.x().handle, 1e4, n_hvg, C.byref(opts), C.byref(res)), ctx.handle)
    assert a.x().info().store == STORE_F64
    scores = np.zeros((n, n_pc))
    comps = np.zeros((n_hvg, n_pc))
    hv = np.zeros(n_hvg, np.uint64)
    _ffi.check(_ffi.lib().srx_result_fetch(a.x().handle, _ffi.ptr(scores), _ffi.ptr(comps), None, None, None, _ffi.ptr(hv)),
               ctx.handle)
    lg = oracle.log1p_transform(oracle.normalize_total(w2, 1e4, ROW))
    # X holds the pipeline's f64 logarithm (within 2.5 ulp, test_log1p_gpu); f32 storage would be off by ~1e-8
    np.testing.assert_allclose(a.x_values(), lg.values, rtol=1e-15, atol=0)
    want_sel = pca_oracle.select_features_hvg(lg, n_hvg)
    assert np.array_equal(hv, want_sel)
    want_scores, want_comps, evr, *_ = pca_oracle.pca_inplace(lg, n_pc, None, None, hv)
    assert_components_within_conditioning(scores, want_scores, evr, STORE_F64, "filtered pipeline scores", tol=1e-8)
    assert_components_within_conditioning(comps, want_comps, evr, STORE_F64, "filtered pipeline components", tol=1e-8)


# ---- e. the transpose at the LDS-bitmap boundaries ----------------------------------------------------------------

# stored rows R of the transposed matrix: the row-ordering pass keeps a bitmap of R bits + a prefix count per 32-bit word
# per wave in LDS (8 * ceil(R / 32) bytes), 4 waves per workgroup up to R = 163,840, then 3, 2, 1; 655,360 fills 160 KiB
LDS_ROWS = [1, 33, 163_840, 163_841, 327_680, 327_681, 655_360]


def _random_csr(n, g, nnz, seed, dtype):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    x = sp.csr_matrix((np.ones(nnz), (rng.integers(0, n, nnz), rng.integers(0, g, nnz))), shape=(n, g))
    x.sum_duplicates()
    x.sort_indices()
    return sp.csr_matrix((rng.uniform(0.5, 50.0, x.nnz).astype(dtype), x.indices, x.indptr), shape=(n, g))


@pytest.mark.parametrize("store,dtype", STORES, ids=["f32", "f64"])
@pytest.mark.parametrize("r", LDS_ROWS)
def test_transpose_roundtrip_at_the_lds_bitmap_limits(ctx, r, store, dtype):
    """to_csc of an R-row CSR matrix (an output wider than 65,536 columns from R = 163,840 on) and back, bit-exact against
    scipy; output rows of up to ~1000 entries, so the ordering pass walks many 64-entry chunks per row."""
    g = 2000
    x = _random_csr(r, g, min(2_000_000, r * g // 4), r, dtype)
    t = _upload(ctx, x, store).x().to_csc()
    assert_holds(ctx, t, _canon(x, "csc"), dtype, store)
    assert_holds(ctx, t.to_csr(), x, dtype, store)


@pytest.mark.parametrize("store,dtype", STORES, ids=["f32", "f64"])
def test_transpose_of_empty_matrices(ctx, store, dtype):
    """No entries at all, and no rows at all (a subset that dropped every row)."""
    import scipy.sparse as sp
    x = sp.csr_matrix((np.zeros(0, dtype), np.zeros(0, np.int32), np.zeros(41, np.int64)), shape=(40, 30))
    a = _upload(ctx, x, store)
    t = a.x().to_csc()
    assert_holds(ctx, t, _canon(x, "csc"), dtype, store)
    assert_holds(ctx, t.to_csr(), x, dtype, store)
    y = _shaped(64, 30, 5, dtype)
    none = _subset(ctx, _upload(ctx, y, store).x(), np.zeros(64, bool), None)
    t = none.to_csc()
    assert_holds(ctx, t, _canon(_scipy_subset(y, np.zeros(64, bool), None), "csc"), dtype, store)
    assert_holds(ctx, _upload(ctx, _canon(y, "csc"), store).x().to_csr(), y, dtype, store)


def test_transpose_refuses_more_rows_than_the_lds_bitmap_holds(ctx):
    """R = 655,361 stored rows: the bitmap and prefix counts of one wave exceed 160 KiB -> SRX_E_ARG, and the context
    stays usable afterwards."""
    from singlerust_amd import _ffi
    x = _random_csr(655_361, 50, 20_000, 7, np.float32)
    a = _upload(ctx, x, STORE_F32)
    with pytest.raises(_ffi.SrxError) as e:
        a.x().to_csc()
    assert e.value.code == _ffi.E_ARG
    y = _random_csr(3000, 400, 60_000, 8, np.float32)
    assert_holds(ctx, _upload(ctx, y, STORE_F32).x().to_csc(), _canon(y, "csc"), np.float32, STORE_F32)
    assert_holds(ctx, a.x().to_csr(), x, np.float32, STORE_F32)          # a CSR handle: a copy

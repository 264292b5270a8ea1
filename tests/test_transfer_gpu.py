"""The transfer workers (transfer.hip) at sizes where a worker reuses its staging buffers.

8 workers with two 4 MiB pinned buffers each: a worker waits on a buffer's event before it fills it a second time (H2D), and its
third DMA overwrites the buffer its first one used (D2H), only when it moves three or more chunks — an array of more than 16
chunks.  Every array here is that long, with a count that is no multiple of 16, and its values name their position
(value[p] = p mod 2^24, exact in f32), so a chunk that lands in the wrong place cannot compare equal.  The CSRs are built
directly (row lengths, then sorted distinct columns per row)."""
import numpy as np
import pytest
import scipy.sparse as sp

from test_pca_transform_gpu import ABSENT, BOUND, comp_err, random_model, restate, transform, upload as upload_query

pytestmark = pytest.mark.gpu

BOUNDS_MSG = "column index out of bounds (>= n_cols = %d)"


def make_csr(n_rows, n_cols, lo, hi, seed):
    """Row r holds lens[r] in [lo, hi] columns off[r] + j * stride[r]: sorted, distinct, spread over the whole column range."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, n_rows)
    if int(lens.sum()) % 16 == 0:
        lens[-1] += 1
    indptr = np.zeros(n_rows + 1, np.uint64)
    indptr[1:] = np.cumsum(lens)
    nnz = int(indptr[-1])
    stride = n_cols // lens
    off = rng.integers(0, n_cols - stride * (lens - 1))          # last column off + stride * (len - 1) < n_cols
    j = np.arange(nnz, dtype=np.int64) - np.repeat(indptr[:-1].astype(np.int64), lens)
    j *= np.repeat(stride, lens)
    j += np.repeat(off, lens)
    assert nnz % 16 and int(j.max()) < n_cols
    return indptr, j.astype(np.uint64)


def position_values(nnz, dtype):
    if np.dtype(dtype) == np.uint16:
        return (np.arange(nnz, dtype=np.int64) % 65521 + 1).astype(np.uint16)      # 65521: prime, no chunk size divides it
    return (np.arange(nnz, dtype=np.int64) % (1 << 24)).astype(dtype)


def device_csr(ctx, n_rows, n_cols, indptr, indices, values, store):
    import singlerust_amd as sr
    return sr.DeviceCsr.upload(ctx, n_rows, n_cols, indptr, indices, values, store)


def pattern(dev):
    from singlerust_amd import _ffi as F
    i = dev.info()
    indptr, indices = np.zeros(i.n_rows + 1, np.uint64), np.zeros(i.nnz, np.uint64)
    F.check(F.lib().srx_matrix_download_pattern(dev.handle, F.ptr(indptr), F.ptr(indices)), dev.ctx.handle)
    return indptr, indices


@pytest.fixture(scope="module")
def wide():
    """100 000 x 70 000 (32-bit indices), ~20.5M non-zeros: more than 19 index chunks of 1 048 576 entries."""
    n_rows, n_cols = 100_000, 70_000
    indptr, indices = make_csr(n_rows, n_cols, 150, 260, seed=1)
    assert len(indices) > 19 * (1 << 20) and int(indices.max()) >= 65_536
    indptr.setflags(write=False)
    indices.setflags(write=False)
    return n_rows, n_cols, indptr, indices


@pytest.fixture(scope="module")
def narrow():
    """90 000 x 60 000 (16-bit indices), ~36M non-zeros: more than 17 index chunks of 2 097 152 entries, two convert chunks."""
    n_rows, n_cols = 90_000, 60_000
    indptr, indices = make_csr(n_rows, n_cols, 300, 500, seed=2)
    assert len(indices) > 17 * (2 << 20) and len(indices) > (32 << 20)
    indptr.setflags(write=False)
    indices.setflags(write=False)
    return n_rows, n_cols, indptr, indices


@pytest.mark.parametrize("dtype,store", [(np.float32, 1), (np.float64, 2)])
def test_32_bit_indices_and_staged_values_round_trip(ctx, wide, dtype, store):
    n_rows, n_cols, indptr, indices = wide
    values = position_values(len(indices), dtype)
    dev = device_csr(ctx, n_rows, n_cols, indptr, indices, values, store)
    assert dev.info().store == store
    got_ptr, got_idx = pattern(dev)
    assert np.array_equal(got_ptr, indptr) and np.array_equal(got_idx, indices)
    got = dev.values()                                    # 82 MB / 164 MB: the D2H workers, three chunks each
    assert got.dtype == dtype and np.array_equal(got, values)
    if store == 1:                                        # converted on the device, fetched as f64
        assert np.array_equal(dev.values(np.float64), values.astype(np.float64))
    dev.free()


def test_16_bit_indices_and_converted_values_round_trip(ctx, narrow):
    import singlerust_amd as sr
    from singlerust_amd.memory import statistics
    n_rows, n_cols, indptr, indices = narrow
    values = position_values(len(indices), np.uint16)
    dev = device_csr(ctx, n_rows, n_cols, indptr, indices, values, 0)
    got_ptr, got_idx = pattern(dev)
    assert np.array_equal(got_ptr, indptr) and np.array_equal(got_idx, indices)
    assert np.array_equal(dev.values(), values.astype(np.float64))
    # the 16-bit mirror and the tile cuts made from the upload
    a = sr.IMAnnData(dev, indptr, indices, [], [])
    want = np.bincount(indices.astype(np.int64), minlength=n_cols)
    assert np.array_equal(statistics.compute_number(a, sr.Direction.Column), want)
    dev.free()


@pytest.mark.parametrize("nnz", [16_777_216, 16_777_217])
def test_staging_limit_of_d2h(ctx, nnz):
    """64 MiB of f32 values take the staging buffer, four bytes more the workers."""
    n_cols = 2_048
    full = nnz // n_cols
    lens = np.full(full + (nnz % n_cols != 0), n_cols, np.int64)
    if nnz % n_cols:
        lens[-1] = nnz % n_cols
    indptr = np.zeros(len(lens) + 1, np.uint64)
    indptr[1:] = np.cumsum(lens)
    indices = (np.arange(nnz, dtype=np.int64) % n_cols).astype(np.uint64)
    values = position_values(nnz, np.float32)
    dev = device_csr(ctx, len(lens), n_cols, indptr, indices, values, 1)
    assert dev.info().nnz == nnz
    assert np.array_equal(dev.values(), values)
    dev.free()


def bounds_error(ctx, shape, at):
    from singlerust_amd import _ffi as F
    n_rows, n_cols, indptr, indices = shape
    bad = indices.copy()
    bad[at] = n_cols
    with pytest.raises(F.SrxError) as ei:
        device_csr(ctx, n_rows, n_cols, indptr, bad, position_values(len(bad), np.float32), 1)
    assert ei.value.code == F.E_BOUNDS and ei.value.msg == BOUNDS_MSG % n_cols, str(ei.value)


def test_out_of_range_column_in_the_last_chunk_32_bit(ctx, wide):
    bounds_error(ctx, wide, -1)


def test_out_of_range_column_in_the_first_chunk_16_bit(ctx, narrow):
    bounds_error(ctx, narrow, 5)


# ---- strided rows: the score matrix of a PCA transform -------------------------------------------------------------
K, GENES, ROWS = 56, 60, 200_003
ROWS_PER_BUFFER = 10_485                  # a 400-byte score row (n_pc = 50): 4 MiB / 400


def query_counts(rng, n):
    x = sp.random(n, GENES, density=0.1, format="csr", random_state=np.random.RandomState(int(rng.integers(1 << 30))),
                  data_rvs=lambda s: rng.integers(1, 30, s).astype(np.float64))
    x.sort_indices()
    return x


@pytest.fixture(scope="module")
def scored():
    """The query, the model parts and the numpy restatement of its scores, per n_pc."""
    rng = np.random.default_rng(50)
    x = query_counts(rng, ROWS)
    feat = rng.permutation(GENES)[:K].astype(np.uint64)
    feat[[2, 31]] = ABSENT
    out = {"x": x, "feat": feat}
    for n_pc in (50, 64):
        V, mu, sd = random_model(rng, K, n_pc)
        out[n_pc] = (V, mu, sd, restate(x, V, mu, sd, 1, 1, feat))
    return out


# n_pc = 50: 400-byte rows at a device pitch of 512, more than 19 staging buffers (three per worker, the last one partial);
# n_pc = 64: pitch = width, the contiguous route (102 MB)
@pytest.mark.parametrize("n_pc", [50, 64])
@pytest.mark.parametrize("store", [1, 2])
def test_score_rows_download(ctx, scored, store, n_pc):
    from singlerust_amd.memory.processing.dim_red import PcaModel
    assert ROWS > 19 * ROWS_PER_BUFFER and ROWS % ROWS_PER_BUFFER
    V, mu, sd, ref = scored[n_pc]
    q = upload_query(ctx, scored["x"], store)
    got = transform(PcaModel.from_parts(ctx, V, mu, sd), q, scored["feat"])
    err = comp_err(got, ref)
    print("store", store, "n_pc", n_pc, "err", err)
    assert err <= BOUND[store], err
    # The first row of a worker's second buffer and the last row, each on its own.  A row is passed as a vector, so comp_err is
    # max |got[r] - ref[r]| / max |ref[r]| over its components: the row's own magnitude, not the matrix's.  (As a 1 x n_pc matrix
    # every component would be divided by its own value in this row; a score is a sum of ~56 terms of either sign, its rounding
    # error follows the terms and not the sum, and a sum that cancels to nearly zero has no bounded elementwise relative error.)
    for r in (ROWS_PER_BUFFER, ROWS - 1):
        e = comp_err(got[r], ref[r])
        print("row", r, "err", e)
        assert e <= BOUND[store], (r, e)


@pytest.mark.parametrize("n", [0, 1])
@pytest.mark.parametrize("store", [1, 2])
def test_score_rows_download_of_tiny_queries(ctx, scored, store, n):
    from singlerust_amd.memory.processing.dim_red import PcaModel
    V, mu, sd, ref = scored[50]
    x = scored["x"][:n]
    got = transform(PcaModel.from_parts(ctx, V, mu, sd), upload_query(ctx, x, store), scored["feat"])
    assert got.shape == (n, 50)
    if n:
        assert comp_err(got[0], ref[0]) <= BOUND[store]          # the row as a vector: see test_score_rows_download

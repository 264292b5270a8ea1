"""The bucket pass (k_bucket) that makes the sparse Gram kernel's owner records, tested through srx_spmm's Gram output.

A workgroup takes a block of 512 cells; wave v of its 16 takes the R = 32 rows [32 v, 32 v + 32) of the block as one flat span of
entries, keeps the first chunks of the span in registers (40 chunks of 64 f32 entries, 20 of f64 entries) and walks the rest a
second time; the owner counters are scanned in pieces of 64.  The cases below put rows, spans and owner counts on every side of
those edges.  Values are small integers, so every sum of X^T X is an integer far below 2^53: scipy's product is exact and the
device result must EQUAL it, whatever order the records of a (block, owner) run come in."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXED_POINT, F64_ATOMICS = 2, 1


def counts_matrix(rng, lens, g):
    """CSR with lens[r] entries in row r at sorted random columns, integer counts 1 .. 6."""
    import scipy.sparse as sp
    lens = np.asarray(lens, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rng.choice(g, n, replace=False)) for n in lens] + [np.zeros(0, dtype=np.int64)])
    data = rng.integers(1, 7, int(lens.sum())).astype(np.float64)
    return sp.csr_matrix((data, indices.astype(np.int64), indptr), shape=(len(lens), g))


def random_lens(rng, n, g, density):
    return rng.binomial(g, density, n)


def gram_and_mode(ctx, x, store):
    from singlerust_amd import _ffi
    import singlerust_amd as sr
    n, g = x.shape
    a = sr.IMAnnData.new_basic(x, ctx=ctx, store=store)
    sel = np.arange(g).astype(np.uint64)
    P = np.zeros((g, 64))
    y, t, gram = np.zeros((n, 64)), np.zeros((g, 64)), np.zeros((g, g))
    _ffi.check(_ffi.lib().srx_spmm(a.x().handle, _ffi.ptr(sel), g, _ffi.ptr(P), _ffi.ptr(y), _ffi.ptr(t), _ffi.ptr(gram)), ctx.handle)
    mode = C.c_int32(0)
    _ffi.check(_ffi.lib().srx_gram_mode_info(ctx.handle, C.byref(mode)), ctx.handle)
    return gram, mode.value


def check_exact(ctx, x, store, want_mode=None):
    gram, mode = gram_and_mode(ctx, x, store)
    want = (x.T @ x).toarray()
    assert np.array_equal(gram, want)
    if want_mode is not None:
        assert mode == want_mode


@pytest.mark.parametrize("store", [1, 2])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 511, 512, 513, 1024, 1025, 1537])
def test_row_counts_at_the_edges_of_wave_runs_and_blocks(ctx, store, n):
    """The last wave run of a block holds 1, 31, 32 rows or is missing; the last block holds 1 row, a full 512 or 1 more."""
    rng = np.random.default_rng(1000 + n)
    g = 320
    check_exact(ctx, counts_matrix(rng, random_lens(rng, n, g, 0.10), g), store, FIXED_POINT)


@pytest.mark.parametrize("store", [1, 2])
@pytest.mark.parametrize("case", ["empty_wave_run", "empty_block", "first_and_last_row_empty", "all_rows_empty"])
def test_empty_rows_runs_and_blocks(ctx, store, case):
    rng = np.random.default_rng(7)
    g = 320
    if case == "empty_wave_run":
        lens = random_lens(rng, 512, g, 0.10)
        lens[64:96] = 0                          # wave 2 of the block has a span of no entries
    elif case == "empty_block":
        lens = random_lens(rng, 1536, g, 0.10)
        lens[512:1024] = 0                       # a block that makes no record, between two that do
    elif case == "first_and_last_row_empty":
        lens = random_lens(rng, 700, g, 0.10)
        lens[0] = lens[-1] = 0
    else:
        lens = np.zeros(600, dtype=np.int64)
    x = counts_matrix(rng, lens, g)
    check_exact(ctx, x, store, FIXED_POINT if x.nnz else None)


@pytest.mark.parametrize("store", [1, 2])
@pytest.mark.parametrize("case", ["long_rows", "long_run_then_short_rows"])
def test_spans_longer_than_the_resident_part(ctx, store, case):
    """Rows of 300 kept entries (k = 320): suffixes of up to 5 pieces, a wave span of 32 x 300 = 9600 entries = 150 chunks, of which the
    first 40 (f32) or 20 (f64) stay in registers and the others are read again by the scatter phase; then such a run beside runs of
    short rows in the same block (and a second block)."""
    rng = np.random.default_rng(11)
    g = 320
    if case == "long_rows":
        lens = np.full(64, 300)
    else:
        lens = np.concatenate([np.full(32, 300), random_lens(rng, 568, g, 0.03)])
    check_exact(ctx, counts_matrix(rng, lens, g), store, FIXED_POINT)


@pytest.mark.parametrize("store", [1, 2])
@pytest.mark.parametrize("k,n,density", [(8, 700, 0.5), (64, 700, 0.3), (2000, 1100, 0.036)])
def test_owner_counts(ctx, store, k, n, density):
    """k = 8: one owner; k = 64: four; k = 2000 (stripes of 4 rows): 250 owners — four pieces of 64 counters, the last one of 58."""
    rng = np.random.default_rng(13 + k)
    check_exact(ctx, counts_matrix(rng, random_lens(rng, n, k, density), k), store, FIXED_POINT)


@pytest.mark.parametrize("store", [1, 2])
@pytest.mark.parametrize("case", ["negative", "wide"])
def test_value_statistics_of_the_count_phase(ctx, store, case):
    """One negative value, or 1 and 3000 side by side, anywhere in the matrix — here in the re-read part of a long span and in a
    short row of another block — sends the launch to the f64 atomics; the sums stay exact (integers)."""
    rng = np.random.default_rng(17)
    g = 320
    lens = np.concatenate([np.full(32, 300), random_lens(rng, 600, g, 0.10)])
    x = counts_matrix(rng, lens, g)
    if case == "negative":
        x.data[9000] = -3.0                      # row 30 of the long run: behind the resident chunks of either storage
    else:
        x.data[:] = 1.0
        x.data[x.indptr[620]] = 3000.0           # a short row of the second block
    assert x.indptr[620 + 1] > x.indptr[620]
    check_exact(ctx, x, store, F64_ATOMICS)

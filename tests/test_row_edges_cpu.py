"""The fixtures and references of row_edges.py, without a device: every (length, alignment) pair is where it claims to be, and
the C oracle and the numpy reference agree on the fixtures — sums, normalised values and min/max bit for bit, variances and
logarithms within the bars test_row_edges_gpu.py holds the device to.  A fixture that stops exercising an edge, or a
reference that misses its own bar, fails here."""
import numpy as np
import pytest

import oracle
from oracle import ROW
import row_edges as R

NAMES = sorted(R.FIXTURES)


def _csr(fx, values, dtype):
    return oracle.Csr(fx.n_rows, fx.n_cols, fx.indptr, fx.indices, values.astype(dtype))


def test_every_length_at_every_alignment():
    fx = R.edges()
    assert len(R.EDGE_LENGTHS) == len(set(R.EDGE_LENGTHS)) == 52
    assert set(fx.pairs) == {(L, a) for L in R.EDGE_LENGTHS for a in R.ALIGNMENTS} and len(fx.pairs) == 208
    ip = fx.indptr.astype(np.int64)
    for (L, a), r in fx.pairs.items():
        assert fx.is_edge[r] and ip[r + 1] - ip[r] == L and ip[r] % 4 == a == fx.align[r], (L, a, r)
    assert len(set(fx.pairs.values())) == 208 and fx.const_row not in fx.pairs.values()
    assert int(fx.is_edge.sum()) == 209 and fx.n_cols == 8192 and fx.nnz == int(fx.lens.sum())
    assert np.all(fx.lens[~fx.is_edge] <= 3)
    # the cache edge: every tail length 0..4 at every offset (f32: 2048 - a cached entries; f64: 2048 - a % 2)
    for v in (4, 2):
        tails = {(a, L - (R.CACHE - a % v)) for (L, a) in fx.pairs if 2044 <= L <= 2052}
        assert tails >= {(a, t) for a in R.ALIGNMENTS for t in range(0, 5)}
    # all four wave slots of a workgroup, also among the rows at the cache edge and the rows longer than the cache
    edge_rows = np.nonzero(fx.is_edge)[0]
    assert set(edge_rows % 4) == {0, 1, 2, 3}
    assert {r % 4 for (L, a), r in fx.pairs.items() if 2044 <= L <= 2052} == {0, 1, 2, 3}
    assert {r % 4 for (L, a), r in fx.pairs.items() if L > 2052} == {0, 1, 2, 3}
    # one launch, one row per wave: fewer workgroups than the smallest cap (8 per CU) of any card
    assert (fx.n_rows + 3) // 4 < 8 * 64


def test_rows_share_their_boundary_vectors():
    """Edge rows directly behind one another (no filler row between them), some of them starting inside a 16-byte vector, and
    non-empty fillers whose whole row lies inside a vector shared with both neighbours."""
    fx = R.edges()
    both = fx.is_edge[:-1] & fx.is_edge[1:] & (fx.lens[:-1] > 0) & (fx.lens[1:] > 0)
    assert both.sum() >= 10
    assert (both & (fx.align[1:] != 0)).sum() >= 5                 # the shared vector holds entries of both edge rows
    assert {int(a) for a in fx.align[1:][both]} == {0, 1, 2, 3}
    assert ((fx.lens == 0) & ~fx.is_edge).sum() >= 5               # an empty row between two edge rows
    for f in (1, 2, 3):
        assert ((fx.lens == f) & ~fx.is_edge).sum() >= 10
    long_then_row = fx.is_edge[:-1] & (fx.lens[:-1] > R.CACHE) & (fx.lens[1:] > 0) & (fx.indptr[1:-1] % 4 != 0)
    assert long_then_row.sum() >= 10                               # a tail loop ends inside a vector the next row starts in


@pytest.mark.parametrize("name", NAMES)
def test_pattern_and_values(name):
    fx = R.FIXTURES[name]()
    ip = fx.indptr.astype(np.int64)
    idx = fx.indices.astype(np.int64)
    assert ip[0] == 0 and ip[-1] == len(idx) == len(fx.values) and np.all(np.diff(ip) == fx.lens)
    assert idx.min() >= 0 and idx.max() < fx.n_cols
    inner = np.ones(len(idx), bool)
    inner[ip[:-1][fx.lens > 0]] = False                            # not a row's first entry
    assert np.all(np.diff(idx)[inner[1:]] > 0)                     # sorted and unique within every row
    for v in (fx.values, fx.minmax_values):
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    assert np.array_equal(fx.values, np.round(fx.values)) and fx.values.min() >= 1 and fx.values.max() <= 49
    assert R.row_sums(name).max() < 2 ** 19
    if fx.const_row is not None:
        r = fx.const_row
        assert fx.lens[r] == 2049 and np.all(fx.values[ip[r]:ip[r + 1]] == 7.0) and R.row_variance(name)[r] == 0.0


def test_cycle_fixture_makes_every_wave_walk_several_rows():
    fx = R.cycle()
    assert fx.n_rows == 40_000 and np.array_equal(fx.lens, np.arange(40_000) % 10) and 170_000 < fx.nnz < 190_000
    assert fx.n_rows >= 4 * (4 * 8 * 304)                          # four rows a wave at 304 CUs, the largest of these cards
    assert set(fx.align) == {0, 1, 2, 3}


def test_planted_extremes():
    fx = R.edges()
    mn, mx = R.min_max("edges")
    e = fx.is_edge & (fx.lens >= 2)
    assert np.all(mn[e] == 0.5) and np.all(mx[e] == 100.0)
    e1 = fx.is_edge & (fx.lens == 1)
    assert np.all(mn[e1] == 100.0) and np.all(mx[e1] == 100.0)
    f = ~fx.is_edge & (fx.lens >= 2)
    assert np.all(mn[f] == 0.25) and np.all(mx[f] == 200.0)
    f1 = ~fx.is_edge & (fx.lens == 1)
    assert set(mn[f1]) == {0.25, 200.0} and np.array_equal(mn[f1], mx[f1])
    assert np.all(np.isposinf(mn[fx.lens == 0])) and np.all(np.isneginf(mx[fx.lens == 0]))
    # unique: the planted values occur once per row, and the entries next to a row boundary lie outside the neighbour's range
    ip = fx.indptr.astype(np.int64)
    for r in np.nonzero(e)[0][:50]:
        v = fx.minmax_values[ip[r]:ip[r + 1]]
        assert (v == 0.5).sum() == 1 and (v == 100.0).sum() == 1 and v[0] == 0.5 and v[-1] == 100.0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", NAMES)
def test_oracle_agrees_with_the_numpy_reference(name, dtype):
    fx = R.FIXTURES[name]()
    m = _csr(fx, fx.values, dtype)
    assert np.array_equal(oracle.compute_number(m, ROW), fx.lens)
    assert np.array_equal(oracle.compute_sum(m, ROW), R.row_sums(name))
    assert np.all(R.row_sums(name)[fx.lens == 0] == 0.0)
    assert np.array_equal(oracle.normalize_total(m, R.TARGET, ROW).values, R.normalized(name))
    mn, mx = oracle.compute_min_max(_csr(fx, fx.minmax_values, dtype), ROW)
    assert np.array_equal(mn, R.min_max(name)[0]) and np.array_equal(mx, R.min_max(name)[1])
    with np.errstate(invalid="ignore"):
        msg, units = R.variance_in_bounds(fx, oracle.compute_variance(m, ROW))
    print(f"{name} {np.dtype(dtype).name}: oracle row variance at {units:.3g} of the bound")
    assert msg is None, msg
    assert units <= 1.0


@pytest.mark.parametrize("name", NAMES)
def test_reference_logarithms_meet_the_device_bars(name):
    """libm's log1p / log1pf on the raw integers and on the normalised values against the longdouble reference, at the bars
    the device routines are held to: the reference and the bars fit together."""
    fx = R.FIXTURES[name]()
    for arg64 in (fx.values, R.normalized(name)):
        o = oracle.log1p_transform(_csr(fx, arg64, np.float64)).values
        assert R.log_err_in_bars(o, arg64, "f64").max() <= 1.0
        arg32 = arg64.astype(np.float32)
        o = oracle.log1p_transform(_csr(fx, arg32, np.float32)).values
        assert o.dtype == np.float32 and R.log_err_in_bars(o, arg32, "f32").max() <= 1.0
        # correctly rounded f32 of the f64 logarithm, and the f64 one within the fast routine's bar of itself
        assert R.log_err_in_bars(R.ld_log1p(arg64).astype(np.float32), arg64, "f32_of_f64").max() == 0.0
        assert R.log_err_in_bars(R.ld_log1p(arg64).astype(np.float64), arg64, "fast").max() <= 1.0


def test_failure_messages_name_row_length_alignment_and_position():
    fx = R.edges()
    r = fx.pairs[(2049, 1)]
    bad = np.zeros(fx.nnz, bool)
    bad[int(fx.indptr[r]) + 2047] = True
    msg = fx.first_bad_value(bad)
    assert f"row {r} " in msg and "L = 2049" in msg and "a = 1" in msg and "position 2047" in msg and "edge row" in msg
    assert fx.first_bad_value(np.zeros(fx.nnz, bool)) is None and fx.first_bad_row(np.zeros(fx.n_rows, bool)) is None
    got = R.row_variance("edges").astype(np.float64)
    got[r] *= 1 + 1e-9
    msg, units = R.variance_in_bounds(fx, got)
    assert "L = 2049" in msg and units > 1.0
    got = R.row_variance("edges").astype(np.float64)
    got[fx.const_row] = 1e-300
    assert "constant" in R.variance_in_bounds(fx, got)[0]

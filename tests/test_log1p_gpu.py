"""GPU accuracy of the device logarithms against high precision (-m gpu).

The pipeline's f64 logarithms (singlerust_amd/csrc/log1p64.hpp) are checked as the device runs them, through what
`srx_pipeline` leaves in X: at f64 storage `log1p_f64_fast` (row tables + direct route), at f32 storage
`(float)log1p_f64_moment`.  The matrices are built so that every row sum is the same in any summation order, so the host forms
the device's exact argument `fl(v * fl(target / sum))` and compares with `np.log1p` in `np.longdouble` (64-bit mantissa).
The fixed-point moment sums of the pipeline and the standalone `log1p_transform_inplace` (f32 and f64, special values
included) are checked the same way.  tests/test_log1p_table_cpu.py checks the algorithm on the host.
"""
import ctypes as C

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

FAST_REL = 2.7e-16                     # log1p_f64_fast (log1p64.hpp)
MOMENT_ABS, MOMENT_REL = 4e-14, 5e-12  # log1p_f64_moment for x >= 2^-10


def _ld_log1p(x):
    assert np.finfo(np.longdouble).nmant >= 63
    return np.log1p(np.asarray(x, dtype=np.float64).astype(np.longdouble))


def exact_sum_matrix(rng, n_rows, n_cols, f64_only=False, n_planted=4):
    """CSR whose row sums do not depend on the summation order, with every value exact in f32 (unless `f64_only`).

    Row kinds: integers 1..63 (the row-table route); multiples of 1/64 and integers >= 64 (the direct route), all multiples
    of 1/64 below 2^53 / 64 in total; a dominant power of two D plus small values totalling below ulp(D) / 2 (every partial
    sum that holds D rounds back to D), which puts the small values' arguments at D times below the target.  Columns
    0..n_planted-1 carry integer counts in the non-dominant rows: variance for the PCA."""
    rows_idx, rows_val = [], []
    free = np.arange(n_planted, n_cols)
    for r in range(n_rows):
        kind = r % 4
        k = int(rng.integers(60, 150))
        cols = np.sort(rng.choice(free, k, replace=False))
        if kind == 0:
            v = rng.integers(1, 64, k).astype(np.float64)
        elif kind == 1:
            v = rng.integers(1, 64 * 64, k) / 64.0
            v[v == np.floor(v)] += 1.0 / 64
        elif kind == 2:
            v = np.where(rng.random(k) < 0.5, rng.integers(64, 1 << 20, k).astype(np.float64), rng.integers(1, 1 << 12, k) / 64.0)
        else:
            d = int(rng.integers(900, 1015)) if f64_only and r % 8 == 3 else int(rng.integers(68, 120))
            v = np.where(rng.random(k) < 0.5, rng.integers(1, 64, k).astype(np.float64), rng.integers(1, 64, k) / 64.0)
            v[k // 2] = 2.0 ** d                    # sum of the rest < 150 * 63 < 2^15 <= ulp(2^d) / 2
        if kind != 3:
            pc = np.arange(n_planted)
            pv = ((r * (pc + 3)) % 37 + 1).astype(np.float64)
            cols, v = np.concatenate([pc, cols]), np.concatenate([pv, v])
        rows_idx.append(cols)
        rows_val.append(v)
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in rows_idx])]).astype(np.uint64)
    m = oracle.Csr(n_rows, n_cols, indptr, np.concatenate(rows_idx).astype(np.uint64), np.concatenate(rows_val))
    return m


def order_free_row_sums(m):
    """The row sums as the device forms them (any order): exact, or the dominant value."""
    out = np.zeros(m.n_rows)
    for r in range(m.n_rows):
        v = m.values[int(m.indptr[r]):int(m.indptr[r + 1])]
        big = v.max()
        out[r] = big if big >= 2.0 ** 66 else float(np.sum(v.astype(np.longdouble)))
    return out


def device_args(m, target):
    s = order_free_row_sums(m)
    scale = np.where(s == 0.0, 0.0, np.float64(target) / np.where(s == 0.0, 1.0, s))
    rows = np.repeat(np.arange(m.n_rows), np.diff(m.indptr.astype(np.int64)))
    return m.values.astype(np.float64) * scale[rows]


def run_pipeline(ctx, m, target, store, n_hvg, n_pc=2):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    a = sr.IMAnnData.new_basic((m.n_rows, m.n_cols, m.indptr, m.indices, m.values), ctx=ctx, store=store)
    opts = F.PcaOpts(n_pc, 1, 1, -1, 0, 0, 0, 0.0, 1)
    res = F.PipelineResult()
    F.check(F.lib().srx_pipeline(a.x().handle, float(target), int(n_hvg), C.byref(opts), C.byref(res)), ctx.handle)
    return a, res


TARGETS = (1e-3, 1.0, 1e4, 2.0 ** 40)


@pytest.mark.parametrize("store", [2, 1])
def test_pipeline_stored_logarithm_against_longdouble(ctx, store):
    """f64 storage: X holds log1p_f64_fast(arg), <= 2.7e-16 relative (2.5 ulp).  f32 storage: X holds
    (float)log1p_f64_moment(arg), within 1 f32 ulp of the correctly rounded value and correctly rounded but for <= 1e-5."""
    rng = np.random.default_rng(31 + store)
    n_total, n_wrong, seen = 0, 0, []
    for t, target in enumerate(TARGETS):
        m = exact_sum_matrix(rng, 2400, 3000, f64_only=(store == 2 and t == 0))
        x = device_args(m, target)
        a, res = run_pipeline(ctx, m, target, store, n_hvg=8)
        assert int(res.pca.k) == 8
        want = _ld_log1p(x)
        if store == 2:
            got = a.x_values(np.float64)
            nz = want != 0
            rel = np.abs(got.astype(np.longdouble)[nz] - want[nz]) / want[nz]
            assert float(rel.max()) <= FAST_REL, (target, float(rel.max()), float(x[nz][int(np.argmax(rel))]))
            assert np.all(got[~nz] == 0.0)
        else:
            got = a.x_values(np.float32)
            want32 = want.astype(np.float32)
            ulp = np.spacing(np.abs(want32)).astype(np.float64)
            d = np.abs(got.astype(np.float64) - want32.astype(np.float64))
            assert np.all(d <= ulp), (target, float((d / ulp).max()))
            n_wrong += int(np.count_nonzero(got != want32))
        n_total += x.size
        seen.append(x)
    x = np.concatenate(seen)
    # the arguments cover both sides of the moment routine's 2^-10 split and 2^-40 .. 2^40 (and subnormal products at f64)
    assert x.min() < 2.0 ** -40 and x.max() >= 2.0 ** 40 and np.count_nonzero(x < 2.0 ** -10) > 10_000
    if store == 2:
        assert np.count_nonzero((x > 0) & (x < 2.2250738585072014e-308)) > 100
    assert n_total >= 1_000_000
    if store == 1:
        assert n_wrong <= 1e-5 * n_total, n_wrong


@pytest.mark.parametrize("store", [2, 1])
def test_pipeline_fixed_point_moments_against_high_precision(ctx, store):
    """The pipeline's per-gene moments are fixed-point sums of y = ln_1p(arg) (half a quantum per value: 2^-44 for the sums,
    2^-38 for the squares at <= 64 rows, genes.hip local_moments).  They come back as the selection's mean and std
    (srx_result_fetch, every gene selected, center + scale): N mean = sum y, N (std^2 + mean^2) = sum y^2.  Genes with ONE
    non-zero and with a few, arguments on both sides of 2^-10.  srx_gene_moments afterwards sums the STORED values."""
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory import statistics
    n, g = 48, 40
    rng = np.random.default_rng(7 + store)
    dense = np.zeros((n, g))
    dense[:, :4] = rng.integers(1, 64, (n, 4))                   # planted
    dense[:, 4:] = np.where(rng.random((n, g - 4)) < 0.15, rng.integers(1, 64, (n, g - 4)), 0)
    dense[:, 10] = 0
    dense[5, 10] = 37.0                                          # ONE non-zero
    dense[:, 11] = 0
    dense[[1, 9, 30, 47], 11] = [1.0, 2.5, 63.0, 1000.0]         # a few, table and direct routes
    import scipy.sparse as sp
    x = sp.csr_matrix(dense)
    x.sort_indices()
    m = oracle.Csr(n, g, x.indptr, x.indices, x.data)
    for target in (0.05, 1e4):
        args = device_args(m, target)
        y = _ld_log1p(args)
        a, res = run_pipeline(ctx, m, target, store, n_hvg=g)
        k = int(res.pca.k)
        assert k == g
        mean, sd, hv = np.zeros(k), np.zeros(k), np.zeros(k, np.uint64)
        F.check(F.lib().srx_result_fetch(a.x().handle, None, None, None, F.ptr(mean), F.ptr(sd), F.ptr(hv)), ctx.handle)
        col = m.indices.astype(np.int64)
        want_s = np.zeros(g, np.longdouble)
        want_q = np.zeros(g, np.longdouble)
        np.add.at(want_s, col, y)
        np.add.at(want_q, col, y * y)
        cnt = np.bincount(col, minlength=g)
        # the routine's own error per value (f32 storage: the degree-5 one above 2^-10)
        per = np.where(args >= 2.0 ** -10, np.maximum(MOMENT_ABS, MOMENT_REL * y.astype(np.float64)),
                       FAST_REL * y.astype(np.float64)) if store == 1 else FAST_REL * y.astype(np.float64)
        rt = np.zeros(g)
        np.add.at(rt, col, per)
        rq = np.zeros(g)
        np.add.at(rq, col, 2 * per * y.astype(np.float64))
        order = hv.astype(np.int64)
        got_s = n * mean
        got_q = n * (sd * sd + mean * mean)
        ws, wq = want_s[order].astype(np.float64), want_q[order].astype(np.float64)
        eps = 2.0 ** -52
        bound_s = cnt[order] * 0.5 * 2.0 ** -44 + rt[order] + 4 * eps * np.abs(ws)
        bound_q = cnt[order] * 0.5 * 2.0 ** -38 + rq[order] + 8 * eps * np.abs(wq)
        assert np.all(np.abs(got_s - ws) <= bound_s), (target, float(np.max(np.abs(got_s - ws) / bound_s)))
        assert np.all(np.abs(got_q - wq) <= bound_q), (target, float(np.max(np.abs(got_q - wq) / bound_q)))
        for gene in (10, 11):
            j = int(np.nonzero(order == gene)[0][0])
            assert abs(got_s[j] - ws[j]) <= bound_s[j] and ws[j] > 0
        # srx_gene_moments after the pipeline: the moments of what X holds now
        c2, s2, q2 = statistics.gene_moments(a)
        assert np.array_equal(c2, cnt)
        stored_err = FAST_REL if store == 2 else 2.0 ** -23
        ys = y.astype(np.float64)
        bs = np.zeros(g)
        np.add.at(bs, col, np.abs(ys))
        assert np.all(np.abs(s2 - want_s.astype(np.float64)) <= (stored_err + cnt * eps) * bs + 1e-300)
        bq = np.zeros(g)
        np.add.at(bq, col, ys * ys)
        assert np.all(np.abs(q2 - want_q.astype(np.float64)) <= (2 * stored_err + 2 * cnt * eps) * bq + 1e-300)


SPECIAL = np.array([-1.0, -1.5, -np.inf, np.inf, np.nan, 0.0, -0.0, -2.0, -1e30])


def _specials_match(got, want):
    same_nan = np.isnan(got) == np.isnan(want)
    ok = ~np.isnan(want)
    return bool(np.all(same_nan) and np.array_equal(got[ok], want[ok]) and
                np.array_equal(np.signbit(got[ok]), np.signbit(want[ok])))


def _transform(ctx, x):
    import singlerust_amd as sr
    from singlerust_amd.memory import processing
    n = x.size
    a = sr.IMAnnData.new_basic((1, n, [0, n], np.arange(n), x), ctx=ctx)
    processing.log1p_transform_inplace(a)
    return a


def test_log1p_f32_negative_range_and_special_values(ctx):
    """apply_log1p<float> (hardware log2 + Goldberg correction) over (-1, 0], the f32 subnormals and the special values:
    -1 -> -inf, < -1 -> NaN, +-0 -> +-0, +inf -> +inf, -inf -> NaN, NaN -> NaN, exactly as IEEE log1p (Rust f32::ln_1p);
    the 3e-7 relative bound of the positive range wherever the result is finite and non-zero."""
    neg = -np.logspace(-45, np.log10(0.999999), 30001)
    near = np.array([-(2.0 ** -25), -(2.0 ** -25) * (1 + 2.0 ** -20), -(2.0 ** -24), -(2.0 ** -24) * 1.5, -(2.0 ** -23),
                     -0.5, -0.75, -(1 - 2.0 ** -24), -(1 - 2.0 ** -23)])
    sub = np.array([1e-45, 1e-40, 2.0 ** -127, -1e-45, -1e-40, -(2.0 ** -127)])
    pos = np.logspace(-30, 30, 4001)
    x = np.concatenate([neg, near, sub, pos, SPECIAL]).astype(np.float32)
    with np.errstate(all="ignore"):
        a = _transform(ctx, x)
        assert a.x_dtype() == np.float32
        got = a.x_values().astype(np.float64)
        want = np.log1p(x.astype(np.float64))
        want_ieee = np.log1p(x)                                     # f32 IEEE log1p
    fin = np.isfinite(want) & (want != 0)
    rel = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
    assert float(rel.max()) < 3e-7, (float(rel.max()), float(x[fin][int(np.argmax(rel))]))
    spec = ~fin
    assert spec.sum() >= SPECIAL.size
    assert _specials_match(got[spec], want_ieee[spec].astype(np.float64))
    # the oracle (log1pf) agrees on the special positions as well
    m = oracle.Csr(1, x.size, [0, x.size], np.arange(x.size), x)
    with np.errstate(all="ignore"):
        o = oracle.log1p_transform(m).values.astype(np.float64)
    assert _specials_match(got[spec], o[spec])


def test_log1p_f64_within_one_ulp_and_special_values(ctx):
    """F64 log1p_transform_inplace (ocml log1p): <= 1 ulp of the longdouble reference over 2^-1074 .. 1e308 and (-1, 0),
    the special values exactly IEEE's."""
    rng = np.random.default_rng(3)
    pos = np.concatenate([2.0 ** rng.uniform(-1074, 1023, 40000), np.logspace(-300, 308, 4001),
                          [5e-324, 2.2250738585072014e-308, 1e308]])
    neg = np.concatenate([-np.logspace(-320, np.log10(1 - 2.0 ** -52), 20001), -(1 - 2.0 ** -rng.uniform(1, 52, 2000)),
                          [-5e-324, -0.5]])
    x = np.concatenate([pos, neg, SPECIAL]).astype(np.float64)
    with np.errstate(all="ignore"):
        a = _transform(ctx, x)
        got = a.x_values(np.float64)
        want = _ld_log1p(x)
        want64 = np.log1p(x)
    fin = np.isfinite(want64) & (want64 != 0)
    ulp = np.spacing(np.abs(want[fin].astype(np.float64)))
    err = np.abs(got[fin].astype(np.longdouble) - want[fin]).astype(np.float64)
    assert np.all(err <= ulp), float((err / ulp).max())
    spec = ~fin
    assert _specials_match(got[spec], want64[spec])

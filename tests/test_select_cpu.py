"""The restatement of the device feature selection (tests/select_ref.py) and the cases of tests/test_select_gpu.py, without a
device: the order against a brute-force sort with the comparator, kq away from an integer at every (G, take) the GPU tests use,
every named value pattern on the route its GPU test claims, the trace's tree against the longdouble sum, and srx_select_op bound
and failing loudly without a device."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import select_ref as ref
from select_ref import CANDIDATES, FALLBACK, FULL, NONE, UNUSED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_order_against_brute_force():
    """A few hundred small arrays with heavy ties, signed zeros included: order_of, true_rank and the selection's mask."""
    rng = ref.rng_of(40)
    for trial in range(300):
        G = int(rng.integers(1, 90))
        var = rng.integers(0, max(2, G // 3), G).astype(np.float64)
        var[rng.random(G) < 0.2] = -0.0
        want = ref.brute_order(var)
        assert np.array_equal(ref.order_of(var), want)
        r = ref.true_rank(var)
        assert np.array_equal(r[want], np.arange(G))
        n = int(rng.integers(1, G + 3))
        sel, bits, prefix = ref.selection(var, n)
        k = min(n, G)
        assert np.array_equal(sel, want[:k])
        assert np.array_equal(ref.genes_of_bits(bits), np.sort(want[:k]))
        assert prefix[0] == 0 and np.array_equal(np.diff(prefix), ref.popcount32(bits)[:-1])
        assert int(prefix[-1]) + int(ref.popcount32(bits)[-1]) == k


def test_variance_plants_exactly():
    v = np.array([0.0, -0.0, 1.5, 1e-300, 1e300, np.nan, np.inf])
    got = ref.variance(*ref.plant(v))
    assert np.array_equal(got.view(np.uint64), v.view(np.uint64))
    assert ref.variance([0, 2], [5.0, 3.0], [9.0, 5.0]).tolist() == [0.0, 5.0 / 2.0 - 1.5 * 1.5]
    # the count is read as (double)(uint32_t)cnt
    assert ref.variance([2 ** 32 + 2], [3.0], [5.0])[0] == 5.0 / 2.0 - 1.5 * 1.5


def gpu_shapes():
    """Every (G, take) of test_select_gpu.py that reaches k_hvg_candidates' quantile."""
    out = {(G, min(n, G)) for G in ref.SHAPE_G for n in ref.takes_of(G)}
    out |= {(len(v), min(n, len(v))) for _, v, n, _ in ref.pattern_cases()}
    out |= {(len(v), n) for _, v, n in ref.nan_cases()}
    out |= {(300, 151), (700, 151), (3000, 2500), (600, 50)}
    return sorted(x for x in out if x[0] >= ref.SAMPLE)


def test_kq_is_never_next_to_an_integer():
    """The device truncates kq = (q + 4 sqrt(q (1 - q) / S)) S + 1 to an index: at 1e-6 from an integer a last-bit difference of
    its sqrt could choose another sample element than the restatement."""
    for G, take in gpu_shapes():
        kq = ref.kq_of(G, take)
        # the comparison kq < S - 1 is not on its edge; beyond it kq is not truncated (take = G gives 513 exactly)
        assert abs(kq - (ref.SAMPLE - 1)) >= 1e-6, (G, take, kq)
        if kq < ref.SAMPLE - 1:
            assert abs(kq - round(kq)) >= 1e-6, (G, take, kq)


def test_shapes_cover_the_edges():
    assert all(min(n, G) <= ref.MAX_K and G <= ref.MAX_G for G in ref.SHAPE_G for n in ref.takes_of(G))
    assert {512, 513, 2048, 8192, 65536} <= set(ref.SHAPE_G)
    assert 8192 in ref.takes_of(65536) and {1024, 1025} <= set(ref.takes_of(8192))
    assert ref.cap_of(65536, 1024) == 4096 and ref.cap_of(65536, 1025) == 4100          # cap switches to 4 take
    # the distinct shapes reach the candidate route, and "every gene a candidate" (kq >= S - 1) at take next to G
    kinds = {(G, n): ref.predict(ref.distinct(G), n, 0) for G in ref.SHAPE_G for n in ref.takes_of(G)}
    assert all(k[0] == FULL and k[1] == UNUSED for (G, n), k in kinds.items() if G < ref.SAMPLE)
    assert all(k[0] == CANDIDATES for (G, n), k in kinds.items() if G >= ref.SAMPLE), [x for x, k in kinds.items() if k[0] == FALLBACK]
    assert kinds[(513, 512)][1] == 513 and kinds[(512, 512)][1] == 512 and kinds[(8192, 8192)][1] == 8192
    assert all(ref.predict(ref.distinct(G), 5, 2)[:2] == ((FALLBACK, NONE) if G >= ref.SAMPLE else (FULL, UNUSED)) for G in ref.SHAPE_G)


def test_patterns_take_the_routes_they_name():
    seen = set()
    for name, var, n, kind in ref.pattern_cases():
        G, take = len(var), min(n, len(var))
        got, counter, thr = ref.predict(var, n, 0)
        seen.add(got)
        assert got == kind, (name, got, kind, counter)
        M = ref.threshold(var, take)[1]
        if name.startswith("zeros") and G >= ref.SAMPLE:
            # 0 is the threshold (M counts every zero of either sign) or lies below it: the cut is ranked among candidates
            assert counter == {"zeros_700_151": 189, "zeros_700_400": 700, "zeros_4097_2000": 4097}[name]
        if name.startswith("too_few"):
            assert M < take
        if name.startswith("too_many"):
            assert M > ref.cap_of(G, take)
        if name == "too_many_zero_20000":
            assert thr == 0.0
        if name.startswith("every_gene"):
            assert thr == -np.inf and M == G == ref.cap_of(G, take) and ref.kq_of(G, take) >= ref.SAMPLE - 1
        if name.startswith("tie_group"):
            size = int(name.split("_")[1][5:])
            cut = np.sort(var)[::-1][take - 1]
            assert cut == 500.0 and np.count_nonzero(var == 500.0) == size       # the cut falls inside the tie group
            assert np.count_nonzero(var >= 500.0) > take or name.startswith("tie_group300_last")
        if name.startswith("twice"):
            vals, counts = np.unique(var, return_counts=True)
            assert np.count_nonzero(counts == 2) >= len(var) // 2 - 1
    assert seen == {FULL, CANDIDATES, FALLBACK}
    by = {name: var for name, var, _, _ in ref.pattern_cases()}
    v = by["twice_adjacent1_4608"]
    assert v[255] == v[256] and v[2047] == v[2048] and v[2048] != v[2049]            # partners across a block and a tile edge
    v = by["twice_half_4100"]
    assert v[0] == v[2050] and v[2049] == v[4099]                                      # partners in different tiles
    z = by["zeros_700_400"]
    assert np.count_nonzero(z == 0) > 300 and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    assert np.count_nonzero(z > 0) < 400                                               # the cut falls among the zeros


def test_nan_cases_are_where_they_claim():
    pos = set(ref.sample_positions(5120).tolist())
    for name, var, n in ref.nan_cases():
        at = np.flatnonzero(np.isnan(var))
        if name == "sampled":
            assert len(at) == 1 and at[0] in pos
        if name == "unsampled":
            assert len(at) == 1 and at[0] not in pos
        if name == "many":
            assert len(at) == 600
        if name == "last":
            assert list(at) == [len(var) - 1]


def test_trace_tree_against_longdouble():
    rng = ref.rng_of(41)
    for G, k in ((1, 1), (700, 151), (5000, 4000), (65536, 8192)):
        cnt, s, q = ref.realistic_moments(max(G, 8), 40, 2)
        cnt, s, q = cnt[:G], s[:G], q[:G]
        genes = rng.permutation(G)[:k]
        for center in (0, 1):
            for scale in (0, 1):
                _, _, _, terms = ref.vectors(genes, s, q, 40, center, scale, G)
                assert np.all(terms >= 0)
                dist = abs(np.longdouble(ref.trace_tree(terms)) - ref.trace_ld(terms))
                assert dist <= ref.trace_bound(terms, k), (G, k, center, scale, float(dist))
    # the tree's order: 1024 partial sums of stride 1024, then halving
    t = np.zeros(3000)
    t[[0, 1024, 2048, 512]] = [1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -52]
    assert ref.trace_tree(t) == (1.0 + 2.0 ** -53 + 2.0 ** -53) + 2.0 ** -52 == 1.0 + 2.0 ** -52


def test_special_columns_of_the_realistic_moments():
    n = 40
    assert ref.negative_variance_constant(n) is not None
    cnt, s, q = ref.realistic_moments(700, n, 1)
    assert cnt[5] == 0 and s[5] == 0 and cnt.max() <= n
    mean = s[7] / n
    assert q[7] / n - mean * mean < 0
    mu, sd, di, terms = ref.vectors([3, 5, 7], s, q, n, 1, 1, 700)
    assert sd[1] == 0 and di[1] == 1 and sd[2] == 0 and di[2] == 1 and mu[0] == 2.5


def test_select_op_is_bound_and_fails_loudly_without_a_device():
    """Exported and bound (test_abi_cpu.py holds the block's layout to the header), null arguments refused with nothing written; with no device visible
    there is no context to call it on and nothing is computed on the host."""
    from singlerust_amd import _ffi
    lib = _ffi.lib()
    assert "srx_select_op" in _ffi.EXPORTS
    a = _ffi.SelectArgs()
    a.trace, a.counter, a.status, a.tail_touched = -7.0, 7, 7, 7
    assert lib.srx_select_op(None, C.byref(a)) == _ffi.E_ARG and lib.srx_last_error(None)
    assert (a.trace, a.counter, a.status, a.tail_touched) == (-7.0, 7, 7, 7)
    assert _ffi.SEL_COUNTER_UNUSED == UNUSED and (_ffi.SEL_HVG, _ffi.SEL_LIST, _ffi.SEL_NO_VECTORS) == (0, 1, 1)
    code = ("import ctypes as C, singlerust_amd as sr\n"
            "from singlerust_amd import _ffi\n"
            "try:\n"
            "    ctx = sr.Context(0)\n"
            "    a = _ffi.SelectArgs()\n"
            "    _ffi.check(_ffi.lib().srx_select_op(ctx.handle, C.byref(a)), ctx.handle)\n"
            "except sr.SrxError as e:\n"
            "    print('refused', e.code, e)\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("refused %d " % _ffi.E_HIP) and "no CPU fallback" in r.stdout, (r.stdout, r.stderr)


def test_rust_i32_constants_fit_an_i32():
    """The Rust module renders the header's constants as i32, and rustc refuses a literal out of that range: the whole
    `extern "C"` module would stop compiling.  No rustc here, so the range is held on the committed text."""
    import re
    text = open(os.path.join(ROOT, "rust", "srx_sys.rs")).read()
    consts = re.findall(r"pub const (\w+): i32 = (-?\d+);", text)
    assert len(consts) > 20 and "SRX_SEL_COUNTER_UNUSED" in dict(consts)
    assert all(-2 ** 31 <= int(v) < 2 ** 31 for _, v in consts), [k for k, v in consts if not -2 ** 31 <= int(v) < 2 ** 31]
    assert ref.MAX_G < UNUSED < NONE                    # no candidate count reaches the mark, and it is not the fallback's

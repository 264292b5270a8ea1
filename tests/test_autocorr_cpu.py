"""Moran's I and Geary's C without a GPU: the two statements of the definition in tests/autocorr_ref.py against each other (exact,
in fractions), the hand-checkable known answer, the library's host arithmetic (srx_autocorr_from_tables) against the fractions
within the header's bound, constant genes, both variance formulas against seeded normal draws, the scale rule at its
extremes, the symbols in every layer and the gfx950 listings of autocorr.hip free of spills and scratch."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import autocorr_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srx_autocorr", "srx_autocorr_csr", "srx_autocorr_from_tables", "srx_autocorr_scales")
KERNELS = ("k_ac_wmax", "k_ac_degrees", "k_ac_s2", "k_ac_moments", "k_ac_walk")


def lattice(rng, n, g, density=0.5, hi=5):
    """Small integer counts, zeros not stored."""
    X = np.where(rng.random((n, g)) < density, rng.integers(1, hi, (n, g)), 0).astype(np.float64)
    return sp.csr_matrix(X)


def frac(s):
    return None if s is None else Fraction(s)


def from_tables(t):
    from singlerust_amd.memory.processing import autocorr_from_tables
    return autocorr_from_tables(t, t["info"])


def assert_within_bounds(got, t):
    """The library's statistics from the tables `t` lie within the header's bounds of the fractions; NaN exactly where the
    reference has a constant gene."""
    st = ref.stats(t)
    bd = ref.bounds(t, st)
    for g, (s, b) in enumerate(zip(st, bd)):
        if s[0] is None:
            assert all(math.isnan(got[k][g]) for k in ("morans_i", "gearys_c", "z_i", "z_c")), g
            continue
        for key, want, tol in (("morans_i", s[0], b[0]), ("gearys_c", s[1], b[1]), ("z_i", s[2], b[2]), ("z_c", s[3], b[3])):
            if want is None:                                  # a z whose Var is not > 0
                assert math.isnan(got[key][g]), (key, g)
                continue
            assert abs(Fraction(float(got[key][g])) - Fraction(want)) <= Fraction(tol), (key, g, got[key][g], float(want), tol)
    assert got["info"]["genes_constant"] == sum(1 for s in st if s[0] is None)
    return st


def assert_graph_moments(info, t):
    """E and Var of both statistics as the library rounds them: relative 2^-50 of the largest term of each formula."""
    s0, s1, s2, e_i, var_i, e_c, var_c = ref.moments_of_graph(t["info"])
    N = Fraction(t["info"]["n"])
    assert info["w"] == float(s0) and info["s1"] == float(s1) and info["s2"] == float(s2)
    assert info["e_i"] == float(e_i) and info["e_c"] == 1.0
    big_i = (N * N * s1 + N * s2 + 3 * s0 * s0) / ((N * N - 1) * s0 * s0) + e_i * e_i
    big_c = ((2 * s1 + s2) * (N - 1) + 4 * s0 * s0) / (2 * (N + 1) * s0 * s0)
    assert abs(Fraction(info["var_i"]) - var_i) <= big_i / 2 ** 50
    assert abs(Fraction(info["var_c"]) - var_c) <= big_c / 2 ** 50


# ---- the definition, twice ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_tables_and_literal_sums_agree_exactly_on_integer_lattices(seed):
    """Integer counts with dyadic weights: the tables are exact, so the statistics from them ARE the textbook double sums."""
    rng = np.random.default_rng(seed)
    n, g = int(rng.integers(4, 14)), 5
    X = lattice(rng, n, g)
    W = ref.random_graph(rng, n, int(rng.integers(1, 4)))
    t = ref.tables(X, W)
    assert min(v for k, v in t["info"].items() if k.startswith("s_")) >= 0
    lit = ref.literal_fraction(X.toarray().tolist(), W.toarray().tolist())
    for s, (i, c) in zip(ref.stats(t), lit):
        assert s[0] == i and s[1] == c
    got = from_tables(t)                                                         # ... and the library's host arithmetic on them
    assert_within_bounds(got, t)
    assert_graph_moments(got["info"], t)


def test_known_answer():
    """tests/golden/kat_autocorr.json: the file is what its maker writes, the tables give its fractions exactly, the library's
    host arithmetic gives them within the header's bound, and z squared is the exact rational."""
    path = os.path.join(ROOT, "tests", "golden", "kat_autocorr.json")
    kat = json.load(open(path))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_autocorr_golden
    finally:
        sys.path.pop(0)
    assert open(path).read() == make_autocorr_golden.text()                       # compared in memory: nothing is written
    n = kat["n"]
    r = [e[0] for e in kat["edges_eighths"]] + [e[1] for e in kat["edges_eighths"]]
    c = [e[1] for e in kat["edges_eighths"]] + [e[0] for e in kat["edges_eighths"]]
    w = [e[2] / 8.0 for e in kat["edges_eighths"]] * 2
    W = sp.csr_matrix((w, (r, c)), shape=(n, n))
    X = sp.csr_matrix(np.array(kat["genes"], np.float64).T)
    t = ref.tables(X, W)
    s0, s1, s2, e_i, var_i, _, var_c = ref.moments_of_graph(t["info"])
    assert (s0, s1, s2, e_i, var_i, var_c) == tuple(frac(kat[k]) for k in ("s0", "s1", "s2", "e_i", "var_i", "var_c"))
    assert frac(kat["morans_i"][0]) == Fraction(-1, 7) and frac(kat["gearys_c"][0]) == Fraction(20, 21)       # the docstring's hand check
    st = ref.stats(t)
    assert [s[0] for s in st] == [frac(v) for v in kat["morans_i"]] and [s[1] for s in st] == [frac(v) for v in kat["gearys_c"]]
    got = from_tables(t)
    assert_within_bounds(got, t)
    assert got["info"]["genes_constant"] == kat["genes_constant"] == 1
    for key, zs in (("z_i", kat["z_i_squared_and_sign"]), ("z_c", kat["z_c_squared_and_sign"])):
        for g, z in enumerate(zs):
            if z is None:
                assert math.isnan(got[key][g])
            else:
                assert math.isclose(got[key][g] ** 2, float(Fraction(z[0])), rel_tol=2.0 ** -48) and math.copysign(1, got[key][g]) == z[1]


@pytest.mark.parametrize("seed", range(4))
def test_host_arithmetic_within_the_headers_bound(seed):
    """Log-normalised-like values with UMAP-like weights, and a gene whose I is nearly 0 by construction of the seed sweep."""
    rng = np.random.default_rng(100 + seed)
    n, g = 60, 12
    X = lattice(rng, n, g, 0.4, 40)
    X.data = np.log1p(X.data * rng.uniform(0.5, 3.0, X.nnz))
    W = ref.random_graph(rng, n, 4, dyadic=False)
    t = ref.tables(X, W)
    got = from_tables(t)
    assert_within_bounds(got, t)
    assert_graph_moments(got["info"], t)
    for key, sc in (("sum", "s_sum"), ("sumsq", "s_sumsq"), ("dsum", "s_dsum"), ("dsumsq", "s_dsumsq"), ("cross", "s_cross")):
        assert got[key].tolist() == [math.ldexp(float(v), -t["info"][sc]) for v in t[key + "_int"]]


def test_extreme_tables_decide_constant_genes_in_integers():
    """den = Q - S^2 / N at the edge: the decision is exact however large the tables are."""
    info = dict(ref.scales(1.0, 1.0, 1.0, 4, 4), n=4, w_int=1 << 58, s1_int=1 << 50, s2_int=1 << 50)
    S = 1 << 61                                   # S = 2^61 2^-s_sum;  S^2 / N = 2^122 / 4 in units of 2^-2 s_sum
    sh = 2 * info["s_sum"] - info["s_sumsq"]
    q_eq = (S * S) >> sh                          # N Q 2^sh == S^2 exactly when Q = q_eq / N
    assert (q_eq << sh) == S * S and q_eq % 4 == 0
    t = {"sum_int": [S, S, S, 0, -S], "sumsq_int": [q_eq // 4, q_eq // 4 + 1, q_eq // 4 - 1, 0, q_eq // 4 + 1],
         "dsum_int": [1, 2, 3, 0, 5], "dsumsq_int": [1 << 40] * 5, "cross_int": [1 << 30, -(1 << 30), 7, 0, 9], "info": info}
    got = from_tables(t)
    assert [math.isnan(v) for v in got["morans_i"]] == [True, False, True, True, False]
    assert got["info"]["genes_constant"] == 3
    assert_within_bounds(got, t)


def test_constant_and_all_zero_genes_are_nan_and_counted():
    rng = np.random.default_rng(5)
    n = 20
    X = lattice(rng, n, 4).toarray()
    X[:, 1] = 3.0                                # constant, every entry stored
    X[:, 2] = 0.0                                # all zero: nothing stored
    X = sp.csr_matrix(X)
    Xz = X.tolil()
    Xz[:, 3] = 0.0
    Xz = sp.csr_matrix(Xz)
    Xz = sp.csr_matrix((np.concatenate([Xz.data, [0.0, -0.0]]), (np.concatenate([Xz.nonzero()[0], [0, 5]]),
                                                                   np.concatenate([Xz.nonzero()[1], [3, 3]]))), shape=X.shape)
    assert Xz.nnz == X.nnz - np.count_nonzero(X.toarray()[:, 3]) + 2               # gene 3: two stored zeros, one of them -0.0
    W = ref.random_graph(rng, n, 3)
    for M in (X, Xz):
        t = ref.tables(M, W)
        got = from_tables(t)
        st = assert_within_bounds(got, t)
        assert st[1][0] is None and st[2][0] is None and math.isnan(got["morans_i"][1]) and math.isnan(got["z_c"][2])
    assert got["info"]["genes_constant"] == 3 and math.isnan(got["gearys_c"][3])


def test_from_tables_refusals():
    from singlerust_amd import _ffi as F
    rng = np.random.default_rng(6)
    t = ref.tables(lattice(rng, 8, 3), ref.random_graph(rng, 8, 2))
    for change, word in (({"n": 1}, b"N = 1"), ({"n": 2 ** 32 - 1}, b"N ="), ({"w_int": 0}, b"W = 0"), ({"s_sumsq": t["info"]["s_sumsq"] - 40}, b"s_sumsq"),
                         ({"s_sumsq": 2 * t["info"]["s_sum"] + 1}, b"s_sumsq")):
        bad = dict(t, info=dict(t["info"], **change))
        with pytest.raises(F.SrxError) as e:
            from_tables(bad)
        assert e.value.code == F.E_ARG and word in F.lib().srx_last_error(None), change
    info = F.AutocorrInfo()
    z = np.zeros(3, np.int64)
    assert F.lib().srx_autocorr_from_tables(F.ptr(z), F.ptr(z), None, F.ptr(z), F.ptr(z), 3, C.byref(info), None) == F.E_ARG
    assert F.lib().srx_autocorr_from_tables(F.ptr(z), F.ptr(z), F.ptr(z), F.ptr(z), F.ptr(z), 3, None, None) == F.E_ARG


# ---- the variance formulas -----------------------------------------------------------------------------------------------------------
def test_variance_formulas_against_normal_draws():
    """E and Var of I and C under normality against 200 000 seeded draws of iid normal values on a 40-vertex graph.  The
    tolerance is 5 standard errors: of the sample mean, s / sqrt(n), and of the sample variance, sqrt((m4 - s^4) / n) with the
    sample's own fourth central moment m4 (the statistics are not normal themselves, so 2 s^4 / n would not do)."""
    rng = np.random.default_rng(2024)
    n, draws = 40, 200_000
    W = ref.random_graph(rng, n, 3, dyadic=False)
    t = ref.tables(sp.csr_matrix(np.ones((n, 1))), W)
    info = from_tables(t)["info"]                                                # the library's E and Var are what is checked
    assert_graph_moments(info, t)
    e_i, var_i, e_c, var_c = info["e_i"], info["var_i"], info["e_c"], info["var_c"]
    Wd = W.toarray()
    s0 = Wd.sum()
    X = rng.standard_normal((draws, n))
    Z = X - X.mean(axis=1, keepdims=True)
    den = (Z * Z).sum(axis=1)
    I = n / s0 * (Z * (Z @ Wd)).sum(axis=1) / den
    d = Wd.sum(axis=1)
    Cc = (n - 1) * (2 * (X * X) @ d - 2 * (X * (X @ Wd)).sum(axis=1)) / (2 * s0 * den)
    for name, sample, e, var in (("I", I, e_i, var_i), ("C", Cc, e_c, var_c)):
        m, s2 = sample.mean(), sample.var(ddof=1)
        m4 = ((sample - m) ** 4).mean()
        print("%s: mean %.6f against %.6f, variance %.6f against %.6f (standard errors %.2e, %.2e)"
              % (name, m, e, s2, var, math.sqrt(s2 / draws), math.sqrt((m4 - s2 * s2) / draws)))
        assert abs(m - e) <= 5 * math.sqrt(s2 / draws), name
        assert abs(s2 - var) <= 5 * math.sqrt((m4 - s2 * s2) / draws), name


# ---- the scale rule -------------------------------------------------------------------------------------------------------------------
def test_scale_rule_never_passes_2_to_62():
    """Every table at the extremes the rule admits, all terms at their largest: |x| just below 2^e_x in every cell, every weight
    the largest, every degree the largest, N up to 2^32 - 2, nnz up to N (N - 1) capped at 2^40."""
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import autocorr_scales
    below = lambda e: math.ldexp(1.0 - 2.0 ** -53, e)                      # the largest double below 2^e
    for ex in (-40, -30, -1, 0, 1, 7, 100):
        for ew in (-35, -30, 0, 3):
            for N in (2, 3, 4, 5, 1000, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 2):
                for nnz in {2, 3, min(N * (N - 1), 2 ** 40), min(N * 15, N * (N - 1))}:
                    x, w = below(ex), below(ew)
                    row = min(nnz, N - 1)                                  # the longest row
                    s_w = 62 - ref.fx_exponent(w) - ref.ceil_log2(nnz)
                    dq = row * round(math.ldexp(w, s_w))
                    d = math.ldexp(float(dq), -s_w)
                    sc = ref.scales(x, w, d, N, nnz)
                    assert sc["s_w"] == s_w and autocorr_scales(N, nnz, x, w, d) == sc          # the library's rule is the reference's
                    worst = {"S": N * round(math.ldexp(x, sc["s_sum"])), "Q": N * round(math.ldexp(x * x, sc["s_sumsq"])),
                             "A": N * round(math.ldexp(d * x, sc["s_dsum"])), "B": N * round(math.ldexp(d * (x * x), sc["s_dsumsq"])),
                             "P": (nnz // 2) * round(math.ldexp(w * (x * x), sc["s_cross"])), "W": nnz * round(math.ldexp(w, s_w)),
                             "S1": nnz * round(math.ldexp(w * w, sc["s_1"])), "S2": N * round(math.ldexp(d * d, sc["s_2"]))}
                    for k, v in worst.items():
                        assert 0 <= v <= 2 ** 62, (k, ex, ew, N, nnz)
    # ... and the rule is not slack by more than the rounding up of e and L: values of exactly 2^(e - 1) with N a power of two
    sc = ref.scales(0.5, 0.5, 0.5, 1024, 4096)
    assert 1024 * round(math.ldexp(0.5, sc["s_sum"])) == 2 ** 61 and autocorr_scales(1024, 4096, 0.5, 0.5, 0.5) == sc
    # the admitted range ends below 2^255: at its edge every product of the definition is finite and every 2^scale normal
    top = below(255)
    sc = autocorr_scales(2 ** 32 - 2, 2 ** 40, top, top, top)
    assert sc == ref.scales(top, top, top, 2 ** 32 - 2, 2 ** 40) and min(sc.values()) > -1022 and math.isfinite(top * (top * top))
    for bad in ((2.0 ** 255, 1.0, 1.0), (1.0, 2.0 ** 255, 1.0), (1.0, 1.0, 2.0 ** 255), (float("nan"), 1.0, 1.0), (-1.0, 1.0, 1.0),
                (1.0, float("inf"), 1.0)):
        with pytest.raises(F.SrxError) as e:
            autocorr_scales(100, 300, *bad)
        assert e.value.code == F.E_ARG and b"2^255" in F.lib().srx_last_error(None), bad
    for n, nnz in ((1, 4), (2 ** 32 - 1, 4), (10, 0)):
        with pytest.raises(F.SrxError):
            autocorr_scales(n, nnz, 1.0, 1.0, 1.0)


# ---- every layer ----------------------------------------------------------------------------------------------------------------------
def test_autocorr_symbols_are_exported_and_bound():
    from singlerust_amd import _ffi, build
    from singlerust_amd.memory import processing
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "srx.h")).read()
    rust = open(os.path.join(ROOT, "rust", "srx_sys.rs")).read()
    shim = open(os.path.join(ROOT, "rust", "shim.rs")).read()
    mirror = open(os.path.join(ROOT, "singlerust_amd", "host", "single_rust.hpp")).read()
    assert "autocorr.hip" in build.SOURCES
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _ffi.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, rust), name
        assert re.search(r"\b%s\s*\(" % name, mirror), name
        assert re.search(r"\b%s\s*\(" % name, shim), name
    for s in ("SrxAutocorrOpts", "SrxAutocorrOut", "SrxAutocorrInfo"):
        assert "pub struct %s" % s in rust, s
    for fn in ("morans_i", "gearys_c", "gene_autocorr", "autocorr_csr", "autocorr_from_tables", "autocorr_scales"):
        assert callable(getattr(processing, fn)), fn
    assert re.search(r"#define\s+SRX_ABI_VERSION\s+6\b", header) and lib.srx_abi_version() == 6        # the calls are additive
    assert C.sizeof(_ffi.AutocorrOpts) == 8 and C.sizeof(_ffi.AutocorrOut) == 14 * 8 and C.sizeof(_ffi.AutocorrInfo) == 240
    for script in ("gen_rust_bindings.py", "gen_ctypes_bindings.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--check"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    for doc, mark in (("INTEGRATION.md", "2s"), ("DESIGN.md", "3v"), ("README.md", "NOT compared: scanpy, squidpy, esda (not installed)")):
        assert mark in open(os.path.join(ROOT, doc)).read(), doc


def test_autocorr_kernels_do_not_spill_registers(tmp_path):
    """The gfx950 code-object metadata of every kernel of autocorr.hip shows no VGPR / SGPR spill and no scratch; the constants
    the reference file states are the source's."""
    from singlerust_amd import build
    out = str(tmp_path / "autocorr.s")
    subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "singlerust_amd", "csrc", "autocorr.hip")], stderr=subprocess.DEVNULL)
    meta = open(out).read()
    seen = set()
    for m in re.finditer(r"\.name:\s+(\S*k_ac_\S*)\n(.*?)\.wavefront_size", meta, flags=re.S):
        body = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        assert spill == 0 and sspill == 0 and scratch == 0, f"{m.group(1)}: {spill} / {sspill} spilled V/SGPRs, {scratch} B of scratch"
        seen |= {k for k in KERNELS if re.search(r"\d%s(I|E|\b)" % k, m.group(1))}
    assert seen == set(KERNELS), set(KERNELS) - seen
    src = open(os.path.join(ROOT, "singlerust_amd", "csrc", "autocorr.hip")).read()
    assert int(re.search(r"constexpr int kAcThreads = (\d+);", src).group(1)) == ref.WAVES * 64
    genes = open(os.path.join(ROOT, "singlerust_amd", "csrc", "genes.hip")).read()
    assert int(re.search(r"constexpr int kMaxTileGenes = (\d+);", genes).group(1)) == ref.TILE_GENES

"""The shared-nearest-neighbour graph without a GPU: the two restatements of tests/snn_ref.py against the hand-worked known
answer and against each other, srx_snn_min_shared (host code) against the fractions restatement at every k, the symbols in
every layer, and the gfx950 listings: snn.hip's kernels free of spills, graph.hip's kernels unchanged in what they need."""
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

import snn_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srx_snn_from_knn", "srx_snn_graph", "srx_snn_min_shared")
KERNELS = ("k_snn_rows", "k_snn_cand", "k_snn_hash", "k_snn_window")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def csr_of_sets(got, n):
    rows = [[] for _ in range(n)]
    for (i, j), (_, _, v) in sorted(got.items()):
        rows[i].append((j, v))
    indptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    indices = np.array([j for r in rows for j, _ in r], dtype=np.uint32)
    data = np.array([v for r in rows for _, v in r], dtype=np.float64)
    return indptr, indices, data


def test_snn_symbols_are_exported_and_bound():
    from singlerust_amd import _ffi, build
    from singlerust_amd.memory import processing
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "srx.h")).read()
    rust = open(os.path.join(ROOT, "rust", "srx_sys.rs")).read()
    shim = open(os.path.join(ROOT, "rust", "shim.rs")).read()
    mirror = open(os.path.join(ROOT, "singlerust_amd", "host", "single_rust.hpp")).read()
    assert "snn.hip" in build.SOURCES
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _ffi.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, rust), name
        assert re.search(r"\b%s\s*\(" % name, mirror), name
        assert re.search(r"\b%s\s*\(" % name, shim), name
    assert "pub struct SrxSnnOpts" in rust and "pub struct SrxSnnInfo" in rust
    for fn in ("snn_graph", "neighbors_snn", "snn_min_shared"):
        assert callable(getattr(processing, fn)), fn
    assert re.search(r"#define\s+SRX_ABI_VERSION\s+6\b", header) and lib.srx_abi_version() == 6
    assert C.sizeof(_ffi.SnnOpts) == 24
    assert (_ffi.SNN_JACCARD, _ffi.SNN_NUMBER, _ffi.SNN_PAIRS_SHARED, _ffi.SNN_PAIRS_KNN) == (0, 1, 0, 1)
    fields = [f for f, _ in _ffi.SnnInfo._fields_]
    for f in ("n", "k", "set_size", "min_shared", "max_shared", "pairs_considered", "pairs_kept", "nnz", "max_row_nnz",
              "max_in_degree", "max_candidates", "short_capacity", "rows_long", "rows_empty"):
        assert f in fields, f
    for script in ("gen_rust_bindings.py", "gen_ctypes_bindings.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--check"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    assert "NOT been compared" in header[header.index("shared-nearest-neighbour"):header.index("srx_snn_opts")]


def test_snn_known_answer():
    """tests/golden/snn_kat.json is what its maker writes, holds the entries worked by hand in the maker's docstring, and the
    scipy restatement gives the same CSR as the set restatement in all four cases."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_snn_golden
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "snn_kat.json")))
    assert kat == json.loads(json.dumps(make_snn_golden.make()))
    idx = np.array(kat["indices"], dtype=np.uint32)
    by_case = {(c["include_self"], c["pairs"]): c for c in kat["cases"]}
    hand = {(1, ref.SHARED): {(0, 1): (3, "1"), (2, 5): (1, "1/5"), (0, 5): (1, "1/5"), (3, 5): (2, "1/2")},
            (1, ref.KNN): {(0, 1): (3, "1"), (2, 5): (1, "1/5"), (0, 5): None, (1, 5): None},
            (0, ref.SHARED): {(0, 1): (1, "1/3"), (3, 5): None, (2, 5): None, (0, 5): (1, "1/3")},
            (0, ref.KNN): {(0, 1): (1, "1/3"), (0, 5): None, (4, 5): (1, "1/3")}}
    for key, case in by_case.items():
        entries = {(i, j): (s, J) for i, j, s, J in case["entries"]}
        for (i, j), want in hand[key].items():
            assert entries.get((i, j)) == want and entries.get((j, i)) == want, (key, i, j)
        K = 2 + key[0]
        for (i, j), (s, J) in entries.items():
            assert Fraction(J) == Fraction(s, 2 * K - s)
        got, considered = ref.by_sets(idx, bool(key[0]), key[1], 0.0)
        assert considered == case["pairs_considered"] == len(entries) // 2
        ptr, ind, dat, info = ref.by_scipy(idx, bool(key[0]), key[1], 0.0)
        sptr, sind, sdat = csr_of_sets(got, 6)
        assert np.array_equal(ptr, sptr) and np.array_equal(ind, sind) and np.array_equal(bits(dat), bits(sdat))
        assert info["pairs_considered"] == considered and info["nnz"] == len(entries)


@pytest.mark.parametrize("n,k", [(3, 1), (4, 2), (9, 3), (40, 5), (60, 15)])
def test_snn_restatements_agree_on_random_lists(n, k):
    rng = np.random.default_rng(100 * n + k)
    idx = ref.random_list(rng, n, k)
    for include_self in (True, False):
        K = k + include_self
        for pairs in (ref.SHARED, ref.KNN):
            for weight in (ref.JACCARD, ref.NUMBER):
                for prune in (0.0, 1.0 / 15.0, ref.jaccard_f64(2, K) if K >= 2 else 0.5, 0.5, 1.0):
                    got, considered = ref.by_sets(idx, include_self, pairs, prune, weight)
                    ptr, ind, dat, info = ref.by_scipy(idx, include_self, pairs, prune, weight)
                    sptr, sind, sdat = csr_of_sets(got, n)
                    assert np.array_equal(ptr, sptr) and np.array_equal(ind, sind)
                    assert np.array_equal(bits(dat), bits(sdat))
                    assert info["pairs_considered"] == considered and info["pairs_kept"] * 2 == info["nnz"] == len(got)
                    if got:
                        assert min(s for s, _, _ in got.values()) >= info["min_shared"]


def lib_min_shared(k, include_self, prune):
    from singlerust_amd.memory.processing import snn_min_shared
    return snn_min_shared(k, include_self, prune)


@pytest.mark.parametrize("include_self", [True, False])
def test_snn_min_shared_matches_fractions_at_every_k(include_self):
    """Every k in 1..64; prune in {0, 1/15, 0.5, 1} and at, just above and just below every attainable s / (2K - s)."""
    for k in range(1, 65):
        K = k + include_self
        prunes = [0.0, 1.0 / 15.0, 0.5, 1.0]
        for s in range(1, K + 1):
            J = float(Fraction(s, 2 * K - s))
            assert J == ref.jaccard_f64(s, K)
            prunes += [J, math.nextafter(J, 0.0)] + ([math.nextafter(J, 2.0)] if J < 1.0 else [])
            # at J the pair is kept (equality), just below too, just above it takes one more shared neighbour
            assert lib_min_shared(k, include_self, J) == s
            assert lib_min_shared(k, include_self, math.nextafter(J, 0.0)) == s
            if J < 1.0:
                assert lib_min_shared(k, include_self, math.nextafter(J, 2.0)) == s + 1
        for p in prunes:
            assert lib_min_shared(k, include_self, p) == ref.min_shared(k, include_self, p), (k, p)
        assert lib_min_shared(k, include_self, 0.0) == 1 and lib_min_shared(k, include_self, 1.0) == K


def test_snn_min_shared_equality_case_and_refusals():
    from singlerust_amd import _ffi
    assert lib_min_shared(15, True, 1.0 / 15.0) == 2            # 2 / (32 - 2) is 1 / 15 to the bit: equality keeps the pair
    assert 2.0 / 30.0 == 1.0 / 15.0
    assert lib_min_shared(15, False, 1.0 / 15.0) == 2           # 1 / 29 < 1 / 15 <= 2 / 28
    assert lib_min_shared(19, True, 1.0 / 15.0) == 3            # 2 / 38 < 1 / 15 <= 3 / 37
    for k, prune, text in ((0, 0.5, "outside 1..64"), (65, 0.5, "outside 1..64"), (15, -0.1, "not in [0, 1]"),
                           (15, 1.0000001, "not in [0, 1]"), (15, float("nan"), "not in [0, 1]")):
        with pytest.raises(_ffi.SrxError) as e:
            lib_min_shared(k, True, prune)
        assert e.value.code == _ffi.E_ARG and text in str(e.value), str(e.value)
    out = C.c_uint32(7)
    assert _ffi.lib().srx_snn_min_shared(15, 1, 0.5, None) == _ffi.E_ARG and out.value == 7


def _listing(tmp_path, name):
    from singlerust_amd import build
    out = str(tmp_path / (name + ".s"))
    subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "singlerust_amd", "csrc", name + ".hip")], stderr=subprocess.DEVNULL)
    return open(out).read()


def test_snn_kernels_do_not_spill_registers(tmp_path):
    """The gfx950 code-object metadata of every kernel of snn.hip: no VGPR / SGPR spill, no scratch, and the LDS that the
    capacities were fixed by (a wave-route workgroup under 32 KiB, a workgroup-route one under 48 KiB, the window under 80)."""
    meta = _listing(tmp_path, "snn")
    seen, lds = set(), {}
    for m in re.finditer(r"\.name:\s+(\S*k_snn_\S*)\n(.*?)\.wavefront_size", meta, flags=re.S):
        body = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        assert spill == 0 and sspill == 0 and scratch == 0, f"{m.group(1)}: {spill} / {sspill} spilled V/SGPRs, {scratch} B of scratch"
        seen |= {k for k in KERNELS if re.search(r"\d%s(I|E|\b)" % k, m.group(1))}
    assert seen == set(KERNELS), set(KERNELS) - seen
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\s*\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+(\S+)", meta, flags=re.S):
        lds[m.group(2)] = int(m.group(1))
    for name, size in lds.items():
        if "k_snn_hashILi64E" in name:
            assert size <= 32 * 1024, (name, size)
        elif "k_snn_hashILi256E" in name:
            assert size <= 48 * 1024, (name, size)
        elif "k_snn_window" in name:
            assert size <= 80 * 1024, (name, size)
    assert sum("k_snn_hash" in n for n in lds) == 4 and sum("k_snn_window" in n for n in lds) == 2


def test_graph_kernels_still_do_not_spill(tmp_path):
    """graph.hip now shares its reverse-list launches with snn.hip through host functions; its kernels are as they were."""
    meta = _listing(tmp_path, "graph")
    names = set()
    for m in re.finditer(r"\.name:\s+(\S*k_graph_\S*)\n(.*?)\.wavefront_size", meta, flags=re.S):
        body = m.group(2)
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1)) == 0, m.group(1)
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1)) == 0, m.group(1)
        names.add(re.search(r"k_graph_[a-z_]+", m.group(1)).group(0))
    assert names == {"k_graph_rows", "k_graph_reverse", "k_graph_rowlen", "k_graph_scatter", "k_graph_order", "k_graph_order_long",
                     "k_graph_merge"}

"""BBKNN without a GPU: the restatements of tests/bbknn_ref.py against the hand-worked known answers and against each other
(the closed form of the trimming equals bbknn's two-pass loop, ties at a threshold included; the list per batch equals the
brute-force search of knn_ref.py on the batch's subset), and the new symbols in every layer."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph

import bbknn_ref as ref
import knn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srx_bbknn_result", "srx_bbknn_points", "srx_bbknn_harmony", "srx_graph_trim")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_csr(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))


def kat():
    with open(os.path.join(ROOT, "tests", "golden", "bbknn_kat.json")) as f:
        return json.load(f)


# ---- known answers ------------------------------------------------------------------------------------------------------------
def test_list_known_answer():
    k = kat()["list"]
    x = np.array(k["points"], dtype=np.float64)[:, None]
    idx, dist = ref.bbknn_list(x, k["batch"], k["n_batches"], k["neighbors_within_batch"])
    assert idx.tolist() == k["indices"]
    assert np.array_equal(dist, np.array(k["distances"], dtype=np.float64))
    # K = k_within * B - 1, and every row holds k_within points of the other batch and k_within - 1 of its own
    batch = np.array(k["batch"])
    assert idx.shape == (6, 3)
    for i in range(6):
        assert (batch[idx[i]] == batch[i]).sum() == 1 and i not in idx[i]


def test_trim_known_answer():
    k = kat()["trim"]
    n = k["n"]

    def csr(entries):
        rows = [[] for _ in range(n)]
        for i, j, v in entries:
            rows[i].append((j, v))
            rows[j].append((i, v))
        rows = [sorted(r) for r in rows]
        return (np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64), np.array([j for r in rows for j, _ in r], dtype=np.uint32),
                np.array([v for r in rows for _, v in r], dtype=np.float64))

    src, want = csr(k["entries"]), csr(k["kept"])
    assert ref.thresholds(src[0], src[2], k["trim"]).tolist() == k["thresholds"]
    got, info = ref.trim_closed(src, k["trim"])
    assert same_csr(got, want)
    assert same_csr(ref.trim_bbknn_loop(src, k["trim"]), want)
    for name, v in k["info"].items():
        assert info[name] == v, name


# ---- the two forms of the trimming --------------------------------------------------------------------------------------------
def _bbknn_graph(x, batch, B, kw):
    idx, dist = ref.bbknn_list(x, batch, B, kw)
    _, Cm, _, _, _ = ref.graph(idx, dist)
    return Cm.indptr.astype(np.uint64), Cm.indices.astype(np.uint32), Cm.data.astype(np.float64)


def test_trimming_forms_agree_on_a_lattice_with_ties():
    """Integer coordinates in -6 .. 6: many distances tie, many weights tie at a row's threshold, and rows stay longer than trim."""
    rng = np.random.default_rng(42)
    n, B, kw, trim = 257, 4, 2, 9
    x = ref.lattice(rng, n, 2, 6)
    c = _bbknn_graph(x, ref.labels("hashed", [65, 64, 64, 64], 1), B, kw)
    got, info = ref.trim_closed(c, trim)
    assert same_csr(got, ref.trim_bbknn_loop(c, trim))
    L0, L1 = np.diff(c[0].astype(np.int64)), np.diff(got[0].astype(np.int64))
    assert ((L0 > trim) & (L1 > trim)).sum() >= 1, "no row stays longer than trim: the tie branch is not exercised"
    assert info["entries_trimmed"] > 0 and info["entries_trimmed"] % 2 == 0
    m = sp.csr_matrix((got[2], got[1].astype(np.int64), got[0].astype(np.int64)), shape=(n, n))
    assert (m != m.T).nnz == 0 and m.diagonal().sum() == 0


@pytest.mark.parametrize("seed,n,k,trim", [(1, 200, 6, 1), (2, 300, 10, 4), (3, 150, 5, 7), (4, 400, 15, 12)])
def test_trimming_forms_agree_on_random_graphs(seed, n, k, trim):
    rng = np.random.default_rng(seed)
    idx = np.array([rng.choice(np.delete(np.arange(n), i), k, replace=False) for i in range(n)])
    w = rng.random((n, k)) if seed % 2 else rng.integers(1, 5, (n, k)) / 4.0          # continuous, or four values: heavy ties
    c = ref.symmetric_from_list(idx, w)
    got, info = ref.trim_closed(c, trim)
    assert same_csr(got, ref.trim_bbknn_loop(c, trim))
    assert info["nnz_before"] - info["nnz_after"] == info["entries_trimmed"] and info["rows_over_trim"] > 0
    # trimming a graph with no row over trim changes nothing
    big, info_big = ref.trim_closed(c, int(np.diff(c[0].astype(np.int64)).max()))
    assert same_csr(big, c) and info_big["rows_over_trim"] == 0


# ---- the list -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["contiguous", "interleaved", "hashed"])
def test_list_per_batch_equals_the_brute_force_on_the_subset(kind):
    rng = np.random.default_rng(7)
    sizes, kw = [40, 3, 57, 21], 3
    n, B = sum(sizes), len(sizes)
    units = rng.integers(-9, 10, (n, 3)).astype(np.int64)
    batch = ref.labels(kind, sizes, 5)
    idx, dist = ref.bbknn_list(units.astype(np.float64), batch, B, kw)
    assert idx.shape == (n, kw * B - 1)
    assert (np.diff(dist, axis=1) >= 0).all()
    for b in range(B):
        members = np.nonzero(batch == b)[0]
        sub = knn_ref.Case("sub", units[members])
        own_i, own_d = sub.expected_k(kw - 1)                                   # the self graph of the batch
        for local, i in enumerate(members):
            mine = np.nonzero(batch[idx[i]] == b)[0]
            assert idx[i][mine].tolist() == members[own_i[local]].tolist()
            assert np.array_equal(dist[i][mine], own_d[local])
        others = np.nonzero(batch != b)[0]
        cross = knn_ref.Case("cross", units[members], query=units[others])
        ci, cd = cross.expected_k(kw)
        for q, i in enumerate(others):
            mine = np.nonzero(batch[idx[i]] == b)[0]
            assert idx[i][mine].tolist() == members[ci[q]].tolist()
            assert np.array_equal(dist[i][mine], cd[q])
    assert ref.pairs_searched(sizes, kw) == n * n and ref.pairs_searched(sizes, 1) == n * n - sum(s * s for s in sizes)
    assert ref.n_searches(sizes, kw) == 3 * B - 2 and ref.n_searches(sizes, 1) == 2 * B - 2


def test_quality_input_on_the_reference():
    """The input of the device's quality test: plain neighbours are batch-pure, the BBKNN rows balanced, and no edge of the
    BBKNN graph leaves a clump, so any community of its graph lies within one clump and spans both batches."""
    x, batch, clump = ref.clumps_two_batches(np.random.default_rng(11))
    n, kw = len(x), 3
    d2 = ref.dist2(x, x)
    d2[np.arange(n), np.arange(n)] = np.inf
    plain = np.argsort(d2, axis=1, kind="stable")[:, :2 * kw - 1]
    assert (batch[plain] == batch[:, None]).all()
    idx, dist = ref.bbknn_list(x, batch, 2, kw)
    assert ((batch[idx] == batch[:, None]).sum(axis=1) == kw - 1).all()
    assert (clump[idx] == clump[:, None]).all()
    _, Cm, _, _, _ = ref.graph(idx, dist)
    n_comp, comp = csgraph.connected_components(Cm, directed=False)
    assert n_comp == 3 and len({(int(a), int(b)) for a, b in zip(comp, clump)}) == 3
    for c in range(3):
        assert set(batch[comp == c]) == {0, 1}


# ---- the layers ---------------------------------------------------------------------------------------------------------------
def test_bbknn_symbols_are_exported_and_bound():
    from singlerust_amd import _ffi, build
    from singlerust_amd.memory import processing
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "srx.h")).read()
    rust = open(os.path.join(ROOT, "rust", "srx_sys.rs")).read()
    shim = open(os.path.join(ROOT, "rust", "shim.rs")).read()
    mirror = open(os.path.join(ROOT, "singlerust_amd", "host", "single_rust.hpp")).read()
    assert "bbknn.hip" in build.SOURCES
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _ffi.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, rust), name
    for name in ("srx_bbknn_result", "srx_bbknn_points", "srx_graph_trim"):
        assert re.search(r"\b%s\s*\(" % name, mirror), name
    for name in ("srx_bbknn_result", "srx_graph_trim"):
        assert re.search(r"\b%s\s*\(" % name, shim), name
    for s in ("SrxBbknnOpts", "SrxBbknnInfo", "SrxTrimInfo"):
        assert "pub struct %s" % s in rust, s
    for fn in ("bbknn", "bbknn_points"):
        assert callable(getattr(processing, fn)), fn
    assert callable(processing.neighbors.__globals__["Graph"].trim)
    assert C.sizeof(_ffi.BbknnOpts) == 16 and C.sizeof(_ffi.TrimInfo) == 104
    assert C.sizeof(_ffi.BbknnInfo) == 72 + C.sizeof(_ffi.TrimInfo) + 48
    for script in ("gen_rust_bindings.py", "gen_ctypes_bindings.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--check"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    section = header[header.index("---- BBKNN"):header.index("srx_bbknn_opts")]
    assert "NOT been" in section and "21 batches" in section

"""srx_paga_from_counts (host code: no GPU) against the definition in tests/paga_ref.py, bit for bit; the hand-checkable known
answer; the spanning tree's properties against scipy; the host call's refusals; the symbols in every layer; and the gfx950
listings of paga.hip's kernels free of register spills and scratch."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import paga_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srx_paga", "srx_paga_csr", "srx_paga_from_counts", "srx_paga_init_positions")
KERNELS = ("k_paga_check_indices", "k_paga_walk", "k_paga_init")
COUNTERS = ("n", "nnz", "n_groups", "groups_empty", "edges_inner", "edges_inter", "pairs_connected", "pairs_clipped", "tree_edges",
            "components")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_matches_ref(got, counts, sizes):
    """All six tables and every counter of `got` (the library) equal the reference's on the same counts, bit for bit."""
    G = len(sizes)
    want = ref.from_counts(ref.sparse_counts(counts), sizes, G)
    assert got["sizes"].tolist() == [int(s) for s in sizes]
    assert got["out_edges"].tolist() == want["out_edges"]
    assert np.array_equal(got["counts"], np.asarray(counts, dtype=np.uint64))
    for name, key in (("connectivities", "connectivities"), ("expected", "expected"), ("tree", "tree")):
        assert np.array_equal(bits(got[name]), bits(ref.dense(want[key], G))), name
    for c in COUNTERS:
        assert got["info"][c] == want["info"][c], c
    return want


def random_counts(rng, G, density, hi, empty=0.0):
    counts = np.where(rng.random((G, G)) < density, rng.integers(1, hi, (G, G)), 0).astype(np.uint64)
    sizes = rng.integers(1, 2000, G).astype(np.uint64)
    gone = rng.random(G) < empty
    sizes[gone] = 0
    counts[gone, :] = 0
    counts[:, gone] = 0
    return counts, sizes


def knn_counts(rng, n, k, G):
    """E of a random k-NN pattern whose labels follow planted clumps (most neighbours fall inside the clump)."""
    labels = rng.integers(0, G, n)
    E = np.zeros((G, G), dtype=np.uint64)
    for i in range(n):
        same = rng.random(k) < 0.7
        tgt = np.where(same, labels[i], rng.integers(0, G, k))
        np.add.at(E[labels[i]], tgt, 1)
    sizes = np.bincount(labels, minlength=G).astype(np.uint64)
    E[sizes == 0, :] = 0
    E[:, sizes == 0] = 0
    return E, sizes


def test_paga_symbols_are_exported_and_bound():
    from singlerust_amd import _ffi, build
    from singlerust_amd.memory import processing
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "srx.h")).read()
    rust = open(os.path.join(ROOT, "rust", "srx_sys.rs")).read()
    shim = open(os.path.join(ROOT, "rust", "shim.rs")).read()
    mirror = open(os.path.join(ROOT, "singlerust_amd", "host", "single_rust.hpp")).read()
    assert "paga.hip" in build.SOURCES
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _ffi.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, rust), name
        assert re.search(r"\b%s\s*\(" % name, mirror), name
        assert re.search(r"\b%s\s*\(" % name, shim), name
    assert "pub struct SrxPagaInfo" in rust and "pub struct SrxPagaTables" in rust
    for fn in ("paga", "paga_csr", "paga_from_counts", "paga_init_positions"):
        assert callable(getattr(processing, fn)), fn
    assert re.search(r"#define\s+SRX_ABI_VERSION\s+6\b", header) and lib.srx_abi_version() == 6
    assert C.sizeof(_ffi.PagaInfo) == 72 and C.sizeof(_ffi.PagaTables) == 48
    for script in ("gen_rust_bindings.py", "gen_ctypes_bindings.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--check"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr


def test_paga_known_answer():
    """tests/golden/kat_paga.json (8 cells, k = 2, 3 groups; one clipped pair, one tie in the tree): the file equals what its
    maker computes from the pattern, and srx_paga_from_counts gives its exact fractions rounded once."""
    from singlerust_amd.memory.processing import paga_from_counts
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_paga.json")))
    n, k, G = kat["n"], kat["k"], kat["n_groups"]
    E, sizes = ref.counts_of(list(range(0, n * k + 1, k)), kat["indices"], kat["labels"], G)
    assert ref.dense_counts(E, G).tolist() == kat["counts"] and sizes == kat["sizes"]
    got = paga_from_counts(kat["counts"], kat["sizes"])
    assert_matches_ref(got, np.array(kat["counts"]), kat["sizes"])
    assert got["out_edges"].tolist() == kat["out_edges"]
    clipped = 0
    for key, frac in kat["ratio"].items():
        g, h = (int(x) for x in key.split(","))
        r, ex = Fraction(frac), Fraction(kat["expected"][key])
        assert Fraction(sum(kat["counts"][g]) * sizes[h] + sum(kat["counts"][h]) * sizes[g], n - 1) == ex
        assert Fraction(kat["counts"][g][h] + kat["counts"][h][g]) / ex == r
        for a, b in ((g, h), (h, g)):
            assert got["expected"][a, b] == float(ex)
            if r > 1:
                assert got["connectivities"][a, b] == 1.0
            else:           # three roundings (expected, the quotient, float(r)) of 2^-53 relative each
                assert abs(got["connectivities"][a, b] - float(r)) <= 3 * 2.0 ** -53 * float(r)
        clipped += r > 1
    assert clipped == 1 == got["info"]["pairs_clipped"]
    assert kat["ratio"]["0,2"] == kat["ratio"]["1,2"]                                    # the tie: (0, 2) comes first
    assert sorted(map(list, zip(*np.nonzero(got["tree"])))) == kat["tree_pairs"] == [[0, 1], [0, 2]]
    for c in COUNTERS:
        assert got["info"][c] == kat["info"][c], c


@pytest.mark.parametrize("G", [1, 2, 3, 17, 64, 300])
def test_paga_random_count_tables_match_the_definition(G):
    from singlerust_amd.memory.processing import paga_from_counts
    rng = np.random.default_rng(100 + G)
    for density, hi, empty in ((0.9, 50, 0.0), (0.15, 1000, 0.2), (3.0 / G, 8, 0.0)):
        counts, sizes = random_counts(rng, G, density, hi, empty)
        assert_matches_ref(paga_from_counts(counts, sizes), counts, sizes)


def test_paga_numerator_needs_more_than_64_bits():
    """Counts near 2^40 with sizes near 2^31: es n_h + es_h n_g passes 2^64, and a numerator that wrapped would show in
    `expected` and, through it, in every connectivity."""
    from singlerust_amd.memory.processing import paga_from_counts
    rng = np.random.default_rng(7)
    G = 5
    counts = (rng.integers(0, 1 << 20, (G, G)) + (1 << 40)).astype(np.uint64)
    counts[1, 3] = counts[3, 1] = 0
    counts[0, 4] = 3
    sizes = ((1 << 31) - rng.integers(1, 1000, G)).astype(np.uint64)
    want = assert_matches_ref(paga_from_counts(counts, sizes), counts, sizes)
    es = want["out_edges"]
    assert es[0] * int(sizes[1]) + es[1] * int(sizes[0]) >= 1 << 64
    assert 0.0 < min(want["connectivities"].values()) < 1.0


@pytest.mark.parametrize("seed", range(6))
def test_paga_tree_is_a_maximum_spanning_forest(seed):
    """On k-NN-like tables: the tree spans the components of conn > 0 with G - components edges, and its total of 1 / conn equals
    scipy's minimum spanning tree's on 1 / conn (ties included: any minimum spanning tree has that total)."""
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse import csgraph
    from singlerust_amd.memory.processing import paga_from_counts
    rng = np.random.default_rng(seed)
    G = (4, 9, 20, 33, 50, 12)[seed]
    counts, sizes = knn_counts(rng, 40 * G, (3, 15, 15, 30, 5, 2)[seed], G)
    got = paga_from_counts(counts, sizes)
    assert_matches_ref(got, counts, sizes)
    conn, tree = got["connectivities"], got["tree"]
    n_comp, comp = csgraph.connected_components(sp.csr_matrix(conn > 0), directed=False)
    assert got["info"]["components"] == n_comp and got["info"]["tree_edges"] == G - n_comp == np.count_nonzero(tree)
    assert np.all(np.tril(tree) == 0) and np.all(tree[tree > 0] == conn[tree > 0])
    n_tree, comp_tree = csgraph.connected_components(sp.csr_matrix(tree + tree.T), directed=False)
    assert n_tree == n_comp and np.array_equal(comp_tree, comp)
    inv = np.zeros_like(conn)
    inv[conn > 0] = 1.0 / conn[conn > 0]
    mst = csgraph.minimum_spanning_tree(sp.csr_matrix(inv))
    assert np.sum(1.0 / tree[tree > 0]) == pytest.approx(mst.sum(), rel=1e-12)


def test_paga_tree_equals_scipy_on_tie_free_tables():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse import csgraph
    from singlerust_amd.memory.processing import paga_from_counts
    rng = np.random.default_rng(11)
    done = 0
    for _ in range(40):
        G = int(rng.integers(3, 25))
        counts, sizes = random_counts(rng, G, 0.5, 40)
        np.fill_diagonal(counts, 5000)                       # (most edges inside the groups, as after a clustering: nothing clipped)
        got = paga_from_counts(counts, sizes)
        conn = got["connectivities"]
        vals = conn[np.triu(conn) > 0]
        if len(np.unique(vals)) != len(vals):
            continue
        inv = np.zeros_like(conn)
        inv[conn > 0] = 1.0 / conn[conn > 0]
        mst = csgraph.minimum_spanning_tree(sp.csr_matrix(np.triu(inv))).toarray()
        assert {(min(g, h), max(g, h)) for g, h in zip(*np.nonzero(mst))} == set(zip(*np.nonzero(got["tree"])))
        done += 1
    assert done >= 10


def test_paga_from_counts_refusals():
    """Each refusal is SRX_E_ARG with a message and writes nothing."""
    from singlerust_amd import _ffi
    lib = _ffi.lib()
    counts, sizes = np.array([[1, 2], [3, 4]], np.uint64), np.array([5, 6], np.uint64)
    conn = np.full((2, 2), 7.0)
    info = _ffi.PagaInfo()
    info.n = 99
    t = _ffi.PagaTables(None, None, None, _ffi.ptr(conn), None, None)

    def refused(*args):
        assert lib.srx_paga_from_counts(*args, C.byref(t), C.byref(info)) == _ffi.E_ARG
        assert lib.srx_last_error(None)
        assert info.n == 99 and np.all(conn == 7.0)

    refused(None, _ffi.ptr(sizes), 2)
    refused(_ffi.ptr(counts), None, 2)
    refused(_ffi.ptr(counts), _ffi.ptr(sizes), 0)
    refused(_ffi.ptr(counts), _ffi.ptr(sizes), _ffi.GROUPS_MAX + 1)
    empty = np.array([5, 0], np.uint64)
    refused(_ffi.ptr(np.array([[1, 0], [1, 0]], np.uint64)), _ffi.ptr(empty), 2)       # a count in the empty group's row
    refused(_ffi.ptr(np.array([[1, 1], [0, 0]], np.uint64)), _ffi.ptr(empty), 2)       # ... in its column
    assert lib.srx_paga_from_counts(_ffi.ptr(np.array([[1, 0], [0, 0]], np.uint64)), _ffi.ptr(empty), 2, C.byref(t), C.byref(info)) == _ffi.OK
    assert info.n == 5 and info.groups_empty == 1 and info.components == 2 and np.all(conn == 0.0)
    # the device calls refuse a null handle or context before anything else
    assert lib.srx_paga(None, None, 2, None, None) == _ffi.E_ARG and lib.srx_last_error(None)
    assert lib.srx_paga_csr(None, None, None, 0, None, 2, None, None) == _ffi.E_ARG and lib.srx_last_error(None)
    assert lib.srx_paga_init_positions(None, None, None, 0, 2, None, None, 2, 0, None) == _ffi.E_ARG and lib.srx_last_error(None)


def test_paga_all_zero_tables():
    from singlerust_amd.memory.processing import paga_from_counts
    got = paga_from_counts(np.zeros((4, 4), np.uint64), np.zeros(4, np.uint64))
    assert got["info"]["components"] == 4 and got["info"]["groups_empty"] == 4 and got["info"]["n"] == 0
    for name in ("connectivities", "expected", "tree"):
        assert not bits(got[name]).any()


def test_paga_kernels_do_not_spill_registers(tmp_path):
    """The gfx950 code-object metadata of every kernel of paga.hip shows no VGPR / SGPR spill and no scratch."""
    from singlerust_amd import build
    out = str(tmp_path / "paga.s")
    subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "singlerust_amd", "csrc", "paga.hip")], stderr=subprocess.DEVNULL)
    meta = open(out).read()
    seen = set()
    for m in re.finditer(r"\.name:\s+(\S*k_paga_\S*)\n(.*?)\.wavefront_size", meta, flags=re.S):
        body = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        assert spill == 0 and sspill == 0 and scratch == 0, f"{m.group(1)}: {spill} / {sspill} spilled V/SGPRs, {scratch} B of scratch"
        seen |= {k for k in KERNELS if re.search(r"\d%s(I|E|\b)" % k, m.group(1))}
    assert seen == set(KERNELS), set(KERNELS) - seen
    # the walk's rows per workgroup, as the reference states them for the tests that place group boundaries
    src = open(os.path.join(ROOT, "singlerust_amd", "csrc", "paga.hip")).read()
    assert int(re.search(r"constexpr uint64_t kPagaRows = (\d+);", src).group(1)) == ref.ROWS_PER_WORKGROUP

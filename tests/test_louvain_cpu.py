"""srx_louvain / srx_louvain_csr / srx_graph_labels_fetch without a GPU: exported and bound in every layer, the struct layout
as the C compiler lays it out, a loud failure without a device (no CPU fallback), the kernels' gfx950 listings free of
register spills and scratch, the host restatement against the golden quality and the known answers, and the golden file
against a fresh networkx run where networkx is installed."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import louvain_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srx_louvain", "srx_louvain_csr", "srx_graph_labels_fetch")
KERNELS = ("k_louvain_degree", "k_louvain_scale", "k_louvain_quant", "k_louvain_classify", "k_louvain_biglist",
           "k_louvain_move", "k_louvain_move_big", "k_louvain_apply", "k_louvain_q_in", "k_louvain_q_tot", "k_louvain_flag",
           "k_louvain_oldof", "k_louvain_members", "k_louvain_coarse", "k_louvain_unfix", "k_louvain_compose", "k_louvain_sizes",
           "k_louvain_keys", "k_louvain_bitonic", "k_louvain_rank", "k_louvain_relabel")


def test_louvain_symbols_are_exported_and_bound():
    from singlerust_amd import _ffi
    from singlerust_amd.memory import processing
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "srx.h")).read()
    rust = open(os.path.join(ROOT, "rust", "srx_sys.rs")).read()
    shim = open(os.path.join(ROOT, "rust", "shim.rs")).read()
    mirror = open(os.path.join(ROOT, "singlerust_amd", "host", "single_rust.hpp")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _ffi.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, rust), name
        assert re.search(r"\b%s\s*\(" % name, mirror), name
        assert re.search(r"\b%s\s*\(" % name, shim), name
    assert "pub struct SrxLouvainOpts" in rust and "pub struct SrxLouvainInfo" in rust
    assert "pub const SRX_LOUVAIN_MAX_LEVELS: i32 = 32;" in rust
    assert "pub fn louvain(adata: &IMAnnData, resolution: f64)" in shim
    assert "louvain(double resolution" in mirror
    assert callable(processing.louvain) and callable(processing.louvain_csr)
    # additive: the ABI version and the number of profiling classes stay
    assert re.search(r"#define\s+SRX_ABI_VERSION\s+6\b", header) and lib.srx_abi_version() == 6
    assert re.search(r"SRX_K_COUNT_ = 13\b", header)
    assert re.search(r"#define\s+SRX_LOUVAIN_MAX_LEVELS\s+32\b", header) and _ffi.LOUVAIN_MAX_LEVELS == 32
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_rust_bindings.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("cname,struct", [("srx_louvain_opts", "LouvainOpts"), ("srx_louvain_info", "LouvainInfo")])
def test_louvain_struct_layout_matches_header(tmp_path, cname, struct):
    """sizeof() and the field offsets of the ctypes mirrors equal what gcc lays out."""
    from singlerust_amd import _ffi
    st = getattr(_ffi, struct)
    fields = [n for n, _ in st._fields_]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "srx.h"\nint main(void){printf("%%zu", sizeof(%s));\n' % cname
            + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f in fields) + "return 0;}\n")
    src, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(src, "w").write(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(st)] + [getattr(st, f).offset for f in fields]
    assert C.sizeof(st) == {"LouvainOpts": 24, "LouvainInfo": 56 + 2 * 8 * 32}[struct]


def test_louvain_fails_loudly_without_a_device():
    """Null handles are SRX_E_ARG with a message; with no device visible nothing is computed on the host (a child process
    with every device hidden, so the test means the same on a GPU machine)."""
    from singlerust_amd import _ffi
    lib = _ffi.lib()
    ip, ix, w = np.array([0, 1, 2], np.uint64), np.array([1, 0], np.uint32), np.ones(2)
    assert lib.srx_louvain(None, None, None, None) == _ffi.E_ARG
    assert lib.srx_last_error(None)
    assert lib.srx_louvain_csr(None, _ffi.ptr(ip), _ffi.ptr(ix), _ffi.ptr(w), 2, None, None, None) == _ffi.E_ARG
    assert lib.srx_graph_labels_fetch(None, None) == _ffi.E_ARG
    code = ("import numpy as np, singlerust_amd as sr\n"
            "from singlerust_amd.memory.processing import louvain_csr\n"
            "try:\n"
            "    louvain_csr(sr.Context(0), (np.array([0, 1, 2], np.uint64), np.array([1, 0], np.uint32), np.ones(2)))\n"
            "except sr.SrxError as e:\n"
            "    print('refused', e.code, e)\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("refused %d " % _ffi.E_HIP) and "no CPU fallback" in r.stdout, (r.stdout, r.stderr)


def test_louvain_kernels_do_not_spill_registers(tmp_path):
    """The gfx950 code-object metadata of every kernel of louvain.hip shows no VGPR / SGPR spill and no scratch."""
    from singlerust_amd import build
    assert "louvain.hip" in build.SOURCES
    out = str(tmp_path / "louvain.s")
    subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "singlerust_amd", "csrc", "louvain.hip")], stderr=subprocess.DEVNULL)
    meta = open(out).read()
    seen, n_kernels = set(), 0
    for m in re.finditer(r"\.name:\s+(\S*k_louvain_\S*)\n(.*?)\.wavefront_size", meta, flags=re.S):
        body = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        assert spill == 0 and sspill == 0 and scratch == 0, f"{m.group(1)}: {spill} / {sspill} spilled V/SGPRs, {scratch} B of scratch"
        n_kernels += 1
        seen |= {k for k in KERNELS if re.search(r"\d%s(I|E|\b)" % k, m.group(1))}
    assert seen == set(KERNELS), set(KERNELS) - seen
    assert n_kernels == len(KERNELS) + 2                   # k_louvain_move<32> / <64>, k_louvain_coarse<false> / <true>


def test_symcsr_kernels_do_not_spill_registers(tmp_path):
    """The same for every kernel of symcsr.hip (the input check of srx_louvain_csr, srx_umap_csr and srx_diffmap_csr)."""
    from singlerust_amd import build
    assert "symcsr.hip" in build.SOURCES
    out = str(tmp_path / "symcsr.s")
    subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "singlerust_amd", "csrc", "symcsr.hip")], stderr=subprocess.DEVNULL)
    meta = open(out).read()
    names = []
    for m in re.finditer(r"\.name:\s+(\S*k_symcsr_\S*)\n(.*?)\.wavefront_size", meta, flags=re.S):
        body = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        assert spill == 0 and sspill == 0 and scratch == 0, f"{m.group(1)}: {spill} / {sspill} spilled V/SGPRs, {scratch} B of scratch"
        names.append(m.group(1))
    assert len(names) == 1 and re.search(r"\dk_symcsr_check(E|\b)", names[0]), names


# ---- the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["separated_3000", "separated_20011", "overlapping_6000", "karate_stored", "karate_unit"])
def test_restatement_reaches_the_golden_quality(name):
    """The quality rule of the GPU tests, on the host restatement: Q >= q_min - (q_max - q_min) over networkx's five seeds."""
    W, planted = ref.fixture_graph(name)
    labels, info = ref.louvain(W)
    floor = ref.quality_floor(name)
    print(name, info["modularity"], "floor", floor, info["level_communities"])
    assert abs(info["modularity"] - ref.modularity(W, labels)) <= 1e-12
    assert info["modularity"] >= floor
    if name.startswith("separated"):
        assert info["n_communities"] == 12 and ref.ari(labels, planted) == 1.0


def test_restatement_known_answers():
    labels, info = ref.louvain(ref.ring_of_cliques(8, 6))
    assert np.array_equal(np.bincount(labels), [6] * 8) and abs(info["modularity"] - 0.8125) <= 1e-12
    labels, info = ref.louvain(ref.two_cliques())
    assert np.array_equal(labels, [1, 1, 1, 0, 0, 0, 0]) and abs(info["modularity"] - 4.0 / 9.0) <= 1e-12
    labels, info = ref.louvain(ref.karate(False))
    assert info["n_communities"] == 3 and abs(info["modularity"] - 0.434521) <= 1e-6
    labels, info = ref.louvain(ref.karate(True))
    assert info["n_communities"] == 4 and abs(info["modularity"] - 0.418803) <= 1e-6
    import scipy.sparse as sp
    labels, info = ref.louvain(sp.csr_matrix((5, 5)))
    assert np.array_equal(labels, np.arange(5)) and info["modularity"] == 0.0 and info["n_levels"] == 0
    labels, info = ref.louvain(sp.csr_matrix(np.array([[0, 0.7], [0.7, 0]])))
    assert np.array_equal(labels, [0, 0]) and info["n_communities"] == 1
    # a converged first level cannot be improved
    W = ref.fixture_graph("separated_3000")[0]
    l0, i0 = ref.louvain(W, max_levels=1)
    assert i0["n_levels"] == 1 and ref.max_excess(W, l0) <= 0.0
    assert ref.max_excess(W, np.arange(W.shape[0])) > 0.0


def test_golden_file_matches_networkx():
    """Where networkx imports, the golden file is regenerated and equals the committed one to 1e-9."""
    pytest.importorskip("networkx")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_louvain_golden as gen
    have = ref.golden()
    doc = gen.build()
    assert doc["karate_edges"] == have["karate_edges"] and list(doc["fixtures"]) == list(have["fixtures"])
    for name, f in doc["fixtures"].items():
        g = have["fixtures"][name]
        assert (f["n"], f["nnz"]) == (g["n"], g["nnz"])
        for a, b in zip(f["seeds"], g["seeds"]):
            assert a["seed"] == b["seed"] and a["n_communities"] == b["n_communities"] and abs(a["modularity"] - b["modularity"]) <= 1e-9


# ---- the exact cases: what tests/test_louvain_exact_gpu.py presupposes ---------------------------------------------------------
ALL_RUNS = ref.EXACT_RUNS + ref.prefix_runs() + [r[:2] for r in ref.guard_runs()]


@pytest.mark.parametrize("name", sorted({r[0] for r in ALL_RUNS}))
def test_exact_case_is_dyadic_and_valid(name):
    """Every weight is a multiple of 2^-20 and 2m < 2^32 (so every sum of the definition is exact in f64 and in the device's
    fixed point), and the graph passes what srx_louvain_csr checks."""
    W = ref.exact_graph(name)
    assert W.shape[0] == W.shape[1] and W.has_sorted_indices and W.data.dtype == np.float64
    assert np.array_equal(np.rint(W.data * ref.DYADIC), W.data * ref.DYADIC) and (W.data > 0).all()
    assert W.data.sum() < 2.0 ** 32
    rows = np.repeat(np.arange(W.shape[0]), np.diff(W.indptr))
    assert (rows != W.indices).all()                                                 # no diagonal
    inner = np.ones(W.nnz, dtype=bool)
    inner[W.indptr[:-1][np.diff(W.indptr) > 0]] = False                              # first entry of every row
    assert (np.diff(W.indices.astype(np.int64), prepend=-1)[inner] > 0).all()        # strictly ascending: no duplicates either
    T = W.T.tocsr()
    T.sort_indices()
    assert np.array_equal(T.indptr, W.indptr) and np.array_equal(T.indices, W.indices)
    assert np.array_equal(T.data.view(np.uint64), W.data.view(np.uint64))            # symmetric bit for bit


@pytest.mark.parametrize("run", ALL_RUNS, ids=ref.run_id)
def test_exact_run_decides_levels_with_a_margin(run):
    """The one decision that is not bit for bit on the device, keeping or discarding a level, rests on its Q, which is held to
    1e-9: no decision of the restatement is closer than 1e-8.  A condition on the inputs; a case that fails it gets another
    seed."""
    labels, info = ref.exact_result(*run)
    W = ref.exact_graph(run[0])
    print(ref.run_id(run), "n", W.shape[0], "nnz", W.nnz, "levels", info["level_communities"], "sweeps", info["level_sweeps"],
          "moves", info["moves"], "Q", info["modularity"], "margin", info["min_margin"])
    assert info["min_margin"] >= 1e-8
    assert W.nnz * 2.0 ** -53 < 1e-9
    assert abs(info["modularity"] - ref.modularity(W, labels, run[1].get("gamma", 1.0))) <= 1e-12


def _first_coarse_graph(name):
    W = ref.exact_graph(name)
    zero = np.zeros(W.shape[0])
    comm = ref._level(W, zero, 1.0, 200)[0]
    return ref.aggregate(W, zero, comm)[:2]


def _deciding_ties(W, k, twom, comm, gamma, active):
    """A copy of ref.gains as far as the candidates' gains: the number of vertices whose best admissible gain beats their own
    and is reached by two targets, so that only the lowest-id rule decides where they go."""
    n = W.shape[0]
    coo = W.tocoo()
    rows, cols, data = coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data
    m = active[rows]
    rows, cols, data = rows[m], cols[m], data[m]
    tot = np.bincount(comm, weights=k, minlength=n)
    size = np.bincount(comm, minlength=n)
    key, inv = np.unique(rows * n + comm[cols], return_inverse=True)
    w_to = np.bincount(inv.ravel(), weights=data, minlength=len(key))
    ur, uc = key // n, key % n
    own = comm[ur]
    is_own = uc == own
    w_own = np.zeros(n)
    w_own[ur[is_own]] = w_to[is_own]
    g_own = w_own - gamma * k * (tot[comm] - k) / twom
    cand = ~is_own & ~((size[own] == 1) & (size[uc] == 1) & (uc < own))
    ur, g = ur[cand], (w_to - gamma * k[ur] * tot[uc] / twom)[cand]
    order = np.lexsort((-g, ur))
    ur, g = ur[order], g[order]
    second = np.zeros(len(ur), dtype=bool)
    second[1:] = (ur[1:] == ur[:-1]) & (g[1:] == g[:-1])
    first = np.ones(len(ur), dtype=bool)
    first[1:] = ur[1:] != ur[:-1]
    tied_best = np.zeros(len(ur), dtype=bool)
    tied_best[:-1] = first[:-1] & second[1:]
    return int((tied_best & (g > g_own[ur])).sum())


def test_exact_cases_reach_what_they_are_there_for():
    """So that a later edit of a generator cannot quietly empty the device test."""
    for name in ("row_classes_last", "row_classes_first"):
        lens = np.diff(ref.exact_graph(name).indptr)
        assert set(ref.ROW_CLASS_LENGTHS) <= set(lens.tolist()), name
    first, last = ref.exact_graph("row_classes_first"), ref.exact_graph("row_classes_last")
    ne = len(ref.ROW_CLASS_LENGTHS)
    assert tuple(np.diff(first.indptr)[:ne]) == tuple(np.diff(last.indptr)[-ne:]) == ref.ROW_CLASS_LENGTHS
    # the second level of coarse_long_rows: rows of every class, with self weights
    Wc, selfc = _first_coarse_graph("coarse_long_rows")
    lens = np.diff(Wc.indptr)
    print("coarse_long_rows level 2:", Wc.shape[0], "vertices, rows of", lens.min(), "to", lens.max(), "entries")
    assert (lens > 64).any() and (lens <= 64).any() and (selfc[lens > 64] > 0).any()
    info = ref.exact_result("coarse_long_rows", {})[1]
    assert info["n_levels"] >= 2
    # chain_300k: more coarse ids than one bitmap pass of the aggregation holds
    info = ref.exact_result("chain_300k", {})[1]
    assert info["level_communities"][0] > 2 ** 17 and info["n_levels"] >= 2
    # ties_int: a level that runs into max_sweeps, an early end by min_gain, and exact ties that only the lowest id decides
    info = ref.exact_result("ties_int", {})[1]
    assert 200 in info["level_sweeps"]
    early = ref.exact_result("ties_int", {"min_gain": ref.TIES_INT_MIN_GAIN})[1]
    assert 0 < early["n_levels"] < info["n_levels"]
    assert [ref.exact_result("ties_int", {"max_levels": m})[1]["n_levels"] for m in (1, 2, 3)] == [1, 2, 3]
    for name in ("ties_int", "unit"):
        W = ref.exact_graph(name)
        k = np.asarray(W.sum(axis=1)).ravel()
        comm, ids, ties = np.arange(W.shape[0], dtype=np.int64), np.arange(W.shape[0]), 0
        for t in range(4):
            active = (ids + t) % 2 == 0
            ties += _deciding_ties(W, k, k.sum(), comm, 1.0, active)
            v, c, g, g_own = ref.gains(W, k, k.sum(), comm, 1.0, active)
            comm = comm.copy()
            comm[v[g > g_own[v]]] = c[g > g_own[v]]
        print(name, "vertices moved by the lowest-id rule in the first four sweeps:", ties)
        assert ties > 0


def test_guard_cases_by_hand():
    """The restatement on the small graphs whose outcome the singleton guard and the lowest-id rule decide, against labels worked
    out by hand from include/srx.h.  The traces (communities by the id they carry during the level):
      path_2 (0-1-2, 2m = 4): sweep 0: 0 joins 1 (g = 1 - 1*2/4 > 0); 2 may not join the lower singleton 1 -> {0,1}{2}.  Sweep 1:
        1 stays (g(own) = g({2}) = 0.5).  Sweep 2: 2 joins {0,1} (0.25 > 0).  One community.
      path_3 (2m = 6): sweep 0: 0 joins 1; 2 may not join 1 and joins 3 -> {0,1}{2,3}; nothing beats that (0.667 against 0).
      path_4 (2m = 8): sweep 0: 0 joins 1, 2 joins 3, 4 may not join 3 -> {0,1}{2,3}{4}.  Sweep 1: 3 joins 4 (0.75 > 0.5)
        -> {0,1}{2}{3,4}.  Sweep 2: 2, alone, meets g({0,1}) = g({3,4}) = 0.25: the lower id, {0,1} -> {0,1,2}{3,4}.
      star_hub_last (hub 4, 2m = 8): sweep 0: 0 and 2 join the hub, which may not join its lower singletons.  Sweep 1: 1 and 3.
      star_hub_first (hub 0): sweep 0: the hub meets four equal gains and joins 1, the lowest; 2 and 4 may not join 0.  Then
        3, then 2 and 4, join {0,1}.
      tie_third: sweep 0: 0 joins 2 (2 and 4 are barred from their lower singletons).  Sweep 1: 1, alone, meets g({0,2}) =
        g({4}) = 12: the lower id, {0,2}.  Sweep 2: 4 joins.  Vertex 3 is isolated."""
    for name, opts, want in ref.guard_runs():
        labels, info = ref.exact_result(name, opts)
        assert np.array_equal(labels, want), (name, opts, labels, want)
    assert [ref.exact_result(n, {})[1][k] for n in ("path_2", "path_4", "star_hub_last", "star_hub_first") for k in ("sweeps", "moves")] \
        == [5, 2, 5, 4, 4, 4, 5, 4]
    info = ref.exact_result("karate_unit", {})[1]
    assert info["level_communities"] == [10, 5, 4] and info["level_sweeps"] == [200, 4, 3]

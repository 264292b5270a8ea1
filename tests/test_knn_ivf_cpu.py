"""The inverted-file k-NN index without a GPU: the new symbols bound in every layer (ctypes, rust/srx_sys.rs, the Rust shim,
the C++ mirror) with the struct layouts gcc gives them, a loud failure without a device (no CPU fallback), the gfx950 listings
of the k_ivf_* kernels free of register spills and scratch with the f32 MFMA in the candidate kernel, and the numpy
restatement (tests/knn_ivf_ref.py) against a brute-force search and one hand-worked case."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import knn_ivf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srx_knn_index_result", "srx_knn_index_points", "srx_knn_index_info_get", "srx_knn_index_fetch", "srx_knn_index_search",
       "srx_neighbors_index", "srx_knn_index_free")
KERNELS = ("k_ivf_sort_pass", "k_ivf_offsets", "k_ivf_segsum", "k_ivf_gather", "k_ivf_dist2", "k_ivf_place", "k_ivf_candidates",
           "k_ivf_select")                   # (the f32 copy is knn.hip's k_knn_fragments: test_knn_cpu.py)


# ---- the layers ---------------------------------------------------------------------------------------------------------------
def test_ivf_symbols_are_exported_and_bound():
    from singlerust_amd import _abi, _ffi, build
    from singlerust_amd.memory import processing
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "srx.h")).read()
    rust = open(os.path.join(ROOT, "rust", "srx_sys.rs")).read()
    shim = open(os.path.join(ROOT, "rust", "shim.rs")).read()
    mirror = open(os.path.join(ROOT, "singlerust_amd", "host", "single_rust.hpp")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _ffi.EXPORTS and name in _abi.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, rust), name
        assert re.search(r"\b%s\s*\(" % name, shim), name
        assert re.search(r"\b%s\s*\(" % name, mirror), name
    for s in ("SrxIvfOpts", "SrxIvfInfo", "SrxIvfSearchInfo"):
        assert "pub struct %s" % s in rust, s
    assert "pub struct SrxKnnIndex " in rust
    assert "pub fn neighbors_approx(adata: &IMAnnData, n_neighbors: usize, n_pcs: usize, n_lists: usize, n_probe: usize)" in shim
    assert "pub fn neighbors(adata: &IMAnnData, n_neighbors: usize, n_pcs: usize, include_self: bool)" in shim     # untouched
    assert all(callable(getattr(processing, f)) for f in ("neighbors_approx", "knn_index", "knn_index_points", "neighbors"))
    assert issubclass(processing.KnnIndex, processing.harmony.OwnedHandle)
    # additive: the ABI version and the number of profiling classes stay, the exact search keeps its file
    assert re.search(r"#define\s+SRX_ABI_VERSION\s+6\b", header) and lib.srx_abi_version() == 6
    assert re.search(r"SRX_K_COUNT_ = 13\b", header)
    assert "knn_ivf.hip" in build.SOURCES and "knn.hip" in build.SOURCES
    text = open(os.path.join(ROOT, "singlerust_amd", "csrc", "knn_ivf.hip")).read()
    assert "knn_device(" in text and "scan_exclusive(" in text and "knn_exact_rows(" in text
    assert not re.search(r"atomicAdd\(\s*\(?\s*(double|float)", text)            # no floating-point atomics


@pytest.mark.parametrize("cname,struct,size", [("srx_ivf_opts", "IvfOpts", 24), ("srx_ivf_info", "IvfInfo", 80),
                                               ("srx_ivf_search_info", "IvfSearchInfo", 64)])
def test_ivf_struct_layout_matches_header(tmp_path, cname, struct, size):
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
    assert C.sizeof(st) == size


def test_ivf_fails_loudly_without_a_device():
    """Null handles are SRX_E_ARG with a message; with no device visible there is no context to index on and nothing is
    computed on the host (a child process with every device hidden, so the test means the same on a GPU machine)."""
    from singlerust_amd import _ffi
    lib = _ffi.lib()
    h = C.c_void_p(77)
    ko = _ffi.KnnOpts(5, 0, 0, 0)
    assert lib.srx_knn_index_points(None, None, 0, 3, None, None, C.byref(h)) == _ffi.E_ARG and h.value == 77
    assert lib.srx_last_error(None)
    assert lib.srx_knn_index_result(None, 0, None, C.byref(h)) == _ffi.E_ARG and h.value == 77
    assert lib.srx_knn_index_info_get(None, None) == _ffi.E_ARG
    assert lib.srx_knn_index_fetch(None, None, None, None) == _ffi.E_ARG
    assert lib.srx_knn_index_search(None, None, 0, C.byref(ko), 0, None, None, None) == _ffi.E_ARG
    assert lib.srx_neighbors_index(None, C.byref(ko), 0, None, C.byref(h)) == _ffi.E_ARG and h.value == 77
    lib.srx_knn_index_free(None)
    code = ("import numpy as np, singlerust_amd as sr\n"
            "from singlerust_amd.memory.processing import knn_index_points\n"
            "try:\n"
            "    knn_index_points(sr.Context(0), np.zeros((10, 3)), n_lists=2)\n"
            "except sr.SrxError as e:\n"
            "    print('refused', e.code, e)\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("refused %d " % _ffi.E_HIP) and "no CPU fallback" in r.stdout, (r.stdout, r.stderr)


def test_ivf_kernels_do_not_spill_registers(tmp_path):
    """The gfx950 code-object metadata of every k_ivf_* kernel shows no VGPR / SGPR spill and no scratch; the candidate kernel
    is there at the six widths of the exact search and the listing holds the 32x32x2 f32 MFMA."""
    from singlerust_amd import build
    out = str(tmp_path / "knn_ivf.s")
    subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "singlerust_amd", "csrc", "knn_ivf.hip")], stderr=subprocess.DEVNULL)
    meta = open(out).read()
    seen, n_cand = set(), 0
    for m in re.finditer(r"\.name:\s+(\S*k_ivf_\S*)\n(.*?)\.wavefront_size", meta, flags=re.S):
        body = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        assert spill == 0 and sspill == 0 and scratch == 0, f"{m.group(1)}: {spill} / {sspill} spilled V/SGPRs, {scratch} B of scratch"
        seen |= {k for k in KERNELS if re.search(r"\d%s(I|E|\b)" % k, m.group(1))}
        n_cand += "k_ivf_candidates" in m.group(1)
    assert seen == set(KERNELS), set(KERNELS) - seen
    assert n_cand == 6
    for m in re.finditer(r"^(_ZN3srx16k_ivf_candidates\S*):[^\n]*\n(.*?)s_endpgm", meta, flags=re.S | re.M):
        assert "v_mfma_f32_32x32x2_f32" in m.group(2) or "v_mfma_f32_32x32x2f32" in m.group(2), m.group(1)
        n_cand -= 1
    assert n_cand == 0


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_restatement_with_every_list_probed_is_brute_force(seed):
    rng = np.random.default_rng(seed)
    ref = rng.integers(-6, 7, (150, 4)).astype(np.int64)                # a coarse lattice: many exact ties
    qry = rng.integers(-6, 7, (40, 4)).astype(np.int64)
    cent = rng.integers(-6, 7, (9, 4)).astype(np.int64)
    for k in (1, 7, 20):
        for q, inc in ((None, False), (None, True), (qry, False)):
            got = R.search(ref, cent, k, 9, q, inc)
            wi, wd = R.brute(ref, k, q, inc)
            assert np.array_equal(got["idx"], wi) and np.array_equal(got["d2"], wd)
            assert got["rows_exhaustive"] == 0 and got["pairs"] == 9 * len(wi) and got["points_scanned"] == 150 * len(wi)
    part = R.search(ref, cent, 7, 2)
    off, mem = part["offsets"], part["members"]
    assert off[0] == 0 and off[-1] == 150 and sorted(mem.tolist()) == list(range(150))
    assert all((np.diff(mem[off[l]:off[l + 1]]) > 0).all() for l in range(9))


def test_restatement_hand_worked_case():
    """8 points on a line, 3 centroids, k = 2, one probe, the self form without self.
        points     0  1  2 | 5  6 | 20 21 | 12      centroids 1, 6, 20
        lists      {0, 1, 2}   {3, 4, 7}   {5, 6}    (12 is 6 from centroid 6 and 8 from centroid 20)
    Point 3 (at 5) is 4 from centroid 1 and 1 from centroid 6.  Lists 0 and 1 hold two other points for each of their rows;
    list 2 holds one, so rows 5 and 6 are searched over all points."""
    ref = np.array([[0], [1], [2], [5], [6], [20], [21], [12]], dtype=np.int64)
    cent = np.array([[1], [6], [20]], dtype=np.int64)
    got = R.search(ref, cent, 2, 1)
    assert got["assign"].tolist() == [0, 0, 0, 1, 1, 2, 2, 1]
    assert got["offsets"].tolist() == [0, 3, 6, 8] and got["members"].tolist() == [0, 1, 2, 3, 4, 7, 5, 6]
    assert got["probes"][:, 0].tolist() == [0, 0, 0, 1, 1, 2, 2, 1]
    assert got["exhaustive"].tolist() == [False] * 5 + [True, True, False]
    assert got["idx"].tolist() == [[1, 2], [0, 2], [1, 0], [4, 7], [3, 7], [6, 7], [5, 7], [4, 3]]
    assert got["d2"].tolist() == [[1, 4], [1, 1], [1, 4], [1, 49], [1, 36], [1, 64], [1, 81], [36, 49]]
    assert (got["pairs"], got["points_scanned"], got["rows_exhaustive"]) == (8, 3 * 3 + 3 * 3 + 2 * 2, 2)
    # point 2 lies 3 from point 3, nearer than point 7 does, but in another list: one probe does not see it, three do
    assert R.brute(ref, 2)[0][3].tolist() == [4, 2] and R.search(ref, cent, 2, 3)["idx"][3].tolist() == [4, 2]


def test_training_restatement_and_the_hash():
    assert int(R.splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF         # splitmix64's first output for seed 0
    o = R.sample_order(1000, 100, 3)
    assert len(set(o.tolist())) == 100 and not np.array_equal(o, R.sample_order(1000, 100, 4))
    assert np.array_equal(R.sample_order(1000, 1000, 3)[:100], o)        # a prefix of the full hash order
    assert R.default_n_lists(3000) == 219 and R.default_n_lists(1) == 1 and R.default_n_lists(1300000) == 4561
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal((100, 3)) + 10 * c for c in range(4)])
    i0 = [float(R.dist2(x, R.train(x, 4, it, 0, 400)).min(axis=1).sum()) for it in (0, 1, 5)]
    assert i0[2] <= i0[1] <= i0[0]


def test_lattice_case_holds_what_the_device_test_needs():
    ref, cent, qry = R.lattice_case()
    lengths = np.bincount(R.assign_points(ref, cent), minlength=len(cent))
    assert set(R.LATTICE_EDGES) <= set(lengths.tolist()) and lengths.max() > 128
    dq = np.sort(R.dist2(qry, cent), axis=1)
    assert all((dq[:, p - 1] == dq[:, p]).any() for p in (1, 2, 5, len(cent) - 1))
    units, bc = R.blind_case()
    assert np.bincount(R.assign_points(units, bc)).tolist() == [550, 550]

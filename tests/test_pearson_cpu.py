"""Pearson-residual gene selection without a GPU: the numpy restatement (pearson_ref.py) against the decimal known answers, the
properties of the inputs the GPU tests draw, the new symbols bound in every layer with the struct layout gcc gives them, NULL
arguments refused, a loud failure without a device, and the kernels' gfx950 listings free of register spills and scratch."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pearson_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srx_pearson_gene_variance", "srx_select_hvg_pearson", "srx_pearson_residuals")
KERNELS = ("k_pr_totals", "k_pr_gene_factor", "k_pr_dense", "k_pr_sparse_csr", "k_pr_gene_direct", "k_pr_finish", "k_pr_block")
INSTANCES = 10          # three of the seven are templates over the value storage (f32 / f64)
# the kernels this file shares with other calls: the value check (matrix.hip, f32 / f64) and the pick of the first ranks (select.hip)
SHARED = {"matrix.hip": ("k_value_scan", 2), "select.hip": ("k_pick_top", 1)}


def kat():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "kat_pearson.json")))


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kat(), ids=lambda c: c["name"])
def test_reference_against_the_known_answers(case):
    X = np.array(case["X"], dtype=np.int64)
    theta = float(case["theta"])                      # ("inf" parses)
    clip = None if case["clip"] is None else float(case["clip"])
    want_z = np.array([[np.longdouble(s) for s in row] for row in case["z"]])
    want_v = np.array([np.longdouble(s) for s in case["v"]])
    z = R.residuals(X, theta, clip)
    eps = float(np.finfo(np.longdouble).eps)
    assert np.all(np.abs(z - want_z) <= 8 * eps * (1 + np.abs(want_z)))
    assert np.all(np.abs(R.variances(z) - want_v) <= 32 * eps * (1 + np.abs(want_v)))
    # the f64 evaluation of the same restatement stays far inside the device's bounds
    z64 = R.residuals(X, theta, clip, dtype=np.float64)
    assert np.all(np.abs(z64 - want_z) <= R.element_bound(want_z, R.mu_of(X), R.used_opts(X.shape[0], theta, clip)[0]))


def test_identity_matrix_by_hand():
    X = np.array([[1, 0], [0, 1]])
    assert np.all(R.mu_of(X) == 0.5)
    assert np.allclose(np.asarray(R.variances(R.residuals(X, 100.0)), dtype=np.float64), 100.0 / 201.0, rtol=1e-15, atol=0)
    assert np.allclose(np.asarray(R.variances(R.residuals(X, float("inf"))), dtype=np.float64), 0.5, rtol=1e-15, atol=0)


def test_reference_edge_cases_and_order():
    X = np.array([[0, 0, 0], [2, 0, 1], [2, 0, 1]])
    z = R.residuals(X)
    assert np.all(z[0] == 0) and np.all(z[:, 1] == 0) and R.variances(z)[1] == 0           # empty cell, empty gene
    assert np.all(R.residuals(np.zeros((3, 2))) == 0)                                         # T == 0
    v, g = np.array([1.0, 3.0, 3.0, 0.0, 2.0]), np.array([1, 1, 1, 0, 1])
    assert list(R.select(v, g, 10)) == [1, 2, 4, 0] and list(R.select(v, g, 2)) == [1, 2] and R.select(v, g, 0).size == 0
    assert R.used_opts(16, 0, 0) == (100.0, 4.0) and R.used_opts(16, float("inf"), 2.5) == (float("inf"), 2.5)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_inputs_hold_what_the_gpu_tests_need(shape):
    n, G = shape
    X = R.make_counts(n, G)
    assert X.shape == (n, G) and X.min() >= 0 and np.array_equal(X, R.make_counts(n, G))
    for pack, Y in ((R.to_csr, X), (R.to_csc, X.T)):
        rows, cols, indptr, indices, values = pack(X, np.uint32)
        assert (rows, cols) == (n, G) and int(indptr[-1]) == int((X > 0).sum()) == values.size and values.min(initial=1) > 0
        for r in range(min(Y.shape[0], 5)):
            seg = indices[int(indptr[r]):int(indptr[r + 1])]
            assert np.array_equal(seg, np.nonzero(Y[r])[0])
    if not R.has_features(n, G):
        return
    p = R.properties(X)
    assert p["upper_clip_default"] and p["upper_clip_one"] and p["lower_clip_one"], p
    assert p["zero_genes"] >= 1 and p["expressed_genes"] >= G / 2, p
    assert p["empty_cells"] >= 1 and p["full_genes"] >= 1 and p["single_genes"] >= 1 and p["full_cells"] >= 1, p
    assert X.max() >= 40 * 5                                                                    # the outlier count


def test_shapes_walk_round_every_tile_size():
    src = open(os.path.join(ROOT, "singlerust_amd", "csrc", "pearson.hip")).read()
    genes = open(os.path.join(ROOT, "singlerust_amd", "csrc", "genes.hip")).read()

    def const(name, text=src):
        return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert const("kPrCellStep") == R.TILES["dense_cell_step"] and const("kPrDenseThreads") == R.TILES["dense_gene_stride"]
    assert const("kPrDenseThreads") * const("kPrGenesPerThread") == R.TILES["dense_gene_tile"]
    assert const("kPrSparseMinRows") == R.TILES["sparse_row_block"] and const("kPrBlockTile") == R.TILES["block_tile"]
    assert const("kMaxTileGenes", genes) == R.TILES["sparse_gene_tile"]
    ns, gs = {s[0] for s in R.SHAPES}, {s[1] for s in R.SHAPES}
    for t in ("dense_cell_step", "sparse_row_block"):
        assert {R.TILES[t] - 1, R.TILES[t], R.TILES[t] + 1} <= ns, t
    for t in ("dense_gene_tile", "dense_gene_stride", "sparse_gene_tile"):
        assert {R.TILES[t] - 1, R.TILES[t], R.TILES[t] + 1} <= gs, t
    assert {R.TILES["block_tile"] - 1, R.TILES["block_tile"], R.TILES["block_tile"] + 1} <= {n * G for n, G in R.SHAPES}
    assert set(R.ISSUE_SHAPES) <= set(R.SHAPES)


# ---- the layers ------------------------------------------------------------------------------------------------------------------------
def test_pearson_symbols_are_exported_and_bound():
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
    for s in ("SrxPearsonOpts", "SrxPearsonInfo"):
        assert "pub struct %s" % s in rust, s
    for f in ("highly_variable_genes_pearson", "pearson_residuals"):
        assert callable(getattr(processing, f)), f
        assert re.search(r"pub fn %s\b" % f, shim), f
        assert re.search(r"\b%s\(" % f, mirror), f
    # additive: the ABI version and the number of profiling classes stay
    assert re.search(r"#define\s+SRX_ABI_VERSION\s+6\b", header) and lib.srx_abi_version() == 6
    assert re.search(r"SRX_K_COUNT_ = 13\b", header)
    assert "pearson.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "singlerust_amd", "csrc", "pearson.hip")).read()
    assert "fp contract(off)" in src and not any("fast-math" in f for f in build.FLAGS)
    # no floating-point atomic (the fixed-point sums add 64-bit integers); the ranking is select.hip's kernel
    assert not re.search(r"atomicAdd\([^;]*\(double\)|unsafeAtomicAdd|atomicAdd_f|__hip_atomic_fetch_add", src)
    assert "rank_keys_device(ctx, d_key" in src and "pick_top(ctx, d_rank" in src and "value_scan(m, " in src
    assert "rank_keys_device(srx_ctx*" not in src                             # declared once, in pca_internal.hpp
    select = open(os.path.join(ROOT, "singlerust_amd", "csrc", "select.hip")).read()
    assert re.search(r"int32_t rank_keys_device\(.*?k_hvg_rank", select, flags=re.S)


@pytest.mark.parametrize("cname,struct,size", [("srx_pearson_opts", "PearsonOpts", 16), ("srx_pearson_info", "PearsonInfo", 96)])
def test_pearson_struct_layout_matches_header(tmp_path, cname, struct, size):
    """sizeof() and the field offsets of the generated ctypes mirrors equal what gcc lays out."""
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


def test_pearson_fails_loudly_without_a_device():
    """NULL handles and outputs are SRX_E_ARG with a message and nothing written; with no device visible nothing is computed on the
    host (a child process with every device hidden, so the test means the same on a GPU machine)."""
    from singlerust_amd import _ffi
    lib = _ffi.lib()
    var, idx, n_out, g = np.full(4, -7.0), np.full(4, 77, dtype=np.uint64), C.c_uint64(99), np.array([0, 1], dtype=np.uint64)
    info = _ffi.PearsonInfo()
    info.total = -7.0
    assert lib.srx_pearson_gene_variance(None, None, _ffi.ptr(var), C.byref(info)) == _ffi.E_ARG and lib.srx_last_error(None)
    assert lib.srx_select_hvg_pearson(None, 2, None, _ffi.ptr(idx), C.byref(n_out), _ffi.ptr(var), C.byref(info)) == _ffi.E_ARG
    assert lib.srx_pearson_residuals(None, _ffi.ptr(g), 2, None, _ffi.ptr(var), C.byref(info)) == _ffi.E_ARG
    assert np.all(var == -7.0) and np.all(idx == 77) and n_out.value == 99 and info.total == -7.0
    code = ("import numpy as np, singlerust_amd as sr\n"
            "from singlerust_amd.memory.processing import highly_variable_genes_pearson\n"
            "try:\n"
            "    a = sr.IMAnnData.new_basic((2, 2, np.array([0, 1, 2]), np.array([0, 1]), np.array([1.0, 1.0])), ctx=sr.Context(0))\n"
            "    highly_variable_genes_pearson(a, 1)\n"
            "except sr.SrxError as e:\n"
            "    print('refused', e.code, e)\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("refused %d " % _ffi.E_HIP) and "no CPU fallback" in r.stdout, (r.stdout, r.stderr)


def test_pearson_kernels_do_not_spill_registers(tmp_path):
    """The gfx950 code-object metadata of every kernel of pearson.hip shows no VGPR / SGPR spill and no scratch."""
    from singlerust_amd import build
    out = str(tmp_path / "pearson.s")
    subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "singlerust_amd", "csrc", "pearson.hip")], stderr=subprocess.DEVNULL)
    meta = open(out).read()
    seen, n_kernels = set(), 0
    for m in re.finditer(r"\.name:\s+(\S*k_pr_\S*)\n(.*?)\.wavefront_size", meta, flags=re.S):
        body = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        assert spill == 0 and sspill == 0 and scratch == 0, f"{m.group(1)}: {spill} / {sspill} spilled V/SGPRs, {scratch} B of scratch"
        n_kernels += 1
        seen |= {k for k in KERNELS if re.search(r"\d%s(I|E|\b)" % k, m.group(1))}
    assert seen == set(KERNELS), set(KERNELS) - seen
    assert n_kernels == INSTANCES
    for source, (kernel, instances) in SHARED.items():
        out = str(tmp_path / (source + ".s"))
        subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                               os.path.join(ROOT, "singlerust_amd", "csrc", source)], stderr=subprocess.DEVNULL)
        bodies = re.findall(r"\.name:\s+\S*\d%s(?:I\S*|E\S*)?\n(.*?)\.wavefront_size" % kernel, open(out).read(), flags=re.S)
        assert len(bodies) == instances, (kernel, len(bodies))
        for body in bodies:
            for field in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
                assert int(re.search(r"\.%s:\s+(\d+)" % field, body).group(1)) == 0, (kernel, field)

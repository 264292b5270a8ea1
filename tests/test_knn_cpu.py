"""srx_knn_result / srx_knn_points without a GPU: exported and bound in every layer (ctypes, rust/srx_sys.rs, the Rust shim,
the C++ mirror), struct layouts as the C compiler lays them out, a loud failure without a device (no CPU fallback), and the
candidate kernel's code object free of register spills and scratch."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srx_knn_result", "srx_knn_points")


def test_knn_symbols_are_exported_and_bound():
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
        assert re.search(r"\b%s\s*\(" % name, shim), name
        assert re.search(r"\b%s\s*\(" % name, mirror), name
    assert "pub struct SrxKnnOpts" in rust and "pub struct SrxKnnInfo" in rust
    assert "pub fn neighbors(adata: &IMAnnData, n_neighbors: usize, n_pcs: usize, include_self: bool)" in shim
    assert callable(processing.neighbors) and callable(processing.knn_points)
    # additive: the ABI version stays, the profiling class is appended and the earlier ids keep their values
    assert re.search(r"#define\s+SRX_ABI_VERSION\s+6\b", header) and lib.srx_abi_version() == 6
    assert re.search(r"SRX_K_BUCKET = 10,", header) and re.search(r"SRX_K_KNN = 11,", header) and _ffi.K_KNN == 11
    assert int(re.search(r"#define\s+SRX_KNN_MAX_DIMS\s+(\d+)", header).group(1)) == _ffi.KNN_MAX_DIMS >= 128


def test_knn_struct_layouts_match_header(tmp_path):
    """sizeof() and the field offsets of the ctypes mirrors equal what gcc lays out."""
    from singlerust_amd import _ffi
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "srx.h"
int main(void){printf("%zu %zu %zu %zu %zu %zu\n", sizeof(srx_knn_opts), sizeof(srx_knn_info), offsetof(srx_knn_opts, include_self),
 offsetof(srx_knn_info, n_candidates), offsetof(srx_knn_info, rows_certified), offsetof(srx_knn_info, rows_recomputed)); return 0;}'''
    src, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(src, "w").write(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(_ffi.KnnOpts), C.sizeof(_ffi.KnnInfo), _ffi.KnnOpts.include_self.offset,
                   _ffi.KnnInfo.n_candidates.offset, _ffi.KnnInfo.rows_certified.offset, _ffi.KnnInfo.rows_recomputed.offset]


def test_knn_fails_loudly_without_a_device():
    """Null handles are SRX_E_ARG with a message; with no device visible there is no context to search on and nothing is
    computed on the host (a child process with every device hidden, so the test means the same on a GPU machine)."""
    from singlerust_amd import _ffi
    lib = _ffi.lib()
    opts = _ffi.KnnOpts(5, 0, 0, 0)
    assert lib.srx_knn_result(None, C.byref(opts), None, None, None) == _ffi.E_ARG
    assert lib.srx_last_error(None)
    assert lib.srx_knn_points(None, None, 0, None, 0, 3, C.byref(opts), None, None, None) == _ffi.E_ARG
    code = ("import numpy as np, singlerust_amd as sr\n"
            "from singlerust_amd.memory.processing import knn_points\n"
            "try:\n"
            "    knn_points(sr.Context(0), np.zeros((10, 3)), k=2)\n"
            "except sr.SrxError as e:\n"
            "    print('refused', e.code, e)\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("refused %d " % _ffi.E_HIP) and "no CPU fallback" in r.stdout, (r.stdout, r.stderr)


def test_knn_kernels_do_not_spill_registers(tmp_path):
    """The same method as test_hot_kernels_do_not_spill_registers: the gfx950 code-object metadata of every instance of the
    candidate kernel (and of the f64 selection, and of the f32 copy both searches use) shows no VGPR spill and no scratch."""
    from singlerust_amd import build
    out = str(tmp_path / "knn.s")
    subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "singlerust_amd", "csrc", "knn.hip")], stderr=subprocess.DEVNULL)
    meta = open(out).read()
    assert "v_mfma_f32_32x32x2_f32" in meta or "v_mfma_f32_32x32x2f32" in meta
    seen = copies = 0
    for m in re.finditer(r"\.name:\s+(\S*(?:k_knn_candidates|k_knn_exact|k_knn_fragments)\S*)\n(.*?)\.wavefront_size", meta, flags=re.S):
        body = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        assert spill == 0 and scratch == 0, f"{m.group(1)}: {spill} spilled VGPRs, {scratch} B of scratch"
        seen += "k_knn_candidates" in m.group(1)
        copies += "k_knn_fragments" in m.group(1)
    assert seen == 6 and copies == 1, (seen, copies)

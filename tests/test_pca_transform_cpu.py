"""Pca::transform (srx_pca_model_* / srx_pca_transform) without a GPU: the entry points are exported and bound in every layer
(ctypes, rust/srx_sys.rs, the Rust shim's PcaModel), the model kernels compile without register spills, and the C++ mirror's
test compiles under -Werror and fails loudly without a device (under -m gpu it must pass)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "singlerust_amd", "lib")
NEW = ("srx_pca_model_from_result", "srx_pca_model_create", "srx_pca_model_info", "srx_pca_model_free", "srx_pca_transform")


def test_transform_symbols_are_exported_and_bound():
    from singlerust_amd import _ffi
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "srx.h")).read()
    rust = open(os.path.join(ROOT, "rust", "srx_sys.rs")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _ffi.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, rust), name
    assert "pub struct SrxPcaModel" in rust
    # additive: the ABI version stays where it was
    assert re.search(r"#define\s+SRX_ABI_VERSION\s+6\b", header)
    assert lib.srx_abi_version() == 6


def test_transform_refuses_null_arguments_without_a_gpu():
    import ctypes as C
    from singlerust_amd import _ffi
    lib = _ffi.lib()
    assert lib.srx_pca_transform(None, None, None, 0.0, 0, None) == _ffi.E_ARG
    assert lib.srx_pca_model_info(None, None, None, None) == _ffi.E_ARG
    h = C.c_void_p()
    assert lib.srx_pca_model_from_result(None, C.byref(h)) == _ffi.E_ARG
    assert lib.srx_pca_model_create(None, 4, 2, None, None, None, None, 1, 1, C.byref(h)) == _ffi.E_ARG
    lib.srx_pca_model_free(None)                              # a no-op


def test_shim_pca_model_calls_only_declared_functions():
    shim = open(os.path.join(ROOT, "rust", "shim.rs")).read()
    rust = open(os.path.join(ROOT, "rust", "srx_sys.rs")).read()
    declared = set(re.findall(r"pub fn (srx_\w+)\(", rust))
    start = shim.index("pub struct PcaModel")
    end = shim.index("fn attach_pca_results", start) if "fn attach_pca_results" in shim[start:] else len(shim)
    body = shim[start:end]
    called = set(re.findall(r"\b(srx_\w+)\s*\(", body))
    assert {"srx_pca_model_from_result", "srx_pca_model_create", "srx_pca_model_info", "srx_pca_model_free",
            "srx_pca_transform"} <= called
    assert called <= declared, called - declared
    for sig in ("pub fn from_adata(adata: &IMAnnData) -> anyhow::Result<PcaModel>",
                "pub fn transform(&self, adata: &IMAnnData) -> anyhow::Result<Array2<f64>>"):
        assert sig in body, sig
    # every srx_ call anywhere in the shim is declared
    assert set(re.findall(r"\b(srx_\w+)\s*\(", shim)) <= declared


def test_model_kernels_do_not_spill_registers(tmp_path):
    """The same method as test_hot_kernels_do_not_spill_registers: the gfx950 code-object metadata of the model kernels shows
    no VGPR spill and no scratch."""
    from singlerust_amd import build
    csrc = os.path.join(ROOT, "singlerust_amd", "csrc")
    out = str(tmp_path / "pca_solve.s")
    subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(csrc, "pca_solve.hip")], stderr=subprocess.DEVNULL)
    meta = open(out).read()
    for kname in ("k_sel_slots", "k_model_panel", "k_model_gatherIfE", "k_model_gatherIdE"):
        m = re.search(r"\.name:\s+(\S*%s\S*)\n(.*?)\.wavefront_size" % re.escape(kname), meta, flags=re.S)
        assert m, f"{kname} not found"
        body = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        assert spill == 0 and scratch == 0, f"{m.group(1)}: {spill} spilled VGPRs, {scratch} B of scratch"


def _compile(tmp_path):
    exe = str(tmp_path / "pca_transform_test")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
           os.path.join(ROOT, "tests", "cpp", "pca_transform_test.cpp"), "-o", exe,
           "-L" + LIBDIR, "-lsrx_hip", "-Wl,-rpath," + LIBDIR]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_transform_test_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch
    exe = _compile(tmp_path)
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    assert "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_cpp_transform_self_projection(tmp_path):
    exe = _compile(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout

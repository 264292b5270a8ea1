"""Regress out / scale / clip / PCA without a GPU: the numpy restatement (regress_ref.py) against a 60-digit `decimal` known answer
(golden/kat_regress.json) and against sklearn's LinearRegression, the properties of the reference, the input conditions every GPU
test relies on (eigenvalue gaps, distance from the clip value, a clipped zero entry), the new symbols bound in every layer with
the struct layout gcc gives them, NULL arguments refused with nothing written, and the gfx950 listings of the kernels of
regress.hip free of register spills and scratch, with no floating-point atomic in the file."""
import ctypes as C
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import pearson_pca_ref as P
import regress_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srx_regress_fit", "srx_regress_sums", "srx_regress_residuals", "srx_regress_gram", "srx_pca_regress")
# the two chunk kernels are the dense route's templates (dense_pca_internal.hpp), compiled here with regress's element
KERNELS = ("k_dense_fill", "k_dense_stored", "k_rg_wsum", "k_rg_wsum_reduce")
# the instantiations: the fill with and without the clip counters, the stored pass also per value storage
INSTANCES = {"k_dense_fill": 2, "k_dense_stored": 4, "k_rg_wsum": 1, "k_rg_wsum_reduce": 1}
PRODUCTS = r"k_dense_(syrk|colsum|finish|scores)"
LD_EPS = float(np.finfo(np.longdouble).eps)


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def test_reference_against_the_decimal_known_answer():
    doc = json.load(open(os.path.join(G.GOLD, "kat_regress.json")))
    X = np.array([[float(v) for v in row] for row in doc["x"]])
    cov = np.array([float(v) for v in doc["cov"]]).reshape(-1, 1)
    e = doc["expected"]
    ld = lambda v: np.array(v, dtype=object).astype(str).astype(np.longdouble)
    ref = G.evaluate(X, cov, True, float(doc["max_value"]))
    close = lambda got, want, scale=1.0: np.all(np.abs(got - want) <= 64 * LD_EPS * (scale + np.abs(want)))
    assert close(ref["cbar"][0], ld(e["cbar"])) and close(ref["A"][0, 0], ld(e["A"]))
    assert close(ref["xbar"], ld(e["xbar"])) and close(ref["W"][0], ld(e["W"]), 1e3) and close(ref["beta"][0], ld(e["beta"]))
    assert close(ref["r"], ld(e["r"])) and close(ref["s"], ld(e["s"])) and close(ref["z"], ld(e["z"]))
    z = ld(e["z"])
    assert (np.abs(z) == float(doc["max_value"])).any() and np.all(z[:, 2] == 0) and ld(e["s"])[2] == 1       # clip active; constant gene
    f64 = G.evaluate(X, cov, True, float(doc["max_value"]), np.float64)
    assert np.all(np.abs(f64["z"] - z.astype(np.float64)) <= 64 * G.U * (1 + np.abs(z.astype(np.float64))))


def test_reference_residuals_are_sklearns():
    from sklearn.linear_model import LinearRegression
    X, cov = G.planted()["X"][:, :64], G.planted_covariates(2)
    r = np.asarray(G.evaluate(X, cov, False, 0.0)["r"], dtype=np.float64)
    want = X - LinearRegression().fit(cov, X).predict(cov)
    err = float(np.abs(r - want).max())
    print("reference against sklearn: %.2e" % err)
    assert err <= 1e-13
    assert np.linalg.cond(np.corrcoef(cov.T)) < 1.1


def test_reference_properties():
    X, genes, const_pos = G.walk_case(63, 17)
    X = X[:, genes.astype(np.int64)]
    assert const_pos is not None and (X[:, const_pos] == 1.5).all() and (X == 0).all(axis=0).any()
    cov = G.walk_covariates(X, 3)
    ref = G.evaluate(X, cov)
    r, ct = ref["r"], ref["ct"]
    assert np.all(np.abs(ct.T @ r) <= 64 * G.U * (np.abs(ct).T @ np.abs(r) + 1e-300))            # normal equations
    assert np.all(np.abs(r.sum(axis=0)) <= 64 * G.U * np.abs(r).sum(axis=0))
    flat = ref["const"]
    assert flat.sum() == 2 and np.all(r[:, flat] == 0) and np.all(ref["s"][flat] == 1) and np.all(ref["z"][:, flat] == 0)
    ss = (np.asarray(ref["z"], dtype=np.float64)[:, ~flat] ** 2).sum(axis=0) / (X.shape[0] - 1)
    assert np.allclose(ss, 1.0, rtol=1e-12)
    with pytest.raises(G.Refused) as e:                                                          # a constant, then a collinear covariate
        G.evaluate(X, np.stack([cov[:, 0], np.full(63, 2.0)], axis=1))
    assert e.value.args == (1, "constant")
    with pytest.raises(G.Refused) as e:
        G.evaluate(X, np.stack([cov[:, 0], cov[:, 1], 2 * cov[:, 0] - 3 * cov[:, 1]], axis=1))
    assert e.value.args == (2, "collinear")


# ---- the input conditions of the GPU tests ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_reference(k, p, max_value):
    return G.evaluate(G.planted()["X"][:, :k], G.planted_covariates(p, G.PCA_SEED), True, max_value)


@pytest.mark.parametrize("k,p,max_value", G.PCA_CASES)
def test_pca_cases_keep_their_eigenvalues_apart(k, p, max_value):
    w = P.pca(np.asarray(planted_reference(k, p, max_value)["z"], dtype=np.float64), 50)["values"]
    for n_pc in (2, 5, 50):
        gap = P.min_relative_gap(w, n_pc)
        print("k=%d p=%d max_value=%g n_pc=%d: smallest relative gap %.2e" % (k, p, max_value, n_pc, gap))
        assert gap >= 1e-3


@pytest.mark.parametrize("k,p,max_value", [(k, p, mv) for k in (64, 240) for p in (0, 2) for mv in (0.25, 2.0, 3.0)])
def test_clipped_cases_stay_away_from_the_clip_value(k, p, max_value):
    ref = planted_reference(k, p, max_value)
    near = float(np.min(np.abs(np.abs(np.asarray(ref["z_raw"], dtype=np.float64)) - max_value)))
    zeros = G.planted()["X"][:, :k] == 0
    print("k=%d p=%d max_value=%g: %.1f %% clipped, nearest entry %.2e from the clip value, %d clipped zero entries"
          % (k, p, max_value, 100 * ref["clipped"].mean(), near, int((ref["clipped"] & zeros).sum())))
    assert near >= 1e-9 and ref["clipped"].any()
    if max_value == 0.25:
        assert (ref["clipped"] & zeros).any()                                                    # the fill kernel's clip is exercised


# ---- the layers ------------------------------------------------------------------------------------------------------------------------
def test_regress_symbols_are_exported_and_bound():
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
    for s in ("SrxRegressOpts", "SrxRegressInfo"):
        assert "pub struct %s" % s in rust, s
    for fn in ("regress_fit", "regress_out", "scale", "regress_gram", "pca_regress_scale"):
        assert callable(getattr(processing, fn)), fn
    assert re.search(r"pub fn pca_regress_scale\b", shim) and re.search(r"\bpca_regress_scale\(", mirror)
    # additive: the ABI version and the number of profiling classes stay
    assert re.search(r"#define\s+SRX_ABI_VERSION\s+6\b", header) and lib.srx_abi_version() == 6
    assert re.search(r"SRX_K_COUNT_ = 13\b", header)
    assert "regress.hip" in build.SOURCES and "dense_pca.hip" in build.SOURCES
    assert re.search(r"regress", header, flags=re.I) and "max_value" in header


def test_regress_source_has_no_floating_point_atomic_and_no_contraction():
    read = lambda name: open(os.path.join(ROOT, "singlerust_amd", "csrc", name)).read()
    src, route, dense = read("regress.hip"), read("dense_pca_internal.hpp"), read("dense_pca.hip")
    assert "fp contract(off)" in src and '#include "dense_pca_internal.hpp"' in src
    # the counts of clipped pairs are the only atomics of the route: in the chunk templates, integers, cast where they are added
    assert "atomicAdd" not in src and "atomicAdd" not in dense
    for text in (src, route, dense):
        assert not re.search(r"unsafeAtomicAdd|__hip_atomic|atomicExch|atomicCAS|atomicMax|atomicMin", text)
        assert not re.search(r"\b(double|float)\s*\*\s*(__restrict__\s*)?cnt\b", text)
    adds = re.findall(r"atomicAdd\(([^;]*);", route)
    assert len(adds) == 3 and all("(unsigned long long)" in a for a in adds), adds
    assert "dense_make_chunk<RgArgs, COUNT>" in src and "rg_maker<true>" in src and "rg_maker<false>" in src
    # the products are dense_pca.hip's, once: this caller neither defines nor launches one
    assert not re.search(r"__global__[^;{]*\b" + PRODUCTS, src) and not re.search(r"hipLaunchKernelGGL\(\(?" + PRODUCTS, src)
    assert len(re.findall(r"__global__[^;{]*\b" + PRODUCTS, dense)) == 6


@pytest.mark.parametrize("cname,struct,size", [("srx_regress_opts", "RegressOpts", 72), ("srx_regress_info", "RegressInfo", 160)])
def test_regress_struct_layout_matches_header(tmp_path, cname, struct, size):
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


def test_null_arguments_are_refused_and_nothing_is_written():
    from singlerust_amd import _ffi
    lib = _ffi.lib()
    g, cov = np.array([0, 1], dtype=np.uint64), np.ones((4, 1))
    out, info = np.full(8, -7.0), _ffi.RegressInfo()
    info.min_pivot = -7.0
    p, gp, cp, ip = _ffi.ptr(out), _ffi.ptr(g), _ffi.ptr(cov), C.byref(info)
    assert lib.srx_regress_fit(None, gp, 2, cp, 1, None, p, p, p, ip) == _ffi.E_ARG
    assert lib.srx_last_error(None)
    assert lib.srx_regress_sums(None, gp, 2, cp, 1, None, p, p, p, ip) == _ffi.E_ARG
    assert lib.srx_regress_residuals(None, gp, 2, cp, 1, None, p, ip) == _ffi.E_ARG
    assert lib.srx_regress_gram(None, gp, 2, cp, 1, None, p, p, ip) == _ffi.E_ARG
    assert lib.srx_pca_regress(None, gp, 2, cp, 1, None, p, None, None, None, None, ip) == _ffi.E_ARG
    assert np.all(out == -7.0) and info.min_pivot == -7.0
    from singlerust_amd.memory.processing import regress
    with pytest.raises(ValueError):
        regress._covariates(None, np.ones((3, 2)), 4)
    assert regress._covariates(None, None, 4).shape == (4, 0) and regress._covariates(None, np.ones(4), 4).shape == (4, 1)


def test_regress_kernels_do_not_spill_registers(tmp_path):
    """The gfx950 code-object metadata of every kernel of regress.hip, its instantiations of the two chunk kernels included,
    shows no VGPR / SGPR spill and no scratch."""
    from singlerust_amd import build
    out = str(tmp_path / "regress.s")
    subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "singlerust_amd", "csrc", "regress.hip")], stderr=subprocess.DEVNULL)
    text = open(out).read()
    count = {k: 0 for k in KERNELS}
    for m in re.finditer(r"\.name:\s+(\S*k_(?:rg|dense)_\S*)\n(.*?)\.wavefront_size", text, flags=re.S):
        body = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        assert spill == 0 and sspill == 0 and scratch == 0, f"{m.group(1)}: {spill} / {sspill} spilled V/SGPRs, {scratch} B of scratch"
        hit = [k for k in KERNELS if re.search(r"\d%s(I|E|\b)" % k, m.group(1))]
        assert len(hit) == 1, m.group(1)
        count[hit[0]] += 1
    assert count == INSTANCES, count
    body = re.search(r"^_ZN3srx\d+k_rg_wsumE\w*:[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.S | re.M).group(1)
    assert "v_fma_f64" not in body and "v_mul_f64" in body and "v_add_f64" in body           # no contraction in the sums

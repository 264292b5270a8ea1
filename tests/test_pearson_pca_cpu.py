"""PCA of the Pearson residuals without a GPU: the numpy restatement (pearson_pca_ref.py) against a `decimal` evaluation of the
covariance of a 5 x 3 count matrix under both totals, the planted input's eigenvalue gaps, the new symbols bound in every layer
with the struct layout gcc gives them, NULL arguments refused with nothing written, and the gfx950 listings of the kernels of
pearson_pca.hip and of the dense route it calls (dense_pca.hip) free of register spills and scratch, with the two products on the
f64 matrix cores."""
import ctypes as C
import decimal
import os
import re
import subprocess

import numpy as np
import pytest

import pearson_pca_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srx_pca_pearson", "srx_pearson_gram")
# per translation unit; the two chunk kernels are templates on the caller's element and are compiled with the caller
KERNELS = {"pearson_pca.hip": ("k_pp_row_sums", "k_pp_gene_sums", "k_dense_fill", "k_dense_stored"),
           "dense_pca.hip": ("k_dense_syrk", "k_dense_syrk_reduce", "k_dense_colsum", "k_dense_colsum_reduce", "k_dense_finish",
                             "k_dense_scores")}
# the instantiations of pearson_pca.hip: the row sums and the stored pass per value storage, no counting form
INSTANCES = {"k_pp_row_sums": 2, "k_pp_gene_sums": 1, "k_dense_fill": 1, "k_dense_stored": 2}
MFMA_KERNELS = ("k_dense_syrk", "k_dense_scores")
PRODUCTS = r"k_dense_(syrk|colsum|finish|scores)"

X53 = np.array([[3, 0, 1], [0, 2, 5], [7, 1, 0], [1, 1, 1], [0, 4, 2]], dtype=np.int64)


def decimal_covariance(X, genes, theta, clip, totals, center):
    """C = (Z^T Z - n m m^T) / (n - 1) of the definition in 60-digit decimal arithmetic: nothing shared with numpy."""
    D = decimal.Decimal
    with decimal.localcontext() as c:
        c.prec = 60
        n = X.shape[0]
        cols = list(genes) if totals == "selected" else list(range(X.shape[1]))
        r = [sum(D(int(X[i, j])) for j in cols) for i in range(n)]
        g = [sum(D(int(X[i, j])) for i in range(n)) for j in range(X.shape[1])]
        T = sum(r)
        cl = D(n).sqrt() if clip is None else D(clip)
        Z = [[D(0)] * len(genes) for _ in range(n)]
        for i in range(n):
            for a, j in enumerate(genes):
                mu = r[i] * g[j] / T
                if mu > 0:
                    s = (mu + mu * mu / D(theta)).sqrt() if theta != float("inf") else mu.sqrt()
                    Z[i][a] = min(max((D(int(X[i, j])) - mu) / s, -cl), cl)
        k = len(genes)
        m = [sum(Z[i][a] for i in range(n)) / n if center else D(0) for a in range(k)]
        return [[(sum(Z[i][a] * Z[i][b] for i in range(n)) - n * m[a] * m[b]) / (n - 1) for b in range(k)] for a in range(k)], Z


@pytest.mark.parametrize("totals", P.TOTALS)
@pytest.mark.parametrize("theta,clip", [(100.0, None), (10.0, 1.0), (float("inf"), None)], ids=["default", "theta10-clip1", "poisson"])
def test_reference_covariance_against_decimal(totals, theta, clip):
    genes = [2, 0]                                   # two of the three genes, unsorted: the two totals differ
    for center in (True, False):
        want, Zd = decimal_covariance(X53, genes, theta, clip, totals, center)
        Z = P.residuals(X53, genes, theta, clip, totals)
        eps = float(np.finfo(np.longdouble).eps)
        zd = np.array([[np.longdouble(str(v)) for v in row] for row in Zd])
        assert np.all(np.abs(Z - zd) <= 8 * eps * (1 + np.abs(zd)))
        if clip is not None:
            assert (np.abs(zd) == clip).any()                       # the clip is active in this case
        got, _ = P.covariance(np.asarray(Z, dtype=np.float64), center)
        w = np.array([[float(v) for v in row] for row in want])
        assert np.all(np.abs(got - w) <= 64 * P.U * np.abs(Z).astype(np.float64).T @ np.abs(Z).astype(np.float64)), (got, w)


def test_the_two_totals_differ_and_agree_on_the_full_list():
    a = P.residuals(X53, [2, 0], totals="all")
    s = P.residuals(X53, [2, 0], totals="selected")
    assert np.abs(a - s).max() > 1e-3
    assert np.array_equal(P.residuals(X53, [0, 1, 2], totals="all"), P.residuals(X53, [0, 1, 2], totals="selected"))


def test_reference_pca_is_a_pca():
    Z = np.asarray(P.residuals(P.planted_counts(), P.planted_genes(64), totals="selected"), dtype=np.float64)
    r = P.pca(Z, 5)
    C, m = P.covariance(Z)
    V = r["components"]
    assert np.allclose(V.T @ V, np.eye(5), atol=1e-12) and np.allclose(C @ V, V * r["values"][:5], atol=1e-10)
    assert np.allclose(r["scores"].var(axis=0, ddof=1), r["values"][:5], rtol=1e-10)
    assert all(V[np.argmax(np.abs(V[:, c])), c] > 0 for c in range(5)) and abs(r["scores"].mean(axis=0)).max() < 1e-12


@pytest.mark.parametrize("k", [64, 240])
def test_planted_input_keeps_its_eigenvalues_apart(k):
    X = P.planted_counts()
    assert X.shape == P.PLANTED_SHAPE and np.array_equal(X, P.planted_counts()) and X.sum(axis=1).min() > 0
    genes = P.planted_genes(k)
    assert np.unique(genes).size == k and not np.all(np.diff(genes.astype(np.int64)) > 0)
    for totals in P.TOTALS:
        Z = P.residuals(X, genes, totals=totals, dtype=np.float64)
        for center in (True, False):
            w = P.pca(Z, 50, center)["values"]
            assert P.min_relative_gap(w, 50) >= 1e-3 and P.min_relative_gap(w, 2) >= 1e-3, (k, totals, center)


# ---- the layers ------------------------------------------------------------------------------------------------------------------------
def test_pearson_pca_symbols_are_exported_and_bound():
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
    for s in ("SrxPearsonPcaOpts", "SrxPearsonPcaInfo"):
        assert "pub struct %s" % s in rust, s
    assert _ffi.PEARSON_TOTALS_ALL == 0 and _ffi.PEARSON_TOTALS_SELECTED == 1
    assert callable(processing.pca_pearson_residuals) and callable(processing.pearson_gram)
    assert re.search(r"pub fn pca_pearson_residuals\b", shim) and re.search(r"\bpca_pearson_residuals\(", mirror)
    # additive: the ABI version and the number of profiling classes stay
    assert re.search(r"#define\s+SRX_ABI_VERSION\s+6\b", header) and lib.srx_abi_version() == 6
    assert re.search(r"SRX_K_COUNT_ = 13\b", header)
    assert "pearson_pca.hip" in build.SOURCES and "dense_pca.hip" in build.SOURCES
    read = lambda name: open(os.path.join(ROOT, "singlerust_amd", "csrc", name)).read()
    src, dense, route, shared = read("pearson_pca.hip"), read("dense_pca.hip"), read("dense_pca_internal.hpp"), read("pearson_internal.hpp")
    assert "fp contract(off)" in shared and '#include "pearson_internal.hpp"' in src and '#include "dense_pca_internal.hpp"' in src
    assert "fp contract(off)" in src and "fp contract(off)" in dense
    for text in (src, dense):
        assert not re.search(r"atomicAdd|unsafeAtomicAdd|__hip_atomic", text)         # no atomics at all: every sum has one owner
    # the chunk templates: only the counts of clipped pairs, integers, cast where they are added; Pearson instantiates neither
    assert not re.search(r"unsafeAtomicAdd|__hip_atomic|atomicExch|atomicCAS|atomicMax|atomicMin", route)
    adds = re.findall(r"atomicAdd\(([^;]*);", route)
    assert len(adds) == 3 and all("(unsigned long long)" in a for a in adds), adds
    assert not re.search(r"\b(double|float)\s*\*\s*(__restrict__\s*)?cnt\b", route)
    assert "dense_make_chunk<PpElem, false>" in src and "dense_make_chunk<PpElem, true>" not in src
    # the products are dense_pca.hip's, once: this caller neither defines nor launches one
    assert not re.search(r"__global__[^;{]*\b" + PRODUCTS, src) and not re.search(r"hipLaunchKernelGGL\(\(?" + PRODUCTS, src)
    assert len(re.findall(r"__global__[^;{]*\b" + PRODUCTS, dense)) == 6
    assert "residuals followed by a PCA" not in header and "batch_key" in header


@pytest.mark.parametrize("cname,struct,size", [("srx_pearson_pca_opts", "PearsonPcaOpts", 80), ("srx_pearson_pca_info", "PearsonPcaInfo", 152)])
def test_pearson_pca_struct_layout_matches_header(tmp_path, cname, struct, size):
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
    g = np.array([0, 1], dtype=np.uint64)
    out, info = np.full(4, -7.0), _ffi.PearsonPcaInfo()
    info.total = -7.0
    assert lib.srx_pca_pearson(None, _ffi.ptr(g), 2, None, _ffi.ptr(out), None, None, None, C.byref(info)) == _ffi.E_ARG
    assert lib.srx_last_error(None)
    assert lib.srx_pearson_gram(None, _ffi.ptr(g), 2, None, _ffi.ptr(out), None, C.byref(info)) == _ffi.E_ARG
    assert np.all(out == -7.0) and info.total == -7.0
    with pytest.raises(ValueError):
        from singlerust_amd.memory.processing import hvg
        hvg._pca_opts(100.0, None, "some", True, 0, 2)


def test_pearson_pca_kernels_do_not_spill_registers(tmp_path):
    """The gfx950 code-object metadata of every kernel of pearson_pca.hip (its instantiations of the two chunk kernels included)
    and of dense_pca.hip shows no VGPR / SGPR spill and no scratch, and the two products issue v_mfma_f64_16x16x4."""
    from singlerust_amd import build
    for source, kernels in KERNELS.items():
        out = str(tmp_path / (source + ".s"))
        subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                               os.path.join(ROOT, "singlerust_amd", "csrc", source)], stderr=subprocess.DEVNULL)
        text = open(out).read()
        count = {k: 0 for k in kernels}
        for m in re.finditer(r"\.name:\s+(\S*k_(?:pp|dense)_\S*)\n(.*?)\.wavefront_size", text, flags=re.S):
            body = m.group(2)
            spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
            sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1))
            scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
            assert spill == 0 and sspill == 0 and scratch == 0, f"{m.group(1)}: {spill} / {sspill} spilled V/SGPRs, {scratch} B of scratch"
            hit = [k for k in kernels if re.search(r"\d%s(I|E|\b)" % k, m.group(1))]
            assert len(hit) == 1, m.group(1)                                          # no kernel of the route is outside the lists
            count[hit[0]] += 1
        if source == "pearson_pca.hip":
            assert count == INSTANCES, count
        else:
            assert all(c == 1 for c in count.values()), count
            for k in MFMA_KERNELS:
                body = re.search(r"^_ZN3srx\d+%sE\w*:[^\n]*\n(.*?)^\.Lfunc_end" % k, text, flags=re.S | re.M).group(1)
                assert body.count("v_mfma_f64_16x16x4") >= 4, k

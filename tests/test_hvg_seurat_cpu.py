"""Seurat v3 gene selection without a GPU: the numpy restatement (hvg_seurat_ref.py) against the decimal known answer and, for
the loess fit, against np.polyfit; the degree rule on the moments against a count of distinct abscissae; the integer logic by
hand; the new symbols bound in every layer with the struct layout gcc gives them; NULL arguments refused through the loaded
library; the new kernels' gfx950 listings free of register spills and scratch."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import hvg_seurat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srx_select_hvg_seurat_v3", "srx_loess_direct", "srx_clipped_group_moments")
KERNELS = ("k_sv_stats", "k_sv_scatter", "k_sv_loess", "k_sv_clip", "k_sv_nv", "k_sv_combine", "k_sv_unfix",
           "k_sv_negate")


def kat():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "kat_seurat_v3.json")))


def planted():
    z = np.load(os.path.join(ROOT, "tests", "golden", "planted_600x240.npz"))
    return sp.csr_matrix((z["values"], z["indices"].astype(np.int64), z["indptr"].astype(np.int64)), shape=(int(z["n_rows"]), int(z["n_cols"])))


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def test_reference_against_the_known_answer():
    """The f64 restatement against the 60-digit decimal evaluation.  Bounds: mean and var are a handful of correctly rounded
    operations on exact sums (4 ulp); a fit over at most five weighted points has normal equations of condition below 1e3, so
    e is within 1e3 x 2^-52 < 1e-12; 10^e turns an absolute error d of e into a relative ln(10) d of reg_var, clip and nv."""
    k = kat()
    r = R.run(np.array(k["X"], np.float64), k["batch"], k["n_batches"], k["n_top"], k["span"])
    want = {key: np.array([[float(s) for s in row] for row in k[key]]) for key in ("mean", "var", "fitted", "clip", "clip_sum", "clip_sumsq", "nv")}
    eps = 2.0 ** -52
    for key in ("mean", "var"):
        assert np.all(np.abs(r[key] - want[key]) <= 4 * eps * np.abs(want[key])), key
    assert np.all(np.abs(r["fitted"] - want["fitted"]) <= 1e-12)
    for key in ("clip", "clip_sum", "clip_sumsq", "nv"):
        assert np.all(np.abs(r[key] - want[key]) <= 3e-12 * np.abs(want[key])), key
    assert k["clipped_entries"] >= 1 and np.any(r["clip_sum"] != R.unfix(R.grouped_int(np.array(k["X"]), k["batch"], 2, r["scales"])[0], r["scales"][0]))
    assert r["rank"].tolist() == k["rank"] and r["nbatches"].tolist() == k["nbatches"]
    assert [None if np.isnan(v) else v for v in r["median"]] == k["median"]
    assert r["selected"].tolist() == k["selected"]
    assert R.select(r["median"], r["nbatches"], k["n_top"], paper=True).tolist() == k["selected_paper"] != k["selected"]
    for key in ("means", "variances", "variances_norm"):
        w = np.array([float(s) for s in k[key]])
        assert np.all(np.abs(r[key] - w) <= 3e-12 * np.abs(w)), key


@pytest.mark.parametrize("case", R.loess_cases(), ids=lambda c: c[0])
def test_loess_against_polyfit_and_the_degree_rule(case):
    """np.polyfit (an SVD of the weighted Vandermonde matrix) on every window with three distinct abscissae or more.  Both solve
    the same least-squares problem; the normal equations square a condition that stays below 1e2 for tricube windows in
    t in (-1, 1): 1e4 x 2^-52 x |y| (below 5) is 1e-11.  And the degree the rule on the weighted moments chooses is
    min(2, distinct weighted abscissae - 1) on every point of every case."""
    _, x, y, span = case
    deg = np.full(x.size, -1)
    fit = R.loess_direct(x, y, span, degrees=deg)
    want_deg, distinct = R.loess_degree(x, span)
    assert np.array_equal(deg, want_deg), (deg, want_deg)
    pf = R.loess_polyfit(x, y, span)
    ok = np.isfinite(pf)
    assert np.array_equal(ok, distinct >= 3)
    assert np.all(np.abs(pf[ok] - fit[ok]) <= 1e-11)
    # a fit of degree 0 is the mean of the weighted ordinates; q = 1 returns y where x is not repeated
    if R.window(x.size, span) == 1 and np.unique(x).size == x.size:
        assert np.array_equal(fit, y)


def test_loess_cases_hold_what_the_gpu_tests_need():
    cases = {c[0]: c for c in R.loess_cases()}
    assert {int(n.split("_")[0][1:]) for n in cases if re.match(r"m\d+_", n)} == set(R.LOESS_SIZES)
    assert {1, 2, 3, 4, 63, 64, 65, 257} <= set(R.LOESS_SIZES) and max(R.LOESS_SIZES) > 1024
    for m in R.LOESS_SIZES:
        if m >= 3:
            assert R.window(m, cases["m%d_q1" % m][3]) == 1 and R.window(m, cases["m%d_q2" % m][3]) == 2
        assert R.window(m, 1.0) == m
    _, x, _, span = cases["run_longer_than_q"]
    assert (x == 0.5).sum() > R.window(x.size, span)
    _, x, _, span = cases["run_of_exactly_q"]
    assert (x == 0.5).sum() == R.window(x.size, span)
    assert np.unique(cases["two_values_span1"][1]).size == 2
    _, x, y, _ = cases["tied_points"]
    tied = np.flatnonzero(x == x[40])
    assert tied.size == 4 and np.unique(y[tied]).size == 4
    assert any(np.any(np.diff(c[1]) < 0) for c in cases.values())                     # x comes unsorted


def test_integer_logic_by_hand():
    nv = np.array([[3.0, 5.0, 5.0, 1.0], [2.0, 2.0, 9.0, 2.0]])
    rank = R.ranks_of(nv)
    assert rank.tolist() == [[2, 0, 1, 3], [1, 2, 0, 3]]
    nb, med = R.combine(rank, 2)
    assert nb.tolist() == [1, 1, 2, 0] and med[:3].tolist() == [1.0, 0.0, 0.5] and np.isnan(med[3])
    assert R.final_order(med, nb).tolist() == [1, 2, 0, 3] and R.final_order(med, nb, paper=True).tolist() == [2, 1, 0, 3]
    assert R.select(med, nb, 9).size == 4 and R.select(med, nb, 2).tolist() == [1, 2]
    r4 = np.tile(np.arange(6), (4, 1))
    r4[:, 0] = [0, 4, 2, 5]
    nb3, med3 = R.combine(r4, 5)                                                      # odd count: the middle one
    assert nb3[0] == 3 and med3[0] == 2.0 and nb3[5] == 0 and np.isnan(med3[5])
    assert R.window(240, 0.3) == 72 and R.window(3, 0.3) == 1 and R.window(10, 1.0) == 10
    assert R.fixed([0.5, 1.5, 2.5, -0.5], 0).tolist() == [0, 2, 2, 0]                 # ties to even


def test_planted_fixture_has_ties_and_clear_cuts():
    """What the whole-selection GPU test relies on: tied nv values in every batch, and a relative gap of the one-batch nv at
    the cuts 20, 40 and 60 that no rounding difference reaches."""
    X = planted()
    r1 = R.run(X, None, 1, 40)
    s = np.sort(r1["nv"][0])[::-1]
    for cut in (20, 40, 60):
        assert (s[cut - 1] - s[cut]) / s[cut - 1] > 1e-3
    b = R.hashed_batches(X.shape[0], 3)
    assert np.bincount(b).min() > 150
    r3 = R.run(X, b, 3, 40)
    for row in list(r3["nv"]) + [r1["nv"][0]]:
        assert np.unique(row).size < row.size
    assert 0 < (r3["nbatches"] == 0).sum() < X.shape[1] and (r3["nbatches"] == 3).sum() > 0
    assert np.any(r3["median"] % 1 == 0.5)                                            # an even count whose middle ranks differ


# ---- the layers --------------------------------------------------------------------------------------------------------------------
def test_seurat_symbols_are_exported_and_bound():
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
    for s in ("SrxSeuratV3Opts", "SrxSeuratV3Tables", "SrxSeuratV3Info"):
        assert "pub struct %s" % s in rust, s
    assert callable(processing.highly_variable_genes_seurat_v3)
    assert re.search(r"pub fn highly_variable_genes_seurat_v3\b", shim) and re.search(r"\bhighly_variable_genes_seurat_v3\(", mirror)
    # additive: the ABI version and the number of profiling classes stay
    assert re.search(r"#define\s+SRX_ABI_VERSION\s+6\b", header) and lib.srx_abi_version() == 6
    assert re.search(r"SRX_K_COUNT_ = 13\b", header)
    assert "hvg_seurat.hip" in build.SOURCES and not any("fast-math" in f for f in build.FLAGS)
    src = open(os.path.join(ROOT, "singlerust_amd", "csrc", "hvg_seurat.hip")).read()
    markers = open(os.path.join(ROOT, "singlerust_amd", "csrc", "markers.hip")).read()
    assert "fp contract(off)" in src
    # the walk is markers.hip's, shared and not copied; the ranking is select.hip's; no floating-point atomic
    assert "k_mk_walk" not in src and "markers_clipped_walk(" in src and "markers_moments(" in src
    assert len(re.findall(r"__global__[^;{]*\bk_mk_walk\b", markers)) == 1 and '#include "markers_internal.hpp"' in markers
    assert "rank_keys_device(ctx" in src and "pick_top(ctx" in src and "value_scan(m, " in src
    assert "rank_keys_device(srx_ctx*" not in src                             # declared once, in pca_internal.hpp
    assert not re.search(r"atomicAdd\([^;]*\(double\)|unsafeAtomicAdd|atomicAdd_f|__hip_atomic_fetch_add", src)
    # the definition names its departures
    block = header[header.index("as Seurat v3 chooses them"):header.index("srx_seurat_v3_opts")]
    for word in ("Departures from scanpy", '"direct"', '"interpolate"', "unstable argsort", "float32", "2^-33"):
        assert word in block, word


@pytest.mark.parametrize("cname,struct,size", [("srx_seurat_v3_opts", "SeuratV3Opts", 16), ("srx_seurat_v3_tables", "SeuratV3Tables", 112),
                                               ("srx_seurat_v3_info", "SeuratV3Info", 88)])
def test_seurat_struct_layout_matches_header(tmp_path, cname, struct, size):
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


def test_null_arguments_are_refused_without_a_device():
    """A NULL handle or context is SRX_E_ARG with a message and nothing written, through the loaded library."""
    from singlerust_amd import _ffi
    lib = _ffi.lib()
    idx, n_out, col = np.full(4, 77, dtype=np.uint64), C.c_uint64(99), np.full(4, -7.0)
    tables = _ffi.SeuratV3Tables()
    tables.means = _ffi.ptr(col)
    info = _ffi.SeuratV3Info()
    info.max_abs = -7.0
    assert lib.srx_select_hvg_seurat_v3(None, 2, None, 1, None, _ffi.ptr(idx), C.byref(n_out), C.byref(tables), C.byref(info)) == _ffi.E_ARG
    assert lib.srx_last_error(None)
    assert lib.srx_loess_direct(None, _ffi.ptr(col), _ffi.ptr(col), 4, 0.3, _ffi.ptr(col)) == _ffi.E_ARG and lib.srx_last_error(None)
    mi = _ffi.MarkersInfo()
    assert lib.srx_clipped_group_moments(None, None, 1, _ffi.ptr(col), _ffi.ptr(col), _ffi.ptr(col), C.byref(mi)) == _ffi.E_ARG
    assert lib.srx_last_error(None)
    assert np.all(idx == 77) and n_out.value == 99 and np.all(col == -7.0) and info.max_abs == -7.0 and mi.n_rows == 0


def test_python_wrapper_refuses_an_unknown_flavor():
    from singlerust_amd.memory.processing import highly_variable_genes_seurat_v3
    with pytest.raises(ValueError):
        highly_variable_genes_seurat_v3(None, 10, flavor="seurat")


def _kernel_meta(tmp_path, source, pattern):
    from singlerust_amd import build
    out = str(tmp_path / (source + ".s"))
    subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "singlerust_amd", "csrc", source)], stderr=subprocess.DEVNULL)
    found = []
    for m in re.finditer(r"\.name:\s+(\S*%s\S*)\n(.*?)\.wavefront_size" % pattern, open(out).read(), flags=re.S):
        body = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        assert spill == 0 and sspill == 0 and scratch == 0, f"{m.group(1)}: {spill} / {sspill} spilled V/SGPRs, {scratch} B of scratch"
        found.append(m.group(1))
    return found


def test_seurat_kernels_do_not_spill_registers(tmp_path):
    """The gfx950 code-object metadata of every kernel of hvg_seurat.hip, and of every instantiation of the walk (the clipped
    ones are new; the unclipped ones keep their count), shows no VGPR / SGPR spill and no scratch."""
    found = _kernel_meta(tmp_path, "hvg_seurat.hip", "k_sv_")
    seen = {k for k in KERNELS if any(re.search(r"\d%s(I|E|\b)" % k, name) for name in found)}
    assert seen == set(KERNELS), set(KERNELS) - seen
    assert len(found) == len(KERNELS)          # none is a template; the value check and the pick are matrix.hip's and select.hip's
    walks = _kernel_meta(tmp_path, "markers.hip", "k_mk_walk")
    # f32 / f64 values x 16-bit mirror / 32-bit indices, unclipped and clipped; the counting pass per index form
    assert len(walks) == 4 + 4 + 2, walks


def test_shim_struct_literals_name_fields_of_the_generated_bindings():
    """There is no rustc where this is built, so nothing compiles rust/shim.rs.  Every field that a struct literal of a
    generated `Srx*` type names in the shim, and every field assigned through a variable declared with such a type, must be a
    field of that struct in rust/srx_sys.rs (the generator drops a trailing underscore: `reserved_` becomes `reserved`)."""
    shim = open(os.path.join(ROOT, "rust", "shim.rs")).read()
    rust = open(os.path.join(ROOT, "rust", "srx_sys.rs")).read()
    structs = {m.group(1): set(re.findall(r"pub (\w+):", m.group(2)))
               for m in re.finditer(r"pub struct (Srx\w+) \{[^\n]*\n(.*?)\n\}", rust, flags=re.S)}
    assert {"SrxSeuratV3Opts", "SrxSeuratV3Tables", "SrxSeuratV3Info", "SrxKnnOpts"} <= set(structs)
    literals = 0
    for m in re.finditer(r"\b(Srx\w+) \{([^{}]*)\}", shim):
        name, body = m.group(1), m.group(2)
        if name not in structs:
            continue
        fields = re.findall(r"(?:^|,)\s*(\w+)\s*:", body)
        assert fields and not [f for f in fields if f not in structs[name]], (name, fields)
        literals += 1
    assert literals >= 10 and re.search(r"SrxSeuratV3Opts \{[^{}]*\breserved: 0", shim)
    assigned = 0
    for m in re.finditer(r"let mut (\w+): (Srx\w+) = ", shim):
        var, name = m.group(1), m.group(2)
        if name not in structs:
            continue
        body = shim[m.end():shim.index("\n    }\n", m.end())]                          # to the end of the method
        for f in re.findall(r"\b%s\.(\w+)\s*=[^=]" % var, body):
            assert f in structs[name], (name, var, f)
            assigned += 1
    assert assigned >= 5
    # the listing in INTEGRATION.md is the shim's text (test_abi_cpu.py holds every fenced block to that)
    assert "reserved_" not in open(os.path.join(ROOT, "INTEGRATION.md")).read().split("## 2o.")[1].split("## 3.")[0]

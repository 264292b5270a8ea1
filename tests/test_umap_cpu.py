"""The UMAP layout without a GPU: the host restatement (tests/umap_ref.py) against hand-computed known answers and its own
schedule identities, srx_umap_fit_ab (host only) against scipy.optimize.curve_fit, the golden 12-vertex graph, the new symbols
bound in every layer with the struct layout gcc gives them, a loud failure without a device, and the kernels' gfx950 listings
free of register spills and scratch."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import umap_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srx_umap", "srx_umap_csr", "srx_graph_embedding_fetch", "srx_umap_fit_ab")
KERNELS = ("k_umap_wmax", "k_umap_active", "k_umap_init_random", "k_umap_absmax", "k_umap_init_pca", "k_umap_epoch")


# ---- 1. the reference checks itself -------------------------------------------------------------------------------------------
def test_hash_against_known_answers():
    """mix() and the negative-sample targets of the vectorised reference equal the answers worked out in Python integers."""
    kat = ref.golden()["hash"]
    assert ref.mix_int(0) == 0 and ref.mix_int(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF      # splitmix64's first output for seed 0
    for z, want in kat["mix"]:
        assert int(ref.mix(np.array([int(z)], dtype=np.uint64))[0]) == int(want) == ref.mix_int(int(z))
    for c in kat["targets"]:
        seed, t, nnz, e, R, p, n = int(c["seed"]), c["t"], c["nnz"], c["e"], c["R"], c["p"], c["n"]
        got = ref.negative_targets(seed, t, nnz, np.array([e], dtype=np.uint64), R, n)
        assert got.shape == (1, R) and int(got[0, p]) == c["k"] == ref.target_int(seed, t, nnz, e, R, p, n)
        assert 0 <= c["k"] < n
    y = ref.random_start(5, 2, 9)
    z = ref.mix_int(9 + 0x9E3779B97F4A7C15 * 4)                                    # coordinate c = 3
    assert y[1, 1] == -10.0 + 20.0 * ((z >> 11) * 2.0 ** -53) and (np.abs(y) <= 10).all()


def test_schedule_identities():
    rng = np.random.default_rng(0)
    for E in (1, 3, 200, 500):
        w = np.r_[rng.random(400), 1.0, 1.0 / E, np.nextafter(1.0 / E, 0.0), 1e-7, 0.999999]
        r = ref.ratios(w)
        hits = sum(ref.sampled(r, t).astype(np.int64) for t in range(1, E + 1))
        assert np.array_equal(hits, np.floor(np.float64(E) * r).astype(np.int64))   # sum_t [sampled] == floor(E r_e)
        assert hits[400] == E and all(ref.sampled(r, t)[400] for t in range(1, E + 1))      # r = 1: every epoch
        never = r < 1.0 / E
        assert never[[402, 403] if E > 1 else [403]].all() and (hits[never] == 0).all()      # r < 1 / E: never


# ---- 2. the curve fit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread,min_dist", [(1.0, 0.1), (1.0, 0.5), (1.0, 0.0), (2.0, 0.25)])
def test_fit_ab_against_scipy(spread, min_dist):
    from scipy.optimize import curve_fit

    from singlerust_amd.memory.processing import fit_ab
    a, b = fit_ab(spread, min_dist)
    x, y = ref.curve_target(spread, min_dist)
    (sa, sb), _ = curve_fit(ref.curve, x, y)
    rss = lambda p, q: float(((ref.curve(x, p, q) - y) ** 2).sum())
    print("library", a, b, "scipy", sa, sb, "rss", rss(a, b), rss(sa, sb))
    assert rss(a, b) <= rss(sa, sb) + 1e-12                                        # an optimality condition, not a tolerance
    assert abs(a - sa) <= 1e-4 * abs(sa) and abs(b - sb) <= 1e-4 * abs(sb)
    if (spread, min_dist) == (1.0, 0.1):
        assert round(a, 3) == 1.577 and round(b, 3) == 0.895


def test_fit_ab_refusals():
    from singlerust_amd import _ffi as F
    lib = F.lib()
    a, b = C.c_double(7.0), C.c_double(7.0)
    for spread, min_dist in ((1.0, 1.5), (1.0, -0.1), (0.0, 0.0), (-1.0, 0.0), (np.nan, 0.1), (np.inf, 0.1), (1.0, np.nan), (1.0, np.inf)):
        assert lib.srx_umap_fit_ab(spread, min_dist, C.byref(a), C.byref(b)) == F.E_ARG, (spread, min_dist)
        assert lib.srx_last_error(None) and a.value == 7.0 and b.value == 7.0
    assert lib.srx_umap_fit_ab(1.0, 0.5, None, C.byref(b)) == F.E_ARG
    assert lib.srx_umap_fit_ab(1.0, 1.0, C.byref(a), C.byref(b)) == F.OK and a.value > 0 and b.value > 0     # min_dist == spread is allowed


# ---- 3. golden --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_golden_graph12(dim):
    """The f64 reference reproduces Y^1 and Y^3 of the longdouble evaluation stored in the golden file, and the counters
    exactly.  Bounds: a term is at most 8 in size (2 alpha times a clipped 4) and comes out of about eight f64 operations and a
    pow, each within an ulp: 8 x 10 x 2^-53 ~ 1e-14 per term at the very worst, and the longest row of this graph sums
    5 entries x 6 terms, so 3e-13 after one epoch.  Each further epoch multiplies a perturbation by the map's local slope;
    the measured growth of the reference's own error is below 20 per epoch on every case of this suite (profiles/umap.md),
    which gives 3e-13 x 400 ~ 1e-10 after three."""
    g = ref.golden()["graph12"]
    W, Y0 = ref.graph12()
    lens = np.diff(W.indptr)
    assert W.shape == (12, 12) and lens[11] == 0 and lens[10] == 1 and W.data.min() == 1e-7 * W.data.max()
    assert np.array_equal(Y0[2], Y0[3]) and 0 < abs(Y0[5, 0] - Y0[4, 0]) < 2e-9 and np.array_equal(Y0[5, 1:], Y0[4, 1:])
    y0 = np.ascontiguousarray(Y0[:, :dim])
    Y, info, kept = ref.layout(W, y0, g["a"], g["b"], g["n_epochs"], rate=g["rate"], seed=g["seed"], keep=(1, 3))
    want = g["dim%d" % dim]
    assert {k: info[k] for k in ref.COUNTERS} == want["counters"]
    e1, e3 = np.abs(kept[1] - np.array(want["Y1"])).max(), np.abs(kept[3] - np.array(want["Y3"])).max()
    print("graph12 dim %d: |f64 - longdouble| after 1 epoch %.3e, after 3 %.3e" % (dim, e1, e3))
    assert e1 <= 3e-13 and e3 <= 1e-10
    assert np.array_equal(kept[3], Y) and np.array_equal(kept[1][11], y0[11])       # the isolated vertex never moves
    act = info["entries_active"]
    assert act == int((np.floor(3.0 * ref.ratios(W.data)) > 0).sum()) < W.nnz       # the 1e-7 entry (and the light ones) never act


# ---- the layers ---------------------------------------------------------------------------------------------------------------------
def test_umap_symbols_are_exported_and_bound():
    from singlerust_amd import _ffi
    from singlerust_amd.memory import processing
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "srx.h")).read()
    rust = open(os.path.join(ROOT, "rust", "srx_sys.rs")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _ffi.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, rust), name
    assert "pub struct SrxUmapOpts" in rust and "pub struct SrxUmapInfo" in rust and "pub const SRX_UMAP_GROUP: i32 = %d;" % _ffi.UMAP_GROUP in rust
    assert all(callable(getattr(processing, f)) for f in ("umap", "umap_csr", "fit_ab", "graph_embedding"))
    # additive: the ABI version and the number of profiling classes stay
    assert re.search(r"#define\s+SRX_ABI_VERSION\s+6\b", header) and lib.srx_abi_version() == 6
    assert re.search(r"SRX_K_COUNT_ = 13\b", header)
    assert re.search(r"#define\s+SRX_UMAP_GROUP\s+%d\b" % _ffi.UMAP_GROUP, header)
    assert (_ffi.UMAP_INIT_GIVEN, _ffi.UMAP_INIT_RANDOM, _ffi.UMAP_INIT_PCA) == (0, 1, 2)
    assert re.search(r"SRX_UMAP_INIT_GIVEN = 0, SRX_UMAP_INIT_RANDOM = 1, SRX_UMAP_INIT_PCA = 2", header)
    # stated once: the symmetric-CSR check in its own translation unit, behind the header its three users include; no
    # kernel with internal linkage in a header; one splitmix64 finaliser; no event guard of a file's own
    csrc = os.path.join(ROOT, "singlerust_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith((".hip", ".hpp", ".inl", ".h"))}
    assert [f for f in text if "void __launch_bounds__(256) k_symcsr_check(" in text[f]] == ["symcsr.hip"]
    assert not [f for f in text if "k_louvain_check" in text[f]]
    assert not [f for f in text if f.endswith((".hpp", ".h")) and re.search(r"static\s+__global__", text[f])]
    for f in ("louvain.hip", "umap.hip", "diffmap.hip"):
        assert '#include "symcsr.hpp"' in text[f]
    assert [f for f in text if "0xBF58476D1CE4E5B9" in text[f]] == ["hash.hpp"]
    assert not [f for f in text if "struct EvGuard" in text[f]]


@pytest.mark.parametrize("cname,struct,size", [("srx_umap_opts", "UmapOpts", 80), ("srx_umap_info", "UmapInfo", 96)])
def test_umap_struct_layout_matches_header(tmp_path, cname, struct, size):
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


def test_umap_fails_loudly_without_a_device():
    """Null handles are SRX_E_ARG with a message; with no device visible nothing is computed on the host (a child process with
    every device hidden, so the test means the same on a GPU machine)."""
    from singlerust_amd import _ffi
    lib = _ffi.lib()
    ip, ix, w = np.array([0, 1, 2], np.uint64), np.array([1, 0], np.uint32), np.ones(2)
    assert lib.srx_umap(None, None, None, None, None, None) == _ffi.E_ARG
    assert lib.srx_last_error(None)
    assert lib.srx_umap_csr(None, _ffi.ptr(ip), _ffi.ptr(ix), _ffi.ptr(w), 2, None, None, None, None) == _ffi.E_ARG
    assert lib.srx_graph_embedding_fetch(None, None, None) == _ffi.E_ARG
    code = ("import numpy as np, singlerust_amd as sr\n"
            "from singlerust_amd.memory.processing import umap_csr\n"
            "try:\n"
            "    umap_csr(sr.Context(0), (np.array([0, 1, 2], np.uint64), np.array([1, 0], np.uint32), np.ones(2)))\n"
            "except sr.SrxError as e:\n"
            "    print('refused', e.code, e)\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("refused %d " % _ffi.E_HIP) and "no CPU fallback" in r.stdout, (r.stdout, r.stderr)


def test_umap_kernels_do_not_spill_registers(tmp_path):
    """The gfx950 code-object metadata of every kernel of umap.hip shows no VGPR / SGPR spill and no scratch, and the file is
    built without -ffast-math."""
    from singlerust_amd import build
    assert "umap.hip" in build.SOURCES and not any("fast-math" in f for f in build.FLAGS)
    out = str(tmp_path / "umap.s")
    subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "singlerust_amd", "csrc", "umap.hip")], stderr=subprocess.DEVNULL)
    meta = open(out).read()
    seen, n_kernels = set(), 0
    for m in re.finditer(r"\.name:\s+(\S*k_umap_\S*)\n(.*?)\.wavefront_size", meta, flags=re.S):
        body = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        assert spill == 0 and sspill == 0 and scratch == 0, f"{m.group(1)}: {spill} / {sspill} spilled V/SGPRs, {scratch} B of scratch"
        n_kernels += 1
        seen |= {k for k in KERNELS if re.search(r"\d%s(I|E|\b)" % k, m.group(1))}
    assert seen == set(KERNELS), set(KERNELS) - seen
    assert n_kernels == len(KERNELS) + 1                   # k_umap_epoch<2> / <3>

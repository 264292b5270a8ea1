"""t-SNE without a GPU: the new symbols bound in every layer with the struct layout gcc gives them, a loud failure without a
device, the kernels' gfx950 listings free of register spills and scratch, and the host restatement (tests/tsne_ref.py) checked
against itself and against scikit-learn: its exact route against a dense O(n^2) evaluation, the error of its theta = 0.5 walk,
its P against scikit-learn's binary search, the named inputs of the GPU tests against their 1 % cap, the golden starts."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import tsne_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srx_tsne_affinities_knn", "srx_tsne_affinities_graph", "srx_tsne_info_get", "srx_tsne_fetch_affinities", "srx_tsne_forces",
       "srx_tsne_run", "srx_tsne_embedding_fetch", "srx_tsne_free")
KERNELS = ("k_tsne_rows", "k_tsne_init_random", "k_tsne_absmax", "k_tsne_init_pca", "k_tsne_bounds", "k_tsne_quant", "k_tsne_up",
           "k_tsne_cells", "k_tsne_scatter", "k_tsne_rank", "k_tsne_walk", "k_tsne_sum", "k_tsne_step", "k_tsne_kl")
# The error of the theta = 0.5 walk against the exact sums, on 1500 points in six clumps (tsne_ref.clumps(1500, 2, seed=3,
# spread=4)) at scale 1 and 30 and L in {3, 5, 7}: max_i |rep_i - exact_i| / max_i |exact_i| and |Z - exact| / exact.  Measured
# with the reference: 1.37e-2 and 5.66e-3 at the worst (profiles/tsne.md has every case); the bound is twice that.
REP_ERR_BOUND = 2 * 1.37e-2
Z_ERR_BOUND = 2 * 5.66e-3


# ---- the layers ---------------------------------------------------------------------------------------------------------------------
def test_tsne_symbols_are_exported_and_bound():
    from singlerust_amd import _abi, _ffi, build
    from singlerust_amd.memory import processing
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "srx.h")).read()
    rust = open(os.path.join(ROOT, "rust", "srx_sys.rs")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _ffi.EXPORTS and name in _abi.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, rust), name
    for s in ("SrxTsneInfo", "SrxTsneOpts", "SrxTsneRunInfo", "SrxTsneForceInfo"):
        assert "pub struct %s" % s in rust, s
    assert "pub struct SrxTsne " in rust
    assert all(callable(getattr(processing, f)) for f in ("tsne_affinities", "tsne_affinities_graph", "tsne_forces", "tsne", "tsne_embedding"))
    assert (_ffi.TSNE_INIT_GIVEN, _ffi.TSNE_INIT_RANDOM, _ffi.TSNE_INIT_PCA) == (0, 1, 2)
    assert (_ffi.TSNE_MAX_K, _ffi.TSNE_MAX_LEVELS, _ffi.TSNE_MAX_ITERS) == (64, 12, 2 ** 20) and ref.MAX_LEVELS == 12
    # additive: the ABI version and the number of profiling classes stay
    assert re.search(r"#define\s+SRX_ABI_VERSION\s+6\b", header) and lib.srx_abi_version() == 6
    assert re.search(r"SRX_K_COUNT_ = 13\b", header)
    assert "tsne.hip" in build.SOURCES
    # the union pattern is built by one function that graph.hip and tsne.hip both call
    csrc = os.path.join(ROOT, "singlerust_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith((".hip", ".hpp", ".inl", ".h"))}
    assert sorted(f for f in text if re.search(r"\bpair_union_csr\(ctx, PairRule", text[f])) == ["graph.hip", "tsne.hip"]
    assert [f for f in text if "k_graph_merge(" in text[f] and "__global__" in text[f]] == ["graph.hip"]
    assert "0xBF58476D1CE4E5B9" not in text["tsne.hip"] and "fp contract(off)" in text["tsne.hip"]
    assert "atomicAdd(&small[TS_Z]" not in text["tsne.hip"]                       # no floating-point atomic: Z is a fixed-order sum


@pytest.mark.parametrize("cname,struct,size", [("srx_tsne_info", "TsneInfo", 56), ("srx_tsne_opts", "TsneOpts", 56),
                                               ("srx_tsne_run_info", "TsneRunInfo", 96), ("srx_tsne_force_info", "TsneForceInfo", 56)])
def test_tsne_struct_layout_matches_header(tmp_path, cname, struct, size):
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


def test_tsne_fails_loudly_without_a_device():
    """Null handles are SRX_E_ARG with a message; with no device visible nothing is computed on the host (a child process with
    every device hidden, so the test means the same on a GPU machine)."""
    from singlerust_amd import _ffi
    lib = _ffi.lib()
    h = C.c_void_p(77)
    idx, dist = np.zeros((4, 2), np.uint32), np.zeros((4, 2))
    assert lib.srx_tsne_affinities_knn(None, _ffi.ptr(idx), _ffi.ptr(dist), 4, 2, 1.5, C.byref(h)) == _ffi.E_ARG and h.value == 77
    assert lib.srx_last_error(None)
    assert lib.srx_tsne_affinities_graph(None, 1.5, C.byref(h)) == _ffi.E_ARG and h.value == 77
    assert lib.srx_tsne_info_get(None, None) == _ffi.E_ARG
    assert lib.srx_tsne_fetch_affinities(None, None, None, None, None) == _ffi.E_ARG
    assert lib.srx_tsne_forces(None, None, 0.5, 0, None, None, None, None) == _ffi.E_ARG
    assert lib.srx_tsne_run(None, None, None, None, None, None) == _ffi.E_ARG
    assert lib.srx_tsne_embedding_fetch(None, None) == _ffi.E_ARG
    lib.srx_tsne_free(None)
    code = ("import numpy as np, singlerust_amd as sr\n"
            "from singlerust_amd.memory.processing import tsne_affinities\n"
            "try:\n"
            "    tsne_affinities(sr.Context(0), np.array([[1, 2], [2, 0], [0, 1]], np.uint32), np.ones((3, 2)), 1.5)\n"
            "except sr.SrxError as e:\n"
            "    print('refused', e.code, e)\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("refused %d " % _ffi.E_HIP) and "no CPU fallback" in r.stdout, (r.stdout, r.stderr)


def test_tsne_kernels_do_not_spill_registers(tmp_path):
    """The gfx950 code-object metadata of every kernel of tsne.hip shows no VGPR / SGPR spill and no scratch, and the file is
    built without -ffast-math."""
    from singlerust_amd import build
    assert "tsne.hip" in build.SOURCES and not any("fast-math" in f for f in build.FLAGS)
    out = str(tmp_path / "tsne.s")
    subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "singlerust_amd", "csrc", "tsne.hip")], stderr=subprocess.DEVNULL)
    meta = open(out).read()
    seen, n_kernels = set(), 0
    for m in re.finditer(r"\.name:\s+(\S*k_tsne_\S*)\n(.*?)\.wavefront_size", meta, flags=re.S):
        body = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        assert spill == 0 and sspill == 0 and scratch == 0, f"{m.group(1)}: {spill} / {sspill} spilled V/SGPRs, {scratch} B of scratch"
        n_kernels += 1
        seen |= {k for k in KERNELS if re.search(r"\d%s(E|\b)" % k, m.group(1))}
    assert seen == set(KERNELS), set(KERNELS) - seen
    assert n_kernels == len(KERNELS)


# ---- the reference checks itself ------------------------------------------------------------------------------------------------------
def test_starts_and_levels():
    kat = ref.golden()["start"]
    for c in kat:
        y = ref.random_start(c["n"], int(c["seed"]))
        assert y.ravel().tolist() == c["y"] and (np.abs(y) <= 1e-4).all()
    z = ref.mix_int(9 + 0x9E3779B97F4A7C15 * 4)                                    # coordinate c = 3 of seed 9
    assert ref.random_start(3, 9)[1, 1] == ((z >> 11) * 2.0 ** -53 - 0.5) * 2e-4
    assert ref.mix_int(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF                   # splitmix64's first output for seed 0
    s = np.random.default_rng(0).standard_normal((50, 5))
    y = ref.pca_start(s)
    assert y.shape == (50, 2) and abs(np.abs(y).max() - 1e-4) < 1e-19
    assert [ref.auto_levels(n) for n in (0, 1, 16, 17, 64, 65, 10 ** 4, 10 ** 5, 1300000, 2 ** 40)] == [1, 1, 1, 2, 2, 3, 6, 8, 10, 12]
    assert ref.default_perplexity(64) == 64 / 3 and ref.default_perplexity(15) == 5.0 and ref.default_perplexity(200) == 30.0
    assert ref.auto_eta(600) == 50.0 and ref.auto_eta(48000) == 1000.0


@pytest.mark.parametrize("n,L", [(1, 1), (2, 1), (3, 2), (300, 4), (300, 12), (700, 6)])
def test_exact_route_equals_the_dense_sums(n, L):
    """theta = 0 never accepts a cell: the walk visits every pair once, and equals the dense O(n^2) evaluation to the last
    bits its order of summation allows.  The terms are the same f64 numbers on both sides, so the two sums differ by at most
    2 gamma_n sum_j |term_ij| with gamma_n = n 2^-53 / (1 - n 2^-53) (Higham, Accuracy and Stability, 4.2)."""
    Y = ref.force_layout("generic", n) * 3.0
    rep, z, Z, info = ref.repulsion(Y, 0.0, L)
    drep, dz = ref.dense_repulsion(Y)
    assert info["cells_accepted"] == 0 and info["pairs_exact"] == n * (n - 1)
    d = Y[:, None, :] - Y[None, :, :]
    q = 1.0 / (1.0 + (d ** 2).sum(axis=2))
    np.fill_diagonal(q, 0.0)
    gam = 2.0 * n * 2.0 ** -53 / (1.0 - n * 2.0 ** -53)
    assert (np.abs(rep - drep) <= gam * (np.abs((q * q)[:, :, None] * d)).sum(axis=1) + 1e-300).all()
    assert (np.abs(z - dz) <= gam * q.sum(axis=1) + 1e-300).all()
    assert abs(Z - dz.sum()) <= gam * dz.sum() * 2


def test_approximation_error_of_the_walk():
    """theta = 0.5, L in {3, 5, 7}, 1500 points in six clumps, at scale 1 and 30: rep and Z of the walk against the exact ones,
    within twice the maximum measured with this reference (the constants above)."""
    X, _ = ref.clumps(1500, 2, seed=3, spread=4.0)
    worst_r = worst_z = 0.0
    for scale in (1.0, 30.0):
        Y = X * scale
        drep, dz = ref.dense_repulsion(Y)
        for L in (3, 5, 7):
            rep, z, Z, info = ref.repulsion(Y, 0.5, L)
            er = float(np.linalg.norm(rep - drep, axis=1).max() / np.linalg.norm(drep, axis=1).max())
            ez = float(abs(Z - dz.sum()) / dz.sum())
            print("scale %g L %d: rep %.3e Z %.3e | accepted %d exact %d pairs %d"
                  % (scale, L, er, ez, info["cells_accepted"], info["cells_exact"], info["pairs_exact"]))
            assert info["cells_accepted"] > 0 and info["pairs_exact"] < 1500 * 1499
            worst_r, worst_z = max(worst_r, er), max(worst_z, ez)
    print("worst: rep %.3e (bound %.3e), Z %.3e (bound %.3e)" % (worst_r, REP_ERR_BOUND, worst_z, Z_ERR_BOUND))
    assert worst_r <= REP_ERR_BOUND and worst_z <= Z_ERR_BOUND


def test_longdouble_switch_keeps_the_decisions():
    Y = ref.force_layout("clump70", 257)
    a, b = ref.repulsion(Y, 0.5, 4), ref.repulsion(Y, 0.5, 4, np.longdouble)
    assert all(a[3][c] == b[3][c] for c in ref.COUNTERS) and b[0].dtype == np.longdouble
    assert 0 < float(np.abs(a[0] - b[0]).max()) < 1e-12


# ---- the affinities ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.AFFINITY_CASES)
def test_named_inputs_stay_inside_the_cap(name):
    """The reference solves every rooted row of the named inputs to 1e-13, P is symmetric and sums to 1 (to the dropped
    zeros), and no row's tolerance exceeds the cap, so the GPU test compares every row element-wise."""
    idx, dist, u = ref.affinity_case(name)
    (indptr, indices, data), beta, info, (cols, p, ci) = ref.affinities(idx, dist, u)
    n, root = info["n"], ci["root"]
    H = ref.row_entropy(ci["x"][root], beta[root])
    assert (np.abs(H - np.log(info["perplexity"])) <= 1e-13).all()
    assert np.allclose(p.sum(axis=1), 1.0, atol=1e-14) and abs(data.sum() - 1.0) < 1e-12
    tol = ref.p_row_tolerance(ci["bound"][root])
    print("%s: rows %d rooted %d, largest row tolerance %.3e" % (name, n, int(root.sum()), float(tol.max()) if tol.size else 0.0))
    assert (tol > ref.P_ROW_CAP).sum() <= 0.01 * n
    if name.startswith("edges"):
        assert (~root).sum() == 4 and root[1] and not root[2] and not root[3] and not root[0] and not root[4]
        assert (p[0] == 1.0 / 15).all() and sorted(p[2])[-5:] == [0.2] * 5 and (p[4] == 1.0 / 15).all() and info["entries_dropped"] > 0


def test_shuffled_rows_give_the_same_reference():
    a = ref.affinities(*ref.affinity_case("edges"))
    b = ref.affinities(*ref.affinity_case("edges_shuffled"))
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1])


def test_p_against_scikit_learn():
    """The reference's conditional p against sklearn.manifold._utils._binary_search_perplexity on the same squared distances.
    scikit-learn stops at |H - log u| <= 1e-5 and works on f32 distances: an entry x = D - m carries a relative error of
    2^-24 of the largest D, which moves H by at most beta * 2^-24 * max D (|dH / dx_j| <= beta p_j |..| <= beta); the bound is
    max_j |dp_j / dH| times the sum of the two, times two.  The measured difference is in profiles/tsne.md."""
    utils = pytest.importorskip("sklearn.manifold._utils")
    worst = 0.0
    for name, u in (("n257", 5.0), ("n1025", 10.0), ("k64", 64 / 3)):
        idx, dist, _ = ref.affinity_case(name)
        D32 = (dist * dist).astype(np.float32)
        cols, p, beta, ci = ref.conditional(np.tile(np.arange(idx.shape[1]), (idx.shape[0], 1)), np.sqrt(D32.astype(np.float64)), u)
        sk = np.asarray(utils._binary_search_perplexity(D32, u, 0), dtype=np.float64)
        dH = 1e-5 + beta * 2.0 ** -24 * D32.max(axis=1).astype(np.float64)
        tol = 2.0 * ci["bound"] * dH + 1e-7                                         # the result is stored in f32
        err = np.abs(sk - p).max(axis=1)
        print("%s: max |sklearn - reference| %.3e, bound %.3e" % (name, float(err.max()), float(tol.max())))
        worst = max(worst, float(err.max()))
        assert (err <= tol).all()
    print("worst %.3e" % worst)

"""srx_neighbors_* / srx_graph_* without a GPU: exported and bound in every layer (ctypes, rust/srx_sys.rs, the Rust shim, the
C++ mirror), the struct layout as the C compiler lays it out, a loud failure without a device (no CPU fallback), the new
kernels' gfx950 listings free of register spills and scratch, and the host restatement's own sanity."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

import graph_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srx_neighbors_result", "srx_neighbors_from_knn", "srx_graph_info_get", "srx_graph_fetch", "srx_graph_fetch_scales",
       "srx_graph_free")
KERNELS = ("k_graph_rows", "k_graph_reverse", "k_graph_rowlen", "k_graph_scatter", "k_graph_order", "k_graph_order_long",
           "k_graph_merge")


def test_graph_symbols_are_exported_and_bound():
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
    for name in ("srx_neighbors_result", "srx_neighbors_from_knn", "srx_graph_fetch", "srx_graph_free"):
        assert re.search(r"\b%s\s*\(" % name, shim), name
    assert "pub struct SrxGraphInfo" in rust and "pub struct SrxGraph " in rust
    assert "pub fn neighbors_graph(adata: &IMAnnData, n_neighbors: usize, n_pcs: usize)" in shim
    assert "pub fn connectivities_from_knn(" in shim
    assert "class Graph" in mirror
    assert callable(processing.neighbors) and callable(processing.connectivities_from_knn)
    # additive: the ABI version stays, the profiling class is appended and the earlier ids keep their values
    assert re.search(r"#define\s+SRX_ABI_VERSION\s+6\b", header) and lib.srx_abi_version() == 6
    assert re.search(r"SRX_K_KNN = 11,", header) and re.search(r"SRX_K_GRAPH = 12,", header)
    assert re.search(r"SRX_K_COUNT_ = 13\b", header) and _ffi.K_GRAPH == 12 and _ffi.K_KNN == 11
    assert (_ffi.GRAPH_DISTANCES, _ffi.GRAPH_CONNECTIVITIES) == (0, 1)


def test_graph_struct_layout_matches_header(tmp_path):
    """sizeof() and the field offsets of the ctypes mirror equal what gcc lays out."""
    from singlerust_amd import _ffi
    fields = [n for n, _ in _ffi.GraphInfo._fields_]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "srx.h"\nint main(void){printf("%zu", sizeof(srx_graph_info));\n'
            + "".join('printf(" %%zu", offsetof(srx_graph_info, %s));\n' % f for f in fields) + "return 0;}\n")
    src, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(src, "w").write(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(_ffi.GraphInfo)] + [getattr(_ffi.GraphInfo, f).offset for f in fields]
    assert len(fields) == 11 and C.sizeof(_ffi.GraphInfo) == 80


def test_graph_fails_loudly_without_a_device():
    """Null handles are SRX_E_ARG with a message; with no device visible there is no context to build on and nothing is
    computed on the host (a child process with every device hidden, so the test means the same on a GPU machine)."""
    from singlerust_amd import _ffi
    lib = _ffi.lib()
    h = C.c_void_p()
    idx, dist = np.zeros((4, 2), np.uint32), np.zeros((4, 2))
    assert lib.srx_neighbors_from_knn(None, _ffi.ptr(idx), _ffi.ptr(dist), 4, 2, C.byref(h)) == _ffi.E_ARG
    assert lib.srx_last_error(None)
    assert lib.srx_neighbors_result(None, C.byref(_ffi.KnnOpts(5, 0, 0, 0)), None, C.byref(h)) == _ffi.E_ARG
    assert lib.srx_graph_info_get(None, None) == _ffi.E_ARG
    assert lib.srx_graph_fetch(None, 0, None, None, None) == _ffi.E_ARG
    assert lib.srx_graph_fetch_scales(None, None, None) == _ffi.E_ARG
    lib.srx_graph_free(None)
    code = ("import numpy as np, singlerust_amd as sr\n"
            "from singlerust_amd.memory.processing import connectivities_from_knn\n"
            "try:\n"
            "    connectivities_from_knn(sr.Context(0), np.array([[1], [0]], np.uint32), np.ones((2, 1)))\n"
            "except sr.SrxError as e:\n"
            "    print('refused', e.code, e)\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("refused %d " % _ffi.E_HIP) and "no CPU fallback" in r.stdout, (r.stdout, r.stderr)


def test_graph_kernels_do_not_spill_registers(tmp_path):
    """As test_knn_kernels_do_not_spill_registers: the gfx950 code-object metadata of every kernel of graph.hip shows no
    VGPR spill and no scratch."""
    from singlerust_amd import build
    assert "graph.hip" in build.SOURCES
    out = str(tmp_path / "graph.s")
    subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "singlerust_amd", "csrc", "graph.hip")], stderr=subprocess.DEVNULL)
    meta = open(out).read()
    seen = set()
    for m in re.finditer(r"\.name:\s+(\S*k_graph_\S*)\n(.*?)\.wavefront_size", meta, flags=re.S):
        body = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        assert spill == 0 and sspill == 0 and scratch == 0, f"{m.group(1)}: {spill} / {sspill} spilled V/SGPRs, {scratch} B of scratch"
        seen |= {k for k in KERNELS if re.search(r"%s(E|\b)" % k, m.group(1))}
    assert seen == set(KERNELS), set(KERNELS) - seen
    assert "v_fma_f64" in meta


# ---- the restatement's own sanity ------------------------------------------------------------------------------------
def _host_knn(x, k):
    from sklearn.neighbors import NearestNeighbors
    nn = NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(x)
    dist, idx = nn.kneighbors(n_neighbors=k)
    return idx, dist


def test_restatement_row_sums_hit_the_target():
    """Row sums of the restated weights equal T to 1e-12 on generic fixtures (the bisection runs until the bracket is one ulp
    wide), C is symmetric with values in (0, 1], and D holds the list."""
    for n, d, k in ((1500, 50, 15), (1000, 3, 5), (800, 10, 30), (300, 2, 1)):
        x = np.random.default_rng(7).standard_normal((n, d))
        idx, dist = _host_knn(x, k)
        D, Cm, sc, A, info = graph_ref.graph(idx, dist)
        free = sc["has_root"] & ~sc["clamped"]
        a = A.data.reshape(n, k)
        if k == 1:
            assert not free.any() and info["rows_no_root"] == n and info["rows_clamped"] == n and (a == 1).all()
        else:
            assert free.all()
            assert np.abs(a[free].sum(axis=1) - sc["T"]).max() <= 1e-12
        assert (Cm != Cm.T).nnz == 0 and Cm.data.min() > 0 and Cm.data.max() <= 1 and Cm.diagonal().sum() == 0
        assert info["nnz_connectivities"] == 2 * n * k - 2 * info["n_mutual"] - info["entries_dropped"]
        assert D.nnz == n * k and np.array_equal(np.sort(D.data), np.sort(dist.ravel()))


def test_restatement_on_the_tie_and_underflow_fixtures():
    """The figures the GPU tests rely on: the 30 x 30 lattice (k = 8) has 784 no-root, clamped rows and a smallest entry near
    4.4e-168; the hand-made underflow list drops 2600 entries and keeps the others."""
    p = np.array(np.meshgrid(np.arange(30.0), np.arange(30.0), indexing="ij")).reshape(2, -1).T
    idx, dist = _host_knn(p, 8)
    D, Cm, sc, A, info = graph_ref.graph(idx, dist)
    assert info["rows_no_root"] == 784 and info["rows_clamped"] == 784 and info["entries_dropped"] == 0
    assert 4.3e-168 < Cm.data.min() < 4.5e-168
    from test_graph_gpu import underflow_list
    idx, dist = underflow_list()
    D, Cm, sc, A, info = graph_ref.graph(idx, dist)
    assert info["rows_no_root"] == 200 and info["rows_clamped"] == 200
    assert info["entries_dropped"] == 2600 and 0 < Cm.data.min() < 1e-200

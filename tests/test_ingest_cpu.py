"""The host restatement of the ingest section of include/srx.h (tests/ingest_ref.py) against cases that can be worked out by hand,
its independence of the order of a row's entries, the new entry points in the generated bindings, and the listing of ingest.hip
(no register spill, no scratch).  No GPU."""
import ctypes as C
import decimal
import os
import re
import subprocess

import numpy as np

import ingest_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srx_umap_transform_knn", "srx_umap_transform_graph", "srx_knn_vote", "srx_knn_vote_graph")


def _decimal_root(ds, T):
    """The root of sum exp(-d / s) = T by bisection in 60-digit decimal arithmetic."""
    decimal.getcontext().prec = 60
    D = decimal.Decimal
    S = lambda s: sum((-D(d) / s).exp() for d in ds)
    lo, hi = D(1) / D(1000), D(1000)
    for _ in range(300):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if S(mid) < T else (lo, mid)
    return hi


def test_sigma_of_the_three_entry_row():
    """kq = 3, distances (0, 1, 2): the nearest entry (d = 0) stays out, S(s) = e^(-1/s) + e^(-2/s) = log2(3)."""
    decimal.getcontext().prec = 60
    T = decimal.Decimal(3).ln() / decimal.Decimal(2).ln()
    want = _decimal_root((1, 2), T)
    # closed form as a cross-check of the bisection: u = e^(-1/s) solves u + u^2 = T
    u = (-1 + (1 + 4 * T).sqrt()) / 2
    assert abs(want - (-1 / u.ln())) < decimal.Decimal("1e-40")
    for perm in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        idx = np.array([[7, 3, 5]])[:, perm]
        dist = np.array([[0.0, 1.0, 2.0]])[:, perm]
        for dtype in (np.float64, np.longdouble):
            m = ref.membership(idx, dist, dtype)
            err = abs(decimal.Decimal(repr(float(m["sigma"][0]))) - want)
            print(perm, np.dtype(dtype).name, "sigma", float(m["sigma"][0]), "|sigma - root|", float(err))
            assert m["has_root"][0] and not m["clamped"][0] and not m["all_zero"][0]
            assert err <= decimal.Decimal("1e-12")
            assert m["cols"].tolist() == [[3, 5, 7]]
            # the nearest entry (reference 7, d = 0) has weight 1, the others exp(-d / sigma)
            w = {int(c): float(x) for c, x in zip(m["cols"][0], m["w"][0])}
            d = {7: 0.0, 3: 1.0, 5: 2.0}
            assert w[7] == 1.0
            for c in (3, 5):
                assert abs(w[c] - float((-decimal.Decimal(d[c]) / want).exp())) <= 1e-12
            assert abs(float(ref._S(m["one"], m["far"], np.where(m["far"], m["d"], 0), m["sigma"])[0]) - float(T)) <= 1e-9


def test_all_zero_row_and_rows_without_a_root():
    Yref = np.arange(20, dtype=np.float64).reshape(10, 2) ** 1.5
    idx = np.array([[4, 1, 9, 6], [0, 2, 3, 5], [1, 2, 3, 4]])
    dist = np.array([[0.0, 0.0, 0.0, 0.0],          # all zero: sigma 0, weights 1, the start is the plain mean
                     [0.0, 0.0, 0.0, 3.0],          # c = 2 = T = log2(4): no root; the floor 1e-3 * 3 / 4
                     [0.5, 1.0, 2.0, 4.0]])
    Y, info, p = ref.transform(idx, dist, Yref, 1.5, 0.9, n_epochs=1)
    assert p["all_zero"].tolist() == [True, False, False] and p["has_root"].tolist() == [False, False, True]
    assert p["clamped"].tolist() == [False, True, False]
    assert (info["rows_all_zero"], info["rows_no_root"], info["rows_clamped"], info["rows_start_nearest"]) == (1, 2, 1, 0)
    assert p["sigma"][0] == 0.0 and (p["w"][0] == 1.0).all()
    assert np.allclose(p["start"][0], Yref[[1, 4, 6, 9]].mean(axis=0), rtol=0, atol=1e-13)
    assert p["sigma"][1] == 1e-3 * 3.0 / 4.0
    assert p["w"][1].tolist() == [1.0, 1.0, 1.0, np.exp(-3.0 / p["sigma"][1])] and p["w"][1][3] == 0.0     # underflows
    assert np.allclose(p["start"][1], Yref[[0, 2, 3]].mean(axis=0), rtol=0, atol=1e-13)
    # an overflowing sum of distances: the floor and sigma are +inf, every weight 1
    m = ref.membership(np.arange(64)[None, :], np.full((1, 64), 1e307))
    assert np.isfinite(m["sigma_star"][0]) and np.isinf(m["sigma"][0]) and m["clamped"][0] and (m["w"][0] == 1.0).all()
    # ... and when the bracket of the root overflows as well, sigma* is +inf itself and the floor is not the larger
    m = ref.membership(np.array([[0, 1, 2]]), np.array([[1e308, 1e308, 1e308]]))
    assert np.isinf(m["sigma"][0]) and not m["clamped"][0] and (m["w"][0] == 1.0).all()


def test_zero_total_weight_starts_at_the_nearest_entry():
    Yref = np.random.default_rng(0).standard_normal((6, 3))
    cols = np.array([[0, 2, 5], [1, 3, 4]])
    w = np.array([[0.0, 0.0, 0.0], [0.25, 0.5, 0.25]])
    y0, nearest = ref.start(w, cols, Yref, np.array([1, 0]))
    assert nearest.tolist() == [True, False]
    assert np.array_equal(y0[0], Yref[2])
    assert np.allclose(y0[1], 0.25 * Yref[1] + 0.5 * Yref[3] + 0.25 * Yref[4], rtol=0, atol=1e-15)


def test_vote_tie_rule():
    labels = np.array([2, 1, 1, 2, 0, 5, 5, 5], dtype=np.uint32)
    idx = np.array([[0, 1, 2, 3],        # labels (2, 1, 1, 2): a tie at two each, the lowest label wins
                    [3, 2, 1, 0],
                    [4, 5, 6, 0],        # (0, 5, 5, 2): 5 twice
                    [4, 0, 1, 5],        # (0, 2, 1, 5): all once, the lowest is 0
                    [5, 6, 7, 4]])       # (5, 5, 5, 0)
    lab, cnt = ref.vote(idx, labels)
    assert lab.tolist() == [1, 1, 5, 0, 5] and cnt.tolist() == [2, 2, 2, 1, 3]
    lab, cnt = ref.vote(np.array([[6], [0]]), labels)
    assert lab.tolist() == [5, 2] and cnt.tolist() == [1, 1]


def test_permuting_a_row_changes_nothing():
    rng = np.random.default_rng(3)
    n_ref, nq, kq = 200, 40, 11
    Yref = rng.standard_normal((n_ref, 2)) * 5
    idx = np.stack([rng.choice(n_ref, kq, replace=False) for _ in range(nq)])
    dist = np.sort(rng.random((nq, kq)) * 3, axis=1)
    dist[3, :4] = 0.0
    dist[4] = 0.0
    labels = rng.integers(0, 4, n_ref)
    Y, info, p = ref.transform(idx, dist, Yref, 1.577, 0.895, n_epochs=3, seed=7)
    perm = np.stack([rng.permutation(kq) for _ in range(nq)])
    idx2, dist2 = np.take_along_axis(idx, perm, axis=1), np.take_along_axis(dist, perm, axis=1)
    Y2, info2, p2 = ref.transform(idx2, dist2, Yref, 1.577, 0.895, n_epochs=3, seed=7)
    assert info == info2 and info["samples"] > 0
    assert np.array_equal(Y.view(np.uint64), Y2.view(np.uint64))
    for k in ("cols", "w", "sigma", "start"):
        assert np.array_equal(p[k], p2[k]), k
    assert all(np.array_equal(a, b) for a, b in zip(ref.vote(idx, labels), ref.vote(idx2, labels)))


def test_epochs_continue_from_their_own_result():
    """The state between two stretches of epochs is the positions alone: what lets the device run them in chunks."""
    rng = np.random.default_rng(5)
    Yref = rng.standard_normal((50, 2)) * 4
    idx = np.stack([rng.choice(50, 8, replace=False) for _ in range(20)])
    dist = rng.random((20, 8)) + 0.1
    m = ref.membership(idx, dist)
    y0, _ = ref.start(m["w"], m["cols"], Yref, m["nearest"])
    full, cf = ref.epochs(m["cols"], m["w"], Yref, y0, 1.5, 0.9, 9, seed=1)
    half, c1 = ref.epochs(m["cols"], m["w"], Yref, y0, 1.5, 0.9, 9, seed=1, stop_after=4)
    rest, c2 = ref.epochs(m["cols"], m["w"], Yref, half, 1.5, 0.9, 9, seed=1, first_epoch=5)
    assert np.array_equal(full.view(np.uint64), rest.view(np.uint64))
    assert cf["samples"] == c1["samples"] + c2["samples"] and cf["epochs_run"] == 9 and c1["epochs_run"] == 4


def test_butterfly_is_a_sum():
    v = np.random.default_rng(1).random((5, 17))
    assert np.allclose(ref.butterfly(v), v.sum(axis=1), rtol=1e-15, atol=0)
    assert ref.butterfly(np.ones((2, 64)))[0] == 64.0


def test_new_entry_points_are_bound():
    from singlerust_amd import _abi
    from singlerust_amd.memory import processing
    for name in NEW:
        assert name in _abi.SIGNATURES and name in _abi.EXPORTS, name
    assert len(_abi.SIGNATURES["srx_umap_transform_knn"][1]) == 11 and len(_abi.SIGNATURES["srx_umap_transform_graph"][1]) == 9
    assert len(_abi.SIGNATURES["srx_knn_vote"][1]) == 9 and len(_abi.SIGNATURES["srx_knn_vote_graph"][1]) == 6
    # the header's structs as a C compiler lays them out: 6 f64 + u64 + 4 i32; 5 pointers; 9 u64 + 4 u32 + 5 f64
    assert C.sizeof(_abi.UmapTransformOpts) == 72 and C.sizeof(_abi.UmapTransformOut) == 40
    assert C.sizeof(_abi.UmapTransformInfo) == 128
    assert _abi.UMAP_TRANSFORM_CHUNK == 64 and _abi.ABI_VERSION == 6
    header = open(os.path.join(ROOT, "include", "srx.h")).read()
    for name in NEW:
        assert re.search(r"int32_t %s\(" % name, header), name
    for text in ("rust/srx_sys.rs", "rust/shim.rs", "singlerust_amd/host/single_rust.hpp"):
        body = open(os.path.join(ROOT, text)).read()
        assert all(name in body for name in NEW), text
    assert all(hasattr(processing, f) for f in ("ingest", "knn_vote", "umap_transform"))


def test_ingest_kernels_do_not_spill_registers(tmp_path):
    """The gfx950 code-object metadata of every kernel of ingest.hip shows no VGPR / SGPR spill and no scratch: the transform
    kernel keeps a query's position and its lane's entries in registers through the epochs of a launch."""
    from singlerust_amd import build
    assert "ingest.hip" in build.SOURCES
    out = str(tmp_path / "ingest.s")
    subprocess.check_call([build._hipcc(), *[f for f in build.FLAGS if f != "-Wall"], "-w", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "singlerust_amd", "csrc", "ingest.hip")], stderr=subprocess.DEVNULL)
    meta = open(out).read()
    seen = []
    for m in re.finditer(r"\.name:\s+(\S*k_ingest_\S*)\n(.*?)\.wavefront_size", meta, flags=re.S):
        body = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1))
        print(m.group(1), "VGPRs", vgprs)
        assert spill == 0 and sspill == 0 and scratch == 0, f"{m.group(1)}: {spill} / {sspill} spilled V/SGPRs, {scratch} B of scratch"
        seen.append(m.group(1))
    assert sum("k_ingest_epochs" in s for s in seen) == 2 and sum("k_ingest_rows" in s for s in seen) == 2
    assert sum("k_ingest_vote" in s for s in seen) == 1 and len(seen) == 5

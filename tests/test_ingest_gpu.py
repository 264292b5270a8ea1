"""srx_umap_transform_knn / _graph and srx_knn_vote / _graph on the device against the definition of include/srx.h
(tests/ingest_ref.py): the membership stage alone, positions and exact counters after 1 and 3 epochs, chunked launches and
stop_after, quality over a full run, the vote bit for bit, the resident path and the refusals.

Tolerance of the element-wise comparisons: the scheme and factor of tests/test_umap_gpu.py.  For each case and each quantity
D = max |f64 numpy - longdouble numpy| is computed here on the CPU and the device gets TOL_FACTOR x D.  The long-double
evaluation bisects sigma to the root itself (ingest_ref's docstring), so D holds the distance the f64 rule's stop leaves
between sigma and the root; the device's exp, pow and summation order differ from numpy's by a few ulp per term.  The
comparison of positions stops at 3 epochs for the reason given at the top of test_umap_gpu.py.  NOT compared: umap-learn,
scanpy (not installed)."""
import ctypes as C

import numpy as np
import pytest

import ingest_ref as ref
import umap_ref

pytestmark = pytest.mark.gpu

A, B = 1.577, 0.895
TOL_FACTOR = 32
KQS = (3, 4, 7, 8, 9, 15, 16, 17, 63, 64)
NQS = (0, 1, 31, 32, 33, 257)
N_REF = 1000
DIMS = (2, 3)
RATES = (0, 1, 5)
SCHEDULES = ((1, 0), (3, 0), (100, 1), (100, 3))
SCALES = (0.01, 1.0, 100.0)


def run(ctx, idx, dist, yref, **kw):
    from singlerust_amd.memory.processing import umap_transform
    kw.setdefault("a", A)
    kw.setdefault("b", B)
    return umap_transform(ctx, idx, dist, yref, **kw)


_YREF = {}


def yref(n_ref, dim):
    if n_ref not in _YREF:
        _YREF[n_ref] = np.random.default_rng(900 + n_ref).standard_normal((n_ref, 3)) * 5.0
    return np.ascontiguousarray(_YREF[n_ref][:, :dim])


_LISTS = {}


def knn_list(nq, kq, n_ref):
    """A query list built once: distinct references per row in arbitrary order, distances of one scale per case with ties and a
    few exact zeros, unsorted."""
    key = (nq, kq, n_ref)
    if key not in _LISTS:
        rng = np.random.default_rng(1000 * kq + nq + n_ref)
        idx = np.argsort(rng.random((nq, n_ref)), axis=1)[:, :kq].astype(np.uint32)
        dist = rng.gamma(2.0, 1.0, (nq, kq)) * SCALES[(kq + nq) % 3]
        if nq > 2:
            dist[1, 1] = dist[1, 0]                         # a tie at some distance
            dist[2, : min(2, kq)] = 0.0                     # zeros: fewer than T of them outside the nearest entry
        _LISTS[key] = (idx, dist)
    return _LISTS[key]


_MEMB = {}


def memb(nq, kq, n_ref):
    """(f64 membership, long-double membership) of a list, computed once and left unchanged."""
    key = (nq, kq, n_ref)
    if key not in _MEMB:
        idx, dist = knn_list(*key)
        _MEMB[key] = (ref.membership(idx, dist), ref.membership(idx, dist, np.longdouble))
    return _MEMB[key]


def gap(x, xl):
    """max |f64 - longdouble| over the finite entries (inf - inf has no distance; the infinite entries are compared exactly)."""
    x, xl = np.asarray(x), np.asarray(xl)
    fin = np.isfinite(x)
    assert np.array_equal(fin, np.isfinite(xl))
    return float(np.abs(x[fin].astype(np.longdouble) - xl[fin]).max()) if fin.any() else 0.0


def close(got, want, tol, what):
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin]), what
    err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    assert err <= tol, (what, err, tol)
    return err


def S_longdouble(m, sigma):
    """S(sigma) of every row in long double, from the sorted distances of the f64 membership and the device's sigma."""
    d = m["d"].astype(np.longdouble)
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        terms = np.where(m["far"], np.exp(-d / sigma.astype(np.longdouble)[:, None]), 0)
    return m["one"].sum(axis=1) + terms.sum(axis=1)


def check_membership(ctx, idx, dist, Y, label, m=None, ml=None):
    m = m or ref.membership(idx, dist)
    ml = ml or ref.membership(idx, dist, np.longdouble)
    nq, kq = idx.shape
    y0, near = ref.start(m["w"], m["cols"], Y, m["nearest"])
    y0l, nearl = ref.start(ml["w"], ml["cols"], Y, ml["nearest"], np.longdouble)
    assert np.array_equal(near, nearl)
    emb, info = run(ctx, idx, dist, Y, n_epochs=1, negative_sample_rate=0, parts=True)
    want = {"rows_no_root": int((~m["has_root"]).sum()), "rows_clamped": int(m["clamped"].sum()),
            "rows_all_zero": int(m["all_zero"].sum()), "rows_start_nearest": int(near.sum())}
    assert all(np.array_equal(m[k], ml[k]) for k in ("has_root", "clamped", "all_zero", "cols"))
    Dw, Ds, Dy = gap(m["w"], ml["w"]), gap(m["sigma"], ml["sigma"]), gap(y0, y0l)
    assert np.array_equal(info["columns"], m["cols"]) and info["columns"].dtype == np.uint32
    for k, v in want.items():
        assert info[k] == v, (label, k, info[k], v)
    assert (info["n_query"], info["n_ref"], info["kq"], info["dim"]) == (nq, len(Y), kq, Y.shape[1])
    ew = close(info["weights"], m["w"], TOL_FACTOR * Dw, "weights")
    es = close(info["sigma"], m["sigma"], TOL_FACTOR * Ds, "sigma")
    ey = close(info["start"], y0, TOL_FACTOR * Dy, "start")
    free = m["has_root"] & ~m["clamped"] & np.isfinite(m["sigma"])
    eS = float(np.abs(S_longdouble(m, info["sigma"])[free] - m["T"]).max()) if free.any() else 0.0
    print("%s: D w %.2e sigma %.2e start %.2e | device w %.2e sigma %.2e start %.2e | max |S - T| %.2e on %d rows | %s"
          % (label, Dw, Ds, Dy, ew, es, ey, eS, int(free.sum()), want))
    assert eS <= 1e-9
    return info


# ---- a. membership --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kq", KQS)
def test_membership(ctx, kq):
    for n_ref in (kq, N_REF):
        for nq in NQS:
            idx, dist = knn_list(nq, kq, n_ref)
            m, ml = memb(nq, kq, n_ref)
            info = check_membership(ctx, idx, dist, yref(n_ref, 2 + (nq + kq) % 2), "kq %d nq %d n_ref %d" % (kq, nq, n_ref), m, ml)
            if nq > 2:
                assert info["rows_no_root"] == 0 and info["rows_all_zero"] == 0


def special_rows():
    """kq = 8 (T = 3, seven entries in the row sum).  Row 0: four exact zeros, three of them in the sum: c = 3 >= T, no root, the
    floor.  Row 1: all zero.  Row 2: distances near 5e307, their sum overflows: the floor and sigma are +inf, every weight 1.
    Row 3: no root and four far entries at 1000 against a floor of 0.5: their weights underflow to 0.  Row 4: an ordinary row."""
    idx = np.array([[5, 3, 9, 1, 7, 0, 2, 8], [11, 4, 6, 2, 0, 9, 3, 10], [1, 2, 3, 4, 5, 6, 7, 8], [8, 7, 6, 5, 4, 3, 2, 1],
                    [0, 2, 4, 6, 8, 10, 1, 3]], dtype=np.uint32)
    dist = np.array([[0.0, 1.0, 0.0, 2.0, 0.0, 3.0, 0.0, 4.0], [0.0] * 8, list(5e307 * (1.0 + 0.02 * np.arange(8))),
                     [1000.0, 0.0, 1000.0, 0.0, 1000.0, 0.0, 1000.0, 0.0], [0.3, 0.5, 0.9, 1.1, 1.4, 2.0, 2.2, 3.1]])
    return idx, dist


def test_membership_special_rows(ctx):
    idx, dist = special_rows()
    Y = yref(12, 2)
    info = check_membership(ctx, idx, dist, Y, "special rows")
    assert (info["rows_no_root"], info["rows_clamped"], info["rows_all_zero"], info["rows_start_nearest"]) == (3, 3, 1, 0)
    w, sigma = info["weights"], info["sigma"]
    assert sigma[0] == 1e-3 * 10.0 / 8.0 and sigma[1] == 0.0 and sigma[2] == np.inf and sigma[3] == 1e-3 * 4000.0 / 8.0
    assert (w[1] == 1.0).all() and (w[2] == 1.0).all()
    assert sorted(w[3].tolist()) == [0.0] * 4 + [1.0] * 4
    assert np.array_equal(info["start"][1], ref.start(np.ones((1, 8)), np.sort(idx[1:2], axis=1), Y, np.array([0]))[0][0])


def test_membership_does_not_depend_on_the_order_within_a_row(ctx):
    rng = np.random.default_rng(8)
    for kq, nq in ((9, 33), (64, 31), (16, 257)):
        idx, dist = knn_list(nq, kq, N_REF)
        perm = np.stack([rng.permutation(kq) for _ in range(nq)])
        idx2, dist2 = np.take_along_axis(idx, perm, axis=1), np.take_along_axis(dist, perm, axis=1)
        Y = yref(N_REF, 3)
        e1, i1 = run(ctx, idx, dist, Y, n_epochs=3, seed=4, parts=True)
        e2, i2 = run(ctx, idx2, dist2, Y, n_epochs=3, seed=4, parts=True)
        assert np.array_equal(e1.view(np.uint64), e2.view(np.uint64)) and i1["samples"] == i2["samples"] > 0
        for k in ("start", "weights", "columns", "sigma"):
            assert np.array_equal(i1[k].view(np.uint8), i2[k].view(np.uint8)), k
    idx, dist = special_rows()
    perm = np.stack([rng.permutation(8) for _ in range(len(idx))])
    a = run(ctx, idx, dist, yref(12, 2), n_epochs=2, parts=True)[1]
    b = run(ctx, np.take_along_axis(idx, perm, axis=1), np.take_along_axis(dist, perm, axis=1), yref(12, 2), n_epochs=2, parts=True)[1]
    for k in ("start", "weights", "columns", "sigma"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


# ---- b. positions and counters of the transform -----------------------------------------------------------------------------------
_START = {}


def reference(nq, kq, dim, rate, E, stop):
    """(Y f64, counters, D) of the definition for the list (nq, kq, N_REF); the membership and start are computed once per list."""
    key = (nq, kq, dim)
    if key not in _START:
        m, ml = memb(nq, kq, N_REF)
        Y = yref(N_REF, dim)
        _START[key] = (ref.start(m["w"], m["cols"], Y, m["nearest"])[0], ref.start(ml["w"], ml["cols"], Y, ml["nearest"], np.longdouble)[0])
    m, _ = memb(nq, kq, N_REF)
    y0, y0l = _START[key]
    Y = yref(N_REF, dim)
    out, c = ref.epochs(m["cols"], m["w"], Y, y0, A, B, E, rate=rate, seed=11, stop_after=stop)
    outl, cl = ref.epochs(m["cols"], m["w"], Y, y0l, A, B, E, rate=rate, seed=11, stop_after=stop, dtype=np.longdouble)
    assert c == cl
    return out, c, gap(out, outl)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kq", KQS)
def test_counters_and_positions(ctx, kq, dim):
    for nq in NQS:
        idx, dist = knn_list(nq, kq, N_REF)
        for rate in RATES:
            for E, stop in SCHEDULES:
                Y, want, D = reference(nq, kq, dim, rate, E, stop)
                emb, info = run(ctx, idx, dist, yref(N_REF, dim), n_epochs=E, stop_after=stop, negative_sample_rate=rate, seed=11)
                err = float(np.abs(emb - Y).max()) if Y.size else 0.0
                print("kq %d nq %d dim %d R %d E %d stop %d: samples %d negatives %d active %d | D %.3e 32D %.3e device %.3e"
                      % (kq, nq, dim, rate, E, stop, info["samples"], info["negatives"], info["entries_active"], D, TOL_FACTOR * D, err))
                assert emb.shape == (nq, dim) and emb.dtype == np.float64 and np.isfinite(emb).all()
                for k in ("entries_active", "samples", "negatives"):
                    assert info[k] == want[k], (k, info[k], want[k])
                assert info["negatives"] == info["samples"] * rate
                assert info["n_epochs"] == E and info["epochs_run"] == (want["epochs_run"] if nq else 0)
                if nq:
                    assert info["w_max"] == want["w_max"] and info["samples"] > 0
                assert (info["a"], info["b"]) == (A, B)
                assert err <= TOL_FACTOR * D


# ---- c. chunked launches and stop_after ----------------------------------------------------------------------------------------------
def test_chunks_and_stop_after(ctx):
    chunk = ref.CHUNK
    E = 3 * chunk + 5
    nq, kq = 257, 16
    idx, dist = knn_list(nq, kq, N_REF)
    Y = yref(N_REF, 2)
    m, _ = memb(nq, kq, N_REF)
    y0 = ref.start(m["w"], m["cols"], Y, m["nearest"])[0]
    for s in (chunk - 1, chunk, chunk + 1, E):
        # one launch per epoch IS the schedule's first s epochs, epoch by epoch; the chunked run must give its bits
        by_epoch, i1 = run(ctx, idx, dist, Y, n_epochs=E, stop_after=s, seed=5, chunk_epochs=1)
        chunked, ic = run(ctx, idx, dist, Y, n_epochs=E, stop_after=s, seed=5)
        odd, io = run(ctx, idx, dist, Y, n_epochs=E, stop_after=s, seed=5, chunk_epochs=7)
        again, ia = run(ctx, idx, dist, Y, n_epochs=E, stop_after=s, seed=5)
        for other, info in ((chunked, ic), (odd, io), (again, ia)):
            assert np.array_equal(by_epoch.view(np.uint64), other.view(np.uint64)), s
            assert {k: v for k, v in info.items() if "ms" not in k} == {k: v for k, v in i1.items() if "ms" not in k}
        assert ic["epochs_run"] == s and ic["n_epochs"] == E
        _, want = ref.epochs(m["cols"], m["w"], Y, y0, A, B, E, seed=5, stop_after=s)
        for k in ("entries_active", "samples", "negatives"):
            assert ic[k] == want[k], (s, k, ic[k], want[k])
    full, _ = run(ctx, idx, dist, Y, n_epochs=E, seed=5)
    assert np.array_equal(full.view(np.uint64), chunked.view(np.uint64))         # stop_after = E is the full run
    other, _ = run(ctx, idx, dist, Y, n_epochs=E, seed=6)
    assert not np.array_equal(full, other) and np.isfinite(full).all()


# ---- d. quality over a full run --------------------------------------------------------------------------------------------------------
def purity_margin(emb_ref, lab_ref, emb_q, lab_q):
    """(share of queries whose nearest cluster centroid in the embedding is their own cluster's, the smallest
    (d_other - d_own) / (d_other + d_own) over the queries: > 0 means every query is nearest to its own)."""
    groups = np.unique(lab_ref)
    cent = np.stack([emb_ref[lab_ref == g].mean(axis=0) for g in groups])
    d = np.sqrt(((emb_q[:, None, :] - cent[None, :, :]) ** 2).sum(axis=2))
    own = np.searchsorted(groups, lab_q)
    d_own = d[np.arange(len(d)), own]
    d_oth = np.where(np.arange(len(groups))[None, :] == own[:, None], np.inf, d).min(axis=1)
    return float((d.argmin(axis=1) == own).mean()), float(((d_oth - d_own) / (d_oth + d_own)).min())


def test_quality_over_a_full_run(ctx):
    """Held-out points around the planted clusters land in their own cluster of the fitted layout: purity 1.0, for the host
    restatement and for the device alike.  The restatement's margin (purity_margin's second figure) on this input, with a layout
    of umap_ref.layout in place of the device's: 0.81, and on the device's own layout 0.665 (0 would be a query as near to
    another centroid as to its own)."""
    from scipy.spatial import cKDTree
    from singlerust_amd.memory.processing import umap_csr
    x, lab, W = umap_ref.planted()
    layout, li = umap_csr(ctx, W, n_epochs=200, seed=1, init="random")
    rng = np.random.default_rng(77)
    pick = rng.choice(len(x), 200, replace=False)
    q = x[pick] + 0.5 * rng.standard_normal((200, x.shape[1]))
    dist, idx = cKDTree(x).query(q, k=16)
    idx = idx.astype(np.uint32)
    Yr, ir, _ = ref.transform(idx, dist, layout, li["a"], li["b"])
    pr, mr = purity_margin(layout, lab, Yr, lab[pick])
    emb, info = run(ctx, idx, dist, layout, a=0.0, b=0.0)
    pd_, md = purity_margin(layout, lab, emb, lab[pick])
    print("purity / margin: restatement %.3f / %.3f, device %.3f / %.3f | samples %d ms %.3f" % (pr, mr, pd_, md, info["samples"], info["ms"]))
    assert (info["a"], info["b"]) == (li["a"], li["b"])                          # a = b = 0: the curve the fit itself was given
    assert info["n_epochs"] == info["epochs_run"] == 100 and info["kq"] == 16 and np.isfinite(emb).all()
    assert all(info[k] == ir[k] for k in ("samples", "entries_active", "negatives", "rows_no_root", "rows_clamped"))
    assert pr == 1.0 and mr > 0.0                                                # the restatement itself reaches it
    assert pd_ == 1.0


# ---- e. the vote ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_groups", (1, 2, 65, 70000))
@pytest.mark.parametrize("k", (1, 2, 63, 64))
def test_vote(ctx, k, n_groups):
    from singlerust_amd.memory.processing import knn_vote
    rng = np.random.default_rng(k * 100003 + n_groups)
    n_ref = 1000
    hi, lo = n_groups - 1, max(n_groups - 3, 0)
    # references 0..63 carry the highest label, 64..127 a lower one; the others few labels (ties by chance) or all distinct ones
    labels = np.where(np.arange(n_ref) < 500, rng.integers(0, min(n_groups, 3), n_ref), (np.arange(n_ref) * 7 + 1) % n_groups)
    labels[:64], labels[64:128] = hi, lo
    labels = labels.astype(np.uint32)
    rows = [np.argsort(rng.random(n_ref))[:k] for _ in range(257)]
    # a tie at every count c: c references of each of the two labels, the rest with labels of their own where there are enough
    spare = np.arange(500, n_ref)
    spare = spare[(labels[spare] != hi) & (labels[spare] != lo)]
    _, first = np.unique(labels[spare], return_index=True)
    spare = spare[first]                                                         # one reference per remaining label
    ties = 0
    for c in range(1, k // 2 + 1):
        rest = k - 2 * c
        if hi != lo and rest <= len(spare):
            rows.append(np.concatenate([rng.permutation(64)[:c], 64 + rng.permutation(64)[:c], rng.permutation(spare)[:rest]]))
            ties += 1
    idx = np.stack([rng.permutation(r) for r in rows]).astype(np.uint32)
    want_l, want_c = ref.vote(idx, labels)
    got_l, conf = knn_vote(ctx, idx, labels, n_groups)
    print("k %d n_groups %d: %d rows, %d built ties, counts %s" % (k, n_groups, len(idx), ties, np.unique(want_c)[:8]))
    assert got_l.dtype == np.uint32 and np.array_equal(got_l, want_l)
    assert np.array_equal(conf, want_c.astype(np.float64) / k)
    if n_groups >= 65:
        assert ties == k // 2
        if k >= 2:
            assert (want_l[257:][want_c[257:] > 1] == lo).all()                  # the lower of the two tied labels
    # the other block lengths
    for nq in (0, 1, 3, 4, 5):
        l2, c2 = knn_vote(ctx, idx[:nq], labels, n_groups)
        assert np.array_equal(l2, want_l[:nq]) and np.array_equal(c2, want_c[:nq].astype(np.float64) / k)


# ---- f. the resident path ----------------------------------------------------------------------------------------------------------------------
def test_resident_path(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import (KnnIndex, dim_red, graph_embedding, graph_labels, ingest, knn_index_points, knn_points,
                                                  knn_vote, louvain, neighbors, umap, umap_transform)
    from test_knn_gpu import _planted, _upload
    x = _planted()
    a = _upload(ctx, x)
    dim_red.pca_inplace(a, 20, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    neighbors(a, n_neighbors=15, connectivities=True)
    rows = np.arange(0, x.shape[0], 5)
    q = _upload(ctx, x[rows])
    with pytest.raises(sr.SrxError):
        ingest(q, a)                                                             # no labels yet
    louvain(a)
    with pytest.raises(sr.SrxError):
        ingest(q, a)                                                             # no embedding yet
    umap(a, init="pca", n_epochs=50, seed=2)
    before = (graph_embedding(a._graph).copy(), graph_labels(a._graph).copy())
    out = ingest(q, a, n_epochs=20, seed=3)
    assert out is q.uns["ingest"] and out["params"]["n_neighbors"] == 16 and out["info"]["kq"] == 16
    assert out["info"]["n_ref"] == a.n_obs() and out["info"]["epochs_run"] == 20
    # the same through the host-pointer entries, fed with the fetched scores, labels and embedding: the same bits
    scores = q.obsm["X_pca"]
    idx, dist, _ = knn_points(ctx, a.obsm["X_pca"], scores, k=16)
    lab, conf = knn_vote(ctx, idx, before[1])
    emb, info = umap_transform(ctx, idx, dist, before[0], n_epochs=20, seed=3)
    assert np.array_equal(q.obs["louvain"], lab) and np.array_equal(q.obs["louvain_confidence"], conf)
    assert np.array_equal(q.obsm["X_umap"].view(np.uint64), emb.view(np.uint64))
    assert {k: v for k, v in info.items() if "ms" not in k} == {k: v for k, v in out["info"].items() if "ms" not in k}
    # a query cell that is a copy of a reference cell: that cell is its nearest neighbour, and it takes the cell's label
    # whenever the vote is not tied
    assert np.array_equal(idx[np.arange(len(rows)), np.argmin(dist, axis=1)], rows.astype(np.uint32))
    labs = before[1][idx.astype(np.int64)]
    top2 = np.sort(np.stack([np.bincount(r, minlength=int(before[1].max()) + 2) for r in labs]), axis=1)[:, -2:]
    untied = top2[:, 1] > top2[:, 0]
    print("copies: %d of %d votes untied, %d take their cell's label" % (untied.sum(), len(rows), (lab == before[1][rows]).sum()))
    assert untied.any() and np.array_equal(lab[untied], before[1][rows][untied])
    # the handle is as it was; three components replace the embedding and the transform follows
    assert np.array_equal(graph_embedding(a._graph).view(np.uint64), before[0].view(np.uint64))
    assert np.array_equal(graph_labels(a._graph), before[1])
    # the approximate search in place of the exact one: probing every list is the exact list
    ix = knn_index_points(ctx, a.obsm["X_pca"], n_lists=8, seed=1)
    q2 = _upload(ctx, x[rows])
    ingest(q2, a, index=ix, n_probe=8, n_epochs=20, seed=3)
    assert isinstance(ix, KnnIndex) and q2.uns["ingest"]["params"]["approximate"]
    assert np.array_equal(q2.obsm["X_umap"].view(np.uint64), emb.view(np.uint64)) and np.array_equal(q2.obs["louvain"], lab)
    ix.free()
    umap(a, init="pca", n_components=3, n_epochs=5)
    e3, i3 = umap_transform(ctx, idx, dist, a._graph, n_epochs=2)
    assert e3.shape == (len(rows), 3) and i3["dim"] == 3
    with pytest.raises(sr.SrxError) as err:
        umap_transform(ctx, idx, dist, a._graph, n_epochs=2, n_components=2)
    assert err.value.code == F.E_ARG and "components" in str(err.value)


# ---- g. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import connectivities_from_knn, knn_points
    lib = F.lib()
    nq, kq, n_ref = 5, 4, 12
    rng = np.random.default_rng(2)
    idx0 = np.argsort(rng.random((nq, n_ref)), axis=1)[:, :kq].astype(np.uint32)
    dist0 = rng.random((nq, kq)) + 0.1
    Y0 = rng.standard_normal((n_ref, 3))
    lab0 = rng.integers(0, 3, n_ref).astype(np.uint32)
    SENT = 12345.0

    def opts(**kw):
        d = dict(a=A, b=B, min_dist=0.5, spread=1.0, gamma=1.0, alpha0=0.25, seed=0, n_epochs=3, stop_after=0, negative_sample_rate=5,
                 chunk_epochs=0)
        d.update(kw)
        return F.UmapTransformOpts(*[d[name] for name, _ in F.UmapTransformOpts._fields_])

    def refused(o=None, idx=idx0, dist=dist0, Y=Y0, kq_=None, n_ref_=None, dim=3, c=None, graph=None):
        k = idx.shape[1] if kq_ is None else kq_
        bufs = [np.full((nq, 3), SENT), np.full((nq, 3), SENT), np.full((nq, 64), SENT), np.full((nq, 64), 0xABCD, dtype=np.uint32),
                np.full(nq, SENT)]
        out = F.UmapTransformOut(*[F.ptr(b) for b in bufs])
        info = F.UmapTransformInfo()
        info.samples = 777
        h = (c or ctx).handle
        o = o or opts()
        if graph is not None:
            rc = lib.srx_umap_transform_graph(graph, F.ptr(idx), F.ptr(dist), nq, k, dim, C.byref(o), C.byref(out), C.byref(info))
        else:
            rc = lib.srx_umap_transform_knn(h, F.ptr(idx), F.ptr(dist), nq, k, None if Y is None else F.ptr(Y),
                                            len(Y0) if n_ref_ is None else n_ref_, dim, C.byref(o), C.byref(out), C.byref(info))
        msg = lib.srx_last_error(h)
        assert rc == F.E_ARG and msg, (rc, msg)
        assert all((b == (0xABCD if b.dtype == np.uint32 else SENT)).all() for b in bufs) and info.samples == 777      # nothing written
        return msg.decode()

    def with_(arr, r, c_, v):
        b = arr.copy()
        b[r, c_] = v
        return b

    wide = np.argsort(rng.random((nq, 80)), axis=1)[:, :65].astype(np.uint32)
    assert "outside 3..64" in refused(kq_=2)
    assert "outside 3..64" in refused(idx=wide, dist=np.ones((nq, 65)), Y=np.zeros((80, 3)), n_ref_=80)
    assert "reference points" in refused(n_ref_=3)
    assert "not below n_ref" in refused(idx=with_(idx0, 2, 1, n_ref))
    assert "not below n_ref" in refused(idx=with_(idx0, 4, 3, 0xFFFFFFFF))
    assert "twice" in refused(idx=with_(idx0, 3, 0, idx0[3, 2]))
    for v in (-1e-300, np.nan, np.inf, -np.inf):
        assert "distance" in refused(dist=with_(dist0, 1, 2, v))
    for v in (np.nan, np.inf, -np.inf):
        assert "NaN or Inf" in refused(Y=with_(Y0, 7, 1, v))
    for d in (0, 1, 4):
        assert "not 2 or 3" in refused(dim=d)
    for r in (-1, 33):
        assert "negative_sample_rate" in refused(opts(negative_sample_rate=r))
    for v in (0.0, -1.0, np.nan, np.inf):
        assert "a and b" in refused(opts(a=v))
        assert "a and b" in refused(opts(b=v))
        assert "gamma" in refused(opts(gamma=v))
        assert "alpha0" in refused(opts(alpha0=v))
        assert "spread" in refused(opts(a=0.0, b=0.0, spread=v))
    assert "min_dist" in refused(opts(a=0.0, b=0.0, min_dist=1.5))
    for e in (-1, 2 ** 20 + 1):
        assert "n_epochs" in refused(opts(n_epochs=e))
    assert "stop_after" in refused(opts(n_epochs=3, stop_after=4))
    assert "stop_after" in refused(opts(stop_after=-1))
    for v in (-1, 65):
        assert "chunk_epochs" in refused(opts(chunk_epochs=v))
    assert "null" in refused(Y=None)
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    assert "sharded" in refused(c=c2)

    # the vote
    def vote_refused(idx=idx0, k=None, labels=lab0, n_groups=3, n_ref_=n_ref, c=None, graph=None):
        lo, co = np.full(nq, 0xABCD, dtype=np.uint32), np.full(nq, 0xABCD, dtype=np.uint32)
        h = (c or ctx).handle
        k = idx.shape[1] if k is None else k
        if graph is not None:
            rc = lib.srx_knn_vote_graph(graph, F.ptr(idx), nq, k, F.ptr(lo), F.ptr(co))
        else:
            rc = lib.srx_knn_vote(h, F.ptr(idx), nq, k, None if labels is None else F.ptr(labels), n_ref_, n_groups, F.ptr(lo), F.ptr(co))
        msg = lib.srx_last_error(h)
        assert rc == F.E_ARG and msg, (rc, msg)
        assert (lo == 0xABCD).all() and (co == 0xABCD).all()
        return msg.decode()

    assert "outside 1..64" in vote_refused(k=0)
    assert "outside 1..64" in vote_refused(idx=wide, k=65, labels=np.zeros(80, dtype=np.uint32), n_ref_=80)
    assert "reference points" in vote_refused(n_ref_=3)
    assert "not below n_ref" in vote_refused(idx=with_(idx0, 0, 0, n_ref))
    assert "twice" in vote_refused(idx=with_(idx0, 3, 0, idx0[3, 2]))
    assert "n_groups" in vote_refused(labels=with_(lab0[None, :], 0, 5, 3)[0])
    assert "n_groups" in vote_refused(n_groups=0)
    assert "null" in vote_refused(labels=None)
    assert "sharded" in vote_refused(c=c2)

    # a graph handle without labels or an embedding; a dim that is not the embedding's
    x = np.random.default_rng(4).standard_normal((40, 5))
    ki, kd, _ = knn_points(ctx, x, k=5)
    g = connectivities_from_knn(ctx, ki, kd)
    gi = np.argsort(rng.random((nq, 40)), axis=1)[:, :kq].astype(np.uint32)
    assert "no srx_louvain" in vote_refused(idx=gi, graph=g.handle)
    assert "no srx_umap" in refused(idx=gi, graph=g.handle, dim=2)
    emb = np.zeros((40, 2))
    o = F.UmapOpts(A, B, 0.5, 1.0, 1.0, 1.0, 0, 3, 0, 2, 5, F.UMAP_INIT_RANDOM, 0)
    F.check(lib.srx_umap(g.handle, None, C.byref(o), None, F.ptr(emb), None), ctx.handle)
    assert "components" in refused(idx=gi, graph=g.handle, dim=3)
    assert "not 2 or 3" in refused(idx=gi, graph=g.handle, dim=5)
    assert "not below n_ref" in refused(idx=with_(gi, 0, 0, 40), graph=g.handle, dim=2)
    # n_query == 0 writes nothing and succeeds; the context and the handle are still usable
    info = F.UmapTransformInfo()
    assert lib.srx_umap_transform_knn(ctx.handle, None, None, 0, kq, F.ptr(Y0), n_ref, 3, None, None, C.byref(info)) == F.OK
    assert info.n_query == 0 and info.samples == 0 and info.n_epochs == 100
    assert lib.srx_knn_vote(ctx.handle, None, 0, kq, F.ptr(lab0), n_ref, 3, None, None) == F.OK
    e, i = run(ctx, gi, dist0, g, n_epochs=3)
    assert i["epochs_run"] == 3 and np.isfinite(e).all() and np.array_equal(run(ctx, gi, dist0, emb, n_epochs=3)[0], e)
    g.free()

"""The weighted neighbour graph on the device (srx_neighbors_from_knn / srx_neighbors_result, through the C ABI) against
the host restatement of the definition in tests/graph_ref.py.

Tolerances are derived, not measured.  Each directed weight a_ij is non-decreasing in sigma and both sides solve the row
equation to |S - T| <= 1e-9, so two valid solutions differ by at most 2e-9 in every weight of an unclamped row; rounding
of exp adds ~1e-15; C = a + b - a b has partial derivatives in [0, 1].  With a factor of about five: directed weights
absolute 1e-8, C absolute 2e-8; rho, D and both sparsity patterns exact; sigma is compared through the row-sum equation
(1e-9) and, on clamped rows, to 4 ulp of the floor formula.  Entries far below the absolute tolerance (the lattice's
~1e-168) are compared to relative 1e-12.

The definition is umap-learn's fuzzy_simplicial_set as scanpy calls it, restated for rows without self; neither package
is installed here, so nothing in this file compares with their output."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import graph_ref

pytestmark = pytest.mark.gpu

TOL_A, TOL_C, TOL_SUM = 1e-8, 2e-8, 1e-9
FIGURES = {}                               # label -> (max |a - a_ref|, max |sum a - T|, max |C - C_ref|) of the last comparison


# ---- helpers --------------------------------------------------------------------------------------------------------
def knn_list(ctx, x, k):
    from singlerust_amd.memory.processing import knn_points
    idx, dist, _ = knn_points(ctx, x, k=k)
    return idx, dist


def build(ctx, idx, dist):
    from singlerust_amd.memory.processing.neighbors import connectivities_from_knn
    return connectivities_from_knn(ctx, idx, dist)


def fetch_all(g):
    from singlerust_amd import _ffi as F
    info = g.info()
    d = g.fetch(F.GRAPH_DISTANCES)
    c = g.fetch(F.GRAPH_CONNECTIVITIES)
    rho, sigma = g.scales()
    return info, d, c, rho, sigma


def as_csr(triple, n):
    ptr, ind, dat = triple
    return sp.csr_matrix((dat, ind.astype(np.int64), ptr.astype(np.int64)), shape=(n, n))


def check_properties(info, d, c):
    """Properties every result has: consistent indptr, ascending unique columns, no diagonal, 0 < C <= 1, C == C^T bitwise."""
    n, k = info["n"], info["k"]
    for (ptr, ind, dat), nnz in ((d, info["nnz_distances"]), (c, info["nnz_connectivities"])):
        assert ptr.dtype == np.uint64 and ind.dtype == np.uint32 and dat.dtype == np.float64
        assert len(ptr) == n + 1 and ptr[0] == 0 and ptr[-1] == nnz == len(ind) == len(dat)
        lens = np.diff(ptr.astype(np.int64))
        assert (lens >= 0).all()
        if nnz:
            assert ind.max() < n
            rows = np.repeat(np.arange(n), lens)
            assert (ind != rows).all()                                        # no diagonal
            same_row = rows[1:] == rows[:-1]
            assert (np.diff(ind.astype(np.int64))[same_row] > 0).all()        # ascending, unique
    assert info["nnz_distances"] == n * k and (np.diff(d[0].astype(np.int64)) == k).all()
    cdat = c[2]
    assert ((cdat > 0) & (cdat <= 1)).all()
    cm = as_csr(c, n)
    ct = cm.T.tocsr()
    ct.sort_indices()
    assert np.array_equal(ct.indptr, cm.indptr) and np.array_equal(ct.indices, cm.indices)
    assert np.array_equal(ct.data.view(np.uint64), cm.data.view(np.uint64))  # the same bits on both sides
    assert info["max_row_nnz"] == (int(np.diff(c[0].astype(np.int64)).max()) if n else 0)


def check_against_restatement(idx, dist, got, label, rel_small=False):
    """Everything the restatement defines; returns (restated info, per-row dict)."""
    info, d, c, rho, sigma = got
    n, k = idx.shape
    D, Cr, sc, A, want = graph_ref.graph(idx, dist)
    check_properties(info, d, c)
    # D and rho: exact
    assert np.array_equal(d[0].astype(np.int64), D.indptr) and np.array_equal(d[1].astype(np.int64), D.indices)
    assert np.array_equal(d[2], D.data)
    assert np.array_equal(rho, sc["rho"])
    # counters
    print(label, "device", info)
    print(label, "restatement", want)
    assert info == want, (label, info, want)
    # directed weights, recovered from rho, sigma and D's rows
    dd = d[2].reshape(n, k)
    a_dev = graph_ref.weights(dd, rho, sigma)
    a_ref = A.data.reshape(n, k)                                              # A is in D's (column) order
    err_a = np.abs(a_dev - a_ref).max()
    T = sc["T"]
    free = sc["has_root"] & ~sc["clamped"]
    err_sum = np.abs(a_dev[free].sum(axis=1) - T).max() if free.any() else 0.0
    ref_sum = np.abs(a_ref[free].sum(axis=1) - T).max() if free.any() else 0.0
    print(f"{label}: max |a - a_ref| {err_a:.3e}; unclamped rows with a root {int(free.sum())}: max |sum a - T| device "
          f"{err_sum:.3e}, restatement {ref_sum:.3e}")
    assert err_a <= TOL_A, (label, err_a)
    assert err_sum <= TOL_SUM, (label, err_sum)
    assert ref_sum <= 1e-12, (label, ref_sum)
    # sigma on clamped rows: the floor formula to 4 ulp; all-zero rows: 0
    cl = sc["clamped"]
    over = cl & np.isinf(sc["floor"])                                         # sum d overflowed: the floor is +inf, so is sigma
    assert (sigma[over] == np.inf).all(), (label, sigma[over])
    cl = cl & ~over                                                           # (inf - inf has no ulp distance)
    if cl.any():
        ulps = np.abs(sigma[cl] - sc["floor"][cl]) / np.spacing(sc["floor"][cl])
        print(f"{label}: clamped rows {int(cl.sum())}, sigma within {ulps.max():.1f} ulp of the floor")
        assert ulps.max() <= 4, (label, ulps.max())
    assert (sigma[sc["all_zero"]] == 0).all() and (sigma[~sc["all_zero"]] > 0).all()
    # C: pattern exact, values
    assert np.array_equal(c[0].astype(np.int64), Cr.indptr) and np.array_equal(c[1].astype(np.int64), Cr.indices)
    err_c = np.abs(c[2] - Cr.data).max() if Cr.nnz else 0.0
    print(f"{label}: nnz_C / (n k) = {Cr.nnz / max(n * k, 1):.3f}, max |C - C_ref| {err_c:.3e}, smallest C {c[2].min() if Cr.nnz else 0:.3e}")
    assert err_c <= TOL_C, (label, err_c)
    FIGURES[label] = (err_a, err_sum, err_c)
    if rel_small:
        rel = np.abs(c[2] - Cr.data) / Cr.data
        print(f"{label}: max relative error of C {rel.max():.3e}")
        assert rel.max() <= 1e-12, (label, rel.max())
    return want, sc


def gaussian(n, d, seed=7):
    return np.random.default_rng(seed).standard_normal((n, d))


# ---- 1. generic -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k", [(4000, 50, 15), (3000, 10, 30), (2000, 3, 5), (3000, 50, 64), (500, 2, 1)])
def test_generic(ctx, n, d, k):
    x = gaussian(n, d)
    idx, dist = knn_list(ctx, x, k)
    g = build(ctx, idx, dist)
    got = fetch_all(g)
    want, sc = check_against_restatement(idx, dist, got, f"gaussian {n}x{d} k={k}")
    if k == 1:                                           # T = 1 = c: no root anywhere, the one weight is 1
        assert want["rows_no_root"] == n and want["rows_clamped"] == n and (got[2][2] == 1.0).all()
    else:
        assert want["rows_no_root"] == 0 and want["rows_clamped"] == 0
        assert 1.2 <= want["nnz_connectivities"] / (n * k) <= 1.75
    # unsorted input rows give the same graph, and a second call is bit-identical
    rng = np.random.default_rng(1)
    perm = np.argsort(rng.random(idx.shape), axis=1)
    g2 = build(ctx, np.take_along_axis(idx, perm, axis=1), np.take_along_axis(dist, perm, axis=1))
    g3 = build(ctx, idx, dist)
    for other in (fetch_all(g2), fetch_all(g3)):
        assert other[0] == got[0]
        for a, b in zip(got[1] + got[2] + (got[3], got[4]), other[1] + other[2] + (other[3], other[4])):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 2. ties ----------------------------------------------------------------------------------------------------------
def test_lattice_ties(ctx):
    """30 x 30 unit lattice, k = 8: the 784 interior rows have c = 4 >= log2 9, so no root and the floor applies; their
    diagonal neighbours get exp(-(sqrt 2 - 1) / floor) ~ 2e-168.  These entries must be present and right to 1e-12 relative."""
    p = np.array(np.meshgrid(np.arange(30.0), np.arange(30.0), indexing="ij")).reshape(2, -1).T
    idx, dist = knn_list(ctx, p, 8)
    got = fetch_all(build(ctx, idx, dist))
    want, sc = check_against_restatement(idx, dist, got, "lattice", rel_small=True)
    assert want["rows_no_root"] == 784 and want["rows_clamped"] == 784
    assert want["entries_dropped"] == 0
    smallest = got[2][2].min()
    print("lattice: smallest C entry", smallest, "nnz_C", want["nnz_connectivities"])
    assert 1e-169 < smallest < 1e-167


def test_exact_duplicates(ctx):
    """A block of k + 1 identical points (all-zero rows: rho = sigma = 0, weights 1) and a pair of duplicates inside a generic
    cloud (d = 0 < rho: weight 1, counted in c)."""
    k = 5
    x = gaussian(600, 4, seed=21)
    x[100:100 + k + 1] = x[100]
    x[300] = x[301]
    idx, dist = knn_list(ctx, x, k)
    got = fetch_all(build(ctx, idx, dist))
    want, sc = check_against_restatement(idx, dist, got, "duplicates")
    assert want["rows_all_zero"] == k + 1 and np.array_equal(np.nonzero(sc["all_zero"])[0], np.arange(100, 106))
    cm = as_csr(got[2], 600)
    assert (cm[100:106][:, 100:106].toarray()[~np.eye(6, dtype=bool)] == 1.0).all()
    assert dist[300].min() == 0.0 and got[3][300] > 0 and cm[300, 301] == 1.0 and cm[301, 300] == 1.0


# ---- 3. underflow ------------------------------------------------------------------------------------------------------
def underflow_list(n=200, k=15):
    """Every row: four neighbours at distance 1 (offsets +-1, +-2: c = 4 = log2 16, no root, sigma = the floor) and eleven far
    ones: offsets +3..+9 (their reverse is absent), +-20 and +-22.  Rows with i % 4 == 0 have their far neighbours at distance 2
    ((d - rho) / sigma = 615: the weight exists), the others at 3 (865: it underflows to 0).  +-20 joins rows of one class
    (both weights present, or both zero), +-22 joins a present row with a zero one."""
    off = np.array([1, -1, 2, -2, 3, 4, 5, 6, 7, 8, 9, 20, -20, 22, -22])
    i = np.arange(n)
    idx = ((i[:, None] + off[None, :]) % n).astype(np.uint32)
    far = np.where(i % 4 == 0, 2.0, 3.0)
    dist = np.concatenate([np.ones((n, 4)), np.repeat(far[:, None], 11, axis=1)], axis=1)
    ratio = (far - 1.0) / (1e-3 * dist.sum(axis=1) / (k + 1))
    assert ((ratio < 700) | (ratio > 800)).all() and (ratio < 700).any() and (ratio > 800).any()
    return idx, dist


def test_underflow_entries_are_dropped(ctx):
    idx, dist = underflow_list()
    n = len(idx)
    got = fetch_all(build(ctx, idx, dist))
    want, sc = check_against_restatement(idx, dist, got, "underflow")
    assert want["rows_no_root"] == n and want["rows_clamped"] == n
    cm = as_csr(got[2], n).tolil()
    stored = as_csr((got[2][0], got[2][1], np.ones_like(got[2][2])), n).toarray() > 0
    # row 1 (zero class): +3 has no reverse edge and underflows: absent on both sides; row 0 (present class): there
    assert not stored[1, 4] and not stored[4, 1]
    assert stored[0, 3] and stored[3, 0] and 0 < cm[0, 3] < 1e-200
    # +-20 inside a class: both zero -> absent; both present -> there
    assert not stored[1, 21] and not stored[21, 1] and stored[0, 20] and stored[20, 0]
    # +-22 joins 0 (present) and 22 (zero): the pair keeps the one weight
    assert stored[0, 22] and stored[22, 0] and cm[0, 22] == cm[22, 0] > 0
    # 150 zero rows: 7 one-directional zeros (two entries each) + 2 at +-20 (one per side); the 100 of them with odd i meet
    # another zero row at +-22 as well
    assert want["entries_dropped"] == 150 * (7 * 2 + 2) + 100 * 2 == 2600
    assert got[0]["entries_dropped"] == 2600


# ---- 4. hub --------------------------------------------------------------------------------------------------------------
def test_hub_row(ctx):
    """Cell 0 is a neighbour of every other cell (in-degree n - 1 with n = 150 000: the in-list ordering walks more than one
    bitmap window): its row of C is complete, sorted and right."""
    n, k = 150_000, 5
    rng = np.random.default_rng(31)
    i = np.arange(1, n)
    others = ((i[:, None] - 1 + np.arange(1, k)[None, :]) % (n - 1)) + 1          # four cells of the ring 1..n-1, never i, never 0
    idx = np.zeros((n, k), dtype=np.uint32)
    idx[1:, 0] = 0
    idx[1:, 1:] = others
    idx[0] = np.arange(1, k + 1)
    dist = rng.uniform(0.5, 2.0, (n, k))
    got = fetch_all(build(ctx, idx, dist))
    want, sc = check_against_restatement(idx, dist, got, "hub")
    assert got[0]["max_row_nnz"] == n - 1
    ptr, ind, dat = got[2]
    assert ptr[1] == n - 1 and np.array_equal(ind[:n - 1], np.arange(1, n, dtype=np.uint32))


HUB_LENGTHS = (1, 2, 63, 64, 65, 511, 512, 513, 1024)        # in-only entries: both sides of a wave and of the short-list limit


def hub_list(n=3000, k=5, seed=33):
    """Nine hubs with in-only lists of exactly HUB_LENGTHS entries: every other cell names four cells of the ring of
    non-hubs behind it, and its first neighbour is its hub (the sources) or one more cell of the ring (the rest); a hub names
    five cells of the rest, so nobody names a hub back.  Cell numbers are shuffled: the lists arrive in no order."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(n).astype(np.uint32)
    hubs, ring = ids[:len(HUB_LENGTHS)], ids[len(HUB_LENGTHS):]
    m = len(ring)
    assert sum(HUB_LENGTHS) + k <= m
    idx = np.zeros((n, k), dtype=np.uint32)
    idx[ring] = ring[(np.arange(m)[:, None] + np.arange(1, k + 1)[None, :]) % m]
    sources, at = {}, 0
    for h, length in zip(hubs, HUB_LENGTHS):
        sources[int(h)] = np.sort(ring[at:at + length])
        idx[ring[at:at + length], 0] = h
        at += length
    idx[hubs] = ring[at:at + k]                                # cells that name no hub
    return idx, rng.uniform(0.5, 2.0, (n, k)), sources


def test_hub_rows_at_the_list_length_edges(ctx):
    idx, dist, sources = hub_list()
    n, k = idx.shape
    B = sp.csr_matrix((np.ones(n * k, bool), idx.ravel().astype(np.int64), np.arange(0, n * k + 1, k)), shape=(n, n))
    in_only = (B.T > B).tocsr()                                # j names i and i does not name j
    in_only.sort_indices()
    for (h, src), length in zip(sources.items(), HUB_LENGTHS):
        assert len(src) == length and np.array_equal(in_only[h].indices, src)
    got = fetch_all(build(ctx, idx, dist))
    check_against_restatement(idx, dist, got, "hub lengths")
    ptr, ind, dat = got[2]
    for h, src in sources.items():
        cols = ind[int(ptr[h]):int(ptr[h + 1])]
        assert np.array_equal(cols, np.sort(np.concatenate([idx[h], src])))
        assert np.array_equal(cols[~np.isin(cols, idx[h])], src)


# ---- 6. resident path ---------------------------------------------------------------------------------------------------
def _pipeline_matrix(ctx, cells=6000, genes=1500, n_pc=20):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    lib = F.lib()
    p = F.SynthParams()
    lib.srx_synth_defaults(C.byref(p), 77, cells, genes, 0.05)
    h = C.c_void_p()
    F.check(lib.srx_synth_generate(ctx.handle, C.byref(p), 0, cells, F.F32, F.STORE_F32, C.byref(h)), ctx.handle)
    ad = sr.IMAnnData(sr.DeviceCsr(ctx, h), None, None, [], [])
    opts = F.PcaOpts(n_pc, -1, -1, -1, 0, 0, 0, 0.0, 12345)
    res = F.PipelineResult()
    F.check(lib.srx_pipeline(ad.x().handle, 1e4, 400, C.byref(opts), C.byref(res)), ctx.handle)
    return ad, int(res.pca.n_pc)


def _scores(ad, n_pc):
    from singlerust_amd import _ffi as F
    out = np.zeros((ad.n_obs(), n_pc))
    F.check(F.lib().srx_result_fetch(ad.x().handle, F.ptr(out), None, None, None, None, None), ad.x().ctx.handle)
    return out


def test_resident_path(ctx):
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import neighbors
    from singlerust_amd.memory.processing.neighbors import Graph
    lib = F.lib()
    ad, n_pc = _pipeline_matrix(ctx)
    n, k = ad.n_obs(), 15
    before = _scores(ad, n_pc)
    # the two-step route: list to the host, graph of the list
    opts = F.KnnOpts(k, 0, 0, 0)
    idx, dist = np.zeros((n, k), np.uint32), np.zeros((n, k))
    F.check(lib.srx_knn_result(ad.x().handle, C.byref(opts), F.ptr(idx), F.ptr(dist), None), ctx.handle)
    two = fetch_all(build(ctx, idx, dist))
    # the resident route
    h, kinfo = C.c_void_p(), F.KnnInfo()
    F.check(lib.srx_neighbors_result(ad.x().handle, C.byref(opts), C.byref(kinfo), C.byref(h)), ctx.handle)
    g = Graph(ctx, h)
    one = fetch_all(g)
    assert kinfo.n_query == n and kinfo.k == k and kinfo.rows_certified + kinfo.rows_recomputed == n
    assert one[0] == two[0]
    for a, b in zip(one[1] + one[2] + (one[3], one[4]), two[1] + two[2] + (two[3], two[4])):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    check_against_restatement(idx, dist, one, "resident")
    assert np.array_equal(_scores(ad, n_pc), before)                         # the PCA result is still there, unchanged
    # a later k-NN call does not touch the handle's buffers
    F.check(lib.srx_knn_result(ad.x().handle, C.byref(F.KnnOpts(7, 0, 0, 0)), None, None, None), ctx.handle)
    again = fetch_all(g)
    assert np.array_equal(again[2][2], one[2][2]) and np.array_equal(again[1][1], one[1][1])
    # include_self = 1 is refused
    h2 = C.c_void_p()
    assert lib.srx_neighbors_result(ad.x().handle, C.byref(F.KnnOpts(k, 0, 1, 0)), None, C.byref(h2)) == F.E_ARG
    assert not h2.value and b"include_self" in lib.srx_last_error(ctx.handle)
    # the Python mirror
    u = neighbors(ad, n_neighbors=k, connectivities=True, knn_lists=True)
    assert u["graph"] == one[0] and u["info"]["k"] == k and u["params"]["n_neighbors"] == k
    cm, dm = ad.obsp["connectivities"], ad.obsp["distances"]
    assert sp.issparse(cm) and cm.shape == (n, n) and cm.nnz == one[0]["nnz_connectivities"]
    assert np.array_equal(cm.data, one[2][2]) and np.array_equal(cm.indices, one[2][1])
    assert np.array_equal(dm.data, one[1][2]) and np.array_equal(dm.indptr, one[1][0].astype(np.int64))
    assert np.array_equal(ad.obsm["knn_indices"], idx) and np.array_equal(ad.obsm["knn_distances"], dist)
    assert ad._graph.info() == one[0]
    with pytest.raises(F.SrxError):
        neighbors(ad, n_neighbors=k, connectivities=True, include_self=True)
    # the default call behaves as before
    ad.obsm.clear()
    v = neighbors(ad, n_neighbors=k)
    assert "graph" not in v and np.array_equal(ad.obsm["knn_indices"], idx)


# ---- 7. errors ----------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    lib = F.lib()
    x = gaussian(300, 5, seed=41)
    idx, dist = knn_list(ctx, x, 6)
    good = fetch_all(build(ctx, idx, dist))

    def refused(i, d, word, n=None, k=None, c=ctx):
        h = C.c_void_p(1)
        n = len(i) if n is None else n
        k = i.shape[1] if k is None else k
        rc = lib.srx_neighbors_from_knn(c.handle, F.ptr(i), F.ptr(d), n, k, C.byref(h))
        msg = lib.srx_last_error(c.handle).decode()
        assert rc == F.E_ARG and not h.value and word in msg, (rc, h.value, msg)

    def with_(arr, r, c_, v):
        out = arr.copy()
        out[r, c_] = v
        return out

    wide = np.zeros((300, 65), np.uint32)
    refused(wide, np.zeros((300, 65)), "outside 1..64")
    refused(idx, dist, "outside 1..64", k=0)
    refused(idx[:6], dist[:6], "only 5 others")                           # k = 6 > n - 1
    refused(with_(idx, 17, 2, 300), dist, "not below n")
    refused(with_(idx, 17, 2, 0xFFFFFFFF), dist, "not below n")
    refused(with_(idx, 17, 2, 17), dist, "names itself")
    refused(with_(idx, 17, 2, idx[17, 4]), dist, "twice")
    for v, in ((-1.0,), (np.nan,), (np.inf,), (-np.inf,)):
        refused(idx, with_(dist, 250, 0, v), "negative, NaN or Inf")
    assert lib.srx_neighbors_from_knn(ctx.handle, F.ptr(idx), F.ptr(dist), 300, 6, None) == F.E_ARG       # NULL out
    h = C.c_void_p()
    assert lib.srx_neighbors_from_knn(None, F.ptr(idx), F.ptr(dist), 300, 6, C.byref(h)) == F.E_ARG
    assert lib.srx_neighbors_from_knn(ctx.handle, None, F.ptr(dist), 300, 6, C.byref(h)) == F.E_ARG
    assert lib.srx_neighbors_result(None, C.byref(F.KnnOpts(5, 0, 0, 0)), None, C.byref(h)) == F.E_ARG
    assert lib.srx_graph_info_get(None, None) == F.E_ARG and lib.srx_graph_fetch(None, 0, None, None, None) == F.E_ARG
    lib.srx_graph_free(None)
    # a matrix without a PCA result; a NULL out on the resident entry
    m = sp.random(50, 30, density=0.3, format="csr", random_state=np.random.RandomState(1))
    a = sr.IMAnnData.new_basic(m, ctx=ctx, store=2)
    assert lib.srx_neighbors_result(a.x().handle, C.byref(F.KnnOpts(5, 0, 0, 0)), None, C.byref(h)) == F.E_ARG
    assert b"no PCA result" in lib.srx_last_error(ctx.handle)
    assert lib.srx_neighbors_result(a.x().handle, C.byref(F.KnnOpts(5, 0, 0, 0)), None, None) == F.E_ARG
    # a context with more than one rank (host transport)
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    refused(idx, dist, "sharded", c=c2)
    # a bad `which`
    g = build(ctx, idx, dist)
    assert lib.srx_graph_fetch(g.handle, 2, None, None, None) == F.E_ARG
    # n = 0: an empty graph
    h0 = C.c_void_p()
    F.check(lib.srx_neighbors_from_knn(ctx.handle, None, None, 0, 5, C.byref(h0)), ctx.handle)
    from singlerust_amd.memory.processing.neighbors import Graph
    g0 = Graph(ctx, h0)
    i0 = g0.info()
    assert i0["n"] == 0 and i0["nnz_connectivities"] == 0 and i0["nnz_distances"] == 0 and i0["k"] == 5
    for which in (0, 1):
        ptr, ind, dat = g0.fetch(which)
        assert ptr.tolist() == [0] and len(ind) == 0 and len(dat) == 0
    # and the context still computes the same graph
    after = fetch_all(build(ctx, idx, dist))
    assert after[0] == good[0] and np.array_equal(after[2][2], good[2][2]) and np.array_equal(after[2][1], good[2][1])


# ---- 8. a larger run, sampled -----------------------------------------------------------------------------------------
@pytest.mark.timeout(1500)
def test_larger_run_sampled(ctx):
    """300 000 x 50 Gaussian, k = 15 through the points path: symmetry, row sums and the properties on the whole device
    output; the restatement on 3000 sampled rows (the in-edges of a sampled row come from the fetched k-NN list)."""
    n, d, k = 300_000, 50, 15
    x = gaussian(n, d, seed=51)
    idx, dist = knn_list(ctx, x, k)
    got = fetch_all(build(ctx, idx, dist))
    info, dtr, ctr, rho, sigma = got
    print("300000 x 50:", info)
    check_properties(info, dtr, ctr)
    sc, a_ref = graph_ref.scales(dist)                                        # rows in the list's own order
    order = np.argsort(idx, axis=1)
    assert np.array_equal(dtr[1].reshape(n, k), np.take_along_axis(idx, order, axis=1))
    assert np.array_equal(dtr[2].reshape(n, k), np.take_along_axis(dist, order, axis=1))
    assert np.array_equal(rho, sc["rho"])
    a_dev = graph_ref.weights(dtr[2].reshape(n, k), rho, sigma)
    free = sc["has_root"] & ~sc["clamped"]
    err_sum = np.abs(a_dev[free].sum(axis=1) - sc["T"]).max()
    err_a = np.abs(a_dev - np.take_along_axis(a_ref, order, axis=1)).max()
    print(f"300000 x 50: unclamped rows with a root {int(free.sum())}, max |sum a - T| {err_sum:.3e}, max |a - a_ref| {err_a:.3e}")
    assert err_sum <= TOL_SUM and err_a <= TOL_A
    assert info["rows_no_root"] == int((~sc["has_root"]).sum()) and info["rows_clamped"] == int(sc["clamped"].sum())
    assert info["rows_all_zero"] == 0
    # sampled rows of C from the restated weights: out-edges of the row and the in-edges found in the list
    A = sp.csr_matrix((a_ref.ravel(), idx.ravel().astype(np.int64), np.arange(0, n * k + 1, k)), shape=(n, n))
    At = A.T.tocsr()
    rows = np.sort(np.random.default_rng(52).choice(n, 3000, replace=False))
    sub = A[rows] + At[rows] - A[rows].multiply(At[rows])
    sub = sub.tocsr()
    sub.eliminate_zeros()
    sub.sort_indices()
    cm = as_csr(ctr, n)[rows]
    cm.sort_indices()
    assert np.array_equal(cm.indptr, sub.indptr) and np.array_equal(cm.indices, sub.indices)
    err_c = np.abs(cm.data - sub.data).max()
    print(f"300000 x 50: 3000 sampled rows, max |C - C_ref| {err_c:.3e}; nnz_C / (n k) = {info['nnz_connectivities'] / (n * k):.3f}")
    assert err_c <= TOL_C
    B = sp.csr_matrix((np.ones(n * k), idx.ravel().astype(np.int64), np.arange(0, n * k + 1, k)), shape=(n, n))
    assert info["n_mutual"] == B.multiply(B.T).nnz // 2 and info["entries_dropped"] == 0
    assert info["nnz_connectivities"] == 2 * n * k - 2 * info["n_mutual"]

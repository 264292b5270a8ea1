"""srx_bbknn_points / srx_bbknn_result / srx_bbknn_harmony / srx_graph_trim on the device against tests/bbknn_ref.py.

The list is compared bit for bit (indices equal, distances the same bits) on coordinates that are integers times a power of
two, where every squared distance is exact in f64.  The graph is compared bit for bit with srx_neighbors_from_knn's graph of
the list the call returned, the trimming bit for bit with the closed form applied to the connectivities fetched from the
source handle, counter for counter."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import bbknn_ref as ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRIM_COUNTERS = ("trim", "rows_over_trim", "nnz_before", "nnz_after", "entries_trimmed", "max_row_nnz_before", "max_row_nnz_after",
                 "rows_emptied", "rows_wave", "rows_short", "rows_long")
EDGE_SIZES = [63, 64, 65, 127, 128, 129, 3]          # both sides of the 64-reference tile and the 128-query workgroup; exactly k_within


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def run(ctx, x, batch, kw=3, trim=0, n_batches=None, n_dims=None, graph=True):
    from singlerust_amd.memory.processing import bbknn_points
    return bbknn_points(ctx, x, batch, kw, n_dims, trim, n_batches, graph)


def check_list(ctx, x, batch, B, kw, n_dims=None):
    """The device's list equals the brute-force restatement's; the counters of the searches follow from the batch sizes."""
    idx, dist, g, info = run(ctx, x, batch, kw, 0, B, n_dims)
    want_i, want_d = ref.bbknn_list(x, batch, B, kw, n_dims)
    assert np.array_equal(idx, want_i), "indices"
    assert np.array_equal(bits(dist), bits(want_d)), "distances"
    sizes = np.bincount(np.asarray(batch, dtype=np.int64), minlength=B) if batch is not None else np.array([len(x)])
    n, K = len(x), kw * B - 1
    assert (info["n"], info["n_batches"], info["neighbors_within_batch"], info["k"]) == (n, B, kw, K)
    assert info["d"] == (n_dims or x.shape[1])
    assert info["min_batch_cells"] == sizes.min() and info["max_batch_cells"] == sizes.max()
    assert info["pairs_searched"] == ref.pairs_searched(sizes, kw)
    assert info["n_searches"] == ref.n_searches(sizes, kw)
    assert info["rows_certified"] + info["rows_recomputed"] == n * (B if kw > 1 else B - 1)
    assert g.info()["k"] == K and g.info()["n"] == n
    return idx, dist, g, info


# ---- the list -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,kind", [(1, "hashed"), (2, "interleaved"), (10, "contiguous"), (50, "hashed")])
def test_list_at_every_width_and_tile_edge(ctx, d, kind):
    rng = np.random.default_rng(100 + d)
    n = sum(EDGE_SIZES)
    x = ref.lattice(rng, n, d, 40 if d > 1 else 400, -3)
    batch = ref.labels(kind, EDGE_SIZES, d)
    idx, dist, g, info = check_list(ctx, x, batch, len(EDGE_SIZES), 3)
    if d == 10:                                                   # two calls give the same bits; the leading coordinates alone
        idx2, dist2, g2, _ = run(ctx, x, batch, 3, 0)
        assert np.array_equal(idx, idx2) and np.array_equal(bits(dist), bits(dist2))
        from singlerust_amd import _ffi as F
        assert same(g.fetch(F.GRAPH_CONNECTIVITIES), g2.fetch(F.GRAPH_CONNECTIVITIES))
        check_list(ctx, x, batch, len(EDGE_SIZES), 3, n_dims=4)


def test_one_batch_is_the_self_graph(ctx):
    """B = 1: the list is srx_knn_points' self graph with k = k_within - 1 and the graph srx_neighbors_from_knn's."""
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import connectivities_from_knn, knn_points
    x = ref.lattice(np.random.default_rng(5), 333, 7, 30)
    for batch in (None, np.zeros(333, dtype=np.uint32)):
        idx, dist, g, info = run(ctx, x, batch, 5, 0, 1)
        ki, kd, _ = knn_points(ctx, x, k=4)
        assert np.array_equal(idx, ki) and np.array_equal(bits(dist), bits(kd))
        assert info["n_searches"] == 1 and info["pairs_searched"] == 333 * 333 and info["k"] == 4
        g2 = connectivities_from_knn(ctx, ki, kd)
        for which in (F.GRAPH_DISTANCES, F.GRAPH_CONNECTIVITIES):
            assert same(g.fetch(which), g2.fetch(which))
        assert g.info() == g2.info()
    check_list(ctx, x, None, 1, 5)


def test_one_neighbour_per_batch_skips_the_own_batch(ctx):
    sizes = [70, 1, 130, 64]
    x = ref.lattice(np.random.default_rng(6), sum(sizes), 3, 25)
    batch = ref.labels("hashed", sizes, 2)
    idx, _, _, info = check_list(ctx, x, batch, 4, 1)
    assert info["k"] == 3 and info["n_searches"] == 6
    assert (batch[idx] != batch[:, None]).all()


def test_the_longest_list_and_one_beyond(ctx):
    """K = 64 (13 neighbours from each of 5 batches, one batch of exactly 13 points); 6 x 11 = 66 is refused."""
    from singlerust_amd import _ffi as F
    sizes = [13, 40, 70, 100, 130]
    x = ref.lattice(np.random.default_rng(8), sum(sizes), 5, 50, -2)
    batch = ref.labels("interleaved", sizes)
    _, _, _, info = check_list(ctx, x, batch, 5, 13)
    assert info["k"] == 64
    with pytest.raises(F.SrxError) as e:
        run(ctx, x, (np.arange(len(x)) % 11).astype(np.uint32), 6, 0, 11)
    assert e.value.code == F.E_ARG and "21 batches" in e.value.msg


@pytest.mark.parametrize("kind", ["contiguous", "interleaved", "hashed"])
def test_a_permutation_of_the_points_permutes_the_result(ctx, kind):
    rng = np.random.default_rng(9)
    sizes = [90, 50, 110]
    n = sum(sizes)
    x = ref.lattice(rng, n, 2, 1 << 20)
    d2 = ref.dist2(x, x)
    assert all(len(np.unique(r)) == n for r in d2), "the distances of a row must be distinct here"
    batch = ref.labels(kind, sizes, 3)
    idx, dist, _, _ = check_list(ctx, x, batch, 3, 3)
    p = rng.permutation(n)                                        # new point j is old point p[j]
    inv = np.argsort(p)
    idx_p, dist_p, _, _ = run(ctx, x[p], batch[p], 3, 0, 3)
    assert np.array_equal(idx_p, inv[idx[p]].astype(np.uint32)) and np.array_equal(bits(dist_p), bits(dist[p]))


def test_exact_duplicates_within_and_across_batches(ctx):
    rng = np.random.default_rng(10)
    pool = ref.lattice(rng, 40, 3, 20)
    x = pool[rng.integers(0, 40, 400)]                            # every location about ten times, in every batch
    batch = ref.labels("hashed", [150, 130, 120], 4)
    idx, dist, _, _ = check_list(ctx, x, batch, 3, 4)
    assert (dist[:, 0] == 0).mean() > 0.9 and not (idx == np.arange(400)[:, None]).any()


# ---- the graph ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clustered():
    x, batch, clump = ref.clumps_two_batches(np.random.default_rng(11))
    return x, batch, clump


def test_graph_is_the_graph_of_the_list(ctx):
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import connectivities_from_knn
    x, batch, _ = clustered()
    for kw in (2, 3):
        idx, dist, g, info = run(ctx, x, batch, kw, 0)
        g2 = connectivities_from_knn(ctx, idx, dist)
        for which in (F.GRAPH_DISTANCES, F.GRAPH_CONNECTIVITIES):
            assert same(g.fetch(which), g2.fetch(which))
        assert same(g.scales(), g2.scales()) and g.info() == g2.info()
        assert info["trim"]["trim"] == 0 and info["trim"]["nnz_after"] == g.info()["nnz_connectivities"]


def test_default_trim_changes_nothing_on_a_clustered_case(ctx):
    from singlerust_amd import _ffi as F
    x, batch, _ = clustered()
    _, _, g0, _ = run(ctx, x, batch, 3, 0)
    _, _, g, info = run(ctx, x, batch, 3, None)
    t = info["trim"]
    assert t["trim"] == 10 * 3 * 2 and t["entries_trimmed"] == 0 and t["rows_over_trim"] == 0
    assert t["nnz_before"] == t["nnz_after"] == g.info()["nnz_connectivities"]
    assert same(g.fetch(F.GRAPH_CONNECTIVITIES), g0.fetch(F.GRAPH_CONNECTIVITIES)) and g.info() == g0.info()
    # the same through srx_graph_trim, which always writes a new block
    tt = g0.trim(60)
    assert tt.trim_info["entries_trimmed"] == 0 and same(tt.fetch(F.GRAPH_CONNECTIVITIES), g0.fetch(F.GRAPH_CONNECTIVITIES))


# ---- the trimming alone -------------------------------------------------------------------------------------------------------
def symmetric(csr):
    import scipy.sparse as sp
    indptr, indices, data = csr
    n = len(indptr) - 1
    m = sp.csr_matrix((bits(data).astype(np.int64), indices.astype(np.int64), indptr.astype(np.int64)), shape=(n, n))
    rows = np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))
    assert not (rows == indices).any(), "diagonal"
    t = m.T.tocsr()
    t.sort_indices()
    assert np.array_equal(t.indptr, m.indptr) and np.array_equal(t.indices, m.indices) and np.array_equal(t.data, m.data), "symmetry"


def check_trim(g, trim):
    """srx_graph_trim equals the closed form on the connectivities fetched from g; D and the scales are copies; g is untouched."""
    from singlerust_amd import _ffi as F
    src = g.fetch(F.GRAPH_CONNECTIVITIES)
    t = g.trim(trim)
    got, info = t.fetch(F.GRAPH_CONNECTIVITIES), t.trim_info
    want, winfo = ref.trim_closed(src, trim, info["wave_capacity"], info["short_capacity"])
    assert np.array_equal(got[0], want[0]), "indptr"
    assert np.array_equal(got[1], want[1]), "indices"
    assert np.array_equal(bits(got[2]), bits(want[2])), "data"
    for c in TRIM_COUNTERS:
        assert info[c] == winfo[c], (c, info[c], winfo[c])
    assert info["rows_wave"] + info["rows_short"] + info["rows_long"] == info["rows_over_trim"]
    assert info["entries_trimmed"] % 2 == 0
    symmetric(got)
    gi, ti = g.info(), t.info()
    assert ti["nnz_connectivities"] == info["nnz_after"] and ti["max_row_nnz"] == info["max_row_nnz_after"]
    assert {k: v for k, v in ti.items() if k not in ("nnz_connectivities", "max_row_nnz")} == \
           {k: v for k, v in gi.items() if k not in ("nnz_connectivities", "max_row_nnz")}
    assert same(t.fetch(F.GRAPH_DISTANCES), g.fetch(F.GRAPH_DISTANCES)) and same(t.scales(), g.scales())
    assert same(g.fetch(F.GRAPH_CONNECTIVITIES), src)
    return t, got, info


def test_trim_at_every_row_length(ctx):
    """Every trim from 1 to beyond the longest row: each row meets L = trim - 1, trim and trim + 1."""
    from singlerust_amd import _ffi as F
    sizes = [100, 90, 110]
    x = ref.lattice(np.random.default_rng(12), 300, 4, 1000, -4)
    _, _, g, _ = run(ctx, x, ref.labels("hashed", sizes, 6), 3, 0)
    L = np.diff(g.fetch(F.GRAPH_CONNECTIVITIES)[0].astype(np.int64))
    assert L.min() >= 8
    seen = set()
    for trim in range(1, int(L.max()) + 2):
        _, _, info = check_trim(g, trim)
        seen |= {s for s in (-1, 0, 1) if (L == trim + s).any()}
        if trim < L.min():
            assert info["rows_over_trim"] == 300                  # every row is over trim
        if trim >= L.max():
            assert info["rows_over_trim"] == 0 and info["entries_trimmed"] == 0
    assert seen == {-1, 0, 1}


def test_trim_with_ties_at_the_threshold(ctx):
    """Integer coordinates in -6 .. 6: many weights tie at a row's threshold and trimmed rows stay longer than trim."""
    from singlerust_amd import _ffi as F
    x = ref.lattice(np.random.default_rng(42), 257, 2, 6)
    _, _, g, _ = run(ctx, x, ref.labels("hashed", [65, 64, 64, 64], 1), 2, 0)
    L0 = np.diff(g.fetch(F.GRAPH_CONNECTIVITIES)[0].astype(np.int64))
    stay = 0
    for trim in (1, 5, 9):
        _, got, _ = check_trim(g, trim)
        L1 = np.diff(got[0].astype(np.int64))
        stay += int(((L0 > trim) & (L1 > trim)).sum())
    assert stay > 0


@functools.lru_cache(maxsize=None)
def hub_points(n):
    """Two points of batch 0 at the centre and n - 2 points of batch 1 far from it: with 2 neighbours per batch every row names
    both hubs, whose rows have n - 1 entries."""
    rng = np.random.default_rng(n)
    x = np.concatenate([np.array([[0.0, 0.0], [1.0, 0.0]]), 5000.0 + ref.lattice(rng, n - 2, 2, 2000)])
    batch = np.array([0, 0] + [1] * (n - 2), dtype=np.uint32)
    return x, batch


@pytest.mark.parametrize("where", ["wave-1", "wave", "wave+1", "short-1", "short", "short+1", "long"])
def test_trim_hub_rows_on_every_route(ctx, where):
    from singlerust_amd import _ffi as F
    _, _, probe, _ = run(ctx, *hub_points(50), 2, 0)
    caps = probe.trim(1).trim_info
    wcap, scap = caps["wave_capacity"], caps["short_capacity"]
    assert 64 <= wcap < scap and scap + 700 <= 5200
    L = {"wave-1": wcap - 1, "wave": wcap, "wave+1": wcap + 1, "short-1": scap - 1, "short": scap, "short+1": scap + 1,
         "long": scap + 700}[where]
    n = L + 1
    _, _, g, _ = run(ctx, *hub_points(n), 2, 0)
    assert g.info()["max_row_nnz"] == L
    for trim in (3, L // 2, L - 1):
        _, _, info = check_trim(g, trim)
        hubs = (info["rows_wave"], info["rows_short"], info["rows_long"])
        route = 0 if L <= wcap else 1 if L <= scap else 2
        assert hubs[route] >= 2 and info["max_row_nnz_before"] == L
        if trim > 16:                                              # the hubs alone are over trim
            assert info["rows_over_trim"] == 2 and hubs[route] == 2


def test_trim_of_an_snn_handle_and_an_index_handle(ctx):
    from singlerust_amd.memory.processing import knn_index_points, snn_graph
    x, batch, _ = clustered()
    _, _, g, _ = run(ctx, x, batch, 3, 0)
    s = snn_graph(g, 0.0)
    for trim in (1, 7, 20):
        check_trim(s, trim)
    ix = knn_index_points(ctx, x, n_lists=8, seed=1)
    gi, _ = ix.graph(k=10, n_probe=3)
    for trim in (2, 9):
        check_trim(gi, trim)
    check_trim(check_trim(g, 4)[0], 2)                             # a trimmed handle is a source as well


# ---- consumers and quality ------------------------------------------------------------------------------------------------------
class Holder:
    """What the wrappers that read ``adata._graph`` need of an adata."""

    def __init__(self, g, n):
        self._graph, self._n, self.obs, self.obsm, self.uns = g, n, {}, {}, {}

    def n_obs(self):
        return self._n


def test_consumers_read_a_trimmed_handle(ctx):
    from singlerust_amd.memory.processing import louvain, paga, snn_graph, umap
    x, batch, _ = clustered()
    n = len(x)
    _, _, g, info = run(ctx, x, batch, 3, 3)
    assert info["trim"]["entries_trimmed"] > 0 and g.info()["nnz_connectivities"] == info["trim"]["nnz_after"]
    ad = Holder(g, n)
    lv = louvain(ad)
    assert lv["n_communities"] >= 3 and ad.obs["louvain"].shape == (n,)
    um = umap(ad, init="random", n_epochs=10)
    assert ad.obsm["X_umap"].shape == (n, 2) and np.isfinite(ad.obsm["X_umap"]).all() and um["n_epochs"] == 10
    pg = paga(ad)
    assert pg["n_groups"] == lv["n_communities"]
    s = snn_graph(g)
    assert s.info()["n"] == n and s.info()["k"] == 5 and s.snn_info["nnz"] > 0


def test_quality_batches_mix_and_clumps_stay(ctx):
    """Two batches drawn from the same three clumps, shifted by more than a clump's diameter: plain neighbours never leave the
    batch, BBKNN rows hold k_within (k_within - 1) of each, and Louvain on the BBKNN graph finds communities that lie within one
    clump, with one that spans both batches in every clump."""
    from singlerust_amd.memory.processing import knn_points, louvain
    x, batch, clump = clustered()
    n, kw = len(x), 3
    plain, _, _ = knn_points(ctx, x, k=2 * kw - 1)
    assert (batch[plain] == batch[:, None]).all()
    idx, _, g, _ = run(ctx, x, batch, kw, None)
    assert ((batch[idx] == batch[:, None]).sum(axis=1) == kw - 1).all() and ((batch[idx] != batch[:, None]).sum(axis=1) == kw).all()
    ad = Holder(g, n)
    louvain(ad)
    lab = ad.obs["louvain"]
    for c in np.unique(lab):
        assert len(set(clump[lab == c])) == 1, "a community crosses clumps"          # purity by clump is 1.0
    for c in range(3):
        assert any(set(batch[lab == m]) == {0, 1} for m in np.unique(lab[clump == c])), "no community of the clump spans both batches"


# ---- the resident entry points ------------------------------------------------------------------------------------------------
def _fitted(ctx):
    import scipy.sparse as sp
    import singlerust_amd as sr
    from singlerust_amd.memory.processing import dim_red
    z = np.load(os.path.join(GOLD, "planted_600x240.npz"))
    x = sp.csr_matrix((z["log_values"], z["indices"].astype(np.int64), z["indptr"].astype(np.int64)),
                      shape=(int(z["n_rows"]), int(z["n_cols"])))
    x.sort_indices()
    dev = sr.DeviceCsr.upload(ctx, 600, 240, x.indptr, x.indices, x.data, 2, csc=False)
    a = sr.IMAnnData(dev, x.indptr, x.indices, [f"c{i}" for i in range(600)], [f"g{j}" for j in range(240)])
    dim_red.pca_inplace(a, 20, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    return a


def test_result_and_harmony_equal_points_on_the_fetched_block(ctx):
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import bbknn, harmony_integrate
    a = _fitted(ctx)
    scores = np.zeros((600, 20))
    F.check(F.lib().srx_result_fetch(a.x().handle, F.ptr(scores), None, None, None, None, None), ctx.handle)
    codes = (np.arange(600) % 3).astype(np.uint32)

    def equal(u, pts, n_dims, trim):
        _, _, g2, info2 = run(ctx, pts, codes, 3, trim, 3, n_dims)
        for which in (F.GRAPH_DISTANCES, F.GRAPH_CONNECTIVITIES):
            assert same(a._graph.fetch(which), g2.fetch(which))
        assert same(a._graph.scales(), g2.scales()) and a._graph.info() == g2.info() == u["graph"]
        skip = ("ms", "ms_sort", "ms_search", "ms_merge", "ms_graph", "ms_trim")
        assert {k: v for k, v in u["info"].items() if k not in skip} == {k: v for k, v in info2.items() if k not in skip}
        assert a.obsp["connectivities"].shape == (600, 600) and a.obsp["distances"].nnz == 600 * 8

    u = bbknn(a, codes, 3, n_pcs=12, trim=4)
    assert u["params"]["n_neighbors"] == 9 and u["params"]["method"] == "bbknn" and u["info"]["d"] == 12
    assert u["info"]["trim"]["entries_trimmed"] > 0
    equal(u, scores, 12, 4)
    harmony_integrate(a, np.array(["s%d" % c for c in codes]), n_clusters=12, n_dims=15)
    u = bbknn(a, codes, 3, use_rep="X_pca_harmony")
    assert u["params"]["use_rep"] == "X_pca_harmony" and u["info"]["d"] == 15 and u["params"]["trim"] == 90
    equal(u, a.obsm["X_pca_harmony"], None, None)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_every_refusal_and_the_empty_graph(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    lib = F.lib()
    x = ref.lattice(np.random.default_rng(13), 60, 4, 10)
    batch = (np.arange(60) % 3).astype(np.uint32)
    idx_out, dist_out = np.full((60, 8), 7, dtype=np.uint32), np.full((60, 8), 7.0)

    def refused(pts=x, b=batch, B=3, kw=3, n_dims=0, n=None, d=None, c=ctx, null_batch=False):
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        h = C.c_void_p()
        o = F.BbknnOpts(kw, n_dims, -1)
        rc = lib.srx_bbknn_points(c.handle, F.ptr(pts), len(pts) if n is None else n, pts.shape[1] if d is None else d,
                                  None if null_batch else F.ptr(np.ascontiguousarray(b, dtype=np.uint32)), B, C.byref(o),
                                  F.ptr(idx_out), F.ptr(dist_out), None, C.byref(h))
        assert rc == F.E_ARG and not h.value
        assert (idx_out == 7).all() and (dist_out == 7.0).all()            # nothing written
        msg = lib.srx_last_error(c.handle).decode()
        assert msg
        return msg

    assert "21 batches" in refused(B=11, kw=6, b=np.arange(60) % 11) and "outside 1 .. 64" in refused(B=1, kw=1, b=np.zeros(60))
    assert "below 1" in refused(kw=-1)
    assert "n_batches" in refused(B=0) and "n_batches" in refused(B=66, kw=1)
    assert "null batch" in refused(null_batch=True)
    bad = batch.copy(); bad[17] = 3
    assert "not below n_batches" in refused(b=bad)
    few = batch.copy(); few[few == 2] = 1; few[:2] = 2
    assert "fewer than" in refused(b=few)
    assert "fewer than" in refused(b=np.arange(60) % 2)                      # batch 2 is empty
    for v in (np.nan, np.inf, -np.inf):
        bx = x.copy(); bx[31, 2] = v
        assert "NaN or Inf" in refused(pts=bx)
    assert "coordinates" in refused(pts=np.zeros((60, 129))) and "coordinates" in refused(d=0)
    assert "n_dims" in refused(n_dims=5) and "n_dims" in refused(n_dims=-1)
    assert "2^32" in refused(n=0xFFFFFFFF)
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    assert "sharded" in refused(c=c2)
    # the resident forms and the trimming
    h = C.c_void_p()
    assert lib.srx_bbknn_result(None, None, 1, None, None, C.byref(h)) == F.E_ARG
    assert lib.srx_bbknn_harmony(None, None, 1, None, None, C.byref(h)) == F.E_ARG
    assert lib.srx_graph_trim(None, 3, None, C.byref(h)) == F.E_ARG
    _, _, g, _ = run(ctx, x, batch, 3, 0)
    for t in (0, -1):
        assert lib.srx_graph_trim(g.handle, t, None, C.byref(h)) == F.E_ARG and not h.value
        assert "below 1" in lib.srx_last_error(ctx.handle).decode()
    assert lib.srx_graph_trim(g.handle, 3, None, None) == F.E_ARG
    # n == 0: an empty graph, which trims to an empty graph; NULL options are the defaults; the list alone
    _, _, e, info = run(ctx, np.zeros((0, 4)), np.zeros(0, dtype=np.uint32), 3, None, 2)
    assert e.info()["n"] == 0 and e.info()["k"] == 5 and e.info()["nnz_connectivities"] == 0 and info["n"] == 0
    assert e.fetch(F.GRAPH_CONNECTIVITIES)[0].tolist() == [0]
    assert e.trim(2).fetch(F.GRAPH_CONNECTIVITIES)[0].tolist() == [0]
    binfo = F.BbknnInfo()
    h = C.c_void_p()
    assert lib.srx_bbknn_points(ctx.handle, F.ptr(x), 60, 4, F.ptr(batch), 3, None, None, None, C.byref(binfo), C.byref(h)) == F.OK
    assert binfo.neighbors_within_batch == 3 and binfo.k == 8 and binfo.trim.trim == 90 and h.value
    lib.srx_graph_free(h)
    idx, dist, none, _ = run(ctx, x, batch, 3, 0, graph=False)
    want_i, want_d = ref.bbknn_list(x, batch, 3, 3)
    assert none is None and np.array_equal(idx, want_i) and np.array_equal(bits(dist), bits(want_d))
    # the context is still usable
    check_list(ctx, x, batch, 3, 3)

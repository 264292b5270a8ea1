"""srx_snn_from_knn / srx_snn_graph on the device against tests/snn_ref.py.  Every comparison is bit for bit (indptr, indices,
data viewed as u64) with the scipy restatement, and every counter must be equal: widths around the wave (k = 64 with self has
K = 65), random and clumped lists over pairs x weight x prune, real lists from the device search, the three routes of the count
kernel (a wave per row, a workgroup per row, windows for a hub's neighbours), the invariants, the consumers and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import snn_ref as ref

pytestmark = pytest.mark.gpu

COUNTERS = ("n", "k", "set_size", "min_shared", "max_shared", "pairs_considered", "pairs_kept", "nnz", "max_row_nnz", "max_in_degree",
            "max_candidates", "sum_candidates", "rows_empty")
PRUNES = (0.0, 1.0 / 15.0, 0.5, 1.0)
WEIGHTS = {ref.JACCARD: "jaccard", ref.NUMBER: "number"}
PAIRS = {ref.SHARED: "shared", ref.KNN: "knn"}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def run(ctx, idx, include_self=True, pairs=ref.SHARED, prune=ref.DEFAULT_PRUNE, weight=ref.JACCARD, distances=None):
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import snn_graph
    g = snn_graph(idx, prune, WEIGHTS[weight], PAIRS[pairs], include_self, ctx=ctx, distances=distances)
    return g, g.fetch(F.GRAPH_CONNECTIVITIES), g.snn_info


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def check(ctx, idx, include_self=True, pairs=ref.SHARED, prune=ref.DEFAULT_PRUNE, weight=ref.JACCARD, want=None):
    """The device's CSR and counters equal the scipy restatement's; the invariants that need no reference hold as well."""
    g, got, info = run(ctx, idx, include_self, pairs, prune, weight)
    want = want or ref.by_scipy(idx, include_self, pairs, prune, weight)
    assert np.array_equal(got[0], want[0]), "indptr"
    assert np.array_equal(got[1], want[1]), "indices"
    assert np.array_equal(bits(got[2]), bits(want[2])), "data"
    for c in COUNTERS:
        assert info[c] == want[3][c], (c, info[c], want[3][c])
    assert info["pairs_kept"] * 2 == info["nnz"] == g.info()["nnz_connectivities"]
    assert g.info()["max_row_nnz"] == info["max_row_nnz"]
    n = len(idx)
    assert info["rows_wave"] + info["rows_long"] <= n
    return g, got, info


def invariants(got, n):
    import scipy.sparse as sp
    indptr, indices, data = got
    m = sp.csr_matrix((bits(data).astype(np.int64), indices.astype(np.int64), indptr.astype(np.int64)), shape=(n, n))
    rows = np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))
    assert not (rows == indices).any(), "diagonal"
    t = m.T.tocsr()
    t.sort_indices()
    assert np.array_equal(t.indptr, m.indptr) and np.array_equal(t.indices, m.indices) and np.array_equal(t.data, m.data), "symmetry"
    for i in range(n):
        r = indices[int(indptr[i]):int(indptr[i + 1])].astype(np.int64)
        assert (np.diff(r) > 0).all(), "ascending"


# ---- widths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 15, 31, 32, 33, 63, 64])
def test_widths(ctx, k):
    for n in (k + 2, 300):
        if n <= k:
            continue
        idx = ref.random_list(np.random.default_rng(1000 + k + n), n, k)
        for include_self in (True, False):
            _, _, info = check(ctx, idx, include_self, prune=0.0)
            assert info["set_size"] == k + include_self
            check(ctx, idx, include_self, prune=ref.jaccard_f64(min(2, k + include_self), k + include_self))


# ---- random valid lists -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_500():
    return ref.random_list(np.random.default_rng(7), 500, 15)


def test_random_lists_both_sides_of_the_prune(ctx):
    idx = random_500()
    _, _, info = check(ctx, idx)
    assert 0 < info["pairs_kept"] < info["pairs_considered"]
    assert info["min_shared"] == 2
    _, got, _ = check(ctx, idx, weight=ref.NUMBER)
    assert got[2].min() == 2.0                                     # s = 2 of K = 16 is 1 / 15 to the bit: equality is kept
    for include_self in (True, False):
        for pairs in (ref.SHARED, ref.KNN):
            check(ctx, idx, include_self, pairs, 0.0)


# ---- planted clumps -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clumped(n, k):
    """The exact list of n points in 4 well-separated clumps, with two pairs of cells given identical neighbour sets (with
    self): b = the first neighbour of a, and knn(b) = {a} u knn(a) \\ {b}."""
    rng = np.random.default_rng(n + k)
    x, lab = ref.clumps(rng, n, 4)
    idx = ref.brute_knn(x, k)
    twins = []
    for a in (0, 1):                      # cells of two different clumps
        b = int(idx[a][0])
        idx[b] = np.array([a] + [j for j in idx[a] if j != b], dtype=np.uint32)
        twins.append((a, b))
    return x, lab, idx, twins


@pytest.mark.parametrize("n,k", [(500, 15), (2000, 19)])
def test_planted_clumps(ctx, n, k):
    _, _, idx, twins = clumped(n, k)
    for pairs in (ref.SHARED, ref.KNN):
        for weight in (ref.JACCARD, ref.NUMBER):
            for p in PRUNES:
                _, got, info = check(ctx, idx, True, pairs, p, weight)
                if p == 1.0:                  # identical sets alone: the two planted pairs, J = 1
                    assert info["nnz"] == 4 and sorted(got[1].tolist()) == sorted(c for t in twins for c in t)
                    assert (got[2] == (1.0 if weight == ref.JACCARD else k + 1.0)).all()
    if k == 15:
        _, got, info = check(ctx, idx, weight=ref.NUMBER)
        assert info["min_shared"] == 2 and got[2].min() == 2.0     # equality at the default prune is kept


# ---- real lists ---------------------------------------------------------------------------------------------------------------
def test_real_lists_graph_handle_and_index_handle(ctx):
    """srx_snn_graph on a handle equals srx_snn_from_knn on the list fetched from it: for the exact graph of the device search
    and for the graph of an inverted-file index."""
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import connectivities_from_knn, knn_index_points, knn_points, snn_graph
    x, _, _, _ = clumped(2000, 19)
    idx, dist, _ = knn_points(ctx, x, k=19)
    src = connectivities_from_knn(ctx, idx, dist)
    ix = knn_index_points(ctx, x, n_lists=16, seed=1)
    src_ivf, _ = ix.graph(k=19, n_probe=4)
    for handle in (src, src_ivf):
        dptr, dind, ddat = handle.fetch(F.GRAPH_DISTANCES)
        lst = dind.reshape(-1, 19)
        for pairs, prune in ((ref.SHARED, ref.DEFAULT_PRUNE), (ref.KNN, 0.0)):
            a = snn_graph(handle, prune, "jaccard", PAIRS[pairs], True)
            b = snn_graph(lst, prune, "jaccard", PAIRS[pairs], True, ctx=ctx, distances=ddat.reshape(-1, 19))
            assert same(a.fetch(F.GRAPH_CONNECTIVITIES), b.fetch(F.GRAPH_CONNECTIVITIES))
            assert same(a.fetch(F.GRAPH_DISTANCES), (dptr, dind, ddat)) and same(b.fetch(F.GRAPH_DISTANCES), (dptr, dind, ddat))
            assert {c: a.snn_info[c] for c in COUNTERS} == {c: b.snn_info[c] for c in COUNTERS}
            want = ref.by_scipy(lst, True, pairs, prune)
            assert same(a.fetch(F.GRAPH_CONNECTIVITIES), want[:3])
        # the handle it was made from is untouched
        assert same(handle.fetch(F.GRAPH_DISTANCES), (dptr, dind, ddat))
    # an SNN handle is a source as well
    again = snn_graph(snn_graph(src), 0.0, "number", "shared", False)
    assert same(again.fetch(F.GRAPH_CONNECTIVITIES), ref.by_scipy(idx, False, ref.SHARED, 0.0, ref.NUMBER)[:3])


# ---- the routes of the count kernel -----------------------------------------------------------------------------------------------
def hub_list(n, k, every, hubs=(0,)):
    """Rows i with i % every == 0 list the hub cells first (a hub row lists cell n // 2 in its own place), the rest of a row and
    the other rows follow a ring."""
    idx = np.empty((n, k), dtype=np.uint32)
    for i in range(n):
        ring = [(i + d) % n for d in range(1, k + 4)]
        if i % every == 0:
            first = [h if h != i else n // 2 for h in hubs]
            idx[i] = (first + [j for j in ring if j not in first])[:k]
        else:
            idx[i] = ring[:k]
    return idx


def test_hub_rows_take_the_window_route(ctx):
    """Every row lists cell 0 (row 0 lists another), so every row's candidates exceed the workgroup route's capacity: n = short_capacity + 100."""
    _, _, probe = run(ctx, ref.random_list(np.random.default_rng(3), 40, 3))
    cap = probe["short_capacity"]
    assert probe["wave_capacity"] < cap <= 8192 - 100, cap
    n = cap + 100
    idx = hub_list(n, 15, 1)
    _, got, info = check(ctx, idx)
    assert info["rows_long"] == n and info["max_in_degree"] == n - 1 and info["rows_wave"] == 0
    invariants(got, n)
    _, got0, info0 = check(ctx, idx, prune=0.0)                     # dense: every pair shares the hub
    assert info0["pairs_considered"] == n * (n - 1) // 2 == info0["pairs_kept"]
    check(ctx, idx, include_self=False, pairs=ref.KNN, prune=0.0)


def test_half_the_rows_long_and_the_workgroup_route(ctx):
    _, _, probe = run(ctx, ref.random_list(np.random.default_rng(3), 40, 3))
    n = probe["short_capacity"] + 100
    idx = hub_list(n, 15, 2, hubs=(0, 1))                      # two hubs of n / 2 each: the rows that list both are long
    _, got, info = check(ctx, idx)
    assert n // 2 <= info["rows_long"] <= n // 2 + 60 and info["rows_wave"] > 0
    invariants(got, n)
    check(ctx, idx, pairs=ref.KNN, prune=0.0, weight=ref.NUMBER)
    # a hub of 700: its neighbours' candidates lie between the two capacities, a workgroup per row with its table in LDS
    idx = hub_list(3000, 15, 4)
    for include_self in (True, False):
        _, got, info = check(ctx, idx, include_self, prune=0.0)
        mid = 3000 - info["rows_wave"] - info["rows_long"]
        assert mid >= 700 and info["rows_long"] == 0 and probe["wave_capacity"] < info["max_candidates"] <= probe["short_capacity"]
    check(ctx, idx, pairs=ref.KNN)
    invariants(got, 3000)


# ---- invariants -----------------------------------------------------------------------------------------------------------------
def test_invariants_permutation_and_determinism(ctx):
    _, _, idx, _ = clumped(500, 15)
    g, got, info = check(ctx, idx, prune=0.0)
    invariants(got, 500)
    rng = np.random.default_rng(5)
    shuffled = np.array([rng.permutation(r) for r in idx], dtype=np.uint32)
    assert not np.array_equal(shuffled, idx)
    for lst in (shuffled, idx):
        _, again, info2 = run(ctx, lst, prune=0.0)
        assert same(got, again) and {c: info[c] for c in COUNTERS} == {c: info2[c] for c in COUNTERS}
    _, got_k, _ = check(ctx, random_500(), include_self=False, pairs=ref.KNN)
    invariants(got_k, 500)


# ---- consumers ------------------------------------------------------------------------------------------------------------------
class Holder:
    """What the wrappers that read ``adata._graph`` need of an adata."""

    def __init__(self, g, n):
        self._graph, self._n, self.obs, self.obsm, self.uns = g, n, {}, {}, {}

    def n_obs(self):
        return self._n


def test_consumers_read_the_handle(ctx):
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import graph_labels, louvain, louvain_csr, paga, umap
    x, lab, idx, _ = clumped(500, 15)
    rng = np.random.default_rng(11)
    dist = np.sort(rng.random(idx.shape), axis=1)
    g, got, info = run(ctx, idx, distances=dist)
    ad = Holder(g, 500)
    linfo = louvain(ad)
    labels = ad.obs["louvain"]
    csr_labels, _ = louvain_csr(ctx, got)
    assert np.array_equal(labels, csr_labels) and np.array_equal(graph_labels(g), labels)
    # on 4 well-separated clumps the labels are the clumps
    assert linfo["n_communities"] == 4
    assert len({(int(a), int(b)) for a, b in zip(lab, labels)}) == 4
    uinfo = umap(ad, init="random", n_epochs=20)
    assert ad.obsm["X_umap"].shape == (500, 2) and np.isfinite(ad.obsm["X_umap"]).all() and uinfo["n_epochs"] == 20
    pinfo = paga(ad)
    assert pinfo["n_groups"] == 4 and pinfo["nnz"] == 500 * 15
    # D is the source list in column order with its distances; rho and sigma are zero
    dptr, dind, ddat = g.fetch(F.GRAPH_DISTANCES)
    order = np.argsort(idx, axis=1)
    assert np.array_equal(dptr, np.arange(501, dtype=np.uint64) * 15)
    assert np.array_equal(dind.reshape(500, 15), np.take_along_axis(idx, order, axis=1))
    assert np.array_equal(bits(ddat.reshape(500, 15)), bits(np.take_along_axis(dist, order, axis=1)))
    rho, sigma = g.scales()
    assert not rho.any() and not sigma.any()
    g0, _, _ = run(ctx, idx)                                       # no distances given: zeros
    assert not g0.fetch(F.GRAPH_DISTANCES)[2].any()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_empty_graph(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import connectivities_from_knn, snn_graph
    lib = F.lib()
    idx = random_500()
    dist = np.ones(idx.shape)

    def refused(lst, d=None, opts=None, c=ctx, k=None, n=None):
        lst = np.ascontiguousarray(lst, dtype=np.uint32)
        h = C.c_void_p()
        o = opts if opts is not None else F.SnnOpts(0, 0, 1, 0, 1.0 / 15.0)
        rc = lib.srx_snn_from_knn(c.handle, F.ptr(lst), None if d is None else F.ptr(np.ascontiguousarray(d, dtype=np.float64)),
                                  len(lst) if n is None else n, lst.shape[1] if k is None else k, C.byref(o), None, C.byref(h))
        assert rc == F.E_ARG and not h.value
        return lib.srx_last_error(c.handle).decode()

    bad = idx.copy(); bad[3, 2] = 500
    assert "not below n" in refused(bad)
    bad = idx.copy(); bad[7, 0] = 7
    assert "names itself" in refused(bad)
    bad = idx.copy(); bad[9, 1] = bad[9, 0]
    assert "twice" in refused(bad)
    for v in (-1.0, np.nan, np.inf):
        bd = dist.copy(); bd[4, 4] = v
        assert "distance" in refused(idx, bd)
    assert "outside 1..64" in refused(idx, k=0) and "outside 1..64" in refused(idx, k=65)
    assert "only 2 others" in refused(np.zeros((3, 3), dtype=np.uint32))
    for p in (-0.001, 1.001, np.nan):
        assert "prune" in refused(idx, opts=F.SnnOpts(0, 0, 1, 0, p))
    assert "weight" in refused(idx, opts=F.SnnOpts(2, 0, 1, 0, 0.1)) and "weight" in refused(idx, opts=F.SnnOpts(-1, 0, 1, 0, 0.1))
    assert "pairs" in refused(idx, opts=F.SnnOpts(0, 2, 1, 0, 0.1))
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    assert "sharded" in refused(idx, c=c2)
    # the handle form refuses the same options, and a null handle
    src = connectivities_from_knn(ctx, idx, dist)
    h = C.c_void_p()
    for o, text in ((F.SnnOpts(0, 0, 1, 0, 2.0), "prune"), (F.SnnOpts(5, 0, 1, 0, 0.1), "weight"), (F.SnnOpts(0, 5, 1, 0, 0.1), "pairs")):
        assert lib.srx_snn_graph(src.handle, C.byref(o), None, C.byref(h)) == F.E_ARG and not h.value
        assert text in lib.srx_last_error(ctx.handle).decode()
    assert lib.srx_snn_graph(None, None, None, C.byref(h)) == F.E_ARG
    # n == 0: an empty graph; NULL options: the defaults
    empty = snn_graph(np.zeros((0, 15), dtype=np.uint32), ctx=ctx)
    assert empty.info()["n"] == 0 and empty.info()["nnz_connectivities"] == 0 and empty.snn_info["nnz"] == 0
    assert empty.fetch(F.GRAPH_CONNECTIVITIES)[0].tolist() == [0]
    h = C.c_void_p()
    info = F.SnnInfo()
    assert lib.srx_snn_from_knn(ctx.handle, F.ptr(idx), None, 500, 15, None, C.byref(info), C.byref(h)) == F.OK
    assert info.set_size == 16 and info.min_shared == 2 and info.nnz == ref.by_scipy(idx)[3]["nnz"]
    lib.srx_graph_free(h)
    # the context is still usable
    check(ctx, idx)

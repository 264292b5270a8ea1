"""The inverted-file search on the device (srx_knn_index_* / srx_neighbors_index) against its definition in include/srx.h:
the exhaustive probe equals the exact search bit for bit, supplied integer centroids equal the numpy restatement
(knn_ivf_ref.py) with its counters, the fetched index is a partition with exact argmins, training is reproducible and
Lloyd's inertia never rises, probes are nested, the graph of the list is the graph of the exact list, and every refusal
leaves the outputs alone."""
import ctypes as C

import numpy as np
import pytest

import knn_ivf_ref as R

pytestmark = pytest.mark.gpu


def P():
    from singlerust_amd.memory import processing
    return processing


def clustered(seed, n, d, n_clusters=12):
    """The clustered data of test_knn_gpu.py."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clusters, d)) * 6.0
    return centres[rng.integers(0, n_clusters, n)] + rng.standard_normal((n, d))


def counters_sum(info):
    assert info["rows_certified"] + info["rows_rescanned"] + info["rows_exhaustive"] == info["n_query"], info


# ---- 1. the exhaustive probe equals the exact search ------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5, 50, 128])
@pytest.mark.parametrize("n", [2, 33, 300, 1100])
def test_exhaustive_probe_equals_exact_search(ctx, n, d):
    rng = np.random.default_rng(100 * n + d)
    x = rng.standard_normal((n, d)) * np.linspace(4, 0.5, d)
    qry = np.concatenate([rng.standard_normal((37, d)) * 2, x[::7]])
    exact = {}

    def want(form, k):
        if (form, k) not in exact:
            exact[form, k] = P().knn_points(ctx, x, qry if form == "query" else None, k=k, include_self=form == "self+")[:2]
        return exact[form, k]

    for n_lists in (1, 2, 7, 64):
        if n_lists > n:
            continue
        # supplied: twice as many centroids as distinct places, so that every second list is empty
        sup = np.repeat(x[rng.permutation(n)[:(n_lists + 1) // 2]] + 0.25, 2, axis=0)[:n_lists]
        for cent in (None, sup):
            ix = P().knn_index_points(ctx, x, centroids=cent, n_lists=n_lists, train_iters=3, seed=5)
            i = ix.info()
            assert i["n_lists"] == n_lists and i["n_ref"] == n and i["d"] == d
            if cent is not None and n_lists >= 2:
                assert i["empty_lists"] >= n_lists // 2
            for form in ("self", "self+", "query"):
                adm = n - (form == "self")
                for k in sorted({1, min(15, adm), min(64, adm)}):
                    idx, dist, info = ix.search(qry if form == "query" else None, k=k, n_probe=n_lists, include_self=form == "self+")
                    wi, wd = want(form, k)
                    label = (n, d, n_lists, cent is None, form, k)
                    assert np.array_equal(idx, wi), label
                    assert np.array_equal(dist.view(np.uint64), wd.view(np.uint64)), label
                    counters_sum(info)
                    assert info["pairs"] == idx.shape[0] * n_lists and info["points_scanned"] == idx.shape[0] * n, (label, info)
            ix.free()


# ---- 1b. every instance of the list-major candidate pass --------------------------------------------------------------------
# One d per instantiated width (knn_ref.WIDTHS); below 128 it is the largest d of its width, so the norm sits in the last
# coordinate slot.  Two explicit centroids and n_probe = n_lists: every list is probed by all 300 rows of the self form (work
# items of 128, 128 and 44 pairs: full blocks, and a partial one with two dead waves) or by the 130 separate queries (128 and
# 2: three dead waves).  Coordinates are integers times 2^-16, so knn_ref's int64 distances are exact and the expectation
# needs no near-tie allowance.
WIDTH_D = (7, 19, 35, 51, 67, 128)
WIDTH_N, WIDTH_NQ, WIDTH_K, WIDTH_EXP = 300, 130, 15, -16


@pytest.fixture(scope="module", params=WIDTH_D)
def width_case(request):
    import knn_ref as KR
    d = request.param
    assert KR.width(d) == KR.WIDTHS[WIDTH_D.index(d)] and (d == 128 or KR.width(d + 1) > KR.width(d))
    rng = np.random.default_rng(7000 + d)
    scale = np.linspace(4, 0.5, d) * 2.0 ** -WIDTH_EXP
    units = np.rint(rng.standard_normal((WIDTH_N, d)) * scale).astype(np.int64)
    qry = np.concatenate([np.rint(rng.standard_normal((WIDTH_NQ - 40, d)) * 2 * scale).astype(np.int64), units[::7][:40]])
    assert len(qry) == WIDTH_NQ
    forms = {"self": KR.Case(f"ivf_width_d{d}", units, exp=WIDTH_EXP),
             "query": KR.Case(f"ivf_width_d{d}_query", units, exp=WIDTH_EXP, query=qry)}
    for case in forms.values():                  # no exact tie at rank k: the k-th and the next distance differ in every row
        _, d2, _ = case.expected()
        assert (d2[:, WIDTH_K - 1] < d2[:, WIDTH_K]).all(), case.name
    cent = np.zeros((3, d))
    cent[0, 0], cent[1, 0] = -1.0, 1.0           # the two halves along the widest axis
    cent[2] = 1e4                                # and a centroid no point is nearest to
    return d, forms, cent


def check_width_forms(ctx, ix, forms, n_lists):
    for form, case in forms.items():
        ref, qry = case.points()
        idx, dist, info = ix.search(qry, k=WIDTH_K, n_probe=n_lists)
        wi, wd, _ = P().knn_points(ctx, ref, qry, k=WIDTH_K)
        assert np.array_equal(idx, wi), case.name
        assert np.array_equal(dist.view(np.uint64), wd.view(np.uint64)), case.name
        ei, ed = case.expected_k(WIDTH_K)
        assert np.array_equal(idx.astype(np.int64), ei) and np.array_equal(dist.view(np.uint64), ed.view(np.uint64)), case.name
        counters_sum(info)
        assert info["pairs"] == len(idx) * n_lists and info["points_scanned"] == len(idx) * WIDTH_N, (case.name, info)


def test_exhaustive_probe_equals_exact_search_at_every_width(ctx, width_case):
    d, forms, cent = width_case
    ix = P().knn_index_points(ctx, forms["self"].points()[0], centroids=cent[:2])
    i = ix.info()
    assert i["n_lists"] == 2 and i["d"] == d and i["empty_lists"] == 0 and i["min_list"] > 64, i
    check_width_forms(ctx, ix, forms, 2)
    ix.free()


def test_an_empty_list_changes_nothing(ctx, width_case):
    d, forms, cent = width_case
    ix = P().knn_index_points(ctx, forms["self"].points()[0], centroids=cent)
    i = ix.info()
    assert i["n_lists"] == 3 and i["empty_lists"] == 1 and i["min_list"] == 0, i
    assert np.diff(ix.fetch()[1].astype(np.int64))[2] == 0
    check_width_forms(ctx, ix, forms, 3)
    ix.free()


# ---- 2. supplied integer centroids against the restatement ------------------------------------------------------------------
def check_against_ref(ctx, ix, ref_u, cent_u, qry_u, k, n_probe, include_self, exp, label):
    want = R.search(ref_u, cent_u, k, n_probe, qry_u, include_self)
    idx, dist, info = ix.search(None if qry_u is None else R.to_f64(qry_u, exp), k=k, n_probe=n_probe, include_self=include_self)
    assert np.array_equal(idx.astype(np.int64), want["idx"]), label
    wd = np.ldexp(np.sqrt(want["d2"].astype(np.float64)), exp)
    assert np.array_equal(dist.view(np.uint64), wd.view(np.uint64)), label
    counters_sum(info)
    for key in ("pairs", "points_scanned", "rows_exhaustive"):
        assert info[key] == want[key], (label, key, info[key], want[key])
    assert info["n_probe"] == n_probe and info["k"] == k
    return want, info


@pytest.fixture(scope="module")
def lattice():
    return R.lattice_case()


def test_lattice_preconditions(lattice):
    """The case holds what it is meant to hold (no device): every tile-edge length, points equidistant from two centroids,
    queries whose n_probe-th and next centroid tie, a list probed by more than 128 queries."""
    ref, cent, qry = lattice
    a = R.assign_points(ref, cent)
    lengths = np.bincount(a, minlength=len(cent))
    assert set(R.LATTICE_EDGES) <= set(lengths.tolist()), lengths
    d2c = np.sort(R.dist2(ref, cent), axis=1)
    assert (d2c[:, 0] == d2c[:, 1]).any()
    dq = np.sort(R.dist2(qry, cent), axis=1)
    for n_probe in (1, 2, 5, len(cent) - 1):
        assert (dq[:, n_probe - 1] == dq[:, n_probe]).any(), n_probe
    assert np.bincount(R.probe_sets(qry, cent, 1)[:, 0]).max() > 128 and lengths.max() > 128
    _, counts = np.unique(ref, axis=0, return_counts=True)
    assert (counts >= R.DUP).sum() == 2


@pytest.mark.parametrize("n_probe", [1, 2, 5, 10])
def test_lattice_equals_restatement(ctx, lattice, n_probe):
    ref, cent, qry = lattice
    assert len(cent) - 1 == 10
    ix = P().knn_index_points(ctx, R.to_f64(ref), centroids=R.to_f64(cent))
    c, off, mem = ix.fetch()
    a = R.assign_points(ref, cent)
    woff, wmem = R.build_lists(a, len(cent))
    assert np.array_equal(c, R.to_f64(cent)) and np.array_equal(off.astype(np.int64), woff) and np.array_equal(mem.astype(np.int64), wmem)
    short = 0
    for k in (1, 15, 40):
        for q, inc in ((None, False), (None, True), (qry, False)):
            want, info = check_against_ref(ctx, ix, ref, cent, q, k, n_probe, inc, R.EXP, (n_probe, k, q is None, inc))
            short += info["rows_exhaustive"]
    if n_probe <= 2:
        assert short > 0                     # rows in the lists of 1, 31, 32, 33 points are short of k = 15 or 40
    ix.free()


def test_blind_lists_are_rescanned_and_exact(ctx):
    units, cent = R.blind_case()
    ix = P().knn_index_points(ctx, R.to_f64(units, -10), centroids=R.to_f64(cent, -10))
    for k in (1, 15):
        want, info = check_against_ref(ctx, ix, units, cent, None, k, 1, False, -10, ("blind", k))
        assert info["rows_exhaustive"] == 0 and info["rows_rescanned"] == info["n_query"] == len(units), info
    ix.free()


# ---- 3. fetch ------------------------------------------------------------------------------------------------------------------
def check_partition(off, mem, n):
    assert off[0] == 0 and off[-1] == n and (np.diff(off.astype(np.int64)) >= 0).all()
    assert np.array_equal(np.sort(mem), np.arange(n, dtype=np.uint32))
    for l in range(len(off) - 1):
        assert (np.diff(mem[int(off[l]):int(off[l + 1])].astype(np.int64)) > 0).all(), l


def test_fetch_trained_index(ctx):
    x = clustered(31, 2500, 20)
    ix = P().knn_index_points(ctx, x, n_lists=40, train_iters=4, seed=3)
    cent, off, mem = ix.fetch()
    check_partition(off, mem, len(x))
    assign = np.zeros(len(x), dtype=np.int64)
    for l in range(40):
        assign[mem[int(off[l]):int(off[l + 1])]] = l
    xl, cl = x.astype(np.longdouble), cent.astype(np.longdouble)
    d2 = np.zeros((len(x), 40), dtype=np.longdouble)
    for j in range(x.shape[1]):
        t = xl[:, j][:, None] - cl[None, :, j]
        d2 += t * t
    got = d2[np.arange(len(x)), assign]
    assert (got <= d2.min(axis=1) * (1 + np.longdouble(1e-12))).all()
    inertia = float(got.sum())
    assert abs(ix.info()["inertia"] - inertia) <= 1e-12 * inertia, (ix.info()["inertia"], inertia)
    ix.free()


def test_fetch_integer_index(ctx, lattice):
    ref, cent, _ = lattice
    ix = P().knn_index_points(ctx, R.to_f64(ref), centroids=R.to_f64(cent))
    _, off, mem = ix.fetch()
    check_partition(off, mem, len(ref))
    d2 = R.dist2(ref, cent)
    assign = np.repeat(np.arange(len(cent)), np.diff(off.astype(np.int64)))
    assert np.array_equal(assign, np.argmin(d2, axis=1)[mem])          # exact in int64, ties to the lower centroid
    inertia = float(d2.min(axis=1).sum()) * 4.0 ** R.EXP
    i = ix.info()
    assert abs(i["inertia"] - inertia) <= 1e-12 * inertia
    lengths = np.diff(off.astype(np.int64))
    assert (i["min_list"], i["max_list"], i["empty_lists"], i["n_train"]) == (lengths.min(), lengths.max(), (lengths == 0).sum(), 0)
    ix.free()


# ---- 4. training ---------------------------------------------------------------------------------------------------------------
def test_training_is_reproducible(ctx):
    x = clustered(41, 3000, 20)
    got = []
    for seed in (7, 7, 8):
        ix = P().knn_index_points(ctx, x, n_lists=50, train_iters=5, seed=seed, max_train_points=1500)
        assert ix.info()["n_train"] == 1500
        got.append(ix.fetch())
        ix.free()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0], got[1]))
    assert got[0][0].tobytes() != got[2][0].tobytes()
    # with no iteration the centroids are the first n_lists points of the hashed sample
    ix = P().knn_index_points(ctx, x, n_lists=50, train_iters=0, seed=7, max_train_points=1500)
    assert np.array_equal(ix.fetch()[0], x[R.sample_order(3000, 1500, 7)[:50]])
    ix.free()


def test_lloyd_inertia_never_rises(ctx):
    x = clustered(42, 3000, 20)
    inertia = []
    for iters in (0, 1, 2, 5, 10):
        ix = P().knn_index_points(ctx, x, n_lists=24, train_iters=iters, seed=1, max_train_points=3000)
        inertia.append(ix.info()["inertia"])
        ix.free()
    print("inertia over train_iters 0, 1, 2, 5, 10:", inertia)
    for a, b in zip(inertia, inertia[1:]):
        assert b <= a * (1 + 1e-12), inertia
    assert inertia[-1] < inertia[0]


# ---- 5. nested probes ----------------------------------------------------------------------------------------------------------
# Mean recall@15 of the numpy restatement (knn_ivf_ref.train + search, defaults, seed 0) on clustered(102, 3000, 50) at
# the default n_probe = 20 of 219 lists, computed on the CPU: 0.9999 (0.5024 at 1 probe, 0.6646 at 4, 0.9971 at 16, 1 at 64).
# The floor is that minus 0.05.
REF_RECALL = 0.9999
DEFAULT_PROBE = 20
RECALL_FLOOR = REF_RECALL - 0.05


def test_nested_probes_and_recall(ctx):
    x = clustered(102, 3000, 50)
    k = 15
    true_idx = P().knn_points(ctx, x, k=k)[0]
    ix = P().knn_index_points(ctx, x)
    n_lists = ix.info()["n_lists"]
    assert n_lists == R.default_n_lists(3000) == 219
    prev = None
    for n_probe in (1, 4, 16, DEFAULT_PROBE, 64):
        idx, _, info = ix.search(k=k, n_probe=n_probe)
        counters_sum(info)
        hits = R.recall(idx, true_idx)
        mask = R_exhaustive_mask(ix, x, n_probe, k)
        assert mask.sum() == info["rows_exhaustive"]
        print(f"n_probe {n_probe}: mean recall {hits.mean() / k:.4f}, exhaustive {info['rows_exhaustive']}, rescanned {info['rows_rescanned']}")
        if prev is not None:
            both = ~mask & ~prev[1]
            assert (hits[both] >= prev[0][both]).all()
        prev = (hits, mask)
        if n_probe == DEFAULT_PROBE:
            idx0, _, info0 = ix.search(k=k, n_probe=0)                  # the default is min(20, n_lists)
            assert info0["n_probe"] == DEFAULT_PROBE and np.array_equal(idx0, idx)
            assert hits.mean() / k >= RECALL_FLOOR, hits.mean() / k
    ix.free()
    # the whole index probed: n_lists above 64 cannot be probed whole, so a second index with 64 lists
    ix = P().knn_index_points(ctx, x, n_lists=64)
    idx, _, _ = ix.search(k=k, n_probe=64)
    assert np.array_equal(idx, true_idx)
    ix.free()


def R_exhaustive_mask(ix, x, n_probe, k):
    """Rows whose probed lists hold fewer than k other points, from the fetched index in numpy (f64)."""
    cent, off, mem = ix.fetch()
    lengths = np.diff(off.astype(np.int64))
    probes = R.probe_sets(x, cent, n_probe)
    return lengths[probes].sum(axis=1) - 1 < k


# ---- 6. the graph --------------------------------------------------------------------------------------------------------------
def test_graph_of_the_whole_probe_is_the_exact_graph(ctx, lattice):
    from singlerust_amd import _ffi as F
    ref, cent, _ = lattice
    x = R.to_f64(ref)
    ix = P().knn_index_points(ctx, x, centroids=R.to_f64(cent))
    g, info = ix.graph(k=15, n_probe=len(cent))
    counters_sum(info)
    idx, dist, _ = P().knn_points(ctx, x, k=15)
    want = P().connectivities_from_knn(ctx, idx, dist)
    for which in (F.GRAPH_DISTANCES, F.GRAPH_CONNECTIVITIES):
        for a, b in zip(g.fetch(which), want.fetch(which)):
            assert a.tobytes() == b.tobytes()
    g.free()
    want.free()
    ix.free()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    lib = F.lib()
    x = clustered(71, 200, 10)
    cent = x[:8].copy()

    def refused(fn, *a, **kw):
        with pytest.raises(F.SrxError) as e:
            fn(*a, **kw)
        assert e.value.code == F.E_ARG and e.value.msg, (e.value.code, e.value.msg)
        return e.value.msg

    build = P().knn_index_points
    refused(build, ctx, x, n_lists=-1)
    refused(build, ctx, x, n_lists=201)
    refused(build, ctx, x, train_iters=-1)
    refused(build, ctx, x, train_iters=1001)
    refused(build, ctx, x[:0])
    refused(build, ctx, np.zeros((50, F.KNN_MAX_DIMS + 1)))
    for v in (np.nan, np.inf, -np.inf):
        bad = cent.copy()
        bad[3, 2] = v
        assert "centroids" in refused(build, ctx, x, centroids=bad)
        y = x.copy()
        y[17, 3] = v
        assert "NaN" in refused(build, ctx, y, n_lists=8)
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    assert "sharded" in refused(build, c2, x, n_lists=8)
    # a refused build leaves the handle slot NULL
    h = C.c_void_p(12345)
    opts = F.IvfOpts(201, 10, 0, 0)
    assert lib.srx_knn_index_points(ctx.handle, F.ptr(x), 200, 10, C.byref(opts), None, C.byref(h)) == F.E_ARG and not h.value

    ix = build(ctx, x, centroids=cent)
    refused(ix.search, k=0)
    refused(ix.search, k=65)
    refused(ix.search, k=5, n_probe=-1)
    refused(ix.search, k=5, n_probe=9)                       # 8 lists
    refused(ix.search, k=5, n_probe=65)
    refused(ix.search, k=5, n_dims=9)
    refused(ix.search, k=5, n_dims=11)
    ix.search(k=5, n_dims=10)
    small = build(ctx, x[:10], centroids=cent[:2])
    refused(small.search, k=10)                              # 9 admissible references without self
    small.search(k=10, include_self=True)
    refused(small.search, x[:3], k=11)
    small.free()
    y = x[:5].copy()
    y[2, 2] = np.nan
    assert "NaN" in refused(ix.search, y, k=5)
    refused(ix.graph, k=200)
    # the outputs of a refused search keep their bytes
    idx = np.full((200, 5), 77, dtype=np.uint32)
    dist = np.full((200, 5), -1.0)
    info = F.IvfSearchInfo()
    info.n_query = 99
    ko = F.KnnOpts(5, 0, 0, 0)
    assert lib.srx_knn_index_search(ix.handle, None, 0, C.byref(ko), 9, F.ptr(idx), F.ptr(dist), C.byref(info)) == F.E_ARG
    assert lib.srx_last_error(ctx.handle)
    assert (idx == 77).all() and (dist == -1.0).all() and info.n_query == 99
    gh = C.c_void_p(5)
    inc = F.KnnOpts(5, 0, 1, 0)
    assert lib.srx_neighbors_index(ix.handle, C.byref(inc), 0, None, C.byref(gh)) == F.E_ARG and not gh.value
    assert lib.srx_knn_index_search(None, None, 0, C.byref(ko), 0, None, None, None) == F.E_ARG
    # and the index still works; a query with no rows writes nothing
    got = ix.search(x[:0], k=5)
    assert got[0].shape == (0, 5) and got[2]["n_query"] == 0
    a, _, _ = ix.search(k=5, n_probe=8)
    assert np.array_equal(a, P().knn_points(ctx, x, k=5)[0])
    ix.free()


def test_neighbors_approx_fills_the_keys_of_neighbors(ctx):
    """The resident path: the index over the scores a fit left on the device, the keys `neighbors` fills, Louvain on the graph."""
    import os
    import scipy.sparse as sp
    import singlerust_amd as sr
    from singlerust_amd.memory.processing import dim_red
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planted_600x240.npz"))
    x = sp.csr_matrix((z["log_values"], z["indices"].astype(np.int64), z["indptr"].astype(np.int64)),
                      shape=(int(z["n_rows"]), int(z["n_cols"])))
    x.sort_indices()
    dev = sr.DeviceCsr.upload(ctx, x.shape[0], x.shape[1], x.indptr, x.indices, x.data, 2)
    a = sr.IMAnnData(dev, x.indptr, x.indices, [f"c{i}" for i in range(x.shape[0])], [f"g{j}" for j in range(x.shape[1])])
    dim_red.pca_inplace(a, 20, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    n = x.shape[0]
    exact = P().neighbors(a, n_neighbors=10)
    exact_idx, exact_dist = a.obsm["knn_indices"].copy(), a.obsm["knn_distances"].copy()
    out = P().neighbors_approx(a, n_neighbors=10, n_lists=12, n_probe=12)
    assert out["params"]["method"] == "ivf" and out["params"]["n_probe"] == 12 and out["index"]["n_lists"] == 12
    assert out["index"]["d"] == 20 and out["info"]["n_query"] == n
    assert np.array_equal(a.obsm["knn_indices"], exact_idx) and np.array_equal(a.obsm["knn_distances"], exact_dist)
    P().neighbors_approx(a, n_neighbors=10, n_pcs=7, n_lists=12, n_probe=12)
    idx7 = a.obsm["knn_indices"].copy()
    P().neighbors(a, n_neighbors=10, n_pcs=7)
    assert np.array_equal(a.obsm["knn_indices"], idx7)
    out = P().neighbors_approx(a, n_neighbors=10, n_lists=12, n_probe=3, connectivities=True, knn_lists=True)
    assert out["graph"]["n"] == n and a.obsp["connectivities"].shape == (n, n) and a.obsm["knn_indices"].shape == (n, 10)
    assert exact["params"]["n_neighbors"] == out["params"]["n_neighbors"] and out["params"]["n_probe"] == 3
    P().louvain(a)
    assert len(a.obs["louvain"]) == n

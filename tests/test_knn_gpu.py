"""Exact k-nearest-neighbour search on the device (srx_knn_result / srx_knn_points) against an f64 brute force on the host:
squared distances in the difference form, coordinate by coordinate, in row chunks; every row sorted by (distance, index).
Indices must match EXACTLY, distances to 1e-12 relative.  sklearn's brute-force search is the second opinion for the sets.

The only rows a comparison may exempt are those where the reference's own consecutive squared distances among its first
k + 1 differ by less than 1e-9 relative (an ulp-level difference in summation order may swap them); on the generic inputs
the tests assert that the reference has NO such row, so nothing is exempted there."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KS = (1, 15, 64)


# ---- host reference ---------------------------------------------------------------------------------------------------
def _chunk_topk(q, r, rows, kk, self_rows):
    """(squared distances, indices) of the kk nearest references of the query rows `rows`, ascending by (distance, index)."""
    d2 = np.zeros((len(rows), r.shape[0]))
    for j in range(r.shape[1]):                                  # difference form, summed in coordinate order
        t = q[rows, j][:, None] - r[None, :, j]
        d2 += t * t
    if self_rows is not None:
        d2[np.arange(len(rows)), self_rows] = np.inf             # a row is not its own neighbour
    kk = min(kk, r.shape[0] - (self_rows is not None))
    thr = np.partition(d2, kk - 1, axis=1)[:, kk - 1]
    out_d, out_i = np.zeros((len(rows), kk)), np.zeros((len(rows), kk), np.int64)
    for a in range(len(rows)):
        c = np.nonzero(d2[a] <= thr[a])[0]                       # ascending indices: a stable sort orders ties by index
        o = c[np.argsort(d2[a, c], kind="stable")][:kk]
        out_i[a], out_d[a] = o, d2[a, o]
    return out_d, out_i


def brute(ref, query=None, kk=65, rows=None, include_self=False):
    """First kk neighbours (squared distances, indices) of `rows` (default: all) of query (None: the self graph of ref)."""
    self_graph = query is None
    q = ref if self_graph else query
    rows = np.arange(q.shape[0]) if rows is None else np.asarray(rows)
    step = max(1, min(256, (1 << 22) // max(ref.shape[0], 1)))
    parts = [rows[s:s + step] for s in range(0, len(rows), step)]
    with ThreadPoolExecutor(16) as ex:
        res = list(ex.map(lambda p: _chunk_topk(q, ref, p, kk, p if (self_graph and not include_self) else None), parts))
    return np.concatenate([a for a, _ in res]), np.concatenate([b for _, b in res])


def near_tie_rows(d2, k):
    """Rows whose reference distances among the first k + 1 have a consecutive relative gap below 1e-9."""
    w = d2[:, :k + 1]
    gap = np.diff(w, axis=1) / np.maximum(w[:, 1:], 1e-300)
    return np.nonzero((gap < 1e-9).any(axis=1))[0]


def check_exact(idx, dist, d2, ref_i, k, label):
    """Device output against the reference's first k; asserts the reference has no near-tie row (cap 0)."""
    bad = near_tie_rows(d2, min(k, d2.shape[1] - 1))
    print(f"{label}: k={k} near-tie rows in the reference: {len(bad)}")
    assert len(bad) == 0, (label, k, bad[:10])
    assert idx.dtype == np.uint32 and idx.shape == (d2.shape[0], k)
    mism = np.nonzero((idx.astype(np.int64) != ref_i[:, :k]).any(axis=1))[0]
    assert len(mism) == 0, (label, k, len(mism), mism[:5], idx[mism[:2]], ref_i[mism[:2], :k])
    want = np.sqrt(d2[:, :k])
    err = np.abs(dist - want) / np.maximum(want, 1e-300)
    err[want == 0] = np.abs(dist[want == 0])
    print(f"{label}: k={k} max relative distance error {err.max():.3e}")
    assert err.max() <= 1e-12, (label, k, err.max())


def gaussian(seed, n, d):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)) * np.linspace(8, 0.5, d)


def clustered(seed, n, d, n_clusters=12):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clusters, d)) * 6.0
    return centres[rng.integers(0, n_clusters, n)] + rng.standard_normal((n, d))


def knn(ctx, ref, query=None, **kw):
    from singlerust_amd.memory.processing import knn_points
    return knn_points(ctx, ref, query, **kw)


def sklearn_sets(ref, k, query=None):
    from sklearn.neighbors import NearestNeighbors
    nn = NearestNeighbors(n_neighbors=k + (query is None), algorithm="brute").fit(ref)
    if query is None:
        return nn.kneighbors(return_distance=False, n_neighbors=k)            # excludes the row itself
    return nn.kneighbors(query, n_neighbors=k, return_distance=False)


# ---- 1. generic data ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gaussian_3000x50", "clustered_3000x50", "clustered_20000x50"])
def test_generic_exact(ctx, name):
    x = {"gaussian_3000x50": lambda: gaussian(101, 3000, 50), "clustered_3000x50": lambda: clustered(102, 3000, 50),
         "clustered_20000x50": lambda: clustered(108, 20011, 50)}[name]()
    # (1.3 M gaps at 20 011 x k = 64: about one seed in two has a reference gap below 1e-9 somewhere; seed 108 has none —
    # smallest relative gap of the host reference 3.1e-9 — so the near-tie guard of check_exact stays at zero rows here too)
    d2, ri = brute(x, kk=65)
    for k in KS:
        idx, dist, info = knn(ctx, x, k=k)
        print(name, k, info)
        assert info["rows_certified"] + info["rows_recomputed"] == x.shape[0]
        check_exact(idx, dist, d2, ri, k, name)
    if x.shape[0] <= 3000:
        sk = sklearn_sets(x, 15)
        assert all(set(a) == set(b) for a, b in zip(sk, ri[:, :15]))


@pytest.mark.parametrize("d", [2, 3, 17, 50, 64, 128])
def test_dimensions(ctx, d):
    # seeds for which the HOST REFERENCE has no near-tie row (smallest relative gap >= 1.2e-8; 200 + 64 has one of 9e-10)
    x = clustered((300 if d == 64 else 200) + d, 3000, d)
    d2, ri = brute(x, kk=65)
    for k in KS:
        idx, dist, info = knn(ctx, x, k=k)
        assert info["d"] == d and info["k"] == k
        check_exact(idx, dist, d2, ri, k, f"d={d}")


# ---- 2. exact ties ------------------------------------------------------------------------------------------------------
def lattice():
    pts = np.array(np.meshgrid(*[[0, 1, 2]] * 6, indexing="ij")).reshape(6, -1).T            # all 729 points
    rng = np.random.default_rng(7)
    pts = np.concatenate([pts, pts[rng.integers(0, 729, 60)]])                                # some duplicated
    return pts[rng.permutation(len(pts))].astype(np.int64)


def integer_expected(ref, query, k, self_skip):
    """Expected output from integer arithmetic: exact squared distances, ties by the lower index."""
    d2 = ((query[:, None, :] - ref[None, :, :]) ** 2).sum(-1)
    if self_skip:
        d2[np.arange(len(query)), np.arange(len(query))] = np.iinfo(np.int64).max
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return order, np.take_along_axis(d2, order, axis=1)


@pytest.mark.parametrize("include_self", [False, True])
@pytest.mark.parametrize("k", [1, 15, 64])
def test_lattice_ties(ctx, k, include_self):
    p = lattice()
    want_i, want_d2 = integer_expected(p, p, k, not include_self)
    idx, dist, info = knn(ctx, p.astype(np.float64), k=k, include_self=include_self)
    print("lattice", k, include_self, info)
    assert np.array_equal(idx.astype(np.int64), want_i)
    assert np.array_equal(dist, np.sqrt(want_d2.astype(np.float64)))
    if not include_self:
        assert not (idx == np.arange(len(p), dtype=np.uint32)[:, None]).any()
        assert (dist[:, 0] == 0).sum() >= 60                      # the duplicates list each other at distance 0


# ---- 3. differences f32 cannot see -------------------------------------------------------------------------------------
def test_f32_blind_differences(ctx):
    rng = np.random.default_rng(11)
    n, d = 1500, 8
    units = rng.integers(-40, 41, (n, d)).astype(np.int64)        # multiples of 2^-10 inside a cluster
    units[:, 0] += (np.arange(n) % 2) * (1 << 24)                 # the second cluster 2^14 away on axis 0
    x = units.astype(np.float64) * 2.0 ** -10                     # exact in f64; f32 loses the low bits next to 2^14
    assert np.array_equal(x * 1024, units)
    for k in (1, 15, 64):
        want_i, want_d2 = integer_expected(units, units, k, True)
        idx, dist, info = knn(ctx, x, k=k)
        print("f32-blind", k, "certified", info["rows_certified"], "recomputed", info["rows_recomputed"])
        assert info["rows_certified"] + info["rows_recomputed"] == n
        assert np.array_equal(idx.astype(np.int64), want_i)
        assert np.array_equal(dist, np.sqrt(want_d2.astype(np.float64) * 2.0 ** -20))


# ---- 4. query against reference ----------------------------------------------------------------------------------------
def test_query_against_reference(ctx):
    ref = clustered(301, 5000, 50)
    qry = clustered(302, 777, 50) * 1.0
    qry[5] = ref[1234]                                            # an exact copy of a reference row
    d2, ri = brute(ref, qry, kk=65)
    for k in KS:
        idx, dist, info = knn(ctx, ref, qry, k=k)
        assert (info["n_ref"], info["n_query"]) == (5000, 777)
        check_exact(idx, dist, d2, ri, k, "query")
        assert idx[5, 0] == 1234 and dist[5, 0] == 0.0
    sk = sklearn_sets(ref, 15, qry)
    assert all(set(a) == set(b) for a, b in zip(sk, ri[:, :15]))


# ---- 5. resident path ---------------------------------------------------------------------------------------------------
def _upload(ctx, x, store=2, csc=False):
    import singlerust_amd as sr
    x = x.tocsc() if csc else x.tocsr()
    x.sort_indices()
    dev = sr.DeviceCsr.upload(ctx, x.shape[0], x.shape[1], x.indptr, x.indices, x.data, store, csc=csc)
    return sr.IMAnnData(dev, x.indptr, x.indices, [f"c{i}" for i in range(x.shape[0])], [f"g{j}" for j in range(x.shape[1])])


def _fetch_scores(a, n_pc):
    from singlerust_amd import _ffi as F
    out = np.zeros((a.n_obs(), n_pc))
    F.check(F.lib().srx_result_fetch(a.x().handle, F.ptr(out), None, None, None, None, None), a.x().ctx.handle)
    return out


def _planted():
    z = np.load(os.path.join(GOLD, "planted_600x240.npz"))
    return sp.csr_matrix((z["log_values"], z["indices"].astype(np.int64), z["indptr"].astype(np.int64)),
                         shape=(int(z["n_rows"]), int(z["n_cols"])))


def _synthetic_cells(n, g, seed):
    rng = np.random.default_rng(seed)
    types = rng.integers(0, 8, n)
    rate = rng.gamma(0.3, 1.0, (8, g)) * 0.4
    x = sp.csr_matrix(rng.poisson(rate[types]).astype(np.float64))
    x.data = np.log1p(x.data)
    return x


@pytest.mark.parametrize("case", ["planted", "planted_csc", "synthetic_20000"])
def test_resident_path(ctx, case):
    import singlerust_amd as sr
    from singlerust_amd.memory.processing import dim_red, neighbors
    if case.startswith("planted"):
        x, n_pc, hvg, k = _planted(), 20, 120, 15
    else:
        x, n_pc, hvg, k = _synthetic_cells(20000, 300, 5), 50, 200, 15
    a = _upload(ctx, x, csc=case.endswith("csc"))
    dim_red.pca_inplace(a, n_pc, None, None, None, sr.FeatureSelection.HighlyVariable(hvg), None)
    before = _fetch_scores(a, n_pc)
    assert np.array_equal(before, a.obsm["X_pca"])
    u = neighbors(a, n_neighbors=k)
    assert u["info"]["n_query"] == x.shape[0] and u["info"]["d"] == n_pc and u["params"]["n_neighbors"] == k
    idx, dist, _ = knn(ctx, before, k=k)
    assert a.obsm["knn_indices"].dtype == np.uint32 and np.array_equal(a.obsm["knn_indices"], idx)
    assert np.array_equal(a.obsm["knn_distances"], dist)                       # bit-identical
    neighbors(a, n_neighbors=k, n_pcs=10)
    idx10, dist10, _ = knn(ctx, np.ascontiguousarray(before[:, :10]), k=k)
    assert np.array_equal(a.obsm["knn_indices"], idx10) and np.array_equal(a.obsm["knn_distances"], dist10)
    idx10b, dist10b, _ = knn(ctx, before, k=k, n_dims=10)
    assert np.array_equal(idx10, idx10b) and np.array_equal(dist10, dist10b)
    assert np.array_equal(_fetch_scores(a, n_pc), before)                      # the resident result is untouched
    if case == "planted":                                                     # against the host reference as well
        d2, ri = brute(before, kk=k + 1)
        assert np.array_equal(idx.astype(np.int64), ri[:, :k])


def test_projected_cells_find_fitted_neighbours(ctx):
    import singlerust_amd as sr
    from singlerust_amd.memory.processing import dim_red
    from singlerust_amd.memory.processing.dim_red import PcaModel
    x = _synthetic_cells(4000, 300, 9)
    fit, held = x[:3200], x[3200:]
    a = _upload(ctx, fit)
    dim_red.pca_inplace(a, 20, None, None, None, sr.FeatureSelection.HighlyVariable(150), None)
    model = PcaModel.from_result(a)
    proj = dim_red.pca_transform(_upload(ctx, held), model)
    ref = a.obsm["X_pca"]
    d2, ri = brute(ref, proj, kk=16)
    idx, dist, info = knn(ctx, ref, proj, k=15)
    assert info["n_query"] == 800
    check_exact(idx, dist, d2, ri, 15, "projected")


# ---- 6. determinism -----------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical(ctx):
    x = clustered(401, 6000, 50)
    i1, d1, f1 = knn(ctx, x, k=15)
    i2, d2, f2 = knn(ctx, x, k=15)
    assert np.array_equal(i1, i2) and np.array_equal(d1, d2) and f1 == f2


# ---- 7. errors ----------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import neighbors
    x = clustered(501, 200, 10)

    def refused(fn, *a, **kw):
        with pytest.raises(F.SrxError) as e:
            fn(*a, **kw)
        assert e.value.code == F.E_ARG and e.value.msg, (e.value.code, e.value.msg)
        return e.value.msg

    refused(knn, ctx, x, k=0)
    refused(knn, ctx, x, k=65)
    refused(knn, ctx, x[:10], k=10)                       # 9 admissible references without self
    knn(ctx, x[:10], k=10, include_self=True)             # ... 10 with it
    refused(knn, ctx, x[:10], x[:3], k=11)
    refused(knn, ctx, x, k=5, n_dims=11)
    refused(knn, ctx, np.zeros((50, F.KNN_MAX_DIMS + 1)), k=5)
    for v in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[17, 3] = v
        assert "NaN" in refused(knn, ctx, y, k=5)
        assert "NaN" in refused(knn, ctx, x, y, k=5)
    idx, dist, info = knn(ctx, x, x[:0], k=5)             # no query rows: nothing written, no error
    assert idx.shape == (0, 5) and info["n_query"] == 0
    a = _upload(ctx, sp.random(50, 30, density=0.3, format="csr", random_state=np.random.RandomState(1)))
    assert "no PCA result" in refused(neighbors, a)
    opts = F.KnnOpts(5, 0, 0, 0)
    assert F.lib().srx_knn_result(None, C.byref(opts), None, None, None) == F.E_ARG
    assert F.lib().srx_knn_points(None, F.ptr(x), 200, None, 0, 10, C.byref(opts), None, None, None) == F.E_ARG
    assert F.lib().srx_knn_points(ctx.handle, F.ptr(x), 200, None, 0, 10, None, None, None, None) == F.E_ARG
    # a context with more than one rank refuses: rows are sharded
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    assert "sharded" in refused(knn, c2, x, k=5)
    # and the context still works
    d2, ri = brute(x, kk=6)
    idx, dist, _ = knn(ctx, x, k=5)
    assert np.array_equal(idx.astype(np.int64), ri[:, :5])
    assert F.lib().srx_knn_points(ctx.handle, F.ptr(x), 200, None, 0, 10, C.byref(opts), None, None, None) == 0      # NULL outputs


# ---- 8. one larger run --------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_larger_run_sampled(ctx):
    """200 000 x 50 clustered, k = 15: 500 seeded sample rows against the host reference on those rows, exact.  (Measured on
    an MI355X: the device search takes well under a second; the host reference for the sample dominates the test.)"""
    import time
    x = clustered(601, 200000, 50)
    t0 = time.time()
    idx, dist, info = knn(ctx, x, k=15)
    dt = time.time() - t0
    print("200000 x 50:", info, f"{dt:.2f} s with the upload")
    assert dt < 120.0
    assert info["rows_certified"] + info["rows_recomputed"] == 200000
    rows = np.sort(np.random.default_rng(602).choice(200000, 500, replace=False))
    d2, ri = brute(x, kk=16, rows=rows)
    check_exact(idx[rows], dist[rows], d2, ri, 15, "200k sample")

"""srx_group_moments / srx_rank_genes_groups[_graph] on the device against the definition in include/srx.h: exact moments of
integer data, the statistics re-evaluated on the device's own moments (bit for bit), the accumulation bound, order freedom,
the ranking, the resident route, the known answer, refusals, one mid-size run and the Python layer.  Every case at f32 and
f64 storage."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import scipy.sparse as sp

import markers_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
STORES = [1, 2]                     # SRX_STORE_F32, SRX_STORE_F64
F64_TABLES = ("sum", "sumsq", "mean", "var", "mean_rest", "var_rest", "score", "lfc", "pct", "pct_rest")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def upload(ctx, X, store):
    import singlerust_amd as sr
    X = sp.csr_matrix(X)
    X.sort_indices()
    return sr.DeviceCsr.upload(ctx, X.shape[0], X.shape[1], X.indptr, X.indices, X.data, store)


def rank(dev, labels, n_groups, n_top=0, logged=-1):
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing.markers import Markers
    labels = np.ascontiguousarray(labels, np.uint32)
    h = C.c_void_p()
    opts = F.RankGenesOpts(n_top, logged)
    F.check(F.lib().srx_rank_genes_groups(dev.handle, F.ptr(labels), n_groups, C.byref(opts), C.byref(h)), dev.ctx.handle)
    return Markers(dev.ctx, h)


def group_moments(dev, labels, n_groups):
    from singlerust_amd import _ffi as F
    i = dev.info()
    labels = np.ascontiguousarray(labels, np.uint32)
    sizes = np.zeros(n_groups, np.uint64)
    cnt = np.zeros((n_groups, i.n_cols), np.uint64)
    s, q = np.zeros((n_groups, i.n_cols)), np.zeros((n_groups, i.n_cols))
    F.check(F.lib().srx_group_moments(dev.handle, F.ptr(labels), n_groups, F.ptr(sizes), F.ptr(cnt), F.ptr(s), F.ptr(q)), dev.ctx.handle)
    return sizes, cnt, s, q


def device_rest(dev, labels, n_groups):
    """(cnt, sum, sumsq) of the REST of every group as the device forms them: S_total - S_g in its fixed-point integers, then
    converted.  The sums are order-free integers at scales that depend on N and max_abs alone, so the group 1 of the two-group
    labelling [label != g] holds exactly that integer: the primitive itself hands it out."""
    labels = np.asarray(labels)
    out = [[], [], []]
    for g in range(n_groups):
        _, c, s, q = group_moments(dev, (labels != g).astype(np.uint32), 2)
        for o, a in zip(out, (c, s, q)):
            o.append(a[1])
    return tuple(np.stack(o) for o in out)


def rows_per_block(n_rows, n_cols):
    """The implementation's rule (markers.hip, mk_rows_per_block): gene tiles of at most 10000 genes (genes.hip)."""
    n_tiles = max(1, -(-n_cols // 10000))
    want = max(1, 1024 // n_tiles)
    return max(64, -(-n_rows // want))


def check_case(ctx, X, labels, n_groups, store, integer=True, logged=-1):
    """Everything the definition promises of one case; returns (markers, tables) for further checks."""
    X = sp.csr_matrix(X)
    labels = np.asarray(labels)
    N, G = X.shape
    dev = upload(ctx, X, store)
    mk = rank(dev, labels, n_groups, logged=logged)
    info = mk.info()
    sizes = mk.sizes()
    T = {k: mk.table(k) for k in ("cnt",) + F64_TABLES}
    assert info["n_rows"] == N and info["n_cols"] == G and info["n_groups"] == n_groups and info["n_top"] == min(100, G)
    assert np.array_equal(sizes, ref.sizes_of(labels, n_groups))
    # the scales are the header's formula
    assert info["max_abs"] == (float(np.abs(X.data).max()) if X.nnz else 0.0)
    assert (info["sum_scale_log2"], info["sq_scale_log2"]) == ref.scales(info["max_abs"], N)
    if integer:
        cnt, s, q = ref.exact_moments_int(X, labels, n_groups)
        assert np.array_equal(T["cnt"], cnt.astype(np.uint64))
        assert np.array_equal(T["sum"], s.astype(np.float64)) and np.array_equal(T["sumsq"], q.astype(np.float64))
    # the primitive gives the same tables
    gs, gc, gsum, gsq = group_moments(dev, labels, n_groups)
    assert np.array_equal(gs, sizes) and np.array_equal(gc, T["cnt"]) and same_bits(gsum, T["sum"]) and same_bits(gsq, T["sumsq"])
    # statistics = the definition evaluated on the device's own moments
    st = ref.statistics(sizes, T["cnt"], T["sum"], T["sumsq"], N, logged != 0, rest=device_rest(dev, labels, n_groups))
    for key in ("mean", "var", "mean_rest", "var_rest", "pct", "pct_rest", "score"):
        assert same_bits(T[key], st[key]), key
    finite = np.isfinite(st["lfc"])
    assert np.array_equal(finite, np.isfinite(T["lfc"]))
    assert np.all(np.abs(T["lfc"][finite] - st["lfc"][finite]) <= 1e-12 + 1e-12 * np.abs(st["lfc"][finite]))
    assert same_bits(T["lfc"][~finite], st["lfc"][~finite]) or np.array_equal(np.isnan(T["lfc"][~finite]), np.isnan(st["lfc"][~finite]))
    # degenerate groups
    deg = (sizes < 2) | (N - sizes.astype(np.int64) < 2)
    assert info["groups_degenerate"] == int(deg.sum()) == st["groups_degenerate"]
    assert not T["score"][deg].any() and not T["var"][deg].any() and not T["var_rest"][deg].any()
    # ranking: the order of the device's own scores
    genes, scores, lfc = mk.top()
    want = ref.order(T["score"])[:, :info["n_top"]]
    assert np.array_equal(genes, want)
    assert same_bits(scores, np.take_along_axis(T["score"], want, 1)) and same_bits(lfc, np.take_along_axis(T["lfc"], want, 1))
    return dev, mk, T


def counts_matrix(seed, n, g, density=None, per_row=None):
    """Integer counts 1 + geometric, canonical CSR."""
    rng = np.random.default_rng(seed)
    if per_row is not None:
        lens = rng.poisson(per_row, n)
        rows = np.repeat(np.arange(n), lens)
        cols = rng.integers(0, g, rows.size)
        m = sp.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(n, g)).tocsr()
        m.sum_duplicates()
        m.data[:] = 1.0
    else:
        m = sp.random(n, g, density=density, format="csr", random_state=rng)
    m.data = rng.geometric(0.5, m.nnz).astype(np.float64)
    m.sort_indices()
    return m


# ---- exact moments -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("shape", ["257x300", "2000x10001", "600x70000"])
def test_exact_moments(ctx, shape, store):
    if shape == "257x300":
        X, k = counts_matrix(1, 257, 300, density=0.1), 5
    elif shape == "2000x10001":
        X, k = counts_matrix(2, 2000, 10001, density=0.02), 7                        # two gene tiles
    else:
        X, k = counts_matrix(3, 600, 70000, per_row=8), 3                            # 32-bit column indices, seven tiles
    labels = np.random.default_rng(10).integers(0, k, X.shape[0])
    check_case(ctx, X, labels, k, store)


# ---- edges ---------------------------------------------------------------------------------------------------------------------
EDGE_SIZES = [0, 1, 2, 63, 64, 65]


def edge_matrix():
    """1100 x 513, labels sorted: groups of 0, 1, 2, 63, 64, 65 and 905 rows.  Group 1 (one row) and group 2 (two rows) are all
    empty rows, every larger group has an empty row; gene 7 is empty, gene 11 is stored in group 4 only, gene 13 is stored in
    every row that is not one of those empty rows (a stored gene and an empty row exclude each other)."""
    n, g = 1100, 513
    sizes = EDGE_SIZES + [n - sum(EDGE_SIZES)]
    labels = np.repeat(np.arange(len(sizes)), sizes)
    X = counts_matrix(4, n, g, density=0.05).tolil()
    X[:, 7] = 0
    X[:, 11] = 0
    X[np.flatnonzero(labels == 4)[::2], 11] = 3
    X[:, 13] = 2
    first = [int(np.flatnonzero(labels == k)[0]) for k in range(len(sizes)) if sizes[k]]
    for r in first + list(np.flatnonzero(labels == 2)):
        X[r, :] = 0
    X = sp.csr_matrix(X)
    X.eliminate_zeros()
    X.sort_indices()
    assert np.diff(X.indptr)[first].max() == 0 and X[:, 7].nnz == 0
    return X, labels, len(sizes)


@pytest.mark.parametrize("store", STORES)
def test_edges(ctx, store):
    X, labels, k = edge_matrix()
    n = X.shape[0]
    assert rows_per_block(*X.shape) == 64                                            # groups of 63 / 64 / 65: a block less one, a block, a block and one
    _, mk, base = check_case(ctx, X, labels, k, store)
    assert mk.info()["groups_degenerate"] == 2                                       # the empty group and the group of one
    rng = np.random.default_rng(5)
    for perm in (np.arange(n)[::-1], rng.permutation(n)):                            # labels reversed, interleaved: the same partition
        _, _, T = check_case(ctx, X[perm], labels[perm], k, store)
        assert all(same_bits(T[key], base[key]) for key in base)
    _, mk1, T1 = check_case(ctx, X, np.zeros(n, np.uint32), 1, store)                # one group: no rest
    assert mk1.info()["groups_degenerate"] == 1 and not T1["score"].any() and np.array_equal(mk1.sizes(), [n])
    assert np.array_equal(T1["sum"][0], np.asarray(X.sum(axis=0)).ravel())


@pytest.mark.parametrize("store", STORES)
def test_block_boundaries(ctx, store):
    """A shape whose rows-per-block rule gives more than the floor of 64: groups of exactly one block and of a block plus one row."""
    n, g = 70000, 40
    rpb = rows_per_block(n, g)
    assert rpb == 69
    sizes = [rpb, rpb + 1, rpb - 1, 2 * rpb, 2 * rpb + 1]
    labels = np.concatenate([np.repeat(np.arange(len(sizes)), sizes), np.full(n - sum(sizes), len(sizes))])
    labels = labels[np.random.default_rng(6).permutation(n)]
    check_case(ctx, counts_matrix(7, n, g, density=0.05), labels, len(sizes) + 1, store)


# ---- the log-normalised case -------------------------------------------------------------------------------------------------
def lognorm_counts():
    X = counts_matrix(8, 3000, 800, density=0.1).tolil()
    X[:, 6] = X[:, 5]                                                                # duplicate columns: tied scores
    X[:, 100:112] = 0                                                                # all-zero genes: score 0, tied
    X = sp.csr_matrix(X)
    X.eliminate_zeros()
    X.sort_indices()
    return X, np.random.default_rng(9).integers(0, 6, 3000), 6


def lognorm_device(ctx, X, store):
    from singlerust_amd import _ffi as F
    dev = upload(ctx, X, store)
    F.check(F.lib().srx_normalize_total_inplace(dev.handle, 1e4, 0), ctx.handle)
    F.check(F.lib().srx_log1p_inplace(dev.handle), ctx.handle)
    assert dev.info().store == store
    return dev, sp.csr_matrix((dev.values(np.float64), X.indices, X.indptr), shape=X.shape)


@pytest.mark.parametrize("store", STORES)
def test_lognormalised_statistics_bound_and_order_freedom(ctx, store):
    X, labels, k = lognorm_counts()
    dev, Y = lognorm_device(ctx, X, store)
    _, mk, T = check_case(ctx, Y, labels, k, store, integer=False)                   # (the same values, uploaded again)
    info, sizes = mk.info(), mk.sizes().astype(np.float64)
    # accumulation bound against the correctly rounded sums
    cnt, s, q = ref.exact_moments_fsum(Y, labels, k)
    assert np.array_equal(T["cnt"], cnt.astype(np.uint64))
    for name, got, want, sh in (("sum", T["sum"], s, info["sum_scale_log2"]), ("sumsq", T["sumsq"], q, info["sq_scale_log2"])):
        err = np.abs(got - want)
        bound = sizes[:, None] * 2.0 ** -(sh + 1) + 2.0 ** -52 * np.abs(want)
        print(name, "scale 2^%d: largest error %.3e, bound there %.3e" % (sh, err.max(), bound.ravel()[err.argmax()]))
        assert np.all(err <= bound)
    # the matrix transformed on the device holds those values: the same tables, twice
    a, b = rank(dev, labels, k), rank(dev, labels, k)
    for key in ("cnt",) + F64_TABLES:
        assert same_bits(a.table(key), T[key]) and same_bits(b.table(key), T[key]), key
    assert all(same_bits(x, y) for x, y in zip(a.top(), b.top()))
    # the rows in another order, uploaded and transformed again
    perm = np.random.default_rng(12).permutation(X.shape[0])
    devp, _ = lognorm_device(ctx, X[perm], store)
    p = rank(devp, labels[perm], k)
    for key in ("cnt", "sum", "sumsq"):
        assert same_bits(p.table(key), T[key]), key
    # many genes tie (the duplicate columns, the empty genes): the order is still (score desc, index asc)
    assert same_bits(T["score"][:, 5], T["score"][:, 6]) and not T["score"][:, 100:112].any()
    for n_top in (1, X.shape[1], 0):
        m2 = rank(dev, labels, k, n_top=n_top)
        want_top = n_top or 100
        assert m2.info()["n_top"] == want_top
        genes, scores, lfc = m2.top()
        want = ref.order(T["score"])[:, :want_top]
        assert genes.shape == (k, want_top) and np.array_equal(genes, want)
        assert same_bits(scores, np.take_along_axis(T["score"], want, 1)) and same_bits(lfc, np.take_along_axis(T["lfc"], want, 1))
    full = ref.order(T["score"])
    assert all(list(row).index(5) + 1 == list(row).index(6) for row in full)        # the tie goes to the lower index


# ---- the resident route ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_resident_route(ctx, store):
    from singlerust_amd import _ffi as F
    lib = F.lib()
    z = np.load(os.path.join(GOLD, "planted_600x240.npz"))
    n, g = int(z["n_rows"]), int(z["n_cols"])
    X = sp.csr_matrix((z["values"], z["indices"].astype(np.int64), z["indptr"].astype(np.int64)), shape=(n, g))
    dev = upload(ctx, X, store)
    popts, res = F.PcaOpts(20, -1, -1, -1, 0, 0, 0, 0.0, 11), F.PipelineResult()
    F.check(lib.srx_pipeline(dev.handle, 1e4, 120, C.byref(popts), C.byref(res)), ctx.handle)
    gh, mk_h = C.c_void_p(), C.c_void_p()
    F.check(lib.srx_neighbors_result(dev.handle, C.byref(F.KnnOpts(15, 0, 0, 0)), None, C.byref(gh)), ctx.handle)
    ropts = F.RankGenesOpts(0, -1)
    assert lib.srx_rank_genes_groups_graph(dev.handle, gh, C.byref(ropts), C.byref(mk_h)) == F.E_ARG and not mk_h.value   # no labels yet
    assert lib.srx_last_error(ctx.handle)
    F.check(lib.srx_louvain(gh, None, None, None), ctx.handle)

    def state():
        scores = np.zeros((n, 20))
        F.check(lib.srx_result_fetch(dev.handle, F.ptr(scores), None, None, None, None, None), ctx.handle)
        cnt, s, q = np.zeros(g, np.uint64), np.zeros(g), np.zeros(g)
        F.check(lib.srx_gene_moments(dev.handle, F.ptr(cnt), F.ptr(s), F.ptr(q)), ctx.handle)
        return dev.values(np.float64), scores, cnt, s, q

    before = state()
    from singlerust_amd.memory.processing.markers import Markers
    F.check(lib.srx_rank_genes_groups_graph(dev.handle, gh, C.byref(ropts), C.byref(mk_h)), ctx.handle)
    resident = Markers(ctx, mk_h)
    after = state()
    assert all(same_bits(x, y) for x, y in zip(before, after))                       # m and its results are as they were
    labels = np.zeros(n, np.uint32)
    F.check(lib.srx_graph_labels_fetch(gh, F.ptr(labels)), ctx.handle)
    k = int(labels.max()) + 1
    assert resident.info()["n_groups"] == k and k >= 2
    host = rank(dev, labels, k)
    for key in ("cnt",) + F64_TABLES:
        assert same_bits(resident.table(key), host.table(key)), key
    assert all(same_bits(x, y) for x, y in zip(resident.top(), host.top())) and np.array_equal(resident.sizes(), host.sizes())
    assert {k_: v for k_, v in resident.info().items() if k_ != "ms"} == {k_: v for k_, v in host.info().items() if k_ != "ms"}
    # a graph of another size is refused
    other = upload(ctx, X[:500], store)
    h2 = C.c_void_p()
    assert lib.srx_rank_genes_groups_graph(other.handle, gh, C.byref(ropts), C.byref(h2)) == F.E_ARG and not h2.value
    assert b"rows" in lib.srx_last_error(ctx.handle)
    resident.free()
    host.free()
    lib.srx_graph_free(gh)


# ---- the known answer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_known_answer(ctx, store):
    from fractions import Fraction
    kat = json.load(open(os.path.join(GOLD, "kat_markers.json")))
    base = json.load(open(os.path.join(GOLD, "kat_4x5.json")))
    X = sp.csr_matrix((np.array(base["data"], np.float64), base["indices"], base["indptr"]), shape=(base["n_rows"], base["n_cols"]))
    mk = rank(upload(ctx, X, store), kat["labels"], kat["n_groups"], n_top=5, logged=0)
    frac = lambda key: np.array([[float(Fraction(v)) for v in row] for row in kat[key]])
    assert np.array_equal(mk.sizes(), kat["n_cells"]) and np.array_equal(mk.table("cnt"), kat["cnt"])
    for key in ("sum", "sumsq", "mean", "var", "mean_rest", "var_rest", "pct", "pct_rest"):
        assert np.array_equal(mk.table(key), frac(key)), key
    assert np.allclose(mk.table("score"), kat["score"], rtol=4e-16, atol=0)
    assert np.allclose(mk.table("lfc"), kat["lfc_unlogged"], rtol=1e-12, atol=1e-12)
    assert np.array_equal(mk.top()[0], kat["ranked"]) and mk.info()["groups_degenerate"] == 0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    lib = F.lib()
    X = counts_matrix(20, 50, 30, density=0.2)
    dev = upload(ctx, X, 2)
    labels = np.random.default_rng(1).integers(0, 3, 50).astype(np.uint32)

    def refused(code, word, d=None, lab=labels, k=3, opts=None, c=None):
        d, c = d or dev, c or ctx
        h = C.c_void_p()
        rc = lib.srx_rank_genes_groups(d.handle, F.ptr(lab), k, None if opts is None else C.byref(opts), C.byref(h))
        msg = lib.srx_last_error(c.handle)
        assert rc == code and msg and word in msg.decode() and not h.value, (rc, msg)
        sizes = np.zeros(max(k, 1), np.uint64)
        rc = lib.srx_group_moments(d.handle, F.ptr(lab), k, F.ptr(sizes), None, None, None)
        assert (rc == code or opts is not None) and lib.srx_last_error(c.handle)

    refused(F.E_ARG, "n_groups", k=0)
    refused(F.E_ARG, "n_groups", k=F.GROUPS_MAX + 1)
    bad = labels.copy()
    bad[17] = 3
    refused(F.E_ARG, "label", lab=bad)
    refused(F.E_ARG, "n_top", opts=F.RankGenesOpts(31, -1))
    refused(F.E_ARG, "CSC", d=sr.DeviceCsr.upload(ctx, 50, 30, X.tocsc().indptr, X.tocsc().indices, X.tocsc().data, 2, csc=True))
    for v in (np.nan, np.inf, -np.inf):
        Y = X.copy()
        Y.data[5] = v
        refused(F.E_NAN, "NaN", d=upload(ctx, Y, 2))
    # the tables do not fit: 4096 groups x 4 000 000 genes x 20 bytes
    wide = sp.csr_matrix((np.ones(3), ([0, 4, 9], [1, 2_000_000, 3_999_999])), shape=(10, 4_000_000))
    refused(F.E_OOM, "fit", d=upload(ctx, wide, 2), lab=np.arange(10, dtype=np.uint32), k=F.GROUPS_MAX)
    # a context with more than one rank
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    refused(F.E_ARG, "sharded", d=upload(c2, X, 2), c=c2)
    # the context is still usable
    check_case(ctx, X, labels, 3, 2)


# ---- one mid-size run ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_midsize_run(ctx, store):
    n, g, k = 50_000, 3000, 20
    X = counts_matrix(30, n, g, density=0.03)
    labels = np.random.default_rng(31).integers(0, k, n)
    mk = rank(upload(ctx, X, store), labels, k)
    cnt, s, q = ref.exact_moments_int(X, labels, k)
    assert np.array_equal(mk.sizes(), ref.sizes_of(labels, k))
    assert np.array_equal(mk.table("cnt"), cnt.astype(np.uint64))
    assert np.array_equal(mk.table("sum"), s.astype(np.float64)) and np.array_equal(mk.table("sumsq"), q.astype(np.float64))
    print("50 000 x 3000, nnz %d, 20 groups, store %d: info.ms = %.3f" % (X.nnz, store, mk.info()["ms"]))


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_python_layer(ctx):
    import singlerust_amd as sr
    from singlerust_amd.memory.processing import dim_red, group_moments as py_group_moments, louvain, neighbors, rank_genes_groups
    from test_knn_gpu import _planted, _upload
    a = _upload(ctx, _planted())
    with pytest.raises(sr.SrxError):
        rank_genes_groups(a)                                                         # no obs["louvain"] yet
    dim_red.pca_inplace(a, 20, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    neighbors(a, n_neighbors=15, connectivities=True)
    louvain(a)
    info = rank_genes_groups(a, n_genes=25)
    u = a.uns["rank_genes_groups"]
    k = int(a.obs["louvain"].max()) + 1
    assert set(u) == {"names", "scores", "logfoldchanges", "pts", "pts_rest", "params", "info"}
    assert u["names"].shape == u["scores"].shape == u["logfoldchanges"].shape == (k, 25)
    assert u["pts"].shape == u["pts_rest"].shape == (k, a.n_vars())
    assert u["params"]["resident_labels"] and u["params"]["groupby"] == "louvain" and u["info"] == info and info["n_groups"] == k
    genes = a._markers.top()[0]
    assert all(u["names"][g_, r] == a.var_names[genes[g_, r]] for g_ in range(k) for r in range(25))
    assert np.all(np.diff(u["scores"], axis=1) <= 0)
    # host labels under another key: the same answer
    a.obs["copy"] = a.obs["louvain"].astype(np.int64)
    rank_genes_groups(a, groupby="copy", n_genes=25, key_added="again")
    v = a.uns["again"]
    assert not v["params"]["resident_labels"]
    assert np.array_equal(v["names"], u["names"]) and same_bits(v["scores"], u["scores"]) and same_bits(v["pts"], u["pts"])
    gm = py_group_moments(a, a.obs["louvain"])
    assert np.array_equal(gm["n_cells"], np.bincount(a.obs["louvain"])) and same_bits(gm["sum"], a._markers.table("sum"))

"""srx_autocorr / srx_autocorr_csr on the device against the definition in tests/autocorr_ref.py: every integer table and graph
sum bit for bit, the statistics within the header's bound of the fractions from those tables.  Row lengths and neighbour
lists around every width of the walk, gene counts around every tile edge and on the 32-bit index route, both storages, exact
integer data, segments beyond the 1024 threads and the first 512 entries, log-normalised data against the literal sums, signed zeros, order freedom, the resident route and every refusal."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import autocorr_ref as ref
from graph_edges import random_list

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
STORES = [1, 2]                     # SRX_STORE_F32, SRX_STORE_F64
INT_TABLES = ("sum_int", "sumsq_int", "dsum_int", "dsumsq_int", "cross_int")
INFO_EXACT = ("n", "n_genes", "nnz", "s_sum", "s_sumsq", "s_dsum", "s_dsumsq", "s_cross", "s_w", "s_1", "s_2", "max_abs", "max_weight",
              "max_degree", "w_int", "s1_int", "s2_int")


def upload(ctx, X, store):
    import singlerust_amd as sr
    X = sp.csr_matrix(X)
    X.sort_indices()
    return sr.DeviceCsr.upload(ctx, X.shape[0], X.shape[1], X.indptr, X.indices, X.data, store)


def run(dev, W, rows_per_block=None):
    from singlerust_amd.memory.processing import autocorr_csr
    W = sp.csr_matrix(W)
    W.sort_indices()
    return autocorr_csr(dev, (W.indptr, W.indices, W.data), rows_per_block)


def check(ctx, X, W, store, rows_per_block=None):
    """Everything the definition promises of one case: the device's tables and graph sums are the reference's integers, the f64
    tables their conversions, the statistics within the header's bounds of the fractions.  Returns (device result, tables)."""
    Xs = ref.as_storage(X, store)
    dev = upload(ctx, Xs, store)
    got = run(dev, W, rows_per_block)
    t = ref.tables(Xs, W)
    for k in INT_TABLES:
        assert got[k].tolist() == t[k], k
    for k in INFO_EXACT:
        assert got["info"][k] == t["info"][k], k
    for key, sc in (("sum", "s_sum"), ("sumsq", "s_sumsq"), ("dsum", "s_dsum"), ("dsumsq", "s_dsumsq"), ("cross", "s_cross")):
        assert got[key].tolist() == [math.ldexp(float(v), -t["info"][sc]) for v in t[key + "_int"]], key
    st = ref.stats(t)
    for g, (s, b) in enumerate(zip(st, ref.bounds(t, st))):
        for key, want, tol in (("morans_i", s[0], b and b[0]), ("gearys_c", s[1], b and b[1]), ("z_i", s[2], b and b[2]), ("z_c", s[3], b and b[3])):
            if want is None:
                assert math.isnan(got[key][g]), (key, g)
            else:
                assert abs(Fraction(float(got[key][g])) - Fraction(want)) <= Fraction(tol), (key, g, got[key][g], float(want), tol)
    assert got["info"]["genes_constant"] == sum(1 for s in st if s[0] is None)
    dev.free()
    return got, t


def counts(rng, n, g, density, hi=6):
    return sp.csr_matrix(np.where(rng.random((n, g)) < density, rng.integers(1, hi, (n, g)), 0).astype(np.float64))


def rows_with_lengths(rng, lengths, g, hi=6, lo_col=0):
    """A count matrix whose row i stores exactly lengths[i] genes, from column lo_col on."""
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    idx = np.concatenate([lo_col + np.sort(rng.choice(g - lo_col, int(k), replace=False)) for k in lengths] + [np.zeros(0, np.int64)])
    return sp.csr_matrix((rng.integers(1, hi, idx.size).astype(np.float64), idx.astype(np.int64), indptr), shape=(len(lengths), g))


def list_graph(n, lists):
    return ref.symmetric_graph(n, lists, lambda a, b: ((a * 7 + b * 3) % 8 + 1) / 8.0)


# ---- 1. the widths of the walk -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_row_lengths_and_neighbour_lists_around_every_width(ctx, store):
    """Rows of 0, 1, 63, 64, 65, 257 genes and one holding every gene; vertex v of the first 70 has exactly the neighbour list
    lengths 0 (isolated), 1, 15, 16, 17 (the waves of a workgroup) and 64 ABOVE it; the last vertices have all their neighbours
    below them (no j > i).  Integer counts with dyadic weights: everything is exact."""
    rng = np.random.default_rng(1)
    g = 300
    up = [0, 1, 15, 16, 17, 64]
    lengths = np.array(([0, 1, 63, 64, 65, 257, g] * 12)[:80])
    n = len(lengths)
    X = rows_with_lengths(rng, lengths, g)
    lists = {v: list(range(v + 1, v + 1 + up[v % 6])) for v in range(6)}           # vertex 0 stays isolated: nobody names it
    lists[1] = [2]
    lists[n - 1], lists[n - 2] = [70, 71], [60]                                   # the last vertices: every neighbour below them
    W = list_graph(n, {v: [j for j in js if j != 0 and j < n] for v, js in lists.items()})
    above = np.diff(sp.triu(W, 1).tocsr().indptr)
    assert W[0].nnz == 0 and sorted(set(above[:6])) == [0, 1, 15, 16, 17, 64] and above[-1] == 0 and W[n - 1].nnz > 0
    got, t = check(ctx, X, W, store)
    assert min(v for k, v in t["info"].items() if k.startswith("s_")) >= 0
    lit = ref.literal_fraction(X.toarray()[:, :3].tolist(), W.toarray().tolist())                     # exact tables ARE the textbook sums
    assert [s[:2] for s in ref.stats(t)[:3]] == lit
    for rpb in (1, 7, 16, 17, 80):                                                                       # the tables do not depend on the blocks
        again = run(upload(ctx, ref.as_storage(X, store), store), W, rpb)
        assert all(again[k].tolist() == t[k] for k in INT_TABLES), rpb


@pytest.mark.parametrize("store", STORES)
def test_segments_beyond_the_workgroup_and_the_first_chunks(ctx, store):
    """The widths the test above does not reach, at G = 2000 in one tile: rows of 1025, 1500 and all 2000 stored genes take the
    plain-load scatter and clear loops beyond the 1024 entries the threads hold in registers, and as NEIGHBOURS rows of 513,
    1025, 1500 and 2000 entries take further trips of the segment loop beyond the first 512.  Each long row has neighbours
    above it, is itself the neighbour of a row below it, and is followed in its block by short rows with neighbours above
    them, whose P a T left uncleared would corrupt.  Integer counts, dyadic weights: exact, bit for bit."""
    rng = np.random.default_rng(2)
    g, n = 2000, 40
    lengths = rng.integers(5, 40, n)
    lengths[[3, 5, 8, 20, 25]] = [1025, 1500, 2000, 513, 1025]
    X = rows_with_lengths(rng, lengths, g)
    lists = {i: rng.choice(np.delete(np.arange(n), i), 3, replace=False) for i in range(n)}
    lists.update({2: [3, 20, 4], 3: [5, 20, 25, 8, 4], 4: [6, 7, 25], 5: [8, 25, 6], 6: [9, 20], 8: [20, 25, 30, 9], 9: [10, 11]})
    W = list_graph(n, lists)
    up = sp.triu(W, 1).tocsr()
    assert all(up[i].nnz > 0 for i in (3, 4, 5, 6, 8, 9)) and {20, 25}.issubset(up[3].indices) and 8 in up[5].indices
    for rpb in (None, 40, 4):                                       # the long rows and their followers in one block; a block edge after row 3
        got, t = check(ctx, X, W, store, rows_per_block=rpb)
    assert min(v for k, v in t["info"].items() if k.startswith("s_")) >= 0 and sum(1 for v in t["cross_int"] if v) > g // 2


@pytest.mark.parametrize("g", [1, 65, 300])
def test_gene_counts_inside_one_tile(ctx, g):
    rng = np.random.default_rng(10 + g)
    n = 90
    check(ctx, counts(rng, n, g, 0.3 if g > 1 else 0.7), ref.random_graph(rng, n, 4), 1 + g % 2)


@pytest.mark.parametrize("g,store", [(10000, 1), (10001, 2), (20001, 1), (65536, 2), (65537, 1), (70001, 2)])
def test_gene_counts_around_every_tile_edge_and_the_32_bit_route(ctx, g, store):
    """One tile of exactly 10000 genes; 10001 and 20001 genes: two and three tiles of ceil(G / tiles) genes, with entries on both
    sides of every cut; 65536: the last G with the 16-bit index mirror; 65537 and 70001: 32-bit indices.  Few entries per row."""
    rng = np.random.default_rng(g)
    n = 48
    tiles = -(-g // ref.TILE_GENES)
    tg = -(-g // tiles)
    edge = sorted({c for k in range(tiles + 1) for c in (k * tg - 1, k * tg, k * tg + 1) if 0 <= c < g} | {0, g - 1})
    X = sp.lil_matrix((n, g))
    for i in range(n):
        for c in rng.choice(edge, min(5, len(edge)), replace=False):
            X[i, c] = float(rng.integers(1, 5))
        for c in rng.choice(g, 12, replace=False):
            X[i, c] = float(rng.integers(1, 5))
    got, t = check(ctx, X.tocsr(), ref.random_graph(rng, n, 5), store, rows_per_block=16)
    assert any(t["cross_int"][c] for c in edge)


# ---- 2. values ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_log_normalised_values_against_the_literal_sums(ctx, store):
    """Log-normalised values with UMAP-like weights: the tables carry rounding, within the quanta the header states; the
    statistics lie within the bound derived from those quanta and den (autocorr_ref.quanta_bounds) of the literal numpy
    evaluation, plus what that f64 evaluation loses itself (autocorr_ref.f64_slack)."""
    rng = np.random.default_rng(20)
    n, g = 300, 60
    X = counts(rng, n, g, 0.25, 30)
    X.data = np.log1p(X.data * 1e4 / 2000.0)
    X = ref.as_storage(X, store)
    W = ref.random_graph(rng, n, 6, dyadic=False)
    got, t = check(ctx, X, W, store)
    I, Cc, parts = ref.literal_f64(X, W)
    qb = ref.quanta_bounds(t, X, W)
    si, sc = ref.f64_slack(parts, n, W.nnz)
    worst = 0.0
    for j in range(g):
        if qb[j] is None:
            continue
        assert abs(got["morans_i"][j] - I[j]) <= qb[j][0] + si[j] + 2.0 ** -52 * abs(I[j]), (j, got["morans_i"][j], I[j], qb[j][0], si[j])
        assert abs(got["gearys_c"][j] - Cc[j]) <= qb[j][1] + sc[j] + 2.0 ** -52 * abs(Cc[j]), (j, got["gearys_c"][j], Cc[j], qb[j][1], sc[j])
        worst = max(worst, abs(got["morans_i"][j] - I[j]))
    print("store %d: largest |I - literal f64| = %.3e" % (store, worst))
    # the quanta themselves: every table within (terms) 2^-(scale + 1) of the exact sum over the stored values
    Xd = np.asarray(X.todense())
    exact_S = [sum(Fraction(v) for v in Xd[:, j] if v) for j in range(4)]
    for j in range(4):
        assert abs(Fraction(t["sum_int"][j], 1) / Fraction(2) ** t["info"]["s_sum"] - exact_S[j]) <= Fraction(n, 2 ** (t["info"]["s_sum"] + 1))


@pytest.mark.parametrize("store", STORES)
def test_negative_values_and_stored_signed_zeros(ctx, store):
    rng = np.random.default_rng(30)
    n, g = 70, 40
    X = counts(rng, n, g, 0.4, 9).tocoo()
    data = X.data - 4.0                                                             # -3 .. 4, with stored zeros
    data[data == 0.0] = np.where(rng.random(np.count_nonzero(data == 0.0)) < 0.5, 0.0, -0.0)
    X = sp.csr_matrix((data, (X.row, X.col)), shape=(n, g))
    assert np.count_nonzero(X.data == 0.0) > 20 and np.signbit(X.data[X.data == 0.0]).any() and (X.data < 0).any()
    got, t = check(ctx, X, ref.random_graph(rng, n, 5), store)
    assert min(t["cross_int"]) < 0 < max(t["cross_int"])
    # a gene of stored zeros alone is constant
    Z = sp.csr_matrix((np.array([0.0, -0.0, 0.0]), (np.array([0, 3, 9]), np.array([0, 0, 0]))), shape=(n, 1))
    got, _ = check(ctx, Z, ref.random_graph(rng, n, 3), store)
    assert math.isnan(got["morans_i"][0]) and got["info"]["genes_constant"] == 1 and got["info"]["max_abs"] == 0.0


# ---- 3. order freedom and the moments primitive ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_order_freedom_repeatability_and_group_moments(ctx, store):
    from singlerust_amd import _ffi as F
    rng = np.random.default_rng(40)
    n, g = 260, 120
    X = counts(rng, n, g, 0.2, 50)
    X.data = np.log1p(X.data)
    X = ref.as_storage(X, store)
    idx, _ = random_list(n, 7, 41)
    W = ref.symmetric_graph(n, {i: idx[i] for i in range(n)}, lambda a, b: float(np.exp(-((a * 31 + b * 17) % 97) / 19.0)))
    dev = upload(ctx, X, store)
    a, b = run(dev, W), run(dev, W, rows_per_block=33)
    for k in INT_TABLES + ("morans_i", "gearys_c", "z_i", "z_c"):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k                       # two calls, other blocks: the same bits
    # cells permuted, matrix and graph together
    p = rng.permutation(n)
    Xp, Wp = X[p], sp.csr_matrix(W[p][:, p])
    c = run(upload(ctx, Xp, store), Wp)
    for k in INT_TABLES + ("morans_i", "gearys_c", "z_i", "z_c"):
        assert np.array_equal(a[k].view(np.uint64), c[k].view(np.uint64)), k
    assert a["info"]["w_int"] == c["info"]["w_int"] and a["info"]["s2_int"] == c["info"]["s2_int"]
    # S and Q are srx_group_moments with one group, bit for bit
    sizes, cnt = np.zeros(1, np.uint64), np.zeros((1, g), np.uint64)
    s, q = np.zeros((1, g)), np.zeros((1, g))
    labels = np.zeros(n, np.uint32)
    F.check(F.lib().srx_group_moments(dev.handle, F.ptr(labels), 1, F.ptr(sizes), F.ptr(cnt), F.ptr(s), F.ptr(q)), ctx.handle)
    assert np.array_equal(s[0].view(np.uint64), a["sum"].view(np.uint64)) and np.array_equal(q[0].view(np.uint64), a["sumsq"].view(np.uint64))


# ---- 4. the resident route -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_resident_route_equals_csr_and_leaves_the_matrix_alone(ctx, store):
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing.autocorr import _Out
    lib = F.lib()
    z = np.load(os.path.join(GOLD, "planted_600x240.npz"))
    n, g = int(z["n_rows"]), int(z["n_cols"])
    X = sp.csr_matrix((z["values"], z["indices"].astype(np.int64), z["indptr"].astype(np.int64)), shape=(n, g))
    dev = upload(ctx, X, store)
    popts, res = F.PcaOpts(20, -1, -1, -1, 0, 0, 0, 0.0, 11), F.PipelineResult()
    F.check(lib.srx_pipeline(dev.handle, 1e4, 120, C.byref(popts), C.byref(res)), ctx.handle)
    gh = C.c_void_p()
    F.check(lib.srx_neighbors_result(dev.handle, C.byref(F.KnnOpts(15, 0, 0, 0)), None, C.byref(gh)), ctx.handle)

    def state():
        scores = np.zeros((n, 20))
        F.check(lib.srx_result_fetch(dev.handle, F.ptr(scores), None, None, None, None, None), ctx.handle)
        cnt, s, q = np.zeros(g, np.uint64), np.zeros(g), np.zeros(g)
        F.check(lib.srx_gene_moments(dev.handle, F.ptr(cnt), F.ptr(s), F.ptr(q)), ctx.handle)
        return dev.values(np.float64), scores, cnt, s, q

    before = state()
    o = _Out(g)
    F.check(lib.srx_autocorr(dev.handle, gh, None, C.byref(o.c), C.byref(o.info)), ctx.handle)
    resident = o.result()
    after = state()
    assert all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(before, after))
    gi = F.GraphInfo()
    F.check(lib.srx_graph_info_get(gh, C.byref(gi)), ctx.handle)
    indptr, indices, data = np.zeros(n + 1, np.uint64), np.zeros(gi.nnz_connectivities, np.uint32), np.zeros(gi.nnz_connectivities)
    F.check(lib.srx_graph_fetch(gh, F.GRAPH_CONNECTIVITIES, F.ptr(indptr), F.ptr(indices), F.ptr(data)), ctx.handle)
    host = run(dev, sp.csr_matrix((data, indices.astype(np.int64), indptr.astype(np.int64)), shape=(n, n)))
    for k in INT_TABLES + ("morans_i", "gearys_c", "z_i", "z_c", "sum", "cross"):
        assert np.array_equal(resident[k].view(np.uint64), host[k].view(np.uint64)), k
    drop = tuple(k for k in resident["info"] if k.startswith("ms"))
    assert {k: v for k, v in resident["info"].items() if k not in drop} == {k: v for k, v in host["info"].items() if k not in drop}
    assert resident["info"]["nnz"] == gi.nnz_connectivities and resident["info"]["ms"] > 0
    # planted structure: the planted genes vary smoothly along the graph of their own PCA
    assert np.nanmax(resident["morans_i"]) > 0.2 and np.nanmax(resident["z_i"]) > 10
    # the refusals that need a handle
    other = upload(ctx, X[:500], store)
    assert lib.srx_autocorr(other.handle, gh, None, None, None) == F.E_ARG and b"rows" in lib.srx_last_error(ctx.handle)
    assert lib.srx_autocorr(dev.handle, None, None, None, None) == F.E_ARG and b"null graph" in lib.srx_last_error(ctx.handle)
    assert lib.srx_autocorr(None, gh, None, None, None) == F.E_ARG
    lib.srx_graph_free(gh)


def test_python_layer_on_the_adata(ctx):
    import singlerust_amd as sr
    from singlerust_amd.memory import processing
    z = np.load(os.path.join(GOLD, "planted_600x240.npz"))
    n, g = int(z["n_rows"]), int(z["n_cols"])
    a = sr.IMAnnData.new_basic((n, g, z["indptr"], z["indices"], z["values"]), ctx=ctx, store=2)
    with pytest.raises(sr._ffi.SrxError):
        processing.morans_i(a)                                                        # no graph yet
    processing.normalize_total_inplace(a, 1e4, sr.Direction.Row)
    processing.log1p_transform_inplace(a)
    processing.dim_red.pca_inplace(a, 10, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    processing.neighbors(a, n_neighbors=10, connectivities=True)
    r = processing.gene_autocorr(a)
    assert a.uns["autocorr"] is r and r["info"]["n"] == n and r["info"]["n_genes"] == g
    assert np.array_equal(processing.morans_i(a).view(np.uint64), r["morans_i"].view(np.uint64))
    assert np.array_equal(processing.gearys_c(a, genes=[5, 0, 7]).view(np.uint64), r["gearys_c"][[5, 0, 7]].view(np.uint64))


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    lib = F.lib()
    rng = np.random.default_rng(50)
    n, g = 40, 12
    X = counts(rng, n, g, 0.4)
    W = ref.random_graph(rng, n, 3)
    dev = upload(ctx, X, 2)

    def call(d, W, n_arg=None):
        W = sp.csr_matrix(W)
        indptr, indices, data = W.indptr.astype(np.uint64), W.indices.astype(np.uint32), W.data.astype(np.float64)
        rc = lib.srx_autocorr_csr(d.handle, F.ptr(indptr), F.ptr(indices) if indices.size else None, F.ptr(data) if data.size else None,
                                  W.shape[0] if n_arg is None else n_arg, None, None, None)
        return rc, lib.srx_last_error(ctx.handle)

    assert call(dev, W)[0] == F.OK
    rc, msg = call(dev.to_csc(), W)
    assert rc == F.E_ARG and b"CSC" in msg
    rc, msg = call(dev, ref.random_graph(rng, n - 1, 3))
    assert rc == F.E_ARG and b"cells" in msg and b"rows" in msg
    rc, msg = call(upload(ctx, X[:1], 2), sp.csr_matrix((1, 1)))
    assert rc == F.E_ARG and b"at least 2" in msg
    rc, msg = call(dev, sp.csr_matrix((n, n)))
    assert rc == F.E_ARG and b"W = 0" in msg
    # everything the symmetric-CSR check refuses
    A = W.toarray()
    D = A.copy(); D[3, 3] = 1.0
    U = A.copy(); i, j = np.argwhere(A > 0)[0]; U[i, j] = A[i, j] * 2
    Ng = A.copy(); Ng[i, j] = Ng[j, i] = -1.0
    for bad, word in ((D, b"diagonal"), (U, b"symmetric"), (Ng, b"weight")):
        rc, msg = call(dev, sp.csr_matrix(bad))
        assert rc == F.E_ARG and word in msg, word
    unsorted = sp.csr_matrix(W).copy()
    lo, hi = unsorted.indptr[i], unsorted.indptr[i + 1]
    assert hi - lo >= 2
    unsorted.indices[lo:hi] = unsorted.indices[lo:hi][::-1].copy()
    unsorted.data[lo:hi] = unsorted.data[lo:hi][::-1].copy()
    rc, msg = lib.srx_autocorr_csr(dev.handle, F.ptr(unsorted.indptr.astype(np.uint64)), F.ptr(unsorted.indices.astype(np.uint32)),
                                   F.ptr(unsorted.data), n, None, None, None), lib.srx_last_error(ctx.handle)
    assert rc == F.E_ARG and b"ascending" in msg
    rng_idx = sp.csr_matrix(W).copy()
    ind = rng_idx.indices.astype(np.uint32)
    ind[0] = n + 5
    assert lib.srx_autocorr_csr(dev.handle, F.ptr(rng_idx.indptr.astype(np.uint64)), F.ptr(ind), F.ptr(rng_idx.data), n, None, None, None) == F.E_ARG
    # NaN and Inf among the stored values
    for v in (np.nan, np.inf):
        Xn = sp.csr_matrix(X).copy()
        Xn.data[7] = v
        rc, msg = call(upload(ctx, Xn, 2), W)
        assert rc == F.E_NAN and b"NaN or Inf" in msg
    # a value outside the admitted range: x x would leave what the scales can hold
    Xb = sp.csr_matrix(X).copy()
    Xb.data[3] = 1e80
    rc, msg = call(upload(ctx, Xb, 2), W)
    assert rc == F.E_ARG and b"2^255" in msg
    # two contexts; several ranks
    c2 = sr.Context(0)
    dev2 = upload(c2, X, 2)
    popts, res = F.PcaOpts(5, -1, -1, -1, 0, 0, 0, 0.0, 11), F.PipelineResult()
    F.check(lib.srx_pipeline(dev2.handle, 1e4, 10, C.byref(popts), C.byref(res)), c2.handle)
    gh = C.c_void_p()
    F.check(lib.srx_neighbors_result(dev2.handle, C.byref(F.KnnOpts(5, 0, 0, 0)), None, C.byref(gh)), c2.handle)
    assert lib.srx_autocorr(dev2.handle, gh, None, None, None) == F.OK
    assert lib.srx_autocorr(dev.handle, gh, None, None, None) == F.E_ARG and b"different contexts" in lib.srx_last_error(ctx.handle)
    lib.srx_graph_free(gh)
    dev2.free()
    c3 = sr.Context(0)
    c3.comm_init_host(2, 0, lambda buf: None)
    d3 = upload(c3, X, 2)
    Wc = sp.csr_matrix(W)
    rc = lib.srx_autocorr_csr(d3.handle, F.ptr(Wc.indptr.astype(np.uint64)), F.ptr(Wc.indices.astype(np.uint32)), F.ptr(Wc.data), n, None, None, None)
    assert rc == F.E_ARG and b"sharded" in lib.srx_last_error(c3.handle)

"""srx_rank_genes_wilcoxon[_graph] on the device against the definition in include/srx.h, through the host reference
(tests/wilcoxon_ref.py): the doubled rank sums and the tie terms by integer equality, the scores and the top lists bit for bit,
the moment-derived tables bit-equal to a t-test call on the same input.  Segment lengths on both sides of every route, tie runs
across every boundary of the sort and of the rank walk, chunking, order freedom, the group edges, the resident route, refusals,
the Python layer and the known answer.  Every case at f32 and f64 storage."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import markers_ref
import wilcoxon_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
STORES = [1, 2]                     # SRX_STORE_F32, SRX_STORE_F64
MOMENT_TABLES = ("cnt", "sum", "sumsq", "mean", "var", "mean_rest", "var_rest", "lfc", "pct", "pct_rest")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def csr(rows, cols, vals, shape):
    """Canonical CSR that KEEPS explicit zeros (a stored 0.0 / -0.0 is an entry); (row, col) pairs must be distinct."""
    m = sp.csr_matrix((np.asarray(vals, np.float64), (np.asarray(rows), np.asarray(cols))), shape=shape)
    m.sort_indices()
    assert m.nnz == len(vals)
    return m


def upload(ctx, X, store):
    import singlerust_amd as sr
    return sr.DeviceCsr.upload(ctx, X.shape[0], X.shape[1], X.indptr, X.indices, X.data, store)


def wilcoxon(dev, labels, n_groups, n_top=0, logged=-1, tie_correct=1, scratch=0):
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing.markers import Markers
    labels = np.ascontiguousarray(labels, np.uint32)
    h = C.c_void_p()
    opts = F.WilcoxonOpts(n_top, logged, tie_correct, 0, scratch)
    F.check(F.lib().srx_rank_genes_wilcoxon(dev.handle, F.ptr(labels), n_groups, C.byref(opts), C.byref(h)), dev.ctx.handle)
    return Markers(dev.ctx, h)


def ttest(dev, labels, n_groups, n_top=0, logged=-1):
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing.markers import Markers
    labels = np.ascontiguousarray(labels, np.uint32)
    h = C.c_void_p()
    opts = F.RankGenesOpts(n_top, logged)
    F.check(F.lib().srx_rank_genes_groups(dev.handle, F.ptr(labels), n_groups, C.byref(opts), C.byref(h)), dev.ctx.handle)
    return Markers(dev.ctx, h)


def tables_of(mk):
    T = {k: mk.table(k) for k in MOMENT_TABLES + ("score", "ranksum2")}
    T["ties"] = mk.ties() if mk.wilcoxon_info()["tie_correct"] else None
    T["top"] = mk.top()
    T["sizes"] = mk.sizes()
    return T


def same_tables(a, b):
    for k in a:
        if k == "top":
            assert all(same_bits(x, y) for x, y in zip(a[k], b[k])), k
        elif a[k] is None:
            assert b[k] is None
        else:
            assert same_bits(a[k], b[k]), k


def check_case(ctx, X, labels, n_groups, store, tie_correct=1, scratch=0, dev=None):
    """Everything the definition promises of one case; returns (device matrix, markers, tables)."""
    labels = np.asarray(labels)
    N, G = X.shape
    dev = dev or upload(ctx, X, store)
    mk = wilcoxon(dev, labels, n_groups, tie_correct=tie_correct, scratch=scratch)
    info, wi = mk.info(), mk.wilcoxon_info()
    T = tables_of(mk)
    want = ref.reference(X, labels, n_groups, store, bool(tie_correct))
    assert info["n_rows"] == N and info["n_cols"] == G and info["n_groups"] == n_groups and info["n_top"] == min(100, G)
    assert wi["tie_correct"] == int(bool(tie_correct)) and wi["n_chunks"] >= 1
    assert np.array_equal(T["sizes"], markers_ref.sizes_of(labels, n_groups))
    # integers: equal
    assert T["ranksum2"].dtype == np.uint64 and np.array_equal(T["ranksum2"], want["ranksum2"])
    assert np.array_equal(T["ranksum2"].sum(axis=0), np.full(G, N * (N + 1), np.uint64))
    if tie_correct:
        assert T["ties"].dtype == np.uint64 and np.array_equal(T["ties"], want["ties"])
    # the score: the stated operations on those integers, bit for bit
    assert same_bits(T["score"], want["score"])
    assert info["groups_degenerate"] == want["groups_degenerate"]
    deg = (T["sizes"] == 0) | (T["sizes"] == N)
    assert not T["score"][deg].any()
    # the ranking: the order of those scores
    genes, scores, lfc = T["top"]
    order = markers_ref.order(T["score"])[:, :info["n_top"]]
    assert np.array_equal(genes, order)
    assert same_bits(scores, np.take_along_axis(T["score"], order, 1)) and same_bits(lfc, np.take_along_axis(T["lfc"], order, 1))
    # the moment-derived tables: those of the t-test call on the same input
    tt = ttest(dev, labels, n_groups)
    for key in MOMENT_TABLES:
        assert same_bits(T[key], tt.table(key)), key
    assert np.array_equal(T["sizes"], tt.sizes())
    ti = tt.info()
    assert all(info[k] == ti[k] for k in ("sum_scale_log2", "sq_scale_log2", "max_abs"))
    tt.free()
    return dev, mk, T


_LIMIT = []


def segment_limit(ctx):
    """srx_wilcoxon_info.segment_limit, asked once per session."""
    if not _LIMIT:
        dev = upload(ctx, csr([0], [0], [1.0], (2, 2)), 2)
        mk = wilcoxon(dev, [0, 1], 2)
        _LIMIT.append(int(mk.wilcoxon_info()["segment_limit"]))
        mk.free()
        dev.free()
    return _LIMIT[0]


def tied_values(rng, n):
    """Few distinct values, negative ones and both stored zeros among them: ties everywhere."""
    return rng.choice(np.array([-1.5, -0.25, 0.0, -0.0, 0.5, 0.5000000001, 1.0, 2.75, 3.0]), n)


# ---- segment lengths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_segment_lengths(ctx, store):
    L = segment_limit(ctx)
    if L:
        lens = [0, 1, 2, 63, 64, 65, L - 1, L, L + 1]
        N = (L + 1 + 64) // 64 * 64                                                 # the next multiple of 64 above L + 1
    else:
        lens, N = [0, 1, 2, 63, 64, 65, 4095, 4096, 4097], 20_000
    lens.append(N)
    rng = np.random.default_rng(40)
    rows, cols = [], []
    for j, c in enumerate(lens):
        rows.append(rng.choice(N, c, replace=False))
        cols.append(np.full(c, j))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    X = csr(rows, cols, tied_values(rng, rows.size), (N, len(lens)))
    assert list(np.diff(X.tocsc().indptr)) == lens
    labels = rng.integers(0, 5, N)
    for tie_correct in (1, 0):
        _, mk, _ = check_case(ctx, X, labels, 5, store, tie_correct=tie_correct)
        wi = mk.wilcoxon_info()
        mk.free()
        assert wi["segments_short"] > 0 and wi["segments_long"] > 0                  # both routes ran
        if L:
            assert wi["segments_short"] == 7 and wi["segments_long"] == 2           # 1 .. L entries; L + 1 and N
    # distinct values throughout (no ties but the zeros): every key moves in the sort
    Y = X.copy()
    Y.data = rng.permutation(Y.nnz).astype(np.float64) - Y.nnz // 3                 # integers, exact at f32; one of them is a stored 0
    check_case(ctx, Y, labels, 5, store)[1].free()


# ---- tie runs across boundaries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_tie_runs_across_boundaries(ctx, store):
    L = segment_limit(ctx) or 4096
    N = 2 * L + 300
    rng = np.random.default_rng(41)
    columns = []                                                                    # (rows, values) per gene
    everyone = np.arange(N)
    columns.append((everyone, np.full(N, 1.25)))                                    # longer than L, all equal: one run, no implicit zero
    # two distinct values, the lower one p times: the run ends at sorted place p, on each side of the multiples of 256 that
    # are also edges of a rank round (1024), of a radix tile and of the LDS sort (L)
    for p in (1, 255, 256, 257, 1023, 1024, 1025, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, N - 1):
        v = np.full(N, 7.5)
        v[rng.choice(N, p, replace=False)] = -2.0 if p % 2 else 0.5
        columns.append((everyone, v))
    for p in (255, 256, 257, 1023, 1024, 1025):                                     # the same inside one LDS sort: L / 2 + 7 stored
        r = rng.choice(N, L // 2 + 7, replace=False)
        v = np.full(r.size, 3.0)
        v[rng.choice(r.size, p, replace=False)] = 0.25
        columns.append((r, v))
    # stored 0.0 and -0.0 beside negative and positive entries: without an implicit zero, and with many
    columns.append((everyone, tied_values(rng, N)))
    r = rng.choice(N, L + 500, replace=False)
    columns.append((r, tied_values(rng, r.size)))
    r = rng.choice(N, 700, replace=False)
    columns.append((r, tied_values(rng, r.size)))
    columns.append((everyone, np.where(rng.random(N) < 0.5, 0.0, -0.0)))            # every cell a stored zero: one run of N
    rows = np.concatenate([c[0] for c in columns])
    cols = np.concatenate([np.full(c[0].size, j) for j, c in enumerate(columns)])
    X = csr(rows, cols, np.concatenate([c[1] for c in columns]), (N, len(columns)))
    labels = rng.integers(0, 3, N)
    dev, mk, T = check_case(ctx, X, labels, 3, store)
    assert int(T["ties"][0]) == N ** 3 - N and int(T["ties"][-1]) == N ** 3 - N and not T["score"][:, [0, -1]].any()
    wi = mk.wilcoxon_info()
    assert wi["n_chunks"] == 1 and wi["segments_long"] >= 18 and wi["segments_short"] >= 7
    mk.free()
    # the same through several chunks: the radix route's tile records, table and scan are rebuilt per chunk, long and short
    # segments side by side
    entry = 2 * ((4 if store == 1 else 8) + 2)
    for parts in (4, 12):
        mk2 = wilcoxon(dev, labels, 3, scratch=X.nnz * entry // parts)
        w2 = mk2.wilcoxon_info()
        assert w2["n_chunks"] >= 3 and w2["scratch_bytes"] >= N * entry and w2["segments_long"] == wi["segments_long"]
        same_tables(tables_of(mk2), T)
        mk2.free()
    check_case(ctx, X, labels, 3, store, tie_correct=0, dev=dev)[1].free()


# ---- chunking ------------------------------------------------------------------------------------------------------------------
def lognorm_matrix(seed, n, g, density):
    rng = np.random.default_rng(seed)
    m = sp.random(n, g, density=density, format="csr", random_state=rng)
    m.data = np.log1p(rng.geometric(0.4, m.nnz) * rng.choice([0.7, 1.0, 1.3, 10.0 / 3.0], m.nnz))      # ties; f32 rounds these
    m.sort_indices()
    return m


@pytest.mark.parametrize("store", STORES)
def test_chunking(ctx, store):
    X = lognorm_matrix(42, 2000, 300, 0.1)
    labels = np.random.default_rng(43).integers(0, 6, 2000)
    dev, mk, base = check_case(ctx, X, labels, 6, store)
    wi = mk.wilcoxon_info()
    entry = 2 * ((4 if store == 1 else 8) + 2)
    assert wi["n_chunks"] == 1 and wi["scratch_bytes"] == X.nnz * entry
    small = X.nnz * entry // 6
    mk2 = wilcoxon(dev, labels, 6, scratch=small)
    w2 = mk2.wilcoxon_info()
    assert w2["n_chunks"] >= 5 and w2["scratch_bytes"] <= small                      # 300 genes in one tile: every chunk ends inside it
    same_tables(tables_of(mk2), base)
    mk2.free()
    # a cap below the longest gene is raised to fit it, and reported
    longest = int(np.diff(X.tocsc().indptr).max())
    mk3 = wilcoxon(dev, labels, 6, scratch=1)
    w3 = mk3.wilcoxon_info()
    assert w3["scratch_bytes"] == longest * entry and 150 <= w3["n_chunks"] <= 300
    same_tables(tables_of(mk3), base)
    for h in (mk, mk3):
        h.free()


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("shape", ["500x10001", "200x66000"])
def test_chunks_and_gene_tiles(ctx, shape, store):
    """Two gene tiles of 5001 genes (G no multiple of the tile) with chunks that span the tile edge and end inside a tile; and 32-bit
    column indices (more than 65536 genes, seven tiles)."""
    if shape == "500x10001":
        X = lognorm_matrix(44, 500, 10001, 0.01)
    else:
        X = lognorm_matrix(45, 200, 66000, 0.002)
    labels = np.random.default_rng(46).integers(0, 4, X.shape[0])
    dev, mk, base = check_case(ctx, X, labels, 4, store)
    entry = 2 * ((4 if store == 1 else 8) + 2)
    mk2 = wilcoxon(dev, labels, 4, scratch=X.nnz * entry * 2 // 7)
    assert 4 <= mk2.wilcoxon_info()["n_chunks"] <= 5
    same_tables(tables_of(mk2), base)
    for h in (mk, mk2):
        h.free()


# ---- order freedom and repeatability ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_order_freedom_and_repeatability(ctx, store):
    L = segment_limit(ctx) or 4096
    N = L + 700                                                                     # gene 0 is stored in every row: the radix route too
    X = sp.hstack([sp.csr_matrix(np.random.default_rng(47).choice([0.5, 1.0, 1.5, 2.0], (N, 1))), lognorm_matrix(48, N, 120, 0.2)]).tocsr()
    X.sort_indices()
    labels = np.random.default_rng(49).integers(0, 7, N)
    dev, mk, base = check_case(ctx, X, labels, 7, store)
    assert mk.wilcoxon_info()["segments_long"] == 1
    again = wilcoxon(dev, labels, 7)                                                # the same call again
    same_tables(tables_of(again), base)
    for h in (mk, again):
        h.free()
    for perm in (np.arange(N)[::-1], np.random.default_rng(50).permutation(N)):
        Xp = X[perm]
        Xp.sort_indices()
        devp = upload(ctx, Xp, store)
        mkp = wilcoxon(devp, labels[perm], 7)
        same_tables(tables_of(mkp), base)
        mkp.free()
        devp.free()


# ---- groups ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_group_edges(ctx, store):
    X = lognorm_matrix(51, 900, 70, 0.15)
    N = X.shape[0]
    rng = np.random.default_rng(52)
    _, mk, T = check_case(ctx, X, np.zeros(N, np.uint32), 1, store)                 # one group: no rest
    assert mk.info()["groups_degenerate"] == 1 and not T["score"].any()
    mk.free()
    labels = rng.choice([0, 2, 3], N)                                               # group 1 is empty
    _, mk, T = check_case(ctx, X, labels, 4, store)
    assert mk.info()["groups_degenerate"] == 1 and not T["ranksum2"][1].any() and not T["score"][1].any()
    mk.free()
    labels = np.zeros(N, np.uint32)                                                 # a group of N - 1 against one cell
    labels[rng.integers(N)] = 1
    _, mk, T = check_case(ctx, X, labels, 2, store)
    assert mk.info()["groups_degenerate"] == 0 and same_bits(T["score"][0], -T["score"][1] + 0.0)
    mk.free()


@pytest.mark.parametrize("store", STORES)
def test_4096_groups(ctx, store):
    X = lognorm_matrix(53, 5000, 60, 0.2)
    labels = np.random.default_rng(54).permutation(np.arange(5000) % 4096)
    check_case(ctx, X, labels, 4096, store)[1].free()


# ---- the resident route ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_resident_route(ctx, store):
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing.markers import Markers
    lib = F.lib()
    z = np.load(os.path.join(GOLD, "planted_600x240.npz"))
    n, g = int(z["n_rows"]), int(z["n_cols"])
    X = sp.csr_matrix((z["values"], z["indices"].astype(np.int64), z["indptr"].astype(np.int64)), shape=(n, g))
    dev = upload(ctx, X, store)
    popts, res = F.PcaOpts(20, -1, -1, -1, 0, 0, 0, 0.0, 11), F.PipelineResult()
    F.check(lib.srx_pipeline(dev.handle, 1e4, 120, C.byref(popts), C.byref(res)), ctx.handle)
    gh, mk_h = C.c_void_p(), C.c_void_p()
    F.check(lib.srx_neighbors_result(dev.handle, C.byref(F.KnnOpts(15, 0, 0, 0)), None, C.byref(gh)), ctx.handle)
    wopts = F.WilcoxonOpts(0, -1, 1, 0, 0)
    assert lib.srx_rank_genes_wilcoxon_graph(dev.handle, gh, C.byref(wopts), C.byref(mk_h)) == F.E_ARG and not mk_h.value   # no labels yet
    assert b"srx_louvain" in lib.srx_last_error(ctx.handle)
    F.check(lib.srx_louvain(gh, None, None, None), ctx.handle)
    before = dev.values(np.float64)
    F.check(lib.srx_rank_genes_wilcoxon_graph(dev.handle, gh, C.byref(wopts), C.byref(mk_h)), ctx.handle)
    resident = Markers(ctx, mk_h)
    assert same_bits(before, dev.values(np.float64))                                # m is as it was
    labels = np.zeros(n, np.uint32)
    F.check(lib.srx_graph_labels_fetch(gh, F.ptr(labels)), ctx.handle)
    k = int(labels.max()) + 1
    assert resident.info()["n_groups"] == k and k >= 2
    host = wilcoxon(dev, labels, k)
    same_tables(tables_of(resident), tables_of(host))
    assert {k_: v for k_, v in resident.info().items() if k_ != "ms"} == {k_: v for k_, v in host.info().items() if k_ != "ms"}
    # and both are the definition on the log-normalised values the device holds
    Y = sp.csr_matrix((before, X.indices, X.indptr), shape=X.shape)
    want = ref.reference(Y, labels, k, 2, True)                                     # (the values read back ARE the stored precision)
    assert np.array_equal(resident.table("ranksum2"), want["ranksum2"]) and np.array_equal(resident.ties(), want["ties"])
    assert same_bits(resident.table("score"), want["score"])
    other = upload(ctx, X[:500], store)
    h2 = C.c_void_p()
    assert lib.srx_rank_genes_wilcoxon_graph(other.handle, gh, C.byref(wopts), C.byref(h2)) == F.E_ARG and not h2.value
    assert b"rows" in lib.srx_last_error(ctx.handle)
    resident.free()
    host.free()
    lib.srx_graph_free(gh)


# ---- the known answer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_known_answer(ctx, store):
    kat = json.load(open(os.path.join(GOLD, "kat_wilcoxon.json")))
    X = sp.csr_matrix((np.array(kat["data"], np.float64), kat["indices"], kat["indptr"]), shape=(kat["n_rows"], kat["n_cols"]))
    dev = upload(ctx, X, store)
    for tie_correct, key in ((0, "score"), (1, "score_tie_correct")):
        mk = wilcoxon(dev, kat["labels"], kat["n_groups"], n_top=4, logged=0, tie_correct=tie_correct)
        assert np.array_equal(mk.sizes(), kat["n_cells"]) and np.array_equal(mk.table("ranksum2"), np.array(kat["ranksum2"], np.uint64))
        if tie_correct:
            assert np.array_equal(mk.ties(), np.array(kat["ties"], np.uint64))
        # the rational's square root against num / sqrt(d) with d from up to four rounded operations: a few ulp
        assert np.allclose(mk.table("score"), kat[key], rtol=1e-15, atol=0)
        assert np.array_equal(mk.top()[0], kat[key.replace("score", "ranked")]) and mk.info()["groups_degenerate"] == 0
        mk.free()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    lib = F.lib()
    X = lognorm_matrix(60, 50, 30, 0.2)
    dev = upload(ctx, X, 2)
    labels = np.random.default_rng(1).integers(0, 3, 50).astype(np.uint32)

    def refused(code, word, d=None, lab=labels, k=3, opts=None):
        d = d or dev
        h = C.c_void_p()
        rc = lib.srx_rank_genes_wilcoxon(d.handle, F.ptr(lab), k, None if opts is None else C.byref(opts), C.byref(h))
        msg = lib.srx_last_error(ctx.handle)
        assert rc == code and msg and word in msg.decode() and not h.value, (rc, msg)

    Y = X.copy()
    Y.data[5] = np.nan
    refused(F.E_NAN, "NaN", d=upload(ctx, Y, 2))
    bad = labels.copy()
    bad[17] = 3
    refused(F.E_ARG, "label", lab=bad)
    refused(F.E_ARG, "CSC", d=sr.DeviceCsr.upload(ctx, 50, 30, X.tocsc().indptr, X.tocsc().indices, X.tocsc().data, 2, csc=True))
    refused(F.E_ARG, "n_top", opts=F.WilcoxonOpts(31, -1, 0, 0, 0))
    # tie_correct with 2^21 + 1 rows (an all-empty matrix): N^3 - N would not fit; without the tie term the same matrix is served
    n_big = (1 << 21) + 1
    empty = sr.DeviceCsr.upload(ctx, n_big, 3, np.zeros(n_big + 1, np.int64), np.zeros(0, np.int64), np.zeros(0), 2)
    lab_big = np.zeros(n_big, np.uint32)
    lab_big[::2] = 1
    refused(F.E_ARG, "tie_correct", d=empty, lab=lab_big, k=2, opts=F.WilcoxonOpts(0, -1, 1, 0, 0))
    mk = wilcoxon(empty, lab_big, 2, tie_correct=0)
    n1 = int(lab_big.sum())
    assert np.array_equal(mk.table("ranksum2"), np.array([[(n_big - n1) * (n_big + 1)] * 3, [n1 * (n_big + 1)] * 3], np.uint64))
    assert not mk.table("score").any()
    # what belongs to one route is refused on the other's handle
    assert lib.srx_markers_fetch_ties(mk.handle, F.ptr(np.zeros(3, np.uint64))) == F.E_ARG and b"tie_correct" in lib.srx_last_error(ctx.handle)
    tt = ttest(dev, labels, 3)
    out = np.zeros((3, 30), np.uint64)
    assert lib.srx_markers_fetch_table(tt.handle, F.MARKERS_RANKSUM2, F.ptr(out)) == F.E_ARG and b"wilcoxon" in lib.srx_last_error(ctx.handle)
    wi = F.WilcoxonInfo()
    assert lib.srx_markers_wilcoxon_info_get(tt.handle, C.byref(wi)) == F.E_ARG and b"t-test" in lib.srx_last_error(ctx.handle)
    assert lib.srx_markers_fetch_ties(tt.handle, F.ptr(np.zeros(30, np.uint64))) == F.E_ARG
    for h in (mk, tt):
        h.free()
    empty.free()
    # the context is still usable
    check_case(ctx, X, labels, 3, 2)[1].free()


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_python_layer(ctx):
    import singlerust_amd as sr
    from singlerust_amd.memory.processing import dim_red, louvain, neighbors, rank_genes_groups
    from test_knn_gpu import _planted, _upload
    a = _upload(ctx, _planted())
    dim_red.pca_inplace(a, 20, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    neighbors(a, n_neighbors=15, connectivities=True)
    louvain(a)
    rank_genes_groups(a, n_genes=25)                                                 # the default call: as before
    t = a.uns["rank_genes_groups"]
    assert t["params"]["method"] == "t-test" and t["params"]["tie_correct"] is False
    welch = a._markers.table("score")
    with pytest.raises(sr.SrxError):
        a._markers.wilcoxon_info()
    info = rank_genes_groups(a, n_genes=25, method="wilcoxon", key_added="wx")
    u = a.uns["wx"]
    k = int(a.obs["louvain"].max()) + 1
    assert set(u) == set(t) == {"names", "scores", "logfoldchanges", "pts", "pts_rest", "params", "info"}
    assert set(u["params"]) == set(t["params"]) and u["params"]["method"] == "wilcoxon" and u["params"]["tie_correct"] is False
    assert u["params"]["resident_labels"] and u["info"] == info and info["n_groups"] == k
    assert u["names"].shape == u["scores"].shape == u["logfoldchanges"].shape == (k, 25)
    assert same_bits(u["pts"], t["pts"]) and same_bits(u["pts_rest"], t["pts_rest"])
    assert np.all(np.diff(u["scores"], axis=1) <= 0) and not same_bits(a._markers.table("score"), welch)
    assert a._markers.wilcoxon_info()["tie_correct"] == 0 and a._markers.table("ranksum2").dtype == np.uint64
    with pytest.raises(sr.SrxError):
        a._markers.ties()
    # host labels under another key, tie-corrected: the same rank sums, scores at least as large in magnitude
    a.obs["copy"] = a.obs["louvain"].astype(np.int64)
    r2 = a._markers.table("ranksum2")
    z0 = a._markers.table("score")
    rank_genes_groups(a, groupby="copy", n_genes=25, key_added="again", method="wilcoxon", tie_correct=True)
    v = a.uns["again"]
    assert not v["params"]["resident_labels"] and v["params"]["tie_correct"] is True
    assert np.array_equal(a._markers.table("ranksum2"), r2) and a._markers.ties().shape == (a.n_vars(),)
    assert np.all(np.abs(a._markers.table("score")) >= np.abs(z0))
    with pytest.raises(sr.SrxError):
        rank_genes_groups(a, method="logreg")

"""Sums over gene lists and gene-set scores on the device (srx_gene_list_sums, srx_score_genes) through the C ABI, against the
Python-int restatement of the definition (score_genes_ref.py).

  sums, counts   bit for bit the reference's, at f32 and f64 storage; exact integer sums for integer counts
  log1p values   with one stored outlier of 1000, so that the quantum (2^-44) lies far above the ulp of the log1p values and
                 every term is rounded.  The definition's bound is asserted twice.  On the INTEGERS (the reference's Python ints,
                 which the device equals bit for bit): |S_int 2^-s - exact| <= c 2^-(s + 1), exact being a sum of Fractions.  On
                 the f64 the device returns, against a long-double sum: c 2^-(s + 1) + ulp(SUM) / 2 + c 2^-64 |sum| — f64(S_int)
                 rounds an integer of up to 62 bits to 53, and the long-double sum has its own error.  Measured at f64 storage:
                 the integers at 0.680 of the bound, the f64 at 0.677 of its bound and 0.7 of the bare c 2^-(s + 1); f32 storage
                 is exact at this scale (24-bit values).  Without the outlier (scale 2^52) no term is rounded at all and the f64
                 stands 1.6 bare bounds from the long-double sum: that is the half ulp of f64(S_int), not the fixed point.
  scores         bit for bit the reference's; within (c_set / |set| + c_ctrl / |ctrl|) 2^-(s + 1) + 4 ulp of the larger mean of
                 the long-double X[:, set].mean(1) - X[:, ctrl].mean(1) on the dense matrix with the library's control lists
Every case prints what it measured before it asserts."""
import ctypes as C
import functools
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import score_genes_ref as S

pytestmark = pytest.mark.gpu
STORES = [np.float32, np.float64]
KAT = json.load(open(os.path.join(S.GOLD, "kat_score_genes.json")))


def F():
    from singlerust_amd import _ffi
    return _ffi


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def pack(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    flat = np.concatenate([np.asarray(l, dtype=np.uint64) for l in lists] + [np.zeros(1, dtype=np.uint64)])
    return ptr, np.ascontiguousarray(flat)


def dev_sums(m, lists, want_sum=True, want_cnt=True):
    """(rc, sum, cnt, info): outputs pre-filled with a mark"""
    f = F()
    n = int(m.info().n_rows)
    ptr, flat = pack(lists)
    s, c, info = np.full((n, len(lists)), -7.0), np.full((n, len(lists)), 77, dtype=np.uint32), f.GeneListInfo()
    rc = f.lib().srx_gene_list_sums(m.handle, f.ptr(ptr), f.ptr(flat), len(lists), f.ptr(s) if want_sum else None, f.ptr(c) if want_cnt else None,
                                    C.byref(info))
    return rc, s, c, info


def dev_score(m, sets, pool=None, ctrl_size=0, n_bins=0, seed=0, as_ref=-1, capacity=None, controls=True):
    f = F()
    n, G = int(m.info().n_rows), int(m.info().n_cols)
    ptr, flat = pack(sets)
    pool_a = None if pool is None else np.ascontiguousarray(pool, dtype=np.uint64)
    cap = G * len(sets) + 8 if capacity is None else capacity
    score, cptr, cg, info = np.full((n, len(sets)), -7.0), np.full(len(sets) + 1, 77, dtype=np.uint64), np.full(cap, 77, dtype=np.uint64), f.ScoreGenesInfo()
    o = f.ScoreGenesOpts(ctrl_size, n_bins, seed, as_ref, 0)
    rc = f.lib().srx_score_genes(m.handle, f.ptr(ptr), f.ptr(flat), len(sets), None if pool_a is None else f.ptr(pool_a),
                                 0 if pool_a is None else pool_a.size, C.byref(o), f.ptr(score), f.ptr(cptr) if controls else None,
                                 f.ptr(cg) if controls else None, cap, C.byref(info))
    if rc != 0:
        assert np.all(score == -7.0) and np.all(cptr == 77) and np.all(cg == 77), "a refused call wrote to its outputs"
        return rc, None, None, info
    ctrl = [cg[int(cptr[s]):int(cptr[s + 1])].copy() for s in range(len(sets))] if controls else None
    return rc, score, ctrl, info


def gene_means(m):
    f = F()
    n, G = int(m.info().n_rows), int(m.info().n_cols)
    s = np.zeros(G)
    f.check(f.lib().srx_compute_sum(m.handle, f.COLUMN, f.ptr(s)), m.ctx.handle)
    return s / float(n)


def hashed_lists(G, n_lists, seed, in_all=None, in_none=None):
    """list t holds the genes the hash keeps (about a quarter), never `in_none`, always `in_all`; no list is empty"""
    out = []
    for t in range(n_lists):
        l = [j for j in range(G) if j != in_none and (j == in_all or S.mix64(seed * 65537 + t * 4099 + j) % 4 == 0)]
        out.append(l or [(t * 7) % G if (t * 7) % G != in_none else (in_none + 1) % G])
    return out


def check_against_reference(ctx, csr, lists, integer=False):
    m = csr.upload(ctx)
    rc, s, c, info = dev_sums(m, lists)
    assert rc == 0, F().lib().srx_last_error(ctx.handle)
    want_s, want_c, scale, Sint = S.list_sums(csr, lists)
    print("n=%d G=%d lists=%d nnz=%d: scale 2^%d, walks %d, max_abs %g" % (csr.n, csr.G, len(lists), csr.values.size, info.sum_scale_log2,
                                                                         info.n_walks, info.max_abs))
    assert info.sum_scale_log2 == scale and info.n_walks == (len(lists) + 63) // 64 and info.longest_list == max(len(l) for l in lists)
    assert (info.n_rows, info.n_cols, info.n_lists) == (csr.n, csr.G, len(lists))
    assert np.array_equal(c, want_c)
    assert same_bits(s, want_s)
    if integer:
        X = csr.dense()
        exact = np.stack([X[:, np.asarray(l, dtype=np.int64)].sum(axis=1) for l in lists], axis=1)
        assert scale >= 0 and np.array_equal(s, exact)
    # each output alone is the same
    assert same_bits(dev_sums(m, lists, want_cnt=False)[1], want_s) and np.array_equal(dev_sums(m, lists, want_sum=False)[2], want_c)
    m.free()
    return s, c, scale, Sint


# ---- sums and counts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("G,n_lists", [(1, 1), (63, 63), (64, 64), (65, 65), (130, 129)])
def test_sums_and_counts_at_every_width(ctx, store, G, n_lists):
    """9 rows (two workgroups of four waves and one more row), row 3 empty; list 0 holds every gene, list 1 one gene; from 64 lists
    on gene 2 is in all 64 lists of the first walk and list 1 holds it alone; at G = 130 gene 5 is in no list (list 0 gives way to a hashed one)."""
    X = S.hashed_counts(9, G, seed=G)
    X[3] = 0
    X[0, 0] = 3
    in_none = 5 if G == 130 else None
    lists = hashed_lists(G, n_lists, 7, in_all=2 if n_lists >= 64 else None, in_none=in_none)
    if in_none is None:
        lists[0] = list(range(G))
    if n_lists > 1:
        lists[1] = [2] if n_lists >= 64 else [G - 1]
    s, c, _, _ = check_against_reference(ctx, S.Csr.from_dense(X, store), lists, integer=True)
    if in_none is not None:
        assert all(in_none not in l for l in lists) and X[:, in_none].any()
    if n_lists >= 64:
        assert all(2 in l for l in lists[:64]) and X[:, 2].any()
        assert np.all(c[:, :64] >= (X[:, 2] != 0)[:, None]) and np.array_equal(s[:, 1], X[:, 2])


@pytest.mark.parametrize("store", STORES)
def test_row_lengths_and_one_cell(ctx, store):
    """rows of 0, 1, 63, 64, 65 and 257 entries at G = 300; then N = 1"""
    G, rows = 300, []
    for i, length in enumerate((0, 1, 63, 64, 65, 257)):
        genes = sorted(range(G), key=lambda j: S.mix64(i * 1009 + j))[:length]
        rows.append([(j, float(1 + S.mix64(i + 31 * j) % 5)) for j in genes])
    lists = hashed_lists(G, 3, 11) + [list(range(0, G, 2))]
    check_against_reference(ctx, S.Csr.from_rows(G, rows, store), lists, integer=True)
    check_against_reference(ctx, S.Csr.from_rows(G, rows[5:], store), lists, integer=True)


@pytest.mark.parametrize("store", STORES)
def test_a_row_of_5000_entries(ctx, store):
    G = 6000
    genes = sorted(range(G), key=lambda j: S.mix64(77 + j))[:5000]
    rows = [[(j, float(1 + j % 3)) for j in genes], [(17, 2.0)], []]
    lists = [list(range(0, G, 40)), [17, 4000], list(range(5900, 6000))]
    check_against_reference(ctx, S.Csr.from_rows(G, rows, store), lists, integer=True)


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("G", [65537, 600000])
def test_32_bit_indices_above_65536_genes(ctx, store, G):
    """no 16-bit mirror above 65536 columns; 5 rows, ~300 entries, genes 65535 and 65536 stored and listed.  At 600000 genes the
    bitmap (75 000 bytes) is read from global memory instead of LDS."""
    rows = []
    for i in range(5):
        genes = sorted({S.mix64(i * 131 + t) % G for t in range(60)} | ({65536, 65535} if i % 2 == 0 else {0}))
        rows.append([(j, float(1 + (i + j) % 7)) for j in genes])
    every = sorted({j for r in rows for j, _ in r})
    lists = [[65536], every[::2], [65535, 65536, 0], every]
    m = S.Csr.from_rows(G, rows, store).upload(ctx)
    assert int(m.info().n_cols) == G
    m.free()
    check_against_reference(ctx, S.Csr.from_rows(G, rows, store), lists, integer=True)


@pytest.mark.parametrize("store", STORES)
def test_stored_zero_and_negative_values_count(ctx, store):
    rows = [[(g, float(v)) for g, v in r] for r in KAT["rows"]]
    s, c, _, _ = check_against_reference(ctx, S.Csr.from_rows(KAT["n_genes"], rows, store), [[1], [1, 2], list(range(8))])
    assert c[:, 0].tolist() == [1, 1, 1, 0, 0, 0] and s[:, 0].tolist() == [1.0, -1.0, 0.0, 0.0, 0.0, 0.0]      # cell 2 stores a 0: counted


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("top,e", [(4.0, 3), ("below 4", 2), (0.25, -1), (2.0 ** -40, -30)])
def test_scale_at_the_edge_of_a_power_of_two(ctx, store, top, e):
    """max_abs = 2^k belongs to e = k + 1; the storage's last value below it to e = k; the floor of e is -30"""
    top = float(np.nextafter(store(4.0), store(0.0))) if top == "below 4" else float(top)
    assert float(store(top)) == top
    rows = [[(0, top), (1, top / 2), (2, -top / 4)], [(1, -top)], [(0, top / 8), (2, top / 8)]]
    lists = [[0, 1, 2], [1]]
    csr = S.Csr.from_rows(3, rows, store)
    m = csr.upload(ctx)
    rc, s, c, info = dev_sums(m, lists)
    m.free()
    assert rc == 0 and info.max_abs == top and info.sum_scale_log2 == 62 - e - 2
    want = S.list_sums(csr, lists)
    assert same_bits(s, want[0]) and np.array_equal(c, want[1])
    # top 2^scale is an integer at every one of these scales: S_int is exact, SUM its correctly rounded f64
    assert s[0, 0] == float(Fraction(top) + Fraction(top / 2) - Fraction(top / 4))


@pytest.mark.parametrize("store", STORES)
def test_log1p_sums_stay_within_the_fixed_point_bound(ctx, store):
    csr = S.planted("values")
    v = np.log1p(csr.values)                                    # full f64 mantissas at f64 storage
    v[0] = 1000.0                                               # one stored outlier: the quantum 2^-44 lies far above the ulp of the rest
    csr = S.Csr(csr.n, csr.G, csr.indptr, csr.indices, v.astype(store))
    lists = [list(range(csr.G)), list(range(0, 240, 3)), [7], list(range(100, 145)), list(range(150, 205))]
    s, c, scale, Sint = check_against_reference(ctx, csr, lists)
    ip, vals = csr.indptr.astype(np.int64), csr.values.astype(np.float64)
    member = [set(l) for l in lists]
    worst_int = worst_f64 = worst_bare = 0.0
    ld_eps = float(np.finfo(np.longdouble).eps)
    for i in range(0, csr.n, 7):                                # every seventh cell: the exact sums are Fractions
        for t, mem in enumerate(member):
            terms = [float(vals[p]) for p in range(ip[i], ip[i + 1]) if int(csr.indices[p]) in mem]
            exact = sum((Fraction(v) for v in terms), Fraction(0))
            bound = Fraction(len(terms), 2 ** (scale + 1))
            assert len(terms) == c[i, t]
            err_int = abs(Fraction(Sint[i][t], 2 ** scale) - exact)
            assert err_int <= bound
            ld = np.sum(np.asarray(terms, dtype=np.longdouble)) if terms else np.longdouble(0)
            err = abs(float(np.longdouble(s[i, t]) - ld))
            allowed = float(bound) + float(np.spacing(s[i, t])) / 2 + len(terms) * ld_eps * abs(float(ld))
            if terms:
                worst_int = max(worst_int, float(err_int / bound))
                worst_f64 = max(worst_f64, err / allowed)
                worst_bare = max(worst_bare, err / float(bound))
            assert err <= allowed
    print("log1p sums, scale 2^%d: integers at %.3f of c 2^-(s+1); f64 at %.3f of that bound + ulp / 2 (%.1f of the bare bound)"
          % (scale, worst_int, worst_f64, worst_bare))


# ---- scores --------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def score_case(name, store):
    """(csr, sets, kwargs) of the score cases, built once"""
    if name == "planted":
        p = S.planted()
        return S.Csr(p.n, p.G, p.indptr, p.indices, p.values.astype(store)), ((3, 40, 41, 100, 239), tuple(range(60, 90)), (7,)), dict(ctrl_size=6, n_bins=9, seed=4)
    G = {"g65": 65, "g130": 130}[name]
    X = np.log1p(S.hashed_counts(9, G, seed=G + 1, density=0.6))
    return S.Csr.from_dense(X, store), ((0, 5, 9), (G - 1, 1)), dict(ctrl_size=3, n_bins=5, seed=2)


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("name", ["g65", "g130", "planted"])
@pytest.mark.parametrize("as_ref", [1, 0])
def test_scores_equal_the_reference_and_the_dense_means(ctx, name, store, as_ref):
    csr, sets, kw = score_case(name, store)
    sets = [list(s) for s in sets]
    m = csr.upload(ctx)
    mean = gene_means(m)
    rc, score, ctrl, info = dev_score(m, sets, as_ref=as_ref, **kw)
    assert rc == 0, F().lib().srx_last_error(ctx.handle)
    rc2, again, ctrl2, _ = dev_score(m, sets, as_ref=as_ref, **kw)
    m.free()
    want, want_ctrl, scale = S.score(csr, mean, sets, None, kw["ctrl_size"], kw["n_bins"], kw["seed"], bool(as_ref))
    assert all(np.array_equal(a, b) for a, b in zip(ctrl, want_ctrl)) and info.sum_scale_log2 == scale
    assert same_bits(score, want)
    assert same_bits(score, again) and all(np.array_equal(a, b) for a, b in zip(ctrl, ctrl2))         # two calls
    assert info.n_sets == len(sets) and info.n_walks == 1 and info.n_ctrl_total == sum(len(c) for c in ctrl)
    assert info.n_items == S.n_items_of(csr.G, kw["n_bins"]) and info.n_pool == csr.G
    # the dense means in long double, with the library's control lists
    X = csr.dense().astype(np.longdouble)
    worst = 0.0
    for s, (genes, cg) in enumerate(zip(sets, ctrl)):
        a, b = X[:, genes].mean(axis=1), X[:, cg.astype(np.int64)].mean(axis=1)
        c_set, c_ctrl = (csr.dense()[:, genes] != 0).sum(axis=1), (csr.dense()[:, cg.astype(np.int64)] != 0).sum(axis=1)
        bound = (c_set / len(genes) + c_ctrl / len(cg)) * 2.0 ** -(scale + 1) + 4 * np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float64))
        err = np.abs((score[:, s].astype(np.longdouble) - (a - b)).astype(np.float64))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound)
    print("%s %s ctrl_as_ref=%d: scale 2^%d, %d controls, score at %.3f of its bound" % (name, np.dtype(store).name, as_ref, scale,
                                                                                        info.n_ctrl_total, worst))


@pytest.mark.parametrize("store", STORES)
def test_score_known_answer(ctx, store):
    csr = S.Csr.from_rows(KAT["n_genes"], [[(g, float(v)) for g, v in r] for r in KAT["rows"]], store)
    m = csr.upload(ctx)
    assert gene_means(m).tolist() == [float(v) for v in KAT["means"]]
    rc, score, ctrl, info = dev_score(m, [KAT["sets"]["a"], KAT["sets"]["b"]], ctrl_size=KAT["ctrl_size"], n_bins=KAT["n_bins"])
    m.free()
    assert rc == 0 and [c.tolist() for c in ctrl] == [KAT["controls"]["a"], KAT["controls"]["b"]]
    assert score[:, 0].tolist() == [float(v) for v in KAT["scores"]["a"]] and score[:, 1].tolist() == [float(v) for v in KAT["scores"]["b"]]
    assert info.n_items == KAT["n_items"] and info.max_abs == 16.0


def test_sets_scored_together_equal_sets_scored_alone_and_in_two_walks(ctx):
    """33 sets (two walks: 66 lists) against the same sets in two calls (17 + 16) and against each alone.  The scale belongs to the
    call (its longest list): every set has 16 genes and, with one control per bin and nine bins, at most 9 controls, so every call
    here has L = 4 — asserted as the condition of the comparison."""
    p = S.planted()
    m = p.upload(ctx)
    sets = [[(7 * s + 3 * t) % p.G for t in range(16)] for s in range(33)]
    assert all(len(set(s)) == 16 for s in sets)
    kw = dict(ctrl_size=1, n_bins=9, seed=1)
    rc, whole, ctrl, info = dev_score(m, sets, **kw)
    assert rc == 0 and info.n_walks == 2 and info.n_sets == 33 and info.longest_list == 16
    parts = [dev_score(m, sets[:17], **kw), dev_score(m, sets[17:], **kw)]
    assert all(q[0] == 0 and q[3].n_walks == 1 and q[3].sum_scale_log2 == info.sum_scale_log2 for q in parts)
    assert same_bits(whole, np.concatenate([parts[0][1], parts[1][1]], axis=1))
    assert all(np.array_equal(a, b) for a, b in zip(ctrl, parts[0][2] + parts[1][2]))
    for s in (0, 16, 17, 32):
        rc, alone, c1, i1 = dev_score(m, [sets[s]], **kw)
        assert rc == 0 and np.array_equal(c1[0], ctrl[s]) and i1.sum_scale_log2 == info.sum_scale_log2
        assert same_bits(alone[:, 0], whole[:, s])
    assert dev_score(m, [sets[0]], controls=False, **kw)[0] == 0         # the control outputs may be NULL
    m.free()


# ---- the handle --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", [1, 2])
def test_the_handle_is_left_as_it_was(ctx, store):
    import singlerust_amd as sr
    f = F()
    lib = f.lib()
    z = np.load(os.path.join(S.GOLD, "planted_600x240.npz"))
    n, g = int(z["n_rows"]), int(z["n_cols"])
    dev = sr.DeviceCsr.upload(ctx, n, g, z["indptr"], z["indices"], z["values"], store=store)
    popts, res = f.PcaOpts(20, -1, -1, -1, 0, 0, 0, 0.0, 11), f.PipelineResult()
    f.check(lib.srx_pipeline(dev.handle, 1e4, 120, C.byref(popts), C.byref(res)), ctx.handle)

    def state():
        scores = np.zeros((n, 20))
        f.check(lib.srx_result_fetch(dev.handle, f.ptr(scores), None, None, None, None, None), ctx.handle)
        cnt, s, q = np.zeros(g, np.uint64), np.zeros(g), np.zeros(g)
        f.check(lib.srx_gene_moments(dev.handle, f.ptr(cnt), f.ptr(s), f.ptr(q)), ctx.handle)
        i = dev.info()
        return dev.values(np.float64), scores, cnt, s, q, np.array([i.dtype, i.store, i.nnz])

    before = state()
    assert dev_sums(dev, [[1, 2, 3], list(range(100))])[0] == 0
    assert dev_score(dev, [[1, 2, 3], [50, 60]], ctrl_size=5, n_bins=9)[0] == 0
    after = state()
    assert all(same_bits(a, b) for a, b in zip(before, after))
    dev.free()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_with_nothing_written(ctx):
    import singlerust_amd as sr
    f = F()
    lib = f.lib()
    X = S.hashed_counts(6, 40, seed=5)
    csr = S.Csr.from_dense(X, np.float64)
    m = csr.upload(ctx)

    def sums_refused(mm, lists, text, code=None, cx=ctx, n_lists=None, ptr=None):
        n = int(mm.info().n_rows)
        p, flat = pack(lists)
        p = p if ptr is None else np.asarray(ptr, dtype=np.uint64)
        k = len(lists) if n_lists is None else n_lists
        s, c, info = np.full((n, max(len(lists), 1)), -7.0), np.full((n, max(len(lists), 1)), 77, dtype=np.uint32), f.GeneListInfo()
        info.max_abs = -7.0
        rc = lib.srx_gene_list_sums(mm.handle, f.ptr(p), f.ptr(flat), k, f.ptr(s), f.ptr(c), C.byref(info))
        msg = lib.srx_last_error(cx.handle).decode()
        assert rc == (f.E_ARG if code is None else code) and text in msg, (text, rc, msg)
        assert np.all(s == -7.0) and np.all(c == 77) and info.max_abs == -7.0

    good = [[1, 2], [3]]
    p, flat = pack(good)
    out = np.full((6, 2), -7.0)
    # (1) NULL arrays, no output
    assert lib.srx_gene_list_sums(m.handle, None, f.ptr(flat), 2, f.ptr(out), None, None) == f.E_ARG and b"null" in lib.srx_last_error(ctx.handle)
    assert lib.srx_gene_list_sums(m.handle, f.ptr(p), None, 2, f.ptr(out), None, None) == f.E_ARG and b"null" in lib.srx_last_error(ctx.handle)
    assert lib.srx_gene_list_sums(m.handle, f.ptr(p), f.ptr(flat), 2, None, None, None) == f.E_ARG and b"no output" in lib.srx_last_error(ctx.handle)
    assert np.all(out == -7.0)
    # (2) n_lists, before everything about the lists
    sums_refused(m, good, "n_lists = 0", n_lists=0)
    sums_refused(m, good, "n_lists = 4097", n_lists=4097)
    # (3) CSC, (4) ranks, (5) a backed session: before the lists are looked at (a bad list goes with each)
    bad = [[1, 1]]
    mc = m.to_csc()
    sums_refused(mc, bad, "CSC")
    assert dev_score(mc, [[1, 2]])[0] == f.E_ARG and b"CSC" in lib.srx_last_error(ctx.handle)
    mc.free()
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    m2 = csr.upload(c2)
    sums_refused(m2, bad, "rank", cx=c2)
    assert dev_score(m2, [[1, 2]])[0] == f.E_ARG and b"rank" in lib.srx_last_error(c2.handle)
    m2.free()
    c2.close()
    c3 = sr.Context(0)
    m3 = csr.upload(c3)
    b = C.c_void_p()
    f.check(lib.srx_backed_create(c3.handle, 40, f.STORE_F32, C.byref(b)), c3.handle)
    sums_refused(m3, bad, "backed", cx=c3)
    assert dev_score(m3, [[1, 2]])[0] == f.E_ARG and b"backed" in lib.srx_last_error(c3.handle)
    lib.srx_backed_destroy(b)
    m3.free()
    c3.close()
    # (7) - (10) the lists
    sums_refused(m, good, "list_ptr[0] = 1", ptr=[1, 2, 3])
    sums_refused(m, good, "list_ptr decreases at list 1", ptr=[0, 2, 1])
    sums_refused(m, [[1], [], [2]], "list 1 is empty")
    sums_refused(m, [[1], [2, 40]], "gene index 40 of list 1 is not below 40")
    sums_refused(m, [[1], [2, 5, 2]], "gene 2 is repeated in list 1")
    # SRX_E_NAN, after the lists
    for badv in (np.nan, np.inf, -np.inf):
        v = csr.values.copy()
        v[3] = badv
        mn = S.Csr(csr.n, csr.G, csr.indptr, csr.indices, v).upload(ctx)
        sums_refused(mn, good, "NaN or Inf", code=f.E_NAN)
        sums_refused(mn, bad, "repeated")
        assert dev_score(mn, [[1, 2]])[0] == f.E_NAN and b"NaN or Inf" in lib.srx_last_error(ctx.handle)
        mn.free()
    # the score: its own (1) and (2), then the controls' refusals through it, SRX_E_NAN before them
    sp, sg = pack([[1, 2]])
    sc = np.full((6, 1), -7.0)
    assert lib.srx_score_genes(m.handle, f.ptr(sp), f.ptr(sg), 1, None, 0, None, None, None, None, 0, None) == f.E_ARG
    assert b"null array" in lib.srx_last_error(ctx.handle)
    assert lib.srx_score_genes(m.handle, f.ptr(sp), f.ptr(sg), 1, None, 0, None, f.ptr(sc), f.ptr(sp), None, 0, None) == f.E_ARG
    assert lib.srx_score_genes(m.handle, f.ptr(sp), f.ptr(sg), 0, None, 0, None, f.ptr(sc), None, None, 0, None) == f.E_ARG
    assert b"n_sets = 0" in lib.srx_last_error(ctx.handle)
    assert lib.srx_score_genes(m.handle, f.ptr(sp), f.ptr(sg), 2049, None, 0, None, f.ptr(sc), None, None, 0, None) == f.E_ARG
    assert b"n_sets = 2049" in lib.srx_last_error(ctx.handle) and np.all(sc == -7.0)
    for kw, text in ((dict(sets=[[1, 2]], n_bins=1), "n_bins = 1"), (dict(sets=[[1, 2]], pool=[1, 2, 3, 3], n_bins=3), "repeated in the pool"),
                     (dict(sets=[[1, 2]], pool=[1, 2, 40], n_bins=3), "pool gene 40"), (dict(sets=[[1]], pool=[1], n_bins=5), "n_items"),
                     (dict(sets=[[1], []], n_bins=5), "set 1 is empty"), (dict(sets=[[1, 40]], n_bins=5), "gene index 40 of set 0"),
                     (dict(sets=[[1, 2, 1]], n_bins=5), "gene 1 is repeated in set 0"), (dict(sets=[[1, 2]], pool=[2, 3, 4, 5, 6], n_bins=3), "not in the pool"),
                     (dict(sets=[[1], list(range(40))], n_bins=5), "the control list of set 1 is empty"),
                     (dict(sets=[[1, 2]], n_bins=5, capacity=1), "capacity is 1")):
        rc, _, _, _ = dev_score(m, kw.pop("sets"), **kw)
        assert rc == f.E_ARG and text in lib.srx_last_error(ctx.handle).decode(), (text, lib.srx_last_error(ctx.handle))
    assert dev_score(m, [[1, 2]], n_bins=5)[0] == 0              # the handle is usable after every refusal
    m.free()


# ---- the consumers ------------------------------------------------------------------------------------------------------------------------------------------
def planted_adata(ctx):
    import singlerust_amd as sr
    z = np.load(os.path.join(S.GOLD, "planted_600x240.npz"))
    names = ["g%03d" % j for j in range(int(z["n_cols"]))]
    a = sr.IMAnnData.new_basic((int(z["n_rows"]), int(z["n_cols"]), z["indptr"], z["indices"], z["log_values"]), var_names=names, ctx=ctx, store=2)
    return a, names


def test_cell_cycle_scores_and_phase(ctx):
    from singlerust_amd.memory.processing import score_genes, score_genes_cell_cycle
    a, names = planted_adata(ctx)
    s_genes, g2m_genes = [names[j] for j in range(10, 55)] + ["MCM5"], [names[j] for j in range(120, 175)]       # disjoint; one name is not found
    out = score_genes_cell_cycle(a, s_genes, g2m_genes, n_bins=9, want_info=True)
    assert out["info"]["dropped"] == {"S_score": ["MCM5"]} and out["info"]["n_sets"] == 2 and out["info"]["n_walks"] == 1
    assert out["S_score"].shape == out["G2M_score"].shape == (600,)
    assert out["phase"].tolist() == S.phase(out["S_score"], out["G2M_score"]).tolist()
    assert set(out["phase"]) <= {"S", "G2M", "G1"}
    assert a.obs["phase"] is out["phase"] and np.array_equal(a.obs["S_score"], out["S_score"])
    # both sets in ONE call with ctrl_size = min(45, 55): the same as score_genes on the dict
    both, ctrl = score_genes(a, {"S_score": list(range(10, 55)), "G2M_score": list(range(120, 175))}, ctrl_size=45, n_bins=9, return_controls=True)
    assert same_bits(both["S_score"], out["S_score"]) and same_bits(both["G2M_score"], out["G2M_score"])
    csr = S.planted()
    want, want_ctrl, _ = S.score(csr, gene_means(a.x()), [list(range(10, 55)), list(range(120, 175))], None, 45, 9)
    assert same_bits(want[:, 0], out["S_score"]) and np.array_equal(ctrl["G2M_score"], want_ctrl[1])
    single = score_genes(a, [names[3], names[77]], ctrl_size=5, n_bins=9)
    assert single.shape == (600,) and np.array_equal(a.obs["score"], single)


def test_qc_gene_fractions_against_scipy(ctx):
    import scipy.sparse as sp
    from singlerust_amd.memory.processing import gene_list_sums, qc_gene_fractions
    import singlerust_amd as sr
    z = np.load(os.path.join(S.GOLD, "planted_600x240.npz"))
    n, g = int(z["n_rows"]), int(z["n_cols"])
    a = sr.IMAnnData.new_basic((n, g, z["indptr"], z["indices"], z["values"]), var_names=["mt-%d" % j if j % 17 == 0 else "g%d" % j for j in range(g)],
                               ctx=ctx, store=2)
    mt = np.array([nm.startswith("mt-") for nm in a.var_names])
    out = qc_gene_fractions(a, {"mt": mt, "ribo": list(range(200, 240))})
    X = sp.csr_matrix((z["values"], z["indices"].astype(np.int64), z["indptr"].astype(np.int64)), shape=(n, g))
    total = np.asarray(X.sum(axis=1)).ravel()
    for key, cols in (("mt", np.flatnonzero(mt)), ("ribo", np.arange(200, 240))):
        sub = X[:, cols]
        assert np.array_equal(out["total_counts_" + key], np.asarray(sub.sum(axis=1)).ravel())             # integer counts: exact
        assert np.array_equal(out["n_genes_by_counts_" + key], sub.getnnz(axis=1))
        with np.errstate(invalid="ignore"):
            assert np.array_equal(out["pct_counts_" + key], 100.0 * np.asarray(sub.sum(axis=1)).ravel() / total, equal_nan=True)
        assert out["pct_counts_" + key] is a.obs["pct_counts_" + key]
    s, c = gene_list_sums(a, [mt])
    assert np.array_equal(s[:, 0], out["total_counts_mt"]) and c.dtype == np.uint32


def test_scores_go_into_regress_out_as_covariates(ctx):
    from singlerust_amd.memory.processing import pca_regress_scale, score_genes_cell_cycle
    a, names = planted_adata(ctx)
    score_genes_cell_cycle(a, list(range(10, 55)), list(range(120, 175)), n_bins=9)
    r = pca_regress_scale(a, ["S_score", "G2M_score"], genes=np.arange(60, 120), n_components=5)
    assert r["scores"].shape == (600, 5) and r["n_cov"] == 2 and np.all(np.isfinite(r["scores"]))

"""The device feature selection (csrc/select.hip: k_gene_var, k_hvg_candidates, k_rank_selected / k_hvg_rank, k_sel_finish) alone,
through srx_select_op — which launches the kernels through the function the pipeline launches them through — against its
definition in tests/select_ref.py: on every ranking route (candidates, every gene, the device-side fallback forced and natural), at
every tile, sample and mask edge, on ties, signed zeros, NaN variances and explicit lists.  Every case is one call on host arrays;
a variance v is planted exactly with cnt = 1, sum = 0, sq = v.  Every device buffer has 8 sentinel elements behind it and `run`
asserts that none changed; every HVG case runs twice and must give the same bytes.

Everything is compared bit for bit, the trace included: its tree is restated in select_ref.trace_tree (see check_vectors).
The planted cases cannot see the operation order of k_gene_var (sum = 0 makes mean * mean exact); test_vectors_realistic_moments
does.  profiles/select.md has the route of every case and which cases fail under six mutations of the kernels."""
import ctypes as C

import numpy as np
import pytest

import select_ref as ref
from select_ref import CANDIDATES, FALLBACK, FULL, NONE, UNUSED

pytestmark = pytest.mark.gpu

F_FILL, U_FILL, I_FILL = -7.25e77, 0xdeadbeef, -77
OUT_NAMES = ("var", "rank", "sel_rank", "bits", "prefix", "mu", "sd", "dinv")
SCALARS = {"trace": F_FILL, "counter": 12345, "status": -5, "tail_touched": -9}


def ffi():
    from singlerust_amd import _ffi
    return _ffi


class Call:
    """The argument block of one call and the arrays it points to."""

    def __init__(self, G, n, *, op=0, route=0, cnt=None, s=None, q=None, genes=None, flags=0, n_cells=1, center=1, scale=1,
                 omit=()):
        F = ffi()
        k = max(min(n, G), 1) if G else 1
        n_words = max((G + 31) // 32, 1)
        self.G, self.n, self.k = G, n, min(n, G)
        self.inp = {"cnt": None if cnt is None else np.ascontiguousarray(cnt, np.uint64),
                    "sum": None if s is None else np.ascontiguousarray(s, np.float64),
                    "sq": None if q is None else np.ascontiguousarray(q, np.float64),
                    "genes": None if genes is None else np.ascontiguousarray(genes, np.uint64)}
        g_alloc = min(max(G, 1), 400000)          # (a refused G may be huge: the arrays are not read then)
        self.out = {"var": np.full(g_alloc, F_FILL), "rank": np.full(g_alloc, U_FILL, np.uint32), "sel_rank": np.full(k, I_FILL, np.int32),
                    "bits": np.full(min(n_words, 20000), U_FILL, np.uint32), "prefix": np.full(min(n_words, 20000), U_FILL, np.uint32),
                    "mu": np.full(k, F_FILL), "sd": np.full(k, F_FILL), "dinv": np.full(k, F_FILL)}
        a = self.a = F.SelectArgs()
        a.G, a.take, a.n_cells, a.op, a.route, a.center, a.scale, a.flags = G, n, n_cells, op, route, center, scale, flags
        for name, x in list(self.inp.items()) + list(self.out.items()):
            setattr(a, name, None if x is None or name in omit else x.ctypes.data)
        for name, v in SCALARS.items():
            setattr(a, name, v)

    def untouched(self):
        fills = {"var": F_FILL, "rank": U_FILL, "sel_rank": I_FILL, "bits": U_FILL, "prefix": U_FILL, "mu": F_FILL, "sd": F_FILL, "dinv": F_FILL}
        return all(np.all(self.out[n_] == fills[n_]) for n_ in OUT_NAMES) and all(getattr(self.a, n_) == v for n_, v in SCALARS.items())

    def go(self, ctx, expect=0):
        F = ffi()
        rc = F.lib().srx_select_op(ctx.handle if ctx is not None else None, C.byref(self.a))
        if expect:
            assert rc == expect, (rc, expect)
            assert self.untouched(), "a refused call wrote an output"
            return self
        F.check(rc, ctx.handle)
        assert self.a.tail_touched == 0, "sentinels behind buffers %s changed" % bin(self.a.tail_touched)
        return self

    def bytes(self):
        return b"".join(self.out[n_].tobytes() for n_ in OUT_NAMES) + bytes(np.array([self.a.trace]).data) + \
            bytes(np.array([self.a.counter, self.a.status], np.int64).data)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def check_vectors(c, genes, s, q, n_cells, center, scale):
    """mu, sd, dinv per slot and the trace against the restatement, bit for bit.  The distance to the longdouble sum is held to
    (ceil(k / 1024) + 16) 2^-53 sum |term| first: the exact assertion implies it, and a failure then says how far off the device is."""
    mu, sd, di, terms = ref.vectors(genes, s, q, n_cells, center, scale, c.G)
    assert same_bits(c.out["mu"], mu) and same_bits(c.out["sd"], sd) and same_bits(c.out["dinv"], di)
    want = ref.trace_tree(terms)
    if not np.isnan(want):
        dist = abs(np.longdouble(c.a.trace) - ref.trace_ld(terms))
        assert dist <= ref.trace_bound(terms, c.k), (float(dist), ref.trace_bound(terms, c.k))
    assert same_bits([c.a.trace], [want]), (c.a.trace, want)


class Truth:
    """What one variance array determines, computed once for all its (n, route) cases."""

    def __init__(self, var):
        self.var = np.asarray(var, np.float64)
        self.cnt, self.s, self.q = ref.plant(self.var)
        self.order = ref.order_of(self.var)
        self.rank = np.empty(len(self.var), np.int64)
        self.rank[self.order] = np.arange(len(self.var))


def check_hvg(ctx, t, n, route, kind=None, center=1, scale=1):
    """One HVG case on planted variances: every assertion of the file's header.  Returns (kind, counter, sel_rank)."""
    G = len(t.var)
    k = min(n, G)
    c = Call(G, n, route=route, cnt=t.cnt, s=t.s, q=t.q, center=center, scale=scale).go(ctx)
    again = Call(G, n, route=route, cnt=t.cnt, s=t.s, q=t.q, center=center, scale=scale).go(ctx)
    assert c.bytes() == again.bytes(), "two calls differ"
    want_kind, want_counter, thr = ref.predict(t.var, n, route)
    assert kind is None or route != 0 or want_kind == kind, (want_kind, kind)
    assert same_bits(c.out["var"], t.var)
    assert c.a.counter == want_counter, (c.a.counter, want_counter, want_kind)
    want_rank = np.where(t.var >= thr, t.rank, NONE) if want_kind == CANDIDATES else t.rank
    got_rank = c.out["rank"].astype(np.int64)
    top = t.rank < k
    assert np.array_equal(got_rank[top], t.rank[top])
    assert np.array_equal(got_rank, want_rank)
    sel = t.order[:k]
    bits, prefix = ref.mask_of(sel, G)
    assert np.array_equal(c.out["sel_rank"], sel)
    assert np.array_equal(c.out["bits"], bits) and np.array_equal(c.out["prefix"], prefix)
    assert len(ref.genes_of_bits(c.out["bits"])) == k
    assert c.a.status == 0
    check_vectors(c, sel, t.s, t.q, 1, center, scale)
    return want_kind, c.a.counter, c.out["sel_rank"].copy()


def check_routes(ctx, t, n, kind=None):
    got = [check_hvg(ctx, t, n, route, kind) for route in ref.ROUTES]
    assert all(np.array_equal(got[0][2], g[2]) for g in got[1:])
    return got[0]


# ---- every shape, every route ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", ref.SHAPE_G)
def test_shapes_distinct(ctx, G):
    t = Truth(ref.distinct(G))
    for n in ref.takes_of(G):
        kind, counter, _ = check_routes(ctx, t, n)
        print("G %d take %d: route 0 = %s, M = %s, cap %d" % (G, n, kind, counter if kind == CANDIDATES else "-", ref.cap_of(G, min(n, G))))


# ---- the value patterns ---------------------------------------------------------------------------------------------------------
PATTERNS = ref.pattern_cases()


@pytest.mark.parametrize("case", PATTERNS, ids=[p[0] for p in PATTERNS])
def test_patterns(ctx, case):
    name, var, n, kind = case
    t = Truth(var)
    got_kind, counter, _ = check_routes(ctx, t, n, kind)
    print("%s: G %d take %d: route 0 = %s, counter %#x, cap %d" % (name, len(var), n, got_kind, counter, ref.cap_of(len(var), min(n, len(var)))))


def test_fallback_walks_every_pair_at_65536(ctx):
    """More than `cap` genes tied at the maximum: the device falls back by itself and 512 workgroups walk 256 x 32 = 8192 pairs,
    sixteen each.  (Also in PATTERNS; here the route is asserted by name.)"""
    t = Truth(ref.too_many_ties(65536, 5000))
    kind, counter, _ = check_hvg(ctx, t, 100, 0)
    assert kind == FALLBACK and counter == NONE


# ---- NaN variances --------------------------------------------------------------------------------------------------------------
NANS = ref.nan_cases()


@pytest.mark.parametrize("route", ref.ROUTES)
@pytest.mark.parametrize("case", NANS, ids=[p[0] for p in NANS])
def test_nan_variances(ctx, case, route):
    """A NaN variance is the status word's bit 0; the ranking it breaks may flag more than `take` genes, and k_sel_finish's clamp
    keeps the mask at `take` bits at most, all below G.  The context then serves a clean call."""
    _, var, n = case
    G = len(var)
    cnt, s, q = ref.plant(var)
    c = Call(G, n, route=route, cnt=cnt, s=s, q=q).go(ctx)
    assert c.a.status & 1
    assert same_bits(c.out["var"], var)
    genes = ref.genes_of_bits(c.out["bits"])
    assert len(genes) <= n and np.all(genes < G)
    assert np.all((c.out["sel_rank"] == I_FILL) | ((c.out["sel_rank"] >= 0) & (c.out["sel_rank"] < G)))
    check_hvg(ctx, Truth(ref.distinct(G, 12)), n, route)


# ---- explicit lists -------------------------------------------------------------------------------------------------------------
def list_of(G, k, order):
    rng = ref.rng_of(21, G, k)
    g = rng.permutation(G)[:k]
    g[0] = G - 1 if G - 1 not in g[1:] else g[0]
    g = np.unique(g)
    while len(g) < k:                                    # (the forced last gene may have collided)
        g = np.unique(np.concatenate([g, rng.integers(0, G, k - len(g))]))
    g = np.sort(g)
    return g[::-1].copy() if order == "descending" else rng.permutation(g) if order == "shuffled" else g


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("G", [33, 65536, 65537, 70000, 300001])
def test_lists(ctx, G, order):
    """select_list's rank table and k_sel_finish without variances (G > 65536: the global-memory variant), with NaN moments inside
    and outside the list: no NaN test on an explicit list, status stays 0."""
    rng = ref.rng_of(22, G)
    n_cells = 50
    s = rng.random(G) * n_cells
    q = s * s / n_cells + rng.random(G)
    for k in (1, 33 if G == 33 else 64, 65, 8192):
        if k > G:
            continue
        genes = list_of(G, k, order)
        s2, q2 = s.copy(), q.copy()
        if k > 1:
            s2[genes[k // 2]] = np.nan                  # a NaN moment inside the list, one outside it
        outside = [g for g in (0, 1, 2) if g not in genes]
        if outside:
            q2[outside[0]] = np.nan
        for center, scale in ((1, 0), (0, 1)):
            c = Call(G, k, op=ffi().SEL_LIST, s=s2, q=q2, genes=genes, n_cells=n_cells, center=center, scale=scale).go(ctx)
            want_rank = np.full(G, NONE, np.uint32)
            want_rank[genes] = np.arange(k)
            bits, prefix = ref.mask_of(genes, G)
            assert np.array_equal(c.out["rank"], want_rank)
            assert np.array_equal(c.out["sel_rank"], genes.astype(np.int32))
            assert np.array_equal(c.out["bits"], bits) and np.array_equal(c.out["prefix"], prefix)
            assert c.a.status == 0 and c.a.counter == UNUSED
            assert np.all(c.out["var"] == F_FILL)
            check_vectors(c, genes, s2, q2, n_cells, center, scale)


def test_list_without_vectors_keeps_the_vectors(ctx):
    """select_list's `vectors = false` form: sum and sq are not read (null here), mu, sd, dinv and the trace are not written."""
    F = ffi()
    for G in (700, 70000):
        genes = list_of(G, 65, "shuffled")
        c = Call(G, 65, op=F.SEL_LIST, genes=genes, flags=F.SEL_NO_VECTORS).go(ctx)
        bits, prefix = ref.mask_of(genes, G)
        assert np.array_equal(c.out["sel_rank"], genes.astype(np.int32))
        assert np.array_equal(c.out["bits"], bits) and np.array_equal(c.out["prefix"], prefix)
        assert all(np.all(c.out[n_] == F_FILL) for n_ in ("mu", "sd", "dinv")) and c.a.trace == F_FILL
        assert c.a.status == 0


# ---- the vectors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("center,scale", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("G,n", [(300, 151), (700, 151), (3000, 2500)])
def test_vectors_realistic_moments(ctx, G, n, center, scale):
    """Moments of random non-negative columns (cnt <= n_cells), with a constant column, an empty one and one whose sq / n - mean^2
    rounds below zero, all three inside the selection or outside it as the ranking has it: var, the selection, mu, sd, dinv and
    the trace bit for bit."""
    n_cells = 40
    cnt, s, q = ref.realistic_moments(G, n_cells, 0)
    var = ref.variance(cnt, s, q)
    c = Call(G, n, cnt=cnt, s=s, q=q, n_cells=n_cells, center=center, scale=scale).go(ctx)
    assert same_bits(c.out["var"], var)
    sel, bits, prefix = ref.selection(var, n)
    assert np.array_equal(c.out["sel_rank"], sel)
    assert np.array_equal(c.out["bits"], bits) and np.array_equal(c.out["prefix"], prefix)
    assert c.a.status == 0 and c.a.counter == ref.predict(var, n, 0)[1]
    check_vectors(c, sel, s, q, n_cells, center, scale)


def test_vectors_of_the_special_columns(ctx):
    """The constant, the empty and the negative-rounding column selected by a list, so that their slots are looked at whatever
    the ranking thinks of them."""
    n_cells, G = 40, 700
    cnt, s, q = ref.realistic_moments(G, n_cells, 1)
    genes = np.array([3, 5, 7, 100, 699, 0], np.uint64)
    mean7 = s[7] / n_cells
    assert q[7] / n_cells - mean7 * mean7 < 0
    for center in (0, 1):
        for scale in (0, 1):
            c = Call(G, len(genes), op=ffi().SEL_LIST, s=s, q=q, genes=genes, n_cells=n_cells, center=center, scale=scale).go(ctx)
            check_vectors(c, genes, s, q, n_cells, center, scale)
            if scale:
                slot = list(np.sort(genes))
                assert c.out["dinv"][slot.index(5)] == 1.0 and c.out["dinv"][slot.index(7)] == 1.0 and c.out["sd"][slot.index(7)] == 0.0


# ---- the entry itself -----------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctx):
    F = ffi()
    G, n = 600, 50
    cnt, s, q = ref.plant(ref.distinct(G))
    hvg = dict(cnt=cnt, s=s, q=q)
    bad = F.E_ARG
    Call(G, 0, **hvg).go(ctx, bad)                                           # take == 0
    Call(0, 5, **hvg).go(ctx, bad)
    Call(65537, 5, **hvg).go(ctx, bad)                                       # outside hvg_on_device's envelope (nothing is read)
    Call(65536, 8193, **hvg).go(ctx, bad)
    Call(G, n, route=3, **hvg).go(ctx, bad)
    Call(G, n, route=-1, **hvg).go(ctx, bad)
    Call(G, n, op=2, **hvg).go(ctx, bad)
    for name in ("cnt", "sum", "sq", "var", "rank", "sel_rank", "bits", "prefix", "mu", "sd", "dinv"):
        Call(G, n, omit=(name,), **hvg).go(ctx, bad)
    Call(G, n, flags=F.SEL_NO_VECTORS, omit=("sum",), **hvg).go(ctx, bad)     # the flag belongs to LIST
    Call(G, n, **hvg).go(None, bad)                                           # null context
    assert F.lib().srx_select_op(ctx.handle, None) == bad
    genes = np.array([5, 7, 599, 1], np.uint64)
    lst = dict(op=F.SEL_LIST, s=s, q=q)
    Call(G, 4, genes=np.array([5, 7, 600, 1], np.uint64), **lst).go(ctx, F.E_BOUNDS)
    Call(G, 4, genes=np.array([5, 7, 5, 1], np.uint64), **lst).go(ctx, bad)
    Call(G, 4, genes=genes, omit=("genes",), **lst).go(ctx, bad)
    Call(G, 4, genes=genes, omit=("sum",), **lst).go(ctx, bad)
    Call(G, 4, genes=genes, omit=("sq",), **lst).go(ctx, bad)
    Call(G, 4, genes=genes, omit=("mu",), **lst).go(ctx, bad)
    Call(G, 4, genes=genes, omit=("rank",), flags=F.SEL_NO_VECTORS, **lst).go(ctx, bad)
    Call(G, 0, genes=genes, **lst).go(ctx, bad)
    Call(2 ** 31, 4, genes=genes, **lst).go(ctx, bad)                         # more columns than a matrix can have (nothing is read)
    Call(2 ** 40, 4, genes=genes, flags=F.SEL_NO_VECTORS, **lst).go(ctx, bad)
    # the context stays usable
    c = Call(G, 4, genes=genes, omit=("sum", "sq", "mu", "sd", "dinv", "var", "cnt"), flags=F.SEL_NO_VECTORS, **lst).go(ctx)
    assert np.array_equal(c.out["sel_rank"], genes.astype(np.int32))
    check_hvg(ctx, Truth(ref.distinct(G)), n, 0)


def synth_host(seed, n, g, density):
    import oracle
    F = ffi()
    p = F.SynthParams()
    F.lib().srx_synth_defaults(C.byref(p), seed, n, g, density)
    ip = np.zeros(n + 1, dtype=np.uint64)
    F.lib().srx_synth_indptr(C.byref(p), 0, n, F.ptr(ip))
    idx, val = np.zeros(int(ip[-1]), np.uint64), np.zeros(int(ip[-1]), np.float32)
    F.lib().srx_synth_fill_host(C.byref(p), 0, n, F.ptr(ip), F.ptr(idx), F.ptr(val))
    return oracle.Csr(n, g, ip, idx, val)


def test_pipeline_nan_on_the_candidate_route_then_clean(ctx):
    """The entry tied to the product: 600 cells x 1000 genes (G >= 512: the candidate route) with one NaN value through srx_pipeline
    is SRX_E_NAN, and the next srx_pipeline on the same context selects what the oracle selects."""
    import oracle
    import singlerust_amd as sr
    F = ffi()
    m = synth_host(35, 600, 1000, 0.1)
    vals = m.values.copy()
    vals[len(vals) // 2] = np.nan
    opts = F.PcaOpts(5, -1, -1, -1, 0, 0, 0, 0.0, 0)
    res = F.PipelineResult()

    def adata(mat):
        return sr.IMAnnData.new_basic((mat.n_rows, mat.n_cols, mat.indptr, mat.indices, mat.values), ctx=ctx, store=1)

    a = adata(m.with_values(vals))
    with pytest.raises(sr.SrxError) as e:
        F.check(F.lib().srx_pipeline(a.x().handle, 1e4, 50, C.byref(opts), C.byref(res)), ctx.handle)
    assert e.value.code == F.E_NAN
    b = adata(m)
    F.check(F.lib().srx_pipeline(b.x().handle, 1e4, 50, C.byref(opts), C.byref(res)), ctx.handle)
    hv = np.zeros(int(res.pca.k), np.uint64)
    F.check(F.lib().srx_result_fetch(b.x().handle, None, None, None, None, None, F.ptr(hv)), ctx.handle)
    lg = oracle.log1p_transform(oracle.normalize_total(m, 1e4, oracle.ROW))
    assert np.array_equal(hv, oracle.select_hvg(oracle.compute_variance(lg, oracle.COLUMN), 50))

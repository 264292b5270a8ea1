"""srx_loess_direct, srx_clipped_group_moments and srx_select_hvg_seurat_v3 on the device against the definition in
include/srx.h (tests/hvg_seurat_ref.py restates it).  Stage by stage: every stage is checked on the device's own output of the
stage before it, so that an allowed rounding difference upstream can never flip a rank downstream.

Tolerances, none of them taken from the device's output:
  loess   device and reference differ in the order of eight sums: 8 x the largest |f64 reference - long-double reference| over
          the same inputs (hvg_seurat_ref.loess_bound; 2.0e-13 over the cases of the kernel's own test, 1.2e-13 on the planted
          fixture, in log10 units).  The whole-selection test feeds the reference numpy's log10 of the device's mean and var
          where the device used its own log10; one ulp of x or y moves a fit by some 1e-16, far inside the bound.
  clip    the largest relative gap between numpy's 10.0 ** e and its long-double evaluation on the device's e, plus four
          roundings of one unit in the last place (2^-52 relative) for sqrt, multiply, add and the device's pow; the sum may
          not exceed 1e-13 (a sanity condition: more is not rounding).  This is the issue's check on the device's e.
  reg_var pow(10, e) is the one operation that cannot be made bit-equal to numpy: neither the C library behind numpy nor the
          device's math library rounds it correctly; each documents an error below one unit in the last place, so the two
          differ by less than 2 ulp.  The device reports the value it used as a table of its own.
  nv      on the device's tables, reg_var among them: bit for bit the reference formula (the order of the operations is
          defined, contraction is off, division and square root are correctly rounded).  So is the clip from reg_var.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import hvg_seurat_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
STORES = [1, 2]                     # SRX_STORE_F32, SRX_STORE_F64
INF = float("inf")


def F():
    from singlerust_amd import _ffi
    return _ffi


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def upload(ctx, X, store):
    import singlerust_amd as sr
    X = sp.csr_matrix(X)
    X.sort_indices()
    return sr.DeviceCsr.upload(ctx, X.shape[0], X.shape[1], X.indptr, X.indices, X.data, store)


def dev_loess(ctx, x, y, span):
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    out = np.full(max(x.size, 1), -7.0)
    F().check(F().lib().srx_loess_direct(ctx.handle, F().ptr(x), F().ptr(y), x.size, float(span), F().ptr(out)), ctx.handle)
    return out[:x.size]


def dev_clipped(dev, labels, n_groups, clip):
    i = dev.info()
    labels = np.ascontiguousarray(labels, np.uint32)
    clip = np.ascontiguousarray(clip, np.float64)
    s, q, info = np.zeros((n_groups, i.n_cols)), np.zeros((n_groups, i.n_cols)), F().MarkersInfo()
    F().check(F().lib().srx_clipped_group_moments(dev.handle, F().ptr(labels), n_groups, F().ptr(clip), F().ptr(s), F().ptr(q), C.byref(info)),
              dev.ctx.handle)
    return s, q, info


def dev_moments(dev, labels, n_groups):
    i = dev.info()
    labels = np.ascontiguousarray(labels, np.uint32)
    s, q = np.zeros((n_groups, i.n_cols)), np.zeros((n_groups, i.n_cols))
    F().check(F().lib().srx_group_moments(dev.handle, F().ptr(labels), n_groups, None, None, F().ptr(s), F().ptr(q)), dev.ctx.handle)
    return s, q


def dev_seurat(dev, n_top, batch=None, n_batches=None, span=0.3, flavor="seurat_v3"):
    from singlerust_amd.memory.processing import seurat_v3_tables
    return seurat_v3_tables(dev, n_top, batch, n_batches, span, flavor)


def planted():
    z = np.load(os.path.join(GOLD, "planted_600x240.npz"))
    return sp.csr_matrix((z["values"], z["indices"].astype(np.int64), z["indptr"].astype(np.int64)), shape=(int(z["n_rows"]), int(z["n_cols"])))


# ---- the loess kernel alone ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loess_reference():
    """name -> (x, y, span, f64 reference), and the bound over all of them: made once, shared, never written to."""
    cases = R.loess_cases()
    bound, worst = R.loess_bound([c[1:] for c in cases])
    return {c[0]: c[1:] + (R.loess_direct(*c[1:]),) for c in cases}, bound, worst


@pytest.mark.parametrize("name", [c[0] for c in R.loess_cases()])
def test_loess_kernel_against_the_reference(ctx, name):
    table, bound, worst = loess_reference()
    x, y, span, want = table[name]
    got = dev_loess(ctx, x, y, span)
    err = float(np.abs(got - want).max())
    print("loess %s: |device - f64 reference| = %.3e, bound %.3e (8 x %.3e)" % (name, err, bound, worst))
    assert 0 < bound < 1e-11
    assert err <= bound
    assert same_bits(got, dev_loess(ctx, x, y, span))                                 # the same call twice
    for v in np.unique(x):                                                            # tied fit points, wherever they sit
        at = np.flatnonzero(x == v)
        assert np.unique(got[at].view(np.uint64)).size == 1
    if R.window(x.size, span) == 1 and np.unique(x).size == x.size:
        assert same_bits(got, np.ascontiguousarray(y, np.float64))                   # q = 1: the point itself
    p = np.random.default_rng(3).permutation(x.size)                                 # another input order: the same fits
    assert np.all(np.abs(dev_loess(ctx, x[p], y[p], span) - want[p]) <= bound)


def test_loess_refusals(ctx):
    lib, x, out = F().lib(), np.array([0.0, 1.0, 2.0]), np.full(3, -7.0)
    for span in (0.0, -0.3, 1.5, float("nan")):
        assert lib.srx_loess_direct(ctx.handle, F().ptr(x), F().ptr(x), 3, span, F().ptr(out)) == F().E_ARG
        assert b"span" in lib.srx_last_error(ctx.handle)
    bad = np.array([0.0, np.nan, 2.0])
    assert lib.srx_loess_direct(ctx.handle, F().ptr(bad), F().ptr(x), 3, 0.3, F().ptr(out)) == F().E_NAN
    assert lib.srx_loess_direct(ctx.handle, F().ptr(x), F().ptr(np.array([0.0, 1.0, INF])), 3, 0.3, F().ptr(out)) == F().E_NAN
    assert lib.srx_loess_direct(ctx.handle, None, F().ptr(x), 3, 0.3, F().ptr(out)) == F().E_ARG
    assert lib.srx_loess_direct(ctx.handle, F().ptr(x), F().ptr(x), 0, 0.3, F().ptr(out)) == F().OK
    assert np.all(out == -7.0)
    assert dev_loess(ctx, x, x, 1.0).size == 3                                        # the context stays usable


# ---- the clipped walk alone ------------------------------------------------------------------------------------------------------------
def counts_matrix(seed, n, g, density=None, per_row=None):
    """Integer counts 1 + geometric, canonical CSR."""
    rng = np.random.default_rng(seed)
    if per_row is not None:
        lens = rng.poisson(per_row, n)
        rows = np.repeat(np.arange(n), lens)
        cols = rng.integers(0, g, rows.size)
        m = sp.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(n, g)).tocsr()
        m.sum_duplicates()
    else:
        m = sp.random(n, g, density=density, format="csr", random_state=rng)
    m.data = rng.geometric(0.4, m.nnz).astype(np.float64)
    m.sort_indices()
    return m


def walk_matrix(shape):
    if shape == "300x1":
        X = counts_matrix(1, 300, 1, density=0.6)                                     # G = 1
    elif shape == "257x300":
        X = counts_matrix(2, 257, 300, density=0.1)
    elif shape == "310x10001":
        X = counts_matrix(3, 310, 10001, density=0.01)                                # two gene tiles, the second of one gene
        X = sp.csr_matrix(sp.hstack([X[:, :10000], sp.csr_matrix(np.arange(1, 311, dtype=np.float64).reshape(-1, 1) % 5)]))
    elif shape == "70x700":
        X = counts_matrix(4, 70, 700, density=0.6)                                    # segments longer than 256 entries
    else:
        X = counts_matrix(5, 300, 70000, per_row=8)                                   # no 16-bit mirror: 32-bit indices, seven tiles
    X = sp.lil_matrix(X)
    for r in (0, X.shape[0] // 2, X.shape[0] - 1):
        X[r, :] = 0                                                                   # empty rows
    X = sp.csr_matrix(X)
    X.eliminate_zeros()
    X.sort_indices()
    return X


WALK_SHAPES = ["300x1", "257x300", "310x10001", "70x700", "300x70000"]


def test_walk_inputs_hold_the_edges():
    for shape in WALK_SHAPES:
        X = walk_matrix(shape)
        lens = np.diff(X.indptr)
        assert (lens == 0).sum() >= 3 and np.all(X.data == np.rint(X.data)) and X.data.min() >= 1
        if shape != "300x1":
            assert np.any(X.indptr[:-1] % 4 != 0)                                     # segments that start off a 4-entry boundary
    assert np.diff(walk_matrix("70x700").indptr).max() > 256
    assert walk_matrix("310x10001").shape[1] % 10000 == 1 and walk_matrix("310x10001")[:, 10000].nnz > 0
    assert walk_matrix("300x70000").shape[1] > 65536


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("shape", WALK_SHAPES)
def test_clipped_walk_bit_for_bit(ctx, shape, store):
    X = walk_matrix(shape)
    N, G = X.shape
    dev = upload(ctx, X, store)
    rng = np.random.default_rng(17)
    sc = R.scales_of(X)
    for n_groups, labels in ((1, np.zeros(N, np.uint32)), (2, rng.integers(0, 2, N)), (7, rng.integers(0, 7, N)),
                             (8, rng.integers(0, 7, N))):                             # (8: group 7 is empty)
        base_s, base_q = dev_moments(dev, labels, n_groups)
        per_group = rng.choice([0.1, 2.7, 1.0, 3.5, INF], size=(n_groups, G))
        per_group[:, 0] = np.linspace(0.3, 4.1, n_groups)                              # clips that differ per group for one gene
        tables = {"inf": np.full((n_groups, G), INF), "zero": np.zeros((n_groups, G)), "below": np.full((n_groups, G), 0.5),
                  "tenth": np.full((n_groups, G), 0.1), "2.7": np.full((n_groups, G), 2.7), "per_group": per_group}
        for name, clip in tables.items():
            s, q, info = dev_clipped(dev, labels, n_groups, clip)
            assert (info.sum_scale_log2, info.sq_scale_log2) == sc and info.n_groups == n_groups, name
            S, Q = R.grouped_int(X, labels, n_groups, sc, clip)
            assert same_bits(s, R.unfix(S, sc[0])) and same_bits(q, R.unfix(Q, sc[1])), (name, n_groups)
            if name == "inf":
                assert same_bits(s, base_s) and same_bits(q, base_q)
            if name == "zero":
                assert not s.any() and not q.any()
            if name == "below":
                assert np.array_equal(q * 2.0, s) and s.any()                          # every entry became 0.5
    dev.free()


def test_clipped_walk_refusals(ctx):
    lib, E = F().lib(), F().E_ARG
    X = walk_matrix("257x300")
    N, G = X.shape
    dev = upload(ctx, X, 2)
    labels, s = np.zeros(N, np.uint32), np.full((1, G), -7.0)
    clip = np.full((1, G), 1.0)

    def call(h, lab, k, cl):
        rc = lib.srx_clipped_group_moments(h, None if lab is None else F().ptr(lab), k, None if cl is None else F().ptr(cl), F().ptr(s), F().ptr(s), None)
        assert np.all(s == -7.0)
        return rc
    assert call(dev.handle, labels, 1, None) == E
    assert call(dev.handle, labels, 0, clip) == E and call(dev.handle, labels, 4097, clip) == E
    assert call(dev.handle, None, 1, clip) == E
    bad = clip.copy()
    bad[0, 5] = -1.0
    assert call(dev.handle, labels, 1, bad) == E and b"clip" in lib.srx_last_error(ctx.handle)
    bad[0, 5] = np.nan
    assert call(dev.handle, labels, 1, bad) == E
    lab2 = labels.copy()
    lab2[9] = 1
    assert call(dev.handle, lab2, 1, clip) == E and b"label" in lib.srx_last_error(ctx.handle)
    csc = dev.to_csc()
    assert call(csc.handle, labels, 1, clip) == E
    csc.free()
    Y = X.copy()
    Y.data[3] = np.inf
    devn = upload(ctx, Y, 2)
    assert call(devn.handle, labels, 1, clip) == F().E_NAN
    devn.free()
    dev_clipped(dev, labels, 1, clip)                                                 # the handle stays usable
    dev.free()


# ---- the whole selection, stage by stage -----------------------------------------------------------------------------------------------
def check_stages(X, batch, n_batches, n_top, sel, T, info, span=0.3, paper=False):
    """Every stage of the definition on the device's own output of the stage before it."""
    N, G = X.shape
    labels = np.zeros(N, np.int64) if batch is None else np.asarray(batch, np.int64)
    sizes = np.bincount(labels, minlength=n_batches)
    sc = R.scales_of(X)
    assert (info["sum_scale_log2"], info["sq_scale_log2"]) == sc and info["n_cells"] == N and info["n_genes"] == G
    assert info["n_batches"] == n_batches and info["min_batch_cells"] == sizes.min() and info["span"] == span
    assert info["max_abs"] == float(X.data.max())
    # 1. the batch moments and the totals: integers, bit for bit
    S, Q = R.grouped_int(X, labels, n_batches, sc)
    mean, var = R.moments(R.unfix(S, sc[0]), R.unfix(Q, sc[1]), sizes)
    assert same_bits(T["mean"], mean) and same_bits(T["var"], var)
    means, variances = R.moments(R.unfix(S.sum(axis=0), sc[0]), R.unfix(Q.sum(axis=0), sc[1]), N)
    assert same_bits(T["means"], means) and same_bits(T["variances"], variances)
    # 2. the trend on the device's mean and var
    cases = [(np.log10(T["mean"][b, T["var"][b] > 0]), np.log10(T["var"][b, T["var"][b] > 0]), span) for b in range(n_batches)]
    bound, worst = R.loess_bound(cases)
    fitted = R.trend(T["mean"], T["var"], span)
    err = float(np.abs(T["fitted"] - fitted).max())
    print("fitted: |device - f64 reference| = %.3e, bound %.3e (8 x %.3e)" % (err, bound, worst))
    assert bound < 1e-11 and err <= bound
    assert not T["fitted"][~(T["var"] > 0)].any()                                     # a constant gene: e = 0
    # 3. the clip on the device's fitted
    e = T["fitted"]
    ld = np.power(np.longdouble(10), e.astype(np.longdouble))
    gap = float(np.max(np.abs((10.0 ** e).astype(np.longdouble) - ld) / ld))
    tol = gap + 4 * 2.0 ** -52
    clip = R.clip_of(T["mean"], R.reg_var_of(e), sizes)
    cerr = float(np.max(np.abs(T["clip"] - clip) / clip))
    print("clip: relative |device - numpy| = %.3e, tolerance %.3e (numpy's pow gap %.3e)" % (cerr, tol, gap))
    assert tol <= 1e-13 and cerr <= tol
    # ... and pow itself, the one operation that is not bit-equal to numpy: the device's reg_var against numpy's, in ulps; from
    # the device's reg_var on, the clip is every bit the stated formula
    rv_ulps = np.abs(T["reg_var"] - R.reg_var_of(e)) / np.spacing(R.reg_var_of(e))
    print("reg_var: largest distance from numpy's pow %.1f ulp, %d of %d entries bit-equal" % (rv_ulps.max(), int((rv_ulps == 0).sum()), rv_ulps.size))
    assert np.all(rv_ulps <= 2)
    assert same_bits(T["clip"], R.clip_of(T["mean"], T["reg_var"], sizes))
    # 4. the clipped sums on the device's clip: integers, bit for bit
    Sc, Qc = R.grouped_int(X, labels, n_batches, sc, T["clip"])
    assert same_bits(T["clip_sum"], R.unfix(Sc, sc[0])) and same_bits(T["clip_sumsq"], R.unfix(Qc, sc[1]))
    # 5. nv on the device's tables, reg_var among them: the reference formula to the last bit
    assert same_bits(T["nv"], R.nv_of(T["mean"], T["reg_var"], T["clip_sum"], T["clip_sumsq"], sizes))
    vn = np.zeros(G)
    for b in range(n_batches):
        vn = vn + T["nv"][b]
    assert same_bits(T["variances_norm"], vn / n_batches)
    # 6. the integer logic on the device's nv, exactly
    rank = R.ranks_of(T["nv"])
    assert same_bits(T["rank"], rank)
    nb, med = R.combine(rank, n_top)
    assert same_bits(T["nbatches"], nb) and same_bits(np.isnan(T["median"]), np.isnan(med))
    assert np.array_equal(T["median"][~np.isnan(med)], med[~np.isnan(med)])
    assert np.array_equal(sel, R.select(med, nb, n_top, paper))
    return bool(np.any(Sc != S))                                                      # whether something was clipped


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("n_batches", [1, 3])
def test_planted_fixture_stage_by_stage(ctx, n_batches, store):
    X = planted()
    dev = upload(ctx, X, store)
    batch = None if n_batches == 1 else R.hashed_batches(X.shape[0], n_batches)
    sel, T, info = dev_seurat(dev, 40, batch, n_batches)
    check_stages(X, batch, n_batches, 40, sel, T, info)
    assert any(np.unique(row).size < row.size for row in T["nv"])                     # exact ties, ordered by gene index
    # the other order, another span, n_top >= G: the same stages
    sel_p, T_p, info_p = dev_seurat(dev, 40, batch, n_batches, flavor="seurat_v3_paper")
    assert all(same_bits(T[k], T_p[k]) for k in T)
    assert np.array_equal(sel_p, R.select(T["median"], T["nbatches"], 40, paper=True))
    if n_batches > 1:
        assert not np.array_equal(sel, sel_p)
    sel_a, T_a, info_a = dev_seurat(dev, 1000, batch, n_batches, span=0.6)
    check_stages(X, batch, n_batches, 1000, sel_a, T_a, info_a, span=0.6)
    assert sel_a.size == X.shape[1] and np.array_equal(np.sort(sel_a), np.arange(X.shape[1])) and np.all(T_a["nbatches"] == n_batches)
    # twice: the same bits
    sel2, T2, _ = dev_seurat(dev, 40, batch, n_batches)
    assert np.array_equal(sel, sel2) and all(same_bits(T[k], T2[k]) for k in T)
    dev.free()


@pytest.mark.parametrize("n_top", [20, 40, 60])
def test_planted_fixture_from_scratch(ctx, n_top):
    """One batch, everything from the counts in numpy: the selected SET is the reference's, no gene left out.  The reference's nv
    has a relative gap of 3.8e-3, 1.5e-3 and 1.4e-3 at these cuts (test_hvg_seurat_cpu.py asserts 1e-3), eleven orders above
    the loess difference."""
    X = planted()
    dev = upload(ctx, X, 2)
    sel, _, _ = dev_seurat(dev, n_top)
    want = R.run(X, None, 1, n_top)["selected"]
    assert sel.size == n_top and set(sel.tolist()) == set(want.tolist())
    dev.free()


def test_known_answer(ctx):
    """The decimal known answer through the C ABI; the bounds are those of test_hvg_seurat_cpu.py's reference test plus the
    loess bound for the other order of the sums."""
    k = json.load(open(os.path.join(GOLD, "kat_seurat_v3.json")))
    X = sp.csr_matrix(np.array(k["X"], np.float64))
    for store in STORES:
        dev = upload(ctx, X, store)
        for flavor, key in (("seurat_v3", "selected"), ("seurat_v3_paper", "selected_paper")):
            sel, T, info = dev_seurat(dev, k["n_top"], np.array(k["batch"], np.uint32), k["n_batches"], k["span"], flavor)
            assert sel.tolist() == k[key]
        want = {key: np.array([[float(s) for s in row] for row in k[key]]) for key in ("mean", "var", "fitted", "clip", "clip_sum", "clip_sumsq", "nv")}
        for key in ("mean", "var"):
            assert np.all(np.abs(T[key] - want[key]) <= 4 * 2.0 ** -52 * np.abs(want[key])), key
        assert np.all(np.abs(T["fitted"] - want["fitted"]) <= 1e-12)
        for key in ("clip", "clip_sum", "clip_sumsq", "nv"):
            assert np.all(np.abs(T[key] - want[key]) <= 3e-12 * np.abs(want[key])), key
        assert T["rank"].tolist() == k["rank"] and T["nbatches"].tolist() == k["nbatches"]
        assert [None if np.isnan(v) else v for v in T["median"]] == k["median"]
        assert check_stages(X, k["batch"], k["n_batches"], k["n_top"], np.array(k["selected_paper"], np.uint64), T, info, span=k["span"],
                            paper=True)                                           # (the example clips an entry)
        dev.free()


def test_refusals_leave_the_outputs_alone(ctx):
    import singlerust_amd as sr
    lib, E = F().lib(), F().E_ARG
    X = planted()
    N, G = X.shape
    dev = upload(ctx, X, 2)
    batch = R.hashed_batches(N, 3)

    def call(m_, n_top=10, b=batch, k=3, opts=None, expect=E, ctx_=ctx, idx=True, n_out_=True, word=None):
        idx_a, n_out, col = np.full(G, 77, dtype=np.uint64), C.c_uint64(99), np.full((3, G), -7.0)
        tables = F().SeuratV3Tables()
        tables.means, tables.nv, tables.clip = F().ptr(col[0]), F().ptr(col), F().ptr(col)
        info = F().SeuratV3Info()
        info.max_abs = -7.0
        rc = lib.srx_select_hvg_seurat_v3(None if m_ is None else m_.handle, n_top, None if b is None else F().ptr(b), k,
                                          None if opts is None else C.byref(opts), F().ptr(idx_a) if idx else None,
                                          C.byref(n_out) if n_out_ else None, C.byref(tables), C.byref(info))
        assert rc == expect, rc
        msg = lib.srx_last_error(None if m_ is None else ctx_.handle)
        assert msg and (word is None or word in msg.decode()), msg
        assert np.all(idx_a == 77) and n_out.value == 99 and np.all(col == -7.0) and info.max_abs == -7.0

    call(None)
    call(dev, idx=False)
    call(dev, n_out_=False)
    call(dev, n_top=0, word="n_top")
    for span in (-0.1, 1.01, float("nan")):
        call(dev, opts=F().SeuratV3Opts(span, 0, 0), word="span")
    call(dev, k=0, word="n_batches")
    call(dev, k=4097, word="n_batches")
    call(dev, b=None, k=3)                                                            # no labels for three batches
    call(dev, k=2, word="label")                                                      # a label >= n_batches, found on the device
    lonely = batch.copy()
    lonely[batch == 2] = 0
    lonely[5] = 2
    call(dev, b=lonely, word="cells")                                                 # a batch of one cell
    call(dev, k=4, word="cells")                                                      # ... and an empty one
    for v, expect, store in ((-1.0, E, 2), (-0.5, E, 1), (np.nan, F().E_NAN, 2), (np.inf, F().E_NAN, 1)):
        Y = X.copy()
        Y.data[11] = v
        bad = upload(ctx, Y, store)
        call(bad, expect=expect)
        bad.free()
    csc = dev.to_csc()
    call(csc, word="CSC")
    csc.free()
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    m2 = upload(c2, X, 2)
    call(m2, ctx_=c2, word="rank")
    m2.free()
    c2.close()
    c3 = sr.Context(0)
    m3 = upload(c3, X, 2)
    bk = C.c_void_p()
    F().check(lib.srx_backed_create(c3.handle, G, F().STORE_F32, C.byref(bk)), c3.handle)
    call(m3, ctx_=c3, word="backed")
    lib.srx_backed_destroy(bk)
    assert dev_seurat(m3, 10, batch, 3)[0].size == 10                                 # accepted again once the session is gone
    m3.free()
    c3.close()
    assert dev_seurat(dev, 10, batch, 3)[0].size == 10                                # the handle is usable after every refusal
    dev.free()


@pytest.mark.parametrize("store", STORES)
def test_the_handle_is_left_as_it_was(ctx, store):
    """Values, dtype, moments cache and the resident PCA result, after a pipeline has left all of them on the handle (the
    values are then ln(1 + x): non-integers are accepted)."""
    lib = F().lib()
    X = planted()
    n, g = X.shape
    dev = upload(ctx, X, store)
    popts, res = F().PcaOpts(20, -1, -1, -1, 0, 0, 0, 0.0, 11), F().PipelineResult()
    F().check(lib.srx_pipeline(dev.handle, 1e4, 120, C.byref(popts), C.byref(res)), ctx.handle)

    def state():
        scores = np.zeros((n, 20))
        F().check(lib.srx_result_fetch(dev.handle, F().ptr(scores), None, None, None, None, None), ctx.handle)
        cnt, s, q = np.zeros(g, np.uint64), np.zeros(g), np.zeros(g)
        F().check(lib.srx_gene_moments(dev.handle, F().ptr(cnt), F().ptr(s), F().ptr(q)), ctx.handle)
        i = dev.info()
        return dev.values(np.float64), scores, cnt, s, q, np.array([i.dtype, i.store, i.nnz])

    before = state()
    sel, T, _ = dev_seurat(dev, 30, R.hashed_batches(n, 3), 3)
    dev_clipped(dev, np.zeros(n, np.uint32), 1, np.full((1, g), 1.5))
    after = state()
    assert all(same_bits(a, b) for a, b in zip(before, after))
    assert sel.size == 30 and np.all(np.isfinite(T["nv"]))
    dev.free()


def test_python_wrapper_end_to_end(ctx):
    import singlerust_amd as sr
    from singlerust_amd.memory.processing import highly_variable_genes_seurat_v3
    X = planted()
    n, g = X.shape
    a = sr.IMAnnData.new_basic(X, ctx=ctx, store=2)
    names = np.array(["b%d" % v for v in R.hashed_batches(n, 3)])                       # labels of any type
    sel, cols = highly_variable_genes_seurat_v3(a, 40, batch=names)
    codes = np.unique(names, return_inverse=True)[1]
    dev = upload(ctx, X, 2)
    want_sel, T, _ = dev_seurat(dev, 40, codes.astype(np.uint32), 3)
    assert np.array_equal(sel, want_sel) and sel.dtype == np.uint64
    assert set(cols) == {"means", "variances", "variances_norm", "highly_variable_rank", "highly_variable_nbatches", "highly_variable"}
    assert same_bits(cols["highly_variable_rank"], T["median"]) and same_bits(cols["variances_norm"], T["variances_norm"])
    assert cols["highly_variable"].sum() == 40 and np.all(cols["highly_variable"][sel.astype(np.int64)])
    assert all(np.array_equal(a.var[k], v, equal_nan=True) for k, v in cols.items())
    assert a.uns["hvg"]["flavor"] == "seurat_v3" and a.uns["hvg"]["n_batches"] == 3
    sel1, cols1 = highly_variable_genes_seurat_v3(dev, 20, flavor="seurat_v3_paper")
    assert sel1.size == 20 and np.all(cols1["highly_variable_nbatches"] <= 1)
    dev.free()

"""Pearson-residual gene selection on the device (srx_pearson_gene_variance / srx_select_hvg_pearson / srx_pearson_residuals)
against the long-double restatement of its definition (pearson_ref.py) and the decimal known answers (golden/kat_pearson.json).

Bounds, u = 2^-53, against the long-double reference:
  elements   |z_dev - z_ref| <= 8u (|z_ref| + min(sqrt(mu), sqrt(theta)))      (non-integer input: 8 + 2 (n + G))
  variances  |v_dev - v_ref| <= 4 (n + 16) u mean_i(z_ref^2) + (cnt_j / n) (sq_quantum + 2 |mean z| sum_quantum)
Every test prints the largest ratio it reached before it asserts.  The shapes walk -1 / 0 / +1 round every size at which the
kernels take another path (pearson_ref.TILES: the dense pass's cell step 1024, gene tile 1024 and thread stride 256, the CSR
correction's row block 64 and gene tile 10000, the block kernel's 256 outputs).  Every input from 8 x 8 on holds an all-zero
gene, an empty cell, a gene stored in every other cell, a single-entry gene, a cell holding every other gene and an outlier
count, and is asserted (from the reference alone, before the device is touched) to reach both clips; 1 x 1, 5 x 3 and 257 x 1
cannot hold those six at once and are plain draws.  Measured on an MI355X: elements reach 0.33 of their bound, variances
0.16 (CSR, quanta included) and 0.04 (CSC); profiles/pearson.md has the table."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import pearson_ref as R

pytestmark = pytest.mark.gpu
INF = float("inf")


def F():
    from singlerust_amd import _ffi
    return _ffi


def upload(ctx, X, dtype=np.uint32, csc=False):
    import singlerust_amd as sr
    n, G, indptr, indices, values = (R.to_csc if csc else R.to_csr)(X, dtype)
    return sr.DeviceCsr.upload(ctx, n, G, indptr, indices, values, csc=csc)


def opts(theta, clip):
    return F().PearsonOpts(0.0 if theta is None else theta, 0.0 if clip is None else clip)


def dev_variance(m, theta=None, clip=None):
    G = int(m.info().n_cols)
    var, info, o = np.full(G, -7.0), F().PearsonInfo(), opts(theta, clip)
    F().check(F().lib().srx_pearson_gene_variance(m.handle, C.byref(o), F().ptr(var), C.byref(info)), m.ctx.handle)
    return var, info


def dev_select(m, n, theta=None, clip=None, with_var=True):
    G = int(m.info().n_cols)
    idx, n_out, var = np.full(max(min(n, G), 1), 2 ** 63, dtype=np.uint64), C.c_uint64(99), np.full(G, -7.0)
    info, o = F().PearsonInfo(), opts(theta, clip)
    F().check(F().lib().srx_select_hvg_pearson(m.handle, n, C.byref(o), F().ptr(idx), C.byref(n_out), F().ptr(var) if with_var else None,
                                               C.byref(info)), m.ctx.handle)
    return idx[:n_out.value], var, info


def dev_residuals(m, genes, theta=None, clip=None):
    g = np.ascontiguousarray(genes, dtype=np.uint64)
    out, o = np.full((int(m.info().n_rows), g.size), -7.0), opts(theta, clip)
    F().check(F().lib().srx_pearson_residuals(m.handle, F().ptr(g), g.size, C.byref(o), F().ptr(out), None), m.ctx.handle)
    return out


@functools.lru_cache(maxsize=None)
def counts(n, G):
    X = R.make_counts(n, G)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def reference(n, G, theta, clip):
    """The long-double reference of one input: computed once, shared, read-only."""
    X = counts(n, G)
    z = R.residuals(X, theta, clip)
    out = {"z": z, "v": R.variances(z), "mu": R.mu_of(X), "g": X.sum(axis=0), "cnt": (X > 0).sum(axis=0),
           "theta": R.used_opts(n, theta, clip)[0]}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def assert_input(n, G):
    """From the reference alone, before the device is touched: both clips bite, a gene without counts, half the genes with."""
    if not R.has_features(n, G):
        return
    p = R.properties(counts(n, G))
    assert p["upper_clip_default"] and p["upper_clip_one"] and p["lower_clip_one"], p
    assert p["zero_genes"] >= 1 and p["expressed_genes"] >= G / 2, p
    assert p["empty_cells"] >= 1 and p["full_genes"] >= 1 and p["single_genes"] >= 1 and p["full_cells"] >= 1, p


def check_elements(z_dev, ref, cols, integer=True, n=0, G=0, what=""):
    z_ref, mu = ref["z"][:, cols], ref["mu"][:, cols]
    bound = R.element_bound(z_ref, mu, ref["theta"], n, G, integer)
    err = np.abs(z_dev.astype(np.longdouble) - z_ref).astype(np.float64)
    ratio = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    same = bool(np.array_equal(z_dev, z_ref.astype(np.float64)))
    print("pearson elements %s: max ratio %.3f of the bound, equal to the rounded reference: %s" % (what, ratio, same))
    assert np.all(err <= bound), (what, ratio)
    return ratio


def check_variances(v_dev, info, ref, what=""):
    bound = R.variance_bound(ref["z"], ref["cnt"], info.sum_quantum, info.sq_quantum)
    err = np.abs(v_dev.astype(np.longdouble) - ref["v"]).astype(np.float64)
    ratio = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    print("pearson variances %s: max ratio %.4f of the bound (quanta %g, %g)" % (what, ratio, info.sum_quantum, info.sq_quantum))
    assert np.all(err[ref["g"] > 0] <= bound[ref["g"] > 0]), (what, ratio)
    assert np.all(v_dev[ref["g"] == 0] == 0.0), what
    return ratio


def whole_case(ctx, n, G, theta, clip, dtype, csc):
    assert_input(n, G)
    X, ref = counts(n, G), reference(n, G, theta, clip)
    what = "%dx%d theta=%s clip=%s %s %s" % (n, G, theta, clip, np.dtype(dtype).name, "csc" if csc else "csr")
    m = upload(ctx, X, dtype, csc)
    rng = np.random.default_rng(n + G)
    # elements: all genes, a permuted subset, a list with repeats
    allg = np.arange(G)
    z = dev_residuals(m, allg, theta, clip)
    check_elements(z, ref, allg, what=what + " all")
    assert np.all(z[:, ref["g"] == 0] == 0.0) and np.all(z[X.sum(axis=1) == 0, :] == 0.0)
    sub = rng.permutation(G)[:max(1, G // 3)]
    check_elements(dev_residuals(m, sub, theta, clip), ref, sub, what=what + " subset")
    rep = rng.integers(0, G, size=G + 3)
    check_elements(dev_residuals(m, rep, theta, clip), ref, rep, what=what + " repeats")
    # variances
    v, info = dev_variance(m, theta, clip)
    check_variances(v, info, ref, what)
    assert (info.n_cells, info.n_genes) == (n, G) and info.n_expressed == int((ref["g"] > 0).sum())
    assert info.n_empty_cells == int((X.sum(axis=1) == 0).sum()) and info.total == float(X.sum())
    assert (info.sum_quantum == 0.0 and info.sq_quantum == 0.0) if csc else (info.sum_quantum > 0.0 and info.sq_quantum > 0.0)
    # selection: exactly the stable descending order of the variances the same call returned, among the genes with counts
    n_expr = int(info.n_expressed)
    for n_top in (G // 3 + 1, n_expr, G + 5, 0):
        sel, v2, _ = dev_select(m, n_top, theta, clip)
        assert np.array_equal(v2, v), what                                     # the same bits as the variance call
        assert np.array_equal(sel, R.select(v2, ref["g"], n_top)), (what, n_top)
        assert sel.size == min(n_top, n_expr)
    m.free()


# ---- every shape, both handles -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("csc", [False, True], ids=["csr", "csc"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_against_the_reference(ctx, shape, csc):
    whole_case(ctx, shape[0], shape[1], None, None, np.uint32, csc)


# ---- every theta x clip x storage x handle on three shapes ------------------------------------------------------------------------------
@pytest.mark.parametrize("csc", [False, True], ids=["csr", "csc"])
@pytest.mark.parametrize("dtype", [np.uint32, np.float32, np.float64], ids=["u32", "f32", "f64"])
@pytest.mark.parametrize("clip", R.CLIPS, ids=["clipdef", "clip1", "clipinf"])
@pytest.mark.parametrize("theta", R.THETAS, ids=["theta100", "theta10", "poisson"])
@pytest.mark.parametrize("shape", R.CROSS_SHAPES, ids=lambda s: "%dx%d" % s)
def test_options_and_storage(ctx, shape, theta, clip, dtype, csc):
    whole_case(ctx, shape[0], shape[1], theta, clip, dtype, csc)


# ---- non-integer values: the three sums round ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("csc", [False, True], ids=["csr", "csc"])
def test_non_integer_values(ctx, csc):
    n, G = 257, 300
    rng = np.random.default_rng(5)
    X = counts(n, G) * rng.uniform(0.25, 1.75, size=(n, G))
    z_ref = R.residuals(X)
    ref = {"z": z_ref, "v": R.variances(z_ref), "mu": R.mu_of(X), "g": X.sum(axis=0), "cnt": (X > 0).sum(axis=0), "theta": 100.0}
    m = upload(ctx, X, np.float64, csc)
    allg = np.arange(G)
    check_elements(dev_residuals(m, allg), ref, allg, integer=False, n=n, G=G, what="non-integer %s" % ("csc" if csc else "csr"))
    v, info = dev_variance(m)
    # the variance bound has no term for the rounding of r, g and T: it is widened by the element bound's factor, squared sums
    # being linear in the elements' relative error
    bound = R.variance_bound(z_ref, ref["cnt"], info.sum_quantum, info.sq_quantum) + \
        2.0 * (2.0 * (n + G)) * R.U * 2.0 * np.asarray((z_ref * z_ref).mean(axis=0), dtype=np.float64)
    err = np.abs(v.astype(np.longdouble) - ref["v"]).astype(np.float64)
    print("pearson variances non-integer: max ratio %.4f" % float(np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound)
    m.free()


# ---- identical columns on both sides of every gene-tile edge -----------------------------------------------------------------------
@pytest.mark.parametrize("csc", [False, True], ids=["csr", "csc"])
def test_copies_of_a_column_get_identical_bits(ctx, csc):
    n, G = 70, 10001          # two gene tiles of the matrix (5001 each), ten of the dense pass
    X = counts(n, G).copy()
    src = int(np.argmax((X > 0).sum(axis=0) * (np.arange(G) > 3)))
    where = [250, 260, 1020, 1030, 4990, 5010, 9000]     # round the thread stride (256), the dense tile (1024), the matrix tile (5001)
    where = [w for w in where if w != src]
    X[:, where] = X[:, [src]]
    m = upload(ctx, X, np.uint32, csc)
    v, info = dev_variance(m)
    group = sorted(where + [src])
    assert len({v[j].tobytes() for j in group}) == 1, v[group]
    sel, _, _ = dev_select(m, int(info.n_expressed))
    pos = [int(np.nonzero(sel == j)[0][0]) for j in group]
    same = sorted(int(p) for p in np.nonzero(v[sel.astype(np.int64)] == v[src])[0])
    members = [int(sel[p]) for p in same]
    assert members == sorted(members) and set(group) <= set(members) and pos == sorted(pos)
    m.free()


# ---- reproducible; CSR and CSC agree; the handle is left as it was ------------------------------------------------------------------
def test_two_calls_give_identical_bits_and_the_handles_agree(ctx):
    n, G = 3000, 130
    X, ref = counts(n, G), reference(n, G, None, None)
    a, b = upload(ctx, X, np.uint32, False), upload(ctx, X, np.uint32, True)
    got = {}
    for name, m in (("csr", a), ("csc", b)):
        v1, i1 = dev_variance(m)
        v2, _ = dev_variance(m)
        s1, _, _ = dev_select(m, 40)
        s2, _, _ = dev_select(m, 40)
        z1, z2 = dev_residuals(m, np.arange(G)), dev_residuals(m, np.arange(G))
        assert v1.tobytes() == v2.tobytes() and s1.tobytes() == s2.tobytes() and z1.tobytes() == z2.tobytes(), name
        got[name] = (v1, i1, z1)
    assert got["csr"][2].tobytes() == got["csc"][2].tobytes()             # elements: the same arithmetic on the same sums
    bound = R.variance_bound(ref["z"], ref["cnt"], got["csr"][1].sum_quantum, got["csr"][1].sq_quantum) + R.variance_bound(ref["z"], ref["cnt"])
    assert np.all(np.abs(got["csr"][0] - got["csc"][0]) <= bound)
    a.free()
    b.free()


@pytest.mark.parametrize("dtype", [np.uint32, np.float32], ids=["u32", "f32"])
def test_the_handle_is_left_as_it_was(ctx, dtype):
    n, G = 257, 300
    X = counts(n, G)
    for csc in (False, True):
        m = upload(ctx, X, dtype, csc)
        before, info0 = m.values(np.float64), m.info()
        mom0 = None
        if not csc:
            mom0 = (np.zeros(G, np.uint64), np.zeros(G), np.zeros(G))
            F().check(F().lib().srx_gene_moments(m.handle, *[F().ptr(a) for a in mom0]), ctx.handle)
        dev_variance(m)
        dev_select(m, 30, 10.0, 1.0)
        dev_residuals(m, [5, 1, 5])
        info1 = m.info()
        assert np.array_equal(m.values(np.float64), before)
        assert (info0.dtype, info0.store, info0.nnz) == (info1.dtype, info1.store, info1.nnz)
        if not csc:
            mom1 = (np.zeros(G, np.uint64), np.zeros(G), np.zeros(G))
            F().check(F().lib().srx_gene_moments(m.handle, *[F().ptr(a) for a in mom1]), ctx.handle)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(mom0, mom1))
        m.free()


# ---- the known answers through the C ABI ---------------------------------------------------------------------------------------------
def test_known_answers(ctx):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_pearson.json")
    for case in json.load(open(path)):
        X = np.array(case["X"], dtype=np.int64)
        n, G = X.shape
        theta = INF if case["theta"] == "inf" else float(case["theta"])
        clip = None if case["clip"] is None else (INF if case["clip"] == "inf" else float(case["clip"]))
        z_ref = np.array([[np.longdouble(s) for s in row] for row in case["z"]])
        v_ref = np.array([np.longdouble(s) for s in case["v"]])
        ref = {"z": z_ref, "v": v_ref, "mu": R.mu_of(X), "g": X.sum(axis=0), "cnt": (X > 0).sum(axis=0), "theta": theta}
        for csc in (False, True):
            m = upload(ctx, X, np.float64, csc)
            check_elements(dev_residuals(m, np.arange(G), theta, clip), ref, np.arange(G), what="KAT " + case["name"])
            v, info = dev_variance(m, theta, clip)
            check_variances(v, info, ref, "KAT " + case["name"])
            m.free()
    # T == 0: every variance 0, nothing selected, no error
    m = upload(ctx, np.zeros((4, 3), dtype=np.int64), np.float64, False)
    v, info = dev_variance(m)
    sel, _, _ = dev_select(m, 2)
    assert np.all(v == 0.0) and sel.size == 0 and info.total == 0.0 and info.n_expressed == 0 and info.n_empty_cells == 4
    assert np.all(dev_residuals(m, [0, 2]) == 0.0)
    m.free()


# ---- refusals: SRX_E_ARG, a message, the outputs untouched ------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(ctx):
    import singlerust_amd as sr
    lib, E = F().lib(), F().E_ARG
    n, G = 65, 65
    X = counts(n, G)
    m = upload(ctx, X, np.float64, False)

    def three(m_, o, genes=(1, 2), expect=E, ctx_=ctx):
        """The three calls with sentinels in every output; each must refuse and leave them."""
        var, idx, n_out = np.full(G, -7.0), np.full(G, 77, dtype=np.uint64), C.c_uint64(99)
        out, info = np.full((n, len(genes)), -7.0), F().PearsonInfo()
        info.ms_dense = -7.0
        g = np.array(genes, dtype=np.uint64)
        op = None if o is None else C.byref(o)
        h = None if m_ is None else m_.handle
        msgs = []
        for rc in (lib.srx_pearson_gene_variance(h, op, F().ptr(var), C.byref(info)),
                   lib.srx_select_hvg_pearson(h, 10, op, F().ptr(idx), C.byref(n_out), F().ptr(var), C.byref(info)),
                   lib.srx_pearson_residuals(h, F().ptr(g), g.size, op, F().ptr(out), C.byref(info))):
            assert rc == expect, rc
            msg = lib.srx_last_error(None if m_ is None else ctx_.handle)
            assert msg
            msgs.append(msg.decode())
        assert np.all(var == -7.0) and np.all(idx == 77) and n_out.value == 99 and np.all(out == -7.0) and info.ms_dense == -7.0
        return msgs

    three(None, F().PearsonOpts(0.0, 0.0))
    for bad in (F().PearsonOpts(-1.0, 0.0), F().PearsonOpts(float("nan"), 0.0)):
        assert all("theta" in s for s in three(m, bad))
    for bad in (F().PearsonOpts(0.0, -1.0), F().PearsonOpts(0.0, float("nan"))):
        assert all("clip" in s for s in three(m, bad))
    # NULL outputs
    var, idx, n_out, g2 = np.full(G, -7.0), np.full(G, 77, dtype=np.uint64), C.c_uint64(99), np.array([1, 2], dtype=np.uint64)
    assert lib.srx_pearson_gene_variance(m.handle, None, None, None) == E
    assert lib.srx_select_hvg_pearson(m.handle, 5, None, None, C.byref(n_out), F().ptr(var), None) == E
    assert lib.srx_select_hvg_pearson(m.handle, 5, None, F().ptr(idx), None, F().ptr(var), None) == E
    assert lib.srx_pearson_residuals(m.handle, F().ptr(g2), 2, None, None, None) == E
    assert lib.srx_pearson_residuals(m.handle, None, 2, None, F().ptr(var), None) == E
    assert np.all(var == -7.0) and np.all(idx == 77) and n_out.value == 99
    # a gene index out of range
    out = np.full((n, 2), -7.0)
    bad_g = np.array([1, G], dtype=np.uint64)
    assert lib.srx_pearson_residuals(m.handle, F().ptr(bad_g), 2, None, F().ptr(out), None) == E and np.all(out == -7.0)
    assert b"out of bounds" in lib.srx_last_error(ctx.handle)
    m.free()
    # a negative, NaN or infinite stored value, at either storage and in either format
    for v, dtype in ((-1.0, np.float64), (np.nan, np.float64), (np.inf, np.float32), (-0.5, np.float32)):
        for csc in (False, True):
            Y = X.astype(np.float64)
            Y[7, 9] = v
            mb = upload(ctx, Y, dtype, csc)              # (np.nonzero keeps a NaN: it is a stored entry)
            assert all("negative, NaN or infinite" in s for s in three(mb, None))
            mb.free()
    # a context with more than one rank
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    m2 = upload(c2, X, np.float64, False)
    assert all("rank" in s for s in three(m2, None, ctx_=c2))
    m2.free()
    c2.close()
    # a backed session open on the context
    c3 = sr.Context(0)
    m3 = upload(c3, X, np.float64, False)
    b = C.c_void_p()
    F().check(lib.srx_backed_create(c3.handle, G, F().STORE_F32, C.byref(b)), c3.handle)
    assert all("backed" in s for s in three(m3, None, ctx_=c3))
    lib.srx_backed_destroy(b)
    dev_variance(m3)                     # ... and accepted again once the session is gone
    m3.free()
    c3.close()


# ---- Python: the selection feeds the PCA unchanged --------------------------------------------------------------------------------------
def test_python_selection_feeds_the_pca(ctx):
    import singlerust_amd as sr
    from singlerust_amd.memory import processing
    n, G, n_top = 1000, 300, 40
    X = counts(n, G)
    a = sr.IMAnnData.new_basic(R.to_csr(X, np.float32), ctx=ctx)
    sel = processing.highly_variable_genes_pearson(a, n_top_genes=n_top)
    v, _ = dev_variance(a.x())
    assert np.array_equal(sel, R.select(v, X.sum(axis=0), n_top))
    assert a.var["highly_variable"].dtype == np.bool_ and int(a.var["highly_variable"].sum()) == n_top
    assert np.array_equal(a.var["residual_variances"], v)
    rank = a.var["highly_variable_rank"]
    assert np.array_equal(rank[sel.astype(np.int64)], np.arange(n_top)) and int(np.isnan(rank).sum()) == G - n_top
    assert np.allclose(a.var["means"], X.mean(axis=0), rtol=1e-12) and np.allclose(a.var["variances"], X.var(axis=0), rtol=1e-9)
    assert a.uns["hvg"]["flavor"] == "pearson_residuals" and a.uns["hvg"]["n_cells"] == n
    z = processing.pearson_residuals(a, sel[:5])
    assert z.shape == (n, 5) and np.array_equal(z, dev_residuals(a.x(), sel[:5]))
    b = a.deep_clone()
    for ad in (a, b):
        processing.normalize_total_inplace(ad, 1e4, sr.Direction.Row)
        processing.log1p_transform_inplace(ad)
    processing.dim_red.pca_inplace(a, 5, None, None, None, sr.FeatureSelection.HighlyVariableCol("highly_variable"), None)
    want = np.sort(sel)
    assert np.array_equal(a.uns["pca"]["selected_features"], want)
    # srx_pca with that explicit list, on a clone that went through the same transform
    opts_ = F().PcaOpts(5, -1, -1, -1, 0, 0, 0, 0.0, 0)
    scores, comps, evr = np.zeros((n, 5)), np.zeros((n_top, 5)), np.zeros(5)
    mean, std, info = np.zeros(n_top), np.zeros(n_top), F().PcaInfo()
    F().check(F().lib().srx_pca(b.x().handle, F().ptr(want), n_top, C.byref(opts_), F().ptr(scores), F().ptr(comps), F().ptr(evr),
                                F().ptr(mean), F().ptr(std), C.byref(info)), ctx.handle)
    # two solves of the same system on two handles: equal up to the order in which the Gram kernel's atomics land
    got = a.obsm["X_pca"]
    for c in range(5):
        sgn = 1.0 if np.dot(got[:, c], scores[:, c]) >= 0 else -1.0
        assert np.max(np.abs(got[:, c] - sgn * scores[:, c])) <= 1e-9 * np.max(np.abs(scores[:, c])), c

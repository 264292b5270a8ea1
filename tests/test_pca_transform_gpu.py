"""Pca::transform on the device (srx_pca_model_* / srx_pca_transform): a fitted PCA applied to other cells, checked against
an independent numpy restatement of src/shared/processing/pca/mod.rs:156-185 (with normalize_total(Row) + ln_1p of
scale/mod.rs:9-15 / transform/mod.rs where the transform bits ask for it) and against the fit's own scores.

Scores are compared per component as max|delta| / max|ref| (an elementwise relative error is meaningless near zero scores)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

ABSENT = np.iinfo(np.uint64).max
BOUND = {1: 1e-5, 2: 1e-10}          # storage -> bound against the restatement


def comp_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    den = np.maximum(np.abs(ref).max(axis=0), 1e-300)
    return float((np.abs(got - ref).max(axis=0) / den).max())


def upload(ctx, x, store, csc=False):
    import singlerust_amd as sr
    x = x.tocsc() if csc else x.tocsr()
    x.sort_indices()
    dev = sr.DeviceCsr.upload(ctx, x.shape[0], x.shape[1], x.indptr, x.indices, x.data, store, csc=csc)
    return sr.IMAnnData(dev, x.indptr, x.indices, [f"c{i}" for i in range(x.shape[0])], [f"g{j}" for j in range(x.shape[1])])


def counts(rng, n, g, density, empty_rows=()):
    x = sp.random(n, g, density=density, format="csr", random_state=np.random.RandomState(int(rng.integers(1 << 30))),
                  data_rvs=lambda s: rng.integers(1, 30, s).astype(np.float64))
    x = x.tolil()
    for r in empty_rows:
        x[r, :] = 0
    x = x.tocsr()
    x.eliminate_zeros()
    x.sort_indices()
    return x


def restate(x, V, mu, sd, center, scale, feat, bits=0, target=1e4):
    """pca/mod.rs:156-185 in f64: ((x - mu) / sd') V over the mapped columns, absent genes as zero columns."""
    y = x.astype(np.float64).toarray()
    if bits & 1:
        s = y.sum(axis=1)
        f = np.where(s == 0, 0.0, target / np.where(s == 0, 1.0, s))
        y = y * f[:, None]
    if bits & 2:
        y = np.log1p(y)
    k = V.shape[0]
    xg = np.zeros((y.shape[0], k))
    for i in range(k):
        if feat[i] != ABSENT:
            xg[:, i] = y[:, int(feat[i])]
    sdp = np.where(sd == 0, 1.0, sd)
    z = (xg - (mu if center else 0.0)) / (sdp if scale else 1.0)
    return z @ V


def transform(model, q, feat=None, target=0.0, bits=0, n_pc=None):
    from singlerust_amd import _ffi as F
    n_pc = n_pc if n_pc is not None else model.info()[1]
    out = np.zeros((q.n_obs(), n_pc))
    fm = None if feat is None else np.ascontiguousarray(feat, np.uint64)
    F.check(F.lib().srx_pca_transform(model.handle, q.x().handle, F.ptr(fm), float(target), int(bits),
                                      F.ptr(out) if out.size else None), q.x().ctx.handle)
    return out


def random_model(rng, k, n_pc):
    V, _ = np.linalg.qr(rng.standard_normal((k, n_pc)))
    mu = rng.uniform(0.0, 3.0, k)
    sd = rng.uniform(0.5, 2.0, k)
    sd[3] = 0.0                                            # a zero-variance feature: treated as 1
    return V, mu, sd


@pytest.mark.parametrize("store", [1, 2])
@pytest.mark.parametrize("bits", [0, 3])
@pytest.mark.parametrize("center,scale", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_transform_matches_restatement(ctx, store, bits, center, scale):
    from singlerust_amd.memory.processing.dim_red import PcaModel
    rng = np.random.default_rng(100 + 10 * store + bits + 2 * center + 4 * scale)
    k, n_pc, g = 40, 7, 120
    x = counts(rng, 300, g, 0.08, empty_rows=(0, 17, 299))
    V, mu, sd = random_model(rng, k, n_pc)
    # the query's gene axis differs from the model's: a permuted subset of its columns, four model genes absent
    feat = rng.permutation(g)[:k].astype(np.uint64)
    feat[[1, 9, 22, 39]] = ABSENT
    q = upload(ctx, x, store)
    model = PcaModel.from_parts(ctx, V, mu, sd, None, center, scale)
    got = transform(model, q, feat, 1e4, bits)
    ref = restate(x, V, mu, sd, center, scale, feat, bits)
    err = comp_err(got, ref)
    assert err <= BOUND[store], err
    # an empty row is the constant alone: -(mu / sd') V over every model row, the absent ones included
    empty = np.asarray(x.getnnz(axis=1) == 0)
    assert empty.sum() >= 3
    cst = -((mu if center else np.zeros(k)) / (np.where(sd == 0, 1.0, sd) if scale else 1.0)) @ V
    den = np.maximum(np.abs(ref).max(axis=0), 1e-300)
    assert float((np.abs(got[empty] - cst).max(axis=0) / den).max()) <= BOUND[store]
    # the query's values are never modified
    assert np.array_equal(q.x_values(np.float64), x.data.astype(np.float32 if store == 1 else np.float64).astype(np.float64))


def fitted(ctx, store, seed=7, n=600, g=500, n_pc=10, n_hvg=200):
    import singlerust_amd as sr
    from singlerust_amd.memory import processing
    from singlerust_amd.memory.processing import dim_red
    rng = np.random.default_rng(seed)
    x = counts(rng, n, g, 0.1)
    a = upload(ctx, x, store)
    processing.normalize_total_inplace(a, 1e4, sr.Direction.Row)
    processing.log1p_transform_inplace(a)
    dim_red.pca_inplace(a, n_pc, None, None, None, sr.FeatureSelection.HighlyVariable(n_hvg), None)
    return a, x


@pytest.mark.parametrize("store,tol", [(1, 1e-6), (2, 1e-12)])
def test_self_projection(ctx, store, tol):
    from singlerust_amd.memory.processing import dim_red
    from singlerust_amd.memory.processing.dim_red import PcaModel
    a, _ = fitted(ctx, store)
    want = a.obsm["X_pca"]
    m1 = PcaModel.from_result(a)
    k, n_pc, sel = m1.info()
    assert (k, n_pc) == (200, 10) and np.array_equal(sel, a.uns["pca"]["selected_features"])
    assert comp_err(dim_red.pca_transform(a, m1), want) <= tol
    m2 = PcaModel.from_uns(a)
    assert comp_err(dim_red.pca_transform(a, m2), want) <= tol
    dim_red.pca_transform_inplace(a, m2)
    assert comp_err(a.obsm["X_pca"], want) <= tol


@pytest.mark.parametrize("store", [1, 2])
def test_raw_counts_fused_path(ctx, store):
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import dim_red
    from singlerust_amd.memory.processing.dim_red import PcaModel
    rng = np.random.default_rng(31 + store)
    x = counts(rng, 900, 700, 0.06, empty_rows=(5,))
    raw = upload(ctx, x, store)
    A, B = raw.deep_clone(), raw.deep_clone()
    opts = F.PcaOpts(12, -1, -1, -1, 0, 0, 0, 0.0, 3)
    res = F.PipelineResult()
    F.check(F.lib().srx_pipeline(A.x().handle, 1e4, 150, C.byref(opts), C.byref(res)), ctx.handle)
    want = np.zeros((900, 12))
    F.check(F.lib().srx_result_fetch(A.x().handle, F.ptr(want), None, None, None, None, None), ctx.handle)
    model = PcaModel.from_result(A)
    got = dim_red.pca_transform(B, model, target_sum=1e4, log1p=True)
    assert comp_err(got, want) <= 1e-5
    assert np.array_equal(B.x_values(np.float64), raw.x_values(np.float64))


def test_held_out_cells(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory import processing
    from singlerust_amd.memory.processing import dim_red
    from singlerust_amd.memory.processing.dim_red import PcaModel
    rng = np.random.default_rng(5)
    x = counts(rng, 800, 400, 0.1)
    full = upload(ctx, x, 2)
    processing.normalize_total_inplace(full, 1e4, sr.Direction.Row)
    processing.log1p_transform_inplace(full)
    keep = (rng.random(800) < 0.7).astype(np.uint8)

    def sub(mask):
        h = C.c_void_p()
        F.check(F.lib().srx_subset(full.x().handle, F.ptr(mask), None, C.byref(h)), ctx.handle)
        return sr.IMAnnData._from_device(sr.DeviceCsr(ctx, h), [], [])
    fit, rest = sub(keep), sub(1 - keep)
    dim_red.pca_inplace(fit, 8, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    u = fit.uns["pca"]
    model = PcaModel.from_result(fit)
    y = sp.csr_matrix((full.x_values(np.float64), x.indices, x.indptr), shape=x.shape)
    ref = restate(y[np.flatnonzero(1 - keep)], u["components"], u["mean"], u["std"], 1, 1, u["selected_features"])
    assert comp_err(dim_red.pca_transform(rest, model), ref) <= 1e-10
    assert comp_err(dim_red.pca_transform(fit, model), fit.obsm["X_pca"]) <= 1e-12


@pytest.mark.parametrize("n_pc", [2, 50, 64, 100])
@pytest.mark.parametrize("store,tol", [(1, 1e-6), (2, 1e-12)])
def test_component_counts(ctx, n_pc, store, tol):
    from singlerust_amd.memory.processing import dim_red
    from singlerust_amd.memory.processing.dim_red import PcaModel
    a, _ = fitted(ctx, store, seed=11, n=700, g=400, n_pc=n_pc, n_hvg=200)
    model = PcaModel.from_result(a)
    assert model.info()[1] == n_pc
    assert comp_err(dim_red.pca_transform(a, model), a.obsm["X_pca"]) <= tol
    # the same model from the host arrays, on a query whose gene axis is the fitted one reversed
    u = a.uns["pca"]
    x = sp.csr_matrix((a.x_values(np.float64), a.indices.astype(np.int64), a.indptr.astype(np.int64)), shape=(700, 400))
    rev = upload(ctx, x[:, ::-1], 2)
    feat = (399 - u["selected_features"]).astype(np.uint64)
    got = dim_red.pca_transform(rev, PcaModel.from_uns(a), feat)
    assert comp_err(got, restate(x, u["components"], u["mean"], u["std"], 1, 1, u["selected_features"])) <= 1e-10


def test_wide_query_uses_32_bit_indices(ctx):
    from singlerust_amd.memory.processing.dim_red import PcaModel
    rng = np.random.default_rng(17)
    g = 70_000
    x = counts(rng, 200, g, 0.002)
    k, n_pc = 30, 5
    V, mu, sd = random_model(rng, k, n_pc)
    feat = np.concatenate([rng.choice(np.arange(65_536, g), 20, replace=False), rng.choice(65_536, 10, replace=False)]).astype(np.uint64)
    # make sure the mapped columns hold values
    x = x.tolil()
    for j, c in enumerate(feat):
        x[j % 200, int(c)] = 3.0 + j
    x = x.tocsr()
    for store in (1, 2):
        q = upload(ctx, x, store)
        got = transform(PcaModel.from_parts(ctx, V, mu, sd), q, feat, 1e4, 3)
        assert comp_err(got, restate(x, V, mu, sd, 1, 1, feat, 3)) <= BOUND[store]


def test_csc_query_and_determinism(ctx):
    from singlerust_amd.memory.processing.dim_red import PcaModel
    rng = np.random.default_rng(23)
    x = counts(rng, 400, 150, 0.1, empty_rows=(3,))
    V, mu, sd = random_model(rng, 50, 9)
    feat = rng.permutation(150)[:50].astype(np.uint64)
    feat[7] = ABSENT
    model = PcaModel.from_parts(ctx, V, mu, sd)
    q, qc = upload(ctx, x, 2), upload(ctx, x, 2, csc=True)
    for bits in (0, 1, 2, 3):
        a1 = transform(model, q, feat, 1e4, bits)
        a2 = transform(model, q, feat, 1e4, bits)
        assert np.array_equal(a1, a2)                                  # bit-identical on every call
        assert comp_err(a1, restate(x, V, mu, sd, 1, 1, feat, bits)) <= 1e-10
        assert comp_err(transform(model, qc, feat, 1e4, bits), a1) <= 1e-12
    assert np.array_equal(q.x_values(np.float64), x.data) and np.array_equal(qc.x_values(np.float64), x.tocsc().data)


def test_zero_row_query(ctx):
    from singlerust_amd.memory.processing.dim_red import PcaModel
    rng = np.random.default_rng(3)
    V, mu, sd = random_model(rng, 12, 4)
    q = upload(ctx, sp.csr_matrix((0, 30)), 1)
    assert q.n_obs() == 0
    out = transform(PcaModel.from_parts(ctx, V, mu, sd), q, np.arange(12, dtype=np.uint64), 1e4, 3)
    assert out.shape == (0, 4)


def test_errors(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing.dim_red import PcaModel
    lib = F.lib()
    rng = np.random.default_rng(9)
    V, mu, sd = random_model(rng, 6, 2)
    q = upload(ctx, counts(rng, 20, 10, 0.3), 1)
    model = PcaModel.from_parts(ctx, V, mu, sd)                   # no sel
    out = np.zeros((20, 2))
    feat = np.arange(6, dtype=np.uint64)

    def rc_transform(p, m, f):
        return lib.srx_pca_transform(p, m, F.ptr(f), 0.0, 0, F.ptr(out))
    assert rc_transform(None, q.x().handle, feat) == F.E_ARG
    assert rc_transform(model.handle, None, feat) == F.E_ARG
    assert rc_transform(model.handle, q.x().handle, None) == F.E_ARG              # feat NULL, model without sel
    dup = feat.copy()
    dup[4] = dup[1]
    assert rc_transform(model.handle, q.x().handle, dup) == F.E_ARG
    oob = feat.copy()
    oob[2] = 10
    assert rc_transform(model.handle, q.x().handle, oob) == F.E_BOUNDS
    assert rc_transform(model.handle, q.x().handle, feat) == F.OK
    other = sr.Context(0)
    q2 = upload(other, counts(rng, 20, 10, 0.3), 1)
    assert rc_transform(model.handle, q2.x().handle, feat) == F.E_ARG             # different contexts

    def rc_create(k, n_pc, comps, m_, s_):
        h = C.c_void_p()
        rc = lib.srx_pca_model_create(ctx.handle, k, n_pc, F.ptr(comps), F.ptr(m_), F.ptr(s_), None, 1, 1, C.byref(h))
        if rc == F.OK:
            lib.srx_pca_model_free(h)
        return rc
    Vc = np.ascontiguousarray(V)
    assert rc_create(6, 2, Vc, mu, sd) == F.OK
    assert rc_create(0, 2, Vc, mu, sd) == F.E_ARG
    assert rc_create(6, 0, Vc, mu, sd) == F.E_ARG
    for bad in (-1.0, np.inf, np.nan):
        s2 = sd.copy()
        s2[1] = bad
        assert rc_create(6, 2, Vc, mu, s2) == F.E_ARG
    V2 = Vc.copy()
    V2[2, 1] = np.nan
    assert rc_create(6, 2, V2, mu, sd) == F.E_ARG
    m2 = mu.copy()
    m2[0] = np.nan
    assert rc_create(6, 2, Vc, m2, sd) == F.E_ARG
    h = C.c_void_p()
    assert lib.srx_pca_model_from_result(q.x().handle, C.byref(h)) == F.E_ARG        # nothing fitted on q
    q2.x().free()
    other.close()


def test_transform_leaves_the_fitted_result_alone(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory import processing
    from singlerust_amd.memory.processing import dim_red
    from singlerust_amd.memory.processing.dim_red import PcaModel
    lib = F.lib()
    rng = np.random.default_rng(41)
    x = counts(rng, 500, 300, 0.1)
    a = upload(ctx, x, 1)
    other = upload(ctx, counts(rng, 250, 300, 0.1), 1)
    processing.normalize_total_inplace(a, 1e4, sr.Direction.Row)
    processing.log1p_transform_inplace(a)
    sel = np.arange(0, 300, 2, dtype=np.uint64)
    opts = F.PcaOpts(6, -1, -1, -1, 0, 0, 0, 0.0, 0)
    F.check(lib.srx_pca(a.x().handle, F.ptr(sel), len(sel), C.byref(opts), None, None, None, None, None, None), ctx.handle)
    before = np.zeros((500, 6))
    F.check(lib.srx_result_fetch(a.x().handle, F.ptr(before), None, None, None, None, None), ctx.handle)
    model = PcaModel.from_result(a)
    dim_red.pca_transform(other, model, target_sum=1e4, log1p=True)
    self_scores = dim_red.pca_transform(a, model)
    after, comps, mean, std, hv = np.zeros((500, 6)), np.zeros((150, 6)), np.zeros(150), np.zeros(150), np.zeros(150, np.uint64)
    F.check(lib.srx_result_fetch(a.x().handle, F.ptr(after), F.ptr(comps), None, F.ptr(mean), F.ptr(std), F.ptr(hv)), ctx.handle)
    assert np.array_equal(before, after)
    assert np.array_equal(hv, sel) and np.array_equal(model.info()[2], sel)
    assert comp_err(self_scores, after) <= 1e-6
    y = sp.csr_matrix((a.x_values(np.float64), x.indices, x.indptr), shape=x.shape)
    assert comp_err(after, restate(y, comps, mean, std, 1, 1, sel)) <= 1e-5


def test_no_interference_with_the_pipeline(ctx):
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import dim_red
    from singlerust_amd.memory.processing.dim_red import PcaModel
    lib = F.lib()
    rng = np.random.default_rng(77)
    x = counts(rng, 3000, 1500, 0.05)
    raw = upload(ctx, x, 1)

    def run():
        c = raw.deep_clone()
        opts = F.PcaOpts(20, -1, -1, -1, 0, 0, 0, 0.0, 5)
        res = F.PipelineResult()
        F.check(lib.srx_pipeline(c.x().handle, 1e4, 300, C.byref(opts), C.byref(res)), ctx.handle)
        s, v, hv = np.zeros((3000, 20)), np.zeros((300, 20)), np.zeros(300, np.uint64)
        F.check(lib.srx_result_fetch(c.x().handle, F.ptr(s), F.ptr(v), None, None, None, F.ptr(hv)), ctx.handle)
        return c, s, v, hv
    c1, s1, v1, h1 = run()
    model = PcaModel.from_result(c1)
    wide = upload(ctx, counts(rng, 5000, 2500, 0.05), 2)        # larger than the fit: every scratch buffer of the path regrows
    feat = rng.permutation(2500)[:300].astype(np.uint64)
    dim_red.pca_transform(wide, model, feat, target_sum=1e4, log1p=True)
    dim_red.pca_transform(raw, model, target_sum=1e4, log1p=True)
    dim_red.pca_transform(c1, model)
    _, s2, v2, h2 = run()
    assert np.array_equal(h1, h2) and np.array_equal(s1, s2)
    # (the components of two plain pipeline runs already differ in the last bits — ~1e-14 — the scores do not)
    assert np.abs(v1 - v2).max() <= 1e-12


def test_full_size_raw_transform(ctx):
    """c3 shape (1.3M x 28k, f32): the model of a pipeline step applied to a raw clone with normalise + log1p on the fly."""
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import dim_red
    from singlerust_amd.memory.processing.dim_red import PcaModel
    lib = F.lib()
    n, g = 1_300_000, 28_000
    p = F.SynthParams()
    lib.srx_synth_defaults(C.byref(p), 3003, n, g, 0.03)
    h = C.c_void_p()
    F.check(lib.srx_synth_generate(ctx.handle, C.byref(p), 0, n, F.F32, F.STORE_F32, C.byref(h)), ctx.handle)
    raw = sr.IMAnnData(sr.DeviceCsr(ctx, h), None, None, [], [])
    A = sr.IMAnnData(raw.x().clone(), None, None, [], [])
    opts = F.PcaOpts(50, -1, -1, -1, 0, 0, 0, 0.0, 12345)
    res = F.PipelineResult()
    F.check(lib.srx_pipeline(A.x().handle, 1e4, 2000, C.byref(opts), C.byref(res)), ctx.handle)
    want = np.zeros((n, 50))
    F.check(lib.srx_result_fetch(A.x().handle, F.ptr(want), None, None, None, None, None), ctx.handle)
    model = PcaModel.from_result(A)
    A.x().free()
    B = sr.IMAnnData(raw.x().clone(), None, None, [], [])
    got = dim_red.pca_transform(B, model, target_sum=1e4, log1p=True)
    assert comp_err(got, want) <= 1e-5
    assert np.array_equal(B.x_values(np.float32), raw.x_values(np.float32))
    B.x().free()
    raw.x().free()

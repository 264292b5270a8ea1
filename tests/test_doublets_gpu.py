"""Doublet detection on the device (srx_doublets_*) against the section "Doublet detection" of include/srx.h restated in
tests/doublets_ref.py: the synthetic matrix bit for bit, the scores of a list within the rounding of their twenty operations, the
chain decision for decision (parents, points, neighbours, scores, threshold, calls), the other transform routes and every refusal.

Not compared: the `scrublet` package, scanpy and scikit-image (none is installed where this was written)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import doublets_ref as ref

pytestmark = pytest.mark.gpu

BOUND = {1: 1e-5, 2: 1e-10}              # storage -> bound of the projected points against numpy (test_pca_transform_gpu.py's)
SCORE_RTOL = 1e-14                       # fewer than twenty correctly rounded f64 operations of 1.1e-16 each
FLOAT = {1: np.float32, 2: np.float64}
N_GENES = 9000
LENGTHS = (0, 0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 9000)


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
def upload(ctx, x, store, dtype=np.float64):
    import singlerust_amd as sr
    x = x.tocsr()
    x.sort_indices()
    dev = sr.DeviceCsr.upload(ctx, x.shape[0], x.shape[1], x.indptr, x.indices, x.data.astype(dtype), store)
    return sr.IMAnnData(dev, x.indptr, x.indices, [f"c{i}" for i in range(x.shape[0])], [f"g{j}" for j in range(x.shape[1])])


def download(dev):
    """(info, indptr int64, indices int32, values in the storage type) of a device matrix."""
    from singlerust_amd import _ffi as F
    i = dev.info()
    indptr, indices = np.zeros(i.n_rows + 1, dtype=np.uint64), np.zeros(i.nnz, dtype=np.uint64)
    F.check(F.lib().srx_matrix_download_pattern(dev.handle, F.ptr(indptr), F.ptr(indices) if i.nnz else None), dev.ctx.handle)
    return i, indptr.astype(np.int64), indices.astype(np.int32), dev.values(FLOAT[i.store])


def as_adata(dev):
    import singlerust_amd as sr
    i = dev.info()
    return sr.IMAnnData._from_device(dev, [f"s{r}" for r in range(i.n_rows)], [f"g{j}" for j in range(i.n_cols)])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_neighbours(pts, knn, label):
    """The device list against the brute force under the (distance, index) rule.  Rows must be EQUAL except where the brute
    force itself cannot decide: the device adds each squared difference with a fused multiply-add (one rounding), numpy rounds
    the product first, and this data is full of near-copies (a synthetic row of a cell with itself lands within rounding of its
    parent; a parent pair drawn twice gives the same point twice).  Each evaluation of sum_j (q_j - r_j)^2 over d coordinates is
    within (d + 3) u of the exact sum (u = 2^-53: the difference, the product and the d - 1 additions), the square root halves
    that and adds its own u, so two evaluations of one distance differ by at most TOL = 2 (d + 5) u relative.  Where a row
    differs, every position must hold a point whose brute-force distance is within TOL of the brute force's at that position;
    exact copies of one point must stand in ascending index order."""
    n, d = pts.shape
    k = knn.shape[1]
    want, wd, dist = ref.knn_brute(pts, k)
    tol = 2.0 * (d + 5) * 2.0 ** -53
    rows = np.nonzero((knn != want).any(axis=1))[0]
    got_d = np.take_along_axis(dist, knn.astype(np.int64), axis=1)
    worst = 0.0
    for r in rows:
        gap = np.abs(got_d[r] - wd[r]) / np.maximum(wd[r], 1e-300)
        worst = max(worst, float(gap.max()))
        assert (gap <= tol).all(), (label, int(r), float(gap.max()))
        assert len(set(knn[r].tolist())) == k and r not in knn[r]
    same = (pts[knn[:, 1:].astype(np.int64)] == pts[knn[:, :-1].astype(np.int64)]).all(axis=2)      # consecutive exact copies
    assert (knn[:, 1:][same] > knn[:, :-1][same]).all()
    print("%s: %d of %d rows differ from the brute force, all inside near-ties (largest relative gap %.2e, allowed %.2e); %d exact-copy pairs in order"
          % (label, len(rows), n, worst, tol, int(same.sum())))


# ---- 1. the simulation, exact -------------------------------------------------------------------------------------------------------------
_EDGE = {}


def edge_pattern():
    """40 cells x 9000 genes: the named row lengths, an even / odd pair at two sizes, a row with row 10's pattern, a row nested
    in row 13, random lengths; and the parent pairs that cover every case of the two passes."""
    if "p" not in _EDGE:
        rng = np.random.default_rng(2024)
        rows = [np.sort(rng.choice(N_GENES, L, replace=False)) for L in LENGTHS]
        rows.append(np.arange(0, N_GENES, 2))                       # 18, 19: disjoint and long together (9000 > the switch-over)
        rows.append(np.arange(1, N_GENES, 2))
        rows.append(np.arange(0, 200, 2))                           # 20, 21: disjoint and short
        rows.append(np.arange(1, 200, 2))
        rows.append(rows[10].copy())                                # 22: row 10's pattern
        rows.append(rows[13][::3].copy())                           # 23: nested in row 13
        rows.append(rows[11].copy())                                # 24: row 11's pattern (the cancellation test negates it)
        while len(rows) < 40:
            rows.append(np.sort(rng.choice(N_GENES, int(rng.integers(1, 3000)), replace=False)))
        indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        indices = np.concatenate(rows).astype(np.int64)
        pairs = [(5, 5), (17, 17), (0, 0), (0, 1), (0, 9), (9, 0), (1, 17), (17, 1), (18, 19), (19, 18), (20, 21), (10, 22), (22, 10),
                 (13, 23), (23, 13), (16, 17), (17, 16), (11, 24),
                 # either side of the wave / workgroup switch-over at 8192 entries of both parents together
                 (14, 14), (13, 15), (15, 13), (14, 15), (15, 14), (15, 15), (16, 0), (16, 2), (2, 16), (16, 3)]
        pairs += [(17, j) for j in range(40)] + [(j, 17) for j in range(0, 40, 3)]
        pairs += [tuple(p) for p in rng.integers(0, 40, (40, 2))]
        _EDGE["p"] = (indptr, indices, np.array(pairs, dtype=np.uint64))
    return _EDGE["p"]


def edge_values(src):
    """The values of the edge matrix in the source type."""
    nnz = int(edge_pattern()[0][-1])
    rng = np.random.default_rng(7)
    if src == np.uint8:
        v = rng.integers(1, 256, nnz)
        v[rng.random(nnz) < 0.5] = 255                              # 255 + 255 must not wrap
    elif src == np.uint16:
        v = rng.integers(1, 65536, nnz)
    elif src == np.int32:
        v = rng.integers(-(1 << 22), 1 << 22, nnz)
        v[v == 0] = 1
    else:
        v = rng.standard_normal(nnz) * 100.0                        # full mantissas: a + b rounds
    return v.astype(src)


def edge_matrix(src):
    indptr, indices, _ = edge_pattern()
    return sp.csr_matrix((edge_values(src).astype(np.float64), indices, indptr), shape=(40, N_GENES))


def edge_expected(src, store):
    key = (np.dtype(src).name, store)
    if key not in _EDGE:
        x = edge_matrix(src)
        x.data = x.data.astype(src).astype(FLOAT[store]).astype(np.float64)     # what the upload stores
        _EDGE[key] = ref.simulate(x, edge_pattern()[2], FLOAT[store])
    return _EDGE[key]


def upload_edge(ctx, src, store):
    import singlerust_amd as sr
    indptr, indices, _ = edge_pattern()
    dev = sr.DeviceCsr.upload(ctx, 40, N_GENES, indptr, indices, edge_values(src), store)
    return sr.IMAnnData(dev, indptr.astype(np.uint64), indices.astype(np.uint64), [f"c{i}" for i in range(40)], [f"g{j}" for j in range(N_GENES)])


@pytest.mark.parametrize("src,store", [(np.uint8, 1), (np.uint8, 2), (np.uint16, 1), (np.int32, 2), (np.float32, 1), (np.float32, 2),
                                       (np.float64, 1), (np.float64, 2)])
def test_simulation_equals_the_union_add(ctx, src, store):
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import simulate_doublets
    a = upload_edge(ctx, src, store)
    pairs = edge_pattern()[2]
    sim, used = simulate_doublets(a, parents=pairs)
    info, indptr, indices, values = download(sim)
    w_indptr, w_indices, w_values = edge_expected(src, store)
    assert (info.n_rows, info.n_cols, info.nnz) == (len(pairs), N_GENES, int(w_indptr[-1]))
    assert info.store == store and info.dtype == (F.F32 if store == 1 else F.F64)
    assert np.array_equal(used, pairs)
    assert np.array_equal(indptr, w_indptr) and np.array_equal(indices, w_indices)
    assert same_bits(values, w_values)
    if src == np.uint8:
        assert values.max() == 510.0
    # a second call gives the same bits
    sim2, _ = simulate_doublets(a, parents=pairs)
    _, indptr2, indices2, values2 = download(sim2)
    assert same_bits(indptr2, indptr) and same_bits(indices2, indices) and same_bits(values2, values)


@pytest.mark.parametrize("store", [1, 2])
def test_exact_cancellation_keeps_its_entry(ctx, store):
    from singlerust_amd.memory.processing import simulate_doublets
    x = edge_matrix(np.float32)
    indptr = edge_pattern()[0]
    x.data[indptr[24]:indptr[25]] = -x.data[indptr[11]:indptr[12]]            # row 24 = -row 11 on the same pattern
    a = upload(ctx, x, store)
    sim, _ = simulate_doublets(a, parents=[(11, 24), (24, 11), (11, 11)])
    info, ip, ix, v = download(sim)
    assert ip.tolist() == [0, 1024, 2048, 3072] and np.array_equal(ix[:1024], x.indices[indptr[11]:indptr[12]])
    assert (v[:2048] == 0.0).all() and (v[2048:] != 0.0).all()


@pytest.mark.parametrize("store", [1, 2])
def test_simulated_matrix_is_a_working_matrix(ctx, store):
    import singlerust_amd as sr
    from singlerust_amd.memory import processing, statistics
    a = upload_edge(ctx, np.uint16, store)
    pairs = edge_pattern()[2].astype(np.int64)
    sim, _ = processing.simulate_doublets(a, parents=pairs)
    s = as_adata(sim)
    row_sum = statistics.compute_sum(a, sr.Direction.Row)
    assert np.array_equal(statistics.compute_sum(s, sr.Direction.Row), row_sum[pairs[:, 0]] + row_sum[pairs[:, 1]])     # integers: exact
    assert np.array_equal(statistics.compute_number(s, sr.Direction.Row), np.diff(edge_expected(np.uint16, store)[0]))
    s.x().prepare()
    sums = processing.normalize_log1p_inplace(s, 1e4)
    assert np.array_equal(sums, row_sum[pairs[:, 0]] + row_sum[pairs[:, 1]])
    v = s.x_values(np.float64)
    assert np.isfinite(v).all() and v.max() > 0


@pytest.mark.parametrize("n", [1, 2, 40])
@pytest.mark.parametrize("seed", [0, 0xDEADBEEFCAFEF00D])
def test_hashed_parents(ctx, n, seed):
    from singlerust_amd.memory.processing import simulate_doublets
    x = edge_matrix(np.float32)[:n]
    a = upload(ctx, x, 1)
    sim, used = simulate_doublets(a, n_sim=37, seed=seed)
    want = ref.parents(n, 37, seed)
    assert np.array_equal(used, want)
    _, indptr, indices, values = download(sim)
    w = ref.simulate(sp.csr_matrix((x.data.astype(np.float32).astype(np.float64), x.indices, x.indptr), shape=x.shape), want, np.float32)
    assert np.array_equal(indptr, w[0]) and np.array_equal(indices, w[1]) and same_bits(values, w[2])


def test_no_synthetic_rows_gives_an_empty_matrix(ctx):
    from singlerust_amd.memory.processing import simulate_doublets
    a = upload_edge(ctx, np.float32, 1)
    sim, used = simulate_doublets(a, n_sim=0)
    info, indptr, indices, values = download(sim)
    assert (info.n_rows, info.n_cols, info.nnz) == (0, N_GENES, 0) and indptr.tolist() == [0] and used.shape == (0, 2)


# ---- 2. scores from a list ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sim", [1, 100])
@pytest.mark.parametrize("k_adj", [1, 7, 64])
def test_scores_of_a_list(ctx, n_sim, k_adj):
    from singlerust_amd.memory.processing import doublet_scores_knn
    n_obs = 50
    rng = np.random.default_rng(10 * n_sim + k_adj)
    idx = rng.integers(0, n_obs + n_sim, (n_obs + n_sim, k_adj)).astype(np.uint32)
    idx[0] = 0                                                      # k_d = 0
    idx[1] = n_obs                                                  # k_d = k_adj
    idx[n_obs] = n_obs + n_sim - 1
    for rho, se_rho in ((0.05, 0.02), (0.3, 0.0)):
        Ld, se = doublet_scores_knn(ctx, idx, n_obs, rho, se_rho)
        wL, ws = ref.scores(idx, n_obs, rho, se_rho, n_sim / n_obs)
        eL, es = float(np.abs(Ld / wL - 1).max()), float(np.abs(se / ws - 1).max())
        print("n_sim %d k_adj %d rho %g: Ld %.2e se %.2e" % (n_sim, k_adj, rho, eL, es))
        assert eL <= SCORE_RTOL and es <= SCORE_RTOL and (Ld > 0).all() and (se > 0).all()


# ---- 3. the chain, decision for decision --------------------------------------------------------------------------------------------------
_CHAIN = {}
TABLES = ("scores_obs", "scores_sim", "se_obs", "se_sim", "z", "predicted", "points", "parents", "knn")


def fit(ctx, x, store, bits=3, n_hvg=120, n_pc=10):
    """(counts, fitted): the raw counts on the device and a clone with the transform applied and a PCA result."""
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory import processing
    counts = upload(ctx, x, store)
    fitted = counts.deep_clone()
    if bits == 3:
        opts, res = F.PcaOpts(n_pc, -1, -1, -1, 0, 0, 0, 0.0, 1), F.PipelineResult()
        F.check(F.lib().srx_pipeline(fitted.x().handle, 1e4, n_hvg, C.byref(opts), C.byref(res)), ctx.handle)
    else:
        if bits & 1:
            processing.normalize_total_inplace(fitted, 1e4, sr.Direction.Row)
        if bits & 2:
            processing.log1p_transform_inplace(fitted)
        processing.dim_red.pca_inplace(fitted, n_pc, None, None, None, sr.FeatureSelection.HighlyVariable(n_hvg), None)
    return counts, fitted


def result_of(fitted, n_pc=10):
    """(scores, components, mean, std, selection) the fit left on the device."""
    from singlerust_amd import _ffi as F
    n, k = fitted.n_obs(), 120
    scores, comps, evr = np.zeros((n, n_pc)), np.zeros((k, n_pc)), np.zeros(n_pc)
    mean, std, sel = np.zeros(k), np.zeros(k), np.zeros(k, dtype=np.uint64)
    F.check(F.lib().srx_result_fetch(fitted.x().handle, F.ptr(scores), F.ptr(comps), F.ptr(evr), F.ptr(mean), F.ptr(std), F.ptr(sel)),
            fitted.x().ctx.handle)
    return scores, comps, mean, std, sel.astype(np.int64)


def chain(ctx, seed, store):
    if (seed, store) not in _CHAIN:
        from singlerust_amd.memory.processing import scrublet
        x, flags = ref.planted(seed)
        counts, fitted = fit(ctx, x, store)
        d = scrublet(fitted, counts, target_sum=1e4, log1p=True, sim_ratio=2.0, k=11, seed=seed + 5)
        _CHAIN[(seed, store)] = dict(x=x, flags=flags, counts=counts, fitted=fitted, d=d, info=d.info(), t={w: d.fetch(w) for w in TABLES})
    return _CHAIN[(seed, store)]


CHAINS = [(0, 1), (0, 2), (3, 1), (3, 2)]


@pytest.mark.parametrize("seed,store", CHAINS)
def test_chain_parents_and_points(ctx, seed, store):
    from singlerust_amd.memory.processing import dim_red, simulate_doublets
    c = chain(ctx, seed, store)
    i, t, x = c["info"], c["t"], c["x"]
    n = x.shape[0]
    assert (i["n_obs"], i["n_sim"], i["k"], i["k_adj"], i["d"]) == (n, 2 * n, 11, 33, 10)
    assert i["rows_certified"] + i["rows_recomputed"] == 3 * n
    assert np.array_equal(t["parents"], ref.parents(n, 2 * n, seed + 5))
    scores, V, mu, sd, sel = result_of(c["fitted"])
    assert same_bits(t["points"][:n], scores)
    sim, used = simulate_doublets(c["counts"], n_sim=2 * n, seed=seed + 5)
    assert np.array_equal(used, t["parents"]) and i["nnz_sim"] == sim.info().nnz
    model = dim_red.PcaModel.from_result(c["fitted"])
    assert same_bits(t["points"][n:], dim_red.pca_transform(as_adata(sim), model, target_sum=1e4, log1p=True))
    ip, ix, dv = ref.simulate(x, t["parents"], np.float64)
    want = ref.project(sp.csr_matrix((dv, ix, ip), shape=(2 * n, x.shape[1])), sel, V, mu, sd)
    err = float((np.abs(t["points"][n:] - want).max(axis=0) / np.abs(want).max(axis=0)).max())
    print("seed %d store %d: projected points against numpy %.3e (bound %.0e)" % (seed, store, err, BOUND[store]))
    assert err <= BOUND[store]
    # the observed cells among the handle's own obs annotations
    assert np.array_equal(c["counts"].obs["doublet_score"], t["scores_obs"]) and np.array_equal(c["counts"].obs["predicted_doublet"], t["predicted"])


@pytest.mark.parametrize("seed,store", CHAINS)
def test_chain_neighbours(ctx, seed, store):
    from singlerust_amd.memory.processing import knn_points
    c = chain(ctx, seed, store)
    pts, knn = c["t"]["points"], c["t"]["knn"]
    assert knn.shape == (pts.shape[0], 33)
    got = knn_points(ctx, pts, k=33)[0]
    assert np.array_equal(knn, got)
    check_neighbours(pts, knn, "seed %d store %d" % (seed, store))


@pytest.mark.parametrize("seed,store", CHAINS)
def test_chain_scores_threshold_and_calls(ctx, seed, store):
    from singlerust_amd.memory.processing import doublets_threshold
    c = chain(ctx, seed, store)
    i, t, d = c["info"], c["t"], c["d"]
    n = i["n_obs"]
    wL, ws = ref.scores(t["knn"], n, 0.05, 0.02, 2.0)
    for name, got, want in (("Ld", np.concatenate([t["scores_obs"], t["scores_sim"]]), wL), ("se", np.concatenate([t["se_obs"], t["se_sim"]]), ws)):
        err = float(np.abs(got / want - 1).max())
        print("seed %d store %d: %s %.2e" % (seed, store, name, err))
        assert err <= SCORE_RTOL
    thr, found, rounds = doublets_threshold(t["scores_sim"])
    assert found and i["threshold_found"] == 1 and i["smooth_rounds"] == rounds and i["threshold"] == thr
    assert (thr, int(found), rounds) == ref.threshold(t["scores_sim"])

    def follows(info, tables, thr):
        pred, z, det, frac, overall = ref.call(t["scores_obs"], t["se_obs"], t["scores_sim"], thr)
        assert np.array_equal(tables["predicted"], pred) and same_bits(tables["z"], z)
        assert info["n_predicted"] == int(pred.sum())
        assert (info["detected_rate"], info["detectable_fraction"], info["overall_rate"]) == (det, frac, overall)
    follows(i, t, thr)
    # re-calling: a given threshold, then the automatic one again
    given = float(np.median(t["scores_obs"])) + 1e-3
    j = d.call(given)
    assert j["threshold"] == given and j["threshold_found"] == 0 and j["smooth_rounds"] == 0 and j == d.info()
    follows(j, {w: d.fetch(w) for w in ("predicted", "z")}, given)
    assert j["n_predicted"] != i["n_predicted"]
    back = d.call(0.0)
    assert {k: v for k, v in back.items() if not k.startswith("ms_")} == {k: v for k, v in i.items() if not k.startswith("ms_")}
    assert same_bits(d.fetch("z"), t["z"]) and np.array_equal(d.fetch("predicted"), t["predicted"])


@pytest.mark.parametrize("seed,store", CHAINS)
def test_chain_quality_and_repeatability(ctx, seed, store):
    from singlerust_amd.memory.processing import scrublet
    c = chain(ctx, seed, store)
    t, flags = c["t"], c["flags"]
    a = ref.auc(t["scores_obs"], flags)
    fp = float((t["predicted"] & ~flags).sum()) / float((~flags).sum())
    print("seed %d store %d: AUC %.4f, threshold %.4f after %d rounds, singlets above %.4f, planted above %d of %d"
          % (seed, store, a, c["info"]["threshold"], c["info"]["smooth_rounds"], fp, int((t["predicted"] & flags).sum()), int(flags.sum())))
    assert a >= 0.98 and fp <= 0.01
    d2 = scrublet(c["fitted"], c["counts"], target_sum=1e4, log1p=True, sim_ratio=2.0, k=11, seed=seed + 5)
    for w in TABLES:
        assert same_bits(d2.fetch(w), t[w]), w
    d2.free()


# ---- 4. other routes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [0, 1, 2])
def test_other_transforms_project_as_pca_transform(ctx, bits):
    from singlerust_amd.memory.processing import dim_red, scrublet, simulate_doublets
    x, _ = ref.planted(1, n=200)
    counts, fitted = fit(ctx, x, 2, bits=bits)
    kw = dict(target_sum=1e4 if bits & 1 else None, log1p=bool(bits & 2))
    d = scrublet(fitted, counts, sim_ratio=1.5, k=8, seed=3, **kw)
    i = d.info()
    assert (i["n_sim"], i["k_adj"]) == (300, 20)
    sim, _ = simulate_doublets(counts, n_sim=300, seed=3)
    pts = d.fetch("points")
    assert same_bits(pts[:200], result_of(fitted)[0])
    assert same_bits(pts[200:], dim_red.pca_transform(as_adata(sim), dim_red.PcaModel.from_result(fitted), **kw))


def test_leading_dimensions_alone(ctx):
    from singlerust_amd.memory.processing import scrublet
    x, _ = ref.planted(2, n=200)
    counts, fitted = fit(ctx, x, 1)
    full = scrublet(fitted, counts, target_sum=1e4, log1p=True, k=8)
    d = scrublet(fitted, counts, target_sum=1e4, log1p=True, k=8, n_dims=5)
    i = d.info()
    assert i["d"] == 5 and i["k"] == 8 and i["k_adj"] == 24 and full.info()["d"] == 10
    pts = d.fetch("points")
    assert pts.shape == (600, 5) and same_bits(pts, np.ascontiguousarray(full.fetch("points")[:, :5]))
    check_neighbours(pts, d.fetch("knn"), "n_dims 5")
    # the default k: round(0.5 sqrt(200)) = 7, k_adj = 21
    dflt = scrublet(fitted, counts, target_sum=1e4, log1p=True).info()
    assert (dflt["k"], dflt["k_adj"], dflt["n_sim"]) == (7, 21, 400)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import scrublet
    lib = F.lib()
    x, _ = ref.planted(4, n=100)
    counts, fitted = fit(ctx, x, 1)
    cm, fm = counts.x().handle, fitted.x().handle
    SENTINEL = 77
    h = C.c_void_p(SENTINEL)

    def refused(rc, code=F.E_ARG, c=ctx):
        assert rc == code, rc
        msg = lib.srx_last_error(c.handle).decode()
        assert msg
        return msg

    def result(f=fm, c=cm, **kw):
        o = F.DoubletOpts(kw.get("sim_ratio", 0.0), kw.get("expected_rate", 0.0), kw.get("stdev_rate", 0.0), 1e4, kw.get("threshold", 0.0), 0,
                          kw.get("k", 5), kw.get("n_dims", 0), kw.get("transform", 3), 0)
        return lib.srx_doublets_result(f, c, C.byref(o), C.byref(h), None)

    # null arguments
    assert lib.srx_doublets_result(None, cm, None, C.byref(h), None) == F.E_ARG
    assert lib.srx_doublets_result(fm, None, None, C.byref(h), None) == F.E_ARG
    refused(lib.srx_doublets_result(fm, cm, None, None, None))
    refused(lib.srx_doublets_simulate(cm, 3, 0, None, None, None))
    idx = np.zeros((4, 2), dtype=np.uint32)
    refused(lib.srx_doublet_scores_knn(ctx.handle, None, 2, 2, 2, 0.05, 0.02, None, None))
    # CSC counts; fitted without a result; shapes that differ
    csc = counts.x().to_csc()
    assert "CSC" in refused(result(c=csc.handle))
    assert "CSC" in refused(lib.srx_doublets_simulate(csc.handle, 3, 0, None, C.byref(h), None))
    assert "no PCA result" in refused(result(f=cm))
    fewer_cells = upload(ctx, x[:90], 1)
    fewer_genes = upload(ctx, x[:, :200], 1)
    refused(result(c=fewer_cells.x().handle))
    refused(result(c=fewer_genes.x().handle))
    # sizes
    empty = C.c_void_p()
    F.check(lib.srx_matrix_alloc(ctx.handle, 0, 240, 0, F.F32, F.STORE_F32, C.byref(empty)), ctx.handle)
    assert "no cells" in refused(lib.srx_doublets_simulate(empty, 3, 0, None, C.byref(h), None))
    lib.srx_matrix_free(empty)
    refused(result(sim_ratio=0.004))                                 # round(0.4) = 0 synthetic rows
    refused(lib.srx_doublets_simulate(cm, (1 << 32) - 100, 0, None, C.byref(h), None))
    refused(result(sim_ratio=5e7))
    # options
    for kw in (dict(sim_ratio=-1.0), dict(sim_ratio=float("inf")), dict(sim_ratio=float("nan")), dict(expected_rate=1.0), dict(expected_rate=-0.1),
               dict(expected_rate=float("nan")), dict(stdev_rate=-0.5), dict(transform=4), dict(transform=-1), dict(k=-1), dict(k=22),
               dict(k=5, sim_ratio=20.0), dict(n_dims=11), dict(threshold=-1.0)):
        refused(result(**kw))
    few = upload(ctx, x[:12], 1)                                     # 36 points: k_adj = 45 exceeds the 35 others
    few_fit = few.deep_clone()
    sr.memory.processing.dim_red.pca_inplace(few_fit, 3, None, None, None, sr.FeatureSelection.HighlyVariable(50), None)
    assert "other points" in refused(result(f=few_fit.x().handle, c=few.x().handle, k=15, transform=0))
    # given parents out of bounds
    par = np.array([[0, 1], [2, 100]], dtype=np.uint64)
    refused(lib.srx_doublets_simulate(cm, 2, 0, F.ptr(par), C.byref(h), None), F.E_BOUNDS)
    # the list form
    refused(lib.srx_doublet_scores_knn(ctx.handle, F.ptr(idx), 2, 2, 0, 0.05, 0.02, None, None))
    refused(lib.srx_doublet_scores_knn(ctx.handle, F.ptr(idx), 0, 4, 2, 0.05, 0.02, None, None))
    bad = idx.copy()
    bad[3, 1] = 4
    refused(lib.srx_doublet_scores_knn(ctx.handle, F.ptr(bad), 2, 2, 2, 0.05, 0.02, None, None))
    refused(lib.srx_doublet_scores_knn(ctx.handle, F.ptr(idx), 2, 2, 2, 0.0, 0.02, None, None))
    refused(lib.srx_doublet_scores_knn(ctx.handle, F.ptr(idx), 2, 2, 2, 0.05, -1.0, None, None))
    assert h.value == SENTINEL
    # a context with more than one rank
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    sharded = upload(c2, x, 1)
    assert "sharded" in refused(lib.srx_doublets_simulate(sharded.x().handle, 3, 0, None, C.byref(h), None), c=c2)
    refused(lib.srx_doublet_scores_knn(c2.handle, F.ptr(idx), 2, 2, 2, 0.05, 0.02, None, None), c=c2)
    assert h.value == SENTINEL
    # the context still works
    d = scrublet(fitted, counts, target_sum=1e4, log1p=True, k=5)
    i = d.info()
    assert (i["n_obs"], i["n_sim"], i["k_adj"]) == (100, 200, 15)
    refused(lib.srx_doublets_fetch(d.handle, 9, F.ptr(idx)))
    refused(lib.srx_doublets_fetch(d.handle, 0, None))
    refused(lib.srx_doublets_call(d.handle, -0.5, None))
    refused(lib.srx_doublets_call(d.handle, float("nan"), None))
    assert d.call(0.0)["threshold_found"] == i["threshold_found"]
    Ld, _ = sr.memory.processing.doublet_scores_knn(ctx, idx, 2)
    assert Ld.shape == (4,) and (Ld > 0).all()

"""srx_tsne_* on the device against the definition of include/srx.h (tests/tsne_ref.py): the affinities through both entries
(exact pattern and counters, bit symmetry, the entropy equation from the fetched beta, P element-wise at a per-row tolerance),
the forces (the three walk counters exactly: the same decisions; attr, rep and z within 32 D), positions after 1 and 3
iterations, determinism and stop_after, both deterministic starts, quality over a full run against the reference's own
seed-to-seed range (tests/golden/tsne_kat.json) and the refusals.

Tolerances.  P: both sides solve H = log u to 1e-9, so a row's p differs by at most 2e-9 max_j |dp_j / dH|; the test allows
five times that plus 1e-15 (tsne_ref.p_row_tolerance), the derivative taken from the reference; a row whose bound exceeds 1e-6
is checked through its entropy alone, and at most 1 % of a case's rows may be such rows (test_tsne_cpu.py shows that the named
inputs have none).  Forces and positions: D = max |f64 numpy - longdouble numpy| of the case, computed here on the CPU; the
device gets 32 D, the factor of the UMAP tests (its order of summation differs from numpy's).  The device's P is what the
reference iterates on, so that the comparison of positions is about the iteration alone.

A handle of n = 2 cannot exist (k >= 2 needs n >= 3: srx_neighbors_from_knn's own rule), so the smallest sizes are 1 and 3."""
import ctypes as C

import numpy as np
import pytest

import tsne_ref as ref

pytestmark = pytest.mark.gpu

TOL_FACTOR = 32


def P():
    from singlerust_amd.memory import processing
    return processing


_HANDLES = {}


def handle(ctx, n):
    """A Tsne handle over n generic points (k = 5, or 2 for n = 3; n = 1: the empty handle), built once, with its fetched P."""
    if n not in _HANDLES:
        if n == 1:
            t = P().tsne_affinities(ctx, np.zeros((1, 5), np.uint32), np.zeros((1, 5)), 2.0)
        else:
            k = 2 if n < 7 else 5
            idx, dist = ref.host_knn(np.random.default_rng(n).standard_normal((n, 4)), k)
            t = P().tsne_affinities(ctx, idx, dist, 1.5 if k == 2 else 2.5)
        _HANDLES[n] = (t, t.affinities()[:3])
    return _HANDLES[n]


# ---- affinities -----------------------------------------------------------------------------------------------------------------------
def check_affinities(t, idx, dist, u, name):
    want_P, want_beta, want, (cols, p, ci) = ref.affinities(idx, dist, u)
    info = t.info()
    indptr, indices, data, beta = t.affinities()
    for key in ("n", "k", "nnz", "n_mutual", "rows_no_root", "entries_dropped", "perplexity"):
        assert info[key] == want[key], (name, key, info[key], want[key])
    assert np.array_equal(indptr, want_P[0]) and np.array_equal(indices, want_P[1])            # the pattern, exactly
    n = info["n"]
    rows = np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))
    dense = np.zeros((n, n))
    dense[rows, indices] = data
    assert np.array_equal(dense.view(np.uint64), dense.T.copy().view(np.uint64))                 # bit-symmetric
    assert (data > 0).all() and all((np.diff(indices[int(a):int(b)].astype(np.int64)) > 0).all()
                                    for a, b in zip(indptr[:-1], indptr[1:]))
    # the entropy equation, evaluated here from the fetched beta
    root = ci["root"]
    assert np.array_equal(np.isinf(beta), ~root)
    logu = np.log(want["perplexity"])
    H = ref.row_entropy(ci["x"][root], beta[root])
    print("%s: n %d k %d nnz %d mutual %d no_root %d dropped %d | max |H - log u| %.3e"
          % (name, n, info["k"], info["nnz"], info["n_mutual"], info["rows_no_root"], info["entries_dropped"],
             float(np.abs(H - logu).max()) if H.size else 0.0))
    assert (np.abs(H - logu) <= 1e-9).all()
    # element-wise, at the per-row tolerance; ill-conditioned rows through the entropy alone
    tol = np.where(root, ref.p_row_tolerance(np.where(root, ci["bound"], 0.0)), 1e-15)
    out = tol > ref.P_ROW_CAP
    assert out.sum() <= 0.01 * n, (name, int(out.sum()))
    pair_tol = (tol[rows] + tol[indices]) / (2.0 * n) + 1e-18
    good = ~(out[rows] | out[indices])
    err = np.abs(data - want_P[2])
    print("%s: max |P - ref| %.3e, max of its bound %.3e, rows out %d" % (name, float(err[good].max()), float(pair_tol[good].max()),
                                                                         int(out.sum())))
    assert (err[good] <= pair_tol[good]).all()
    return indptr, indices, data, beta


@pytest.mark.parametrize("name", ref.AFFINITY_CASES)
def test_affinities_both_entries(ctx, name):
    from singlerust_amd import _ffi as F
    idx, dist, u = ref.affinity_case(name)
    t = P().tsne_affinities(ctx, idx, dist, u)
    got = check_affinities(t, idx, dist, u, name)
    # a graph handle made from the list: its resident D, read where it lies; the graph is left untouched
    g = P().connectivities_from_knn(ctx, idx, dist)
    before = g.fetch(F.GRAPH_DISTANCES) + g.fetch(F.GRAPH_CONNECTIVITIES)
    t2 = P().tsne_affinities_graph(g, u)
    got2 = check_affinities(t2, idx, dist, u, name + " (graph)")
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, got2))
    after = g.fetch(F.GRAPH_DISTANCES) + g.fetch(F.GRAPH_CONNECTIVITIES)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, after))
    # the same bytes from a second call
    again = P().tsne_affinities(ctx, idx, dist, u).affinities()
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, again))
    if name == "edges":
        i = t.info()
        assert i["rows_no_root"] == 4 and i["entries_dropped"] > 0 and 2 * i["n_mutual"] < i["n"] * i["k"]     # pairs joined one way
        sh = ref.affinity_case("edges_shuffled")
        other = P().tsne_affinities(ctx, *sh).affinities()
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, other))             # the order within a row


def test_affinities_of_no_and_one_point(ctx):
    for n in (0, 1):
        t = P().tsne_affinities(ctx, np.zeros((n, 5), np.uint32), np.zeros((n, 5)), 2.0)
        i = t.info()
        indptr, indices, data, beta = t.affinities()
        assert (i["n"], i["k"], i["nnz"], i["n_mutual"], i["rows_no_root"], i["entries_dropped"]) == (n, 5, 0, 0, 0, 0)
        assert indptr.tolist() == [0] * (n + 1) and indices.size == 0 and data.size == 0 and beta.size == n
        y0 = np.array([[0.5, -2.0]])[:n]
        emb, info = P().tsne_run(t, init=y0, n_iter=4)
        assert np.array_equal(emb, y0) and info["iters_run"] == 0 and info["n"] == n                          # the start is returned
        assert np.array_equal(P().tsne_embedding(t), y0)
        attr, rep, z, fi = P().tsne_forces(t, y0)
        assert not attr.any() and not rep.any() and not z.any() and fi["pairs_exact"] == 0
    g = P().connectivities_from_knn(ctx, np.zeros((0, 5), np.uint32), np.zeros((0, 5)))
    assert P().tsne_affinities_graph(g, 2.0).info()["n"] == 0


# ---- forces -----------------------------------------------------------------------------------------------------------------------------
def check_forces(ctx, n, Y, theta, levels, name):
    t, Pm = handle(ctx, n)
    L = levels or ref.auto_levels(n)
    rep, z, Z, want = ref.repulsion(Y, theta, L)
    repl, zl, Zl, wantl = ref.repulsion(Y, theta, L, np.longdouble)
    attr, attrl = ref.attraction(Pm, Y), ref.attraction(Pm, Y, np.longdouble)
    assert all(want[c] == wantl[c] for c in ref.COUNTERS)
    D = float(max(np.abs(rep - repl).max(), np.abs(z - zl).max(), np.abs(attr - attrl).max()))
    a, r, zz, fi = P().tsne_forces(t, Y, theta, levels)
    err = float(max(np.abs(a - attr).max(), np.abs(r - rep).max(), np.abs(zz - z).max()))
    print("%s n %d theta %g L %d: accepted %d exact %d pairs %d | D %.3e 32D %.3e device %.3e"
          % (name, n, theta, L, fi["cells_accepted"], fi["cells_exact"], fi["pairs_exact"], D, TOL_FACTOR * D, err))
    for c in ref.COUNTERS:
        assert fi[c] == want[c], (name, n, theta, L, c, fi[c], want[c])                                       # the same decisions
    assert fi["levels"] == L and fi["side"] == want["side"] and fi["lo"] == want["lo"]
    assert err <= TOL_FACTOR * D
    return D


@pytest.mark.parametrize("n", [1, 3, 65, 257, 1025])
def test_forces_theta_levels(ctx, n):
    Y = ref.force_layout("generic", n)
    for theta in (0.0, 0.5, 8.0):
        for levels in (1, 2, 0, 12):
            check_forces(ctx, n, Y, theta, levels, "generic")
    if n > 1:
        r0, z0, _, i0 = ref.repulsion(Y, 0.0, 1)
        assert i0["cells_accepted"] == 0 and i0["pairs_exact"] == n * (n - 1)                                 # theta = 0: every pair


@pytest.mark.parametrize("name", ref.FORCE_LAYOUTS)
def test_forces_edge_layouts(ctx, name):
    n = 257
    Y = ref.force_layout(name, n)
    if name == "boundaries":
        _, side, U, _ = ref.pyramid(Y, 12)
        assert side == 2.0 ** 20 + 1.0 and (U[3:] % np.uint64(2 ** 20) == 0).all() and (U[3] == 2 ** 31).all()     # on the edges
        assert int(U.max()) == int(U[1, 0]) == int(U[1, 1]) == int(U[2, 1]) < 2 ** 32 and int(U.min()) == 0       # the maximum
    if name == "clump70":
        code = ref.pyramid(Y, 12)[3][12]["code_of"]
        assert (code[40:110] == code[40]).all()
    for theta in (0.0, 0.5):
        for levels in (0, 12):
            check_forces(ctx, n, Y, theta, levels, name)
    if name == "coincident":
        a, r, z, fi = P().tsne_forces(handle(ctx, n)[0], Y, 0.5, 0)
        assert fi["side"] == 1.0 and not r.any() and (z == n - 1).all() and fi["pairs_exact"] == n * (n - 1)


# ---- iterations ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ex_iters", [0, 2])
def test_positions_after_1_and_3_iterations(ctx, ex_iters):
    n = 257
    t, Pm = handle(ctx, n)
    y0 = ref.random_start(n, 4242)
    for n_iter, stop in ((1000, 1), (1000, 3), (3, 0)):
        Y, want, _ = ref.layout(Pm, y0, n_iter, exaggeration_iters=ex_iters, stop_after=stop)
        Yl, wantl, _ = ref.layout(Pm, y0, n_iter, exaggeration_iters=ex_iters, stop_after=stop, dtype=np.longdouble)
        assert all(want[c] == wantl[c] for c in ref.COUNTERS)
        D = float(np.abs(Y - Yl).max())
        emb, info = P().tsne_run(t, init=y0, n_iter=n_iter, exaggeration_iters=ex_iters, stop_after=stop)
        err = float(np.abs(emb - Y).max())
        print("iterations ex %d T %d stop %d: D %.3e 32D %.3e device %.3e max|y| %.3e | Z %.6e kl %.6e (ref %.6e %.6e)"
              % (ex_iters, n_iter, stop, D, TOL_FACTOR * D, err, float(np.abs(Y).max()), info["Z"], info["kl"], want["Z"], want["kl"]))
        assert err <= TOL_FACTOR * D
        # the walk of iteration 1 reads the start itself: the same decisions, exactly
        for key in (ref.COUNTERS if (stop or n_iter) == 1 else ()) + ("n", "n_iter", "iters_run", "levels", "eta"):
            assert info[key] == want[key], (key, info[key], want[key])
        assert abs(info["side"] - want["side"]) <= 1e-9 * want["side"]
        assert abs(info["Z"] - want["Z"]) <= 1e-9 * want["Z"] and abs(info["kl"] - want["kl"]) <= 1e-9 * abs(want["kl"]) + 1e-12
        assert np.array_equal(P().tsne_embedding(t).view(np.uint64), emb.view(np.uint64))                    # the fetch
    assert want["eta"] == 50.0


def test_determinism_and_stop_after(ctx):
    n = 257
    t, _ = handle(ctx, n)
    a, ia = P().tsne_run(t, init="random", seed=5, n_iter=1000, stop_after=6, exaggeration_iters=3)
    b, ib = P().tsne_run(t, init="random", seed=5, n_iter=1000, stop_after=6, exaggeration_iters=3)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert {k: v for k, v in ia.items() if k != "ms"} == {k: v for k, v in ib.items() if k != "ms"}
    full, _ = P().tsne_run(t, init="random", seed=5, n_iter=6, exaggeration_iters=3)
    assert np.array_equal(a.view(np.uint64), full.view(np.uint64))                                           # the first 6 of 1000
    other, _ = P().tsne_run(t, init="random", seed=6, n_iter=6, exaggeration_iters=3)
    assert not np.array_equal(a, other)


# ---- starts ---------------------------------------------------------------------------------------------------------------------------------
def test_hashed_start_is_the_stated_hash(ctx):
    """A learning rate of 1e-300 moves nothing (y + vel == y in f64), so one iteration returns the start itself."""
    t, _ = handle(ctx, 65)
    for seed in (0, 9, 2 ** 64 - 1):
        emb, _ = P().tsne_run(t, init="random", seed=seed, n_iter=1, learning_rate=1e-300)
        assert np.array_equal(emb.view(np.uint64), ref.random_start(65, seed).view(np.uint64))
        assert (np.abs(emb) <= 1e-4).all()


def test_pca_start_and_the_resident_path(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import dim_red, neighbors, tsne
    from test_knn_gpu import _planted, _upload
    a = _upload(ctx, _planted())
    with pytest.raises(sr.SrxError):
        tsne(a)                                                                      # no graph yet
    dim_red.pca_inplace(a, 20, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    neighbors(a, n_neighbors=15, connectivities=True)
    scores = a.obsm["X_pca"].copy()
    before = a._graph.fetch(F.GRAPH_DISTANCES)
    tsne(a, n_iter=1, learning_rate=1e-300)
    y0 = ref.pca_start(scores)
    assert np.array_equal(a.obsm["X_tsne"].view(np.uint64), y0.view(np.uint64)) and abs(np.abs(y0).max() - 1e-4) < 1e-18
    info = tsne(a, n_iter=20, key_added="X_tsne20")
    assert info["iters_run"] == 20 and np.isfinite(a.obsm["X_tsne20"]).all() and a.uns["tsne"]["affinities"]["perplexity"] == 5.0
    # the same bits from the caller's list and the start computed on the host
    idx, dist = before[1].reshape(-1, 15), before[2].reshape(-1, 15)
    t = P().tsne_affinities(ctx, idx, dist)
    emb, i2 = P().tsne_run(t, init=y0, n_iter=20)
    assert np.array_equal(emb.view(np.uint64), a.obsm["X_tsne20"].view(np.uint64))
    after = a._graph.fetch(F.GRAPH_DISTANCES)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(before, after))
    # NULL opts: every default with the PCA start
    dflt, di = np.zeros((a.n_obs(), 2)), F.TsneRunInfo()
    F.check(F.lib().srx_tsne_run(a._tsne.handle, a.x().handle, None, None, F.ptr(dflt), C.byref(di)), ctx.handle)
    assert di.n_iter == di.iters_run == 1000 and di.eta == 50.0 and np.isfinite(dflt).all() and di.kl > 0


# ---- quality --------------------------------------------------------------------------------------------------------------------------------
def test_quality_over_a_full_run(ctx):
    """600 points in six separated clumps in 10 dimensions, k = 30, u = 10, the default run from three hashed seeds: the exact
    KL and the label purity, both recomputed here densely from the fetched P and Y, lie inside the reference's own
    seed-to-seed range (five other seeds, theta = 0.5) widened by that range on both sides."""
    g = ref.golden()["quality"]
    x, labels = ref.clumps(g["n"], g["dim"], seed=g["data_seed"])
    idx, dist = ref.host_knn(x, g["k"])
    t = P().tsne_affinities(ctx, idx, dist, g["perplexity"])
    Pm = t.affinities()[:3]
    for key in ("kl", "purity"):
        lo, hi = g[key + "_range"]
        g[key + "_allowed"] = (lo - (hi - lo), hi + (hi - lo))
    for seed in (1, 2, 3):
        emb, info = P().tsne_run(t, init="random", seed=seed)
        kl, pur = ref.exact_kl(Pm, emb), ref.purity(emb, labels)
        print("quality seed %d: exact KL %.4f (reference range %s, sklearn exact %.4f), purity %.4f (range %s, sklearn %.4f), "
              "device KL at theta %.4f" % (seed, kl, g["kl_range"], g["sklearn_kl"], pur, g["purity_range"], g["sklearn_purity"],
                                           info["kl"]))
        assert info["iters_run"] == 1000
        assert g["kl_allowed"][0] <= kl <= g["kl_allowed"][1]
        assert g["purity_allowed"][0] <= pur <= g["purity_allowed"][1]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import dim_red
    from test_knn_gpu import _planted, _upload
    lib = F.lib()
    idx, dist, u = ref.affinity_case("k2")
    n = idx.shape[0]
    SENT = 0xABCD

    def no_handle(i=idx, d=dist, nn=None, k=None, pu=u, c=None):
        out = C.c_void_p(SENT)
        h = (c or ctx).handle
        rc = lib.srx_tsne_affinities_knn(h, F.ptr(i), F.ptr(d), i.shape[0] if nn is None else nn, i.shape[1] if k is None else k,
                                         pu, C.byref(out))
        msg = lib.srx_last_error(h)
        assert rc == F.E_ARG and msg and out.value == SENT, (rc, msg, out.value)                              # *out untouched
        return msg.decode()

    for pu in (1.0, 0.5, 2.0, 2.5, -1.0, np.nan, np.inf):
        assert "perplexity" in no_handle(pu=pu)
    wide = np.zeros((100, 65), np.uint32)
    assert "k = 65" in no_handle(i=wide, d=np.zeros((100, 65)), pu=3.0)
    assert "k = 1" in no_handle(i=idx[:, :1].copy(), d=dist[:, :1].copy(), pu=0.0)
    i3, d3, _ = ref.affinity_case("n3")
    assert "perplexity" in no_handle(i=i3, d=d3, pu=0.0)                                                      # min(30, 2 / 3) <= 1
    assert "only 1 others" in no_handle(i=i3[:2].copy(), d=d3[:2].copy(), pu=1.5)                            # n = 2
    # everything srx_neighbors_from_knn refuses about a list
    for what, (r, c, v) in {"not below n": (3, 1, n), "names itself": (3, 1, 3), "twice": (3, 1, int(idx[3, 0]))}.items():
        bad = idx.copy()
        bad[r, c] = v
        assert what in no_handle(i=bad)
    for v in (-1.0, np.nan, np.inf):
        bad = dist.copy()
        bad[7, 1] = v
        assert "distance" in no_handle(d=bad)
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    assert "sharded" in no_handle(c=c2)
    out = C.c_void_p(SENT)
    assert lib.srx_tsne_affinities_knn(ctx.handle, F.ptr(idx), F.ptr(dist), n, 2, u, None) == F.E_ARG
    assert lib.srx_tsne_affinities_graph(None, u, C.byref(out)) == F.E_ARG and out.value == SENT
    g1 = P().connectivities_from_knn(ctx, idx[:, :1].copy(), dist[:, :1].copy())
    assert lib.srx_tsne_affinities_graph(g1.handle, 0.0, C.byref(out)) == F.E_ARG and out.value == SENT     # k = 1
    g2 = P().connectivities_from_knn(ctx, idx, dist)
    assert lib.srx_tsne_affinities_graph(g2.handle, 2.0, C.byref(out)) == F.E_ARG and out.value == SENT     # u = k
    assert b"perplexity" in lib.srx_last_error(ctx.handle)

    # the run and the forces
    t = P().tsne_affinities(ctx, idx, dist, u)
    y0 = ref.random_start(n, 1)

    def opts(**kw):
        d = dict(theta=0.5, exaggeration=12.0, learning_rate=0.0, seed=0, n_iter=3, exaggeration_iters=1, stop_after=0, levels=0,
                 init=F.TSNE_INIT_GIVEN, reserved_=0)
        d.update(kw)
        return F.TsneOpts(*[d[name] for name, _ in F.TsneOpts._fields_])

    def refused(o, init=y0, mat=None, th=None):
        emb = np.full((600 if th is not None else n, 2), 12345.0)
        info = F.TsneRunInfo()
        info.cells_exact = 777
        rc = lib.srx_tsne_run((th or t).handle, mat, C.byref(o), None if init is None else F.ptr(init), F.ptr(emb), C.byref(info))
        msg = lib.srx_last_error(ctx.handle)
        assert rc == F.E_ARG and msg, (rc, msg)
        assert (emb == 12345.0).all() and info.cells_exact == 777                                             # nothing written
        return msg.decode()

    for v in (-0.5, np.nan, np.inf):
        assert "theta" in refused(opts(theta=v))
        assert "exaggeration" in refused(opts(exaggeration=v))
        assert "learning_rate" in refused(opts(learning_rate=v))
    for v in (-1, 13):
        assert "levels" in refused(opts(levels=v))
    for v in (-1, 2 ** 20 + 1):
        assert "n_iter" in refused(opts(n_iter=v))
        assert "exaggeration_iters" in refused(opts(exaggeration_iters=v))
    assert "stop_after" in refused(opts(n_iter=3, stop_after=4))
    assert "stop_after" in refused(opts(stop_after=-1))
    assert "unknown start" in refused(opts(init=7))
    assert "start positions" in refused(opts(), init=None)
    for v in (np.nan, np.inf, -np.inf):
        bad = y0.copy()
        bad[7, 1] = v
        assert "NaN or Inf" in refused(opts(), init=bad)
    with pytest.raises(sr.SrxError):
        P().tsne_embedding(t)                                                        # every call above left the handle as it was
    # the PCA start: no matrix, no result, too few components, another size, another context
    a = _upload(ctx, _planted())
    gi, gd = ref.host_knn(np.random.default_rng(0).standard_normal((600, 3)), 6)
    th = P().tsne_affinities(ctx, gi, gd)
    pca = opts(init=F.TSNE_INIT_PCA)
    assert "matrix" in refused(pca, init=None, th=th)
    assert "no PCA result" in refused(pca, init=None, th=th, mat=a.x().handle)
    dim_red.pca_inplace(a, 1, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    assert "components" in refused(pca, init=None, th=th, mat=a.x().handle)
    fewer = _upload(ctx, _planted()[:300])
    dim_red.pca_inplace(fewer, 5, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    assert "cells" in refused(pca, init=None, th=th, mat=fewer.x().handle)
    other = _upload(sr.Context(0), _planted())
    dim_red.pca_inplace(other, 5, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    assert "contexts" in refused(pca, init=None, th=th, mat=other.x().handle)
    # the forces
    for theta, levels, what in ((-1.0, 0, "theta"), (np.nan, 0, "theta"), (np.inf, 0, "theta"), (0.5, -1, "levels"), (0.5, 13, "levels")):
        r = np.full((n, 2), 5.0)
        assert lib.srx_tsne_forces(t.handle, F.ptr(y0), theta, levels, None, F.ptr(r), None, None) == F.E_ARG
        assert what in lib.srx_last_error(ctx.handle).decode() and (r == 5.0).all()
    bad = y0.copy()
    bad[0, 0] = np.nan
    r = np.full((n, 2), 5.0)
    assert lib.srx_tsne_forces(t.handle, F.ptr(bad), 0.5, 0, None, F.ptr(r), None, None) == F.E_ARG and (r == 5.0).all()
    for fn, args in (("srx_tsne_run", (None, None, None, None, None, None)), ("srx_tsne_forces", (None, None, 0.5, 0, None, None, None, None)),
                     ("srx_tsne_fetch_affinities", (None, None, None, None, None)), ("srx_tsne_embedding_fetch", (None, None)),
                     ("srx_tsne_info_get", (None, None))):
        assert getattr(lib, fn)(*args) == F.E_ARG, fn
    # the context and the handle are still usable
    emb, info = P().tsne_run(t, init=y0, n_iter=3)
    assert info["iters_run"] == 3 and np.isfinite(emb).all()

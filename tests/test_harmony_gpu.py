"""srx_harmony_result / srx_harmony_points / srx_harmony_fetch / srx_knn_harmony / srx_neighbors_harmony on the device against
the definition of include/srx.h (tests/harmony_ref.py).

Tolerance.  For every input the reference runs in f64 and in longdouble; G is their largest relative difference per table
(Z_corr, R, Y, O, E, the round objectives; |difference| over the table's largest magnitude).  The device must lie within
64 G of the f64 reference: it adds in another fixed order than numpy's pairwise sums.  profiles/harmony.md has the measured
gaps and the device's distances."""
import ctypes as C
import os

import numpy as np
import pytest

import harmony_ref as ref

pytestmark = pytest.mark.gpu

TOL_FACTOR = 64
FIXED = dict(epsilon_cluster=0.0, epsilon_harmony=0.0, max_rounds=3, max_cluster_iters=5)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _edge(n, d, types, batches, seed):
    Z, batch, _ = ref.planted(n, d, types, batches, seed)
    return Z, batch


def _case(name):
    """(Z, batch, B, keyword arguments) of a named fixed-count case."""
    if name == "planted_two":
        Z, batch, _ = ref.planted_two()
        return Z, batch, 2, dict(n_clusters=20)
    if name == "planted_seven":
        Z, batch, _ = ref.planted_seven()
        return Z, batch, 7, dict(n_clusters=65)
    if name == "n1":
        return np.array([[1.5]]), np.zeros(1, dtype=np.uint32), 1, dict(n_clusters=1, n_blocks=1)
    if name == "n63_d2_K2_B2":
        Z, batch = _edge(63, 2, 2, 2, 11)
        return Z, batch, 2, dict(n_clusters=2)
    if name == "n64_d31_K63_B7_blocks100":          # more blocks than cells; batch 3 empty, batch 6 a single cell
        Z, batch = _edge(64, 31, 3, 6, 12)
        batch = batch.copy()
        batch[batch == 3] = 2
        batch[5] = 6
        return Z, batch, 7, dict(n_clusters=63, n_blocks=100)
    if name == "n65_d50_K64_B64":
        Z, batch = _edge(65, 50, 3, 64, 13)
        return Z, batch, 64, dict(n_clusters=64)
    if name == "n257_d64_K65_B65_theta0_block1":
        Z, batch = _edge(257, 64, 4, 65, 14)
        return Z, batch, 65, dict(n_clusters=65, n_blocks=1, theta=0.0)
    if name == "n257_d65_K100_B256_noinit":
        Z, batch = _edge(257, 65, 4, 256, 15)
        return Z, batch, 256, dict(n_clusters=100, init_iters=-1)
    if name == "n257_d128_K256_B2":                 # Y does not fit the LDS: read through the caches
        Z, batch = _edge(257, 128, 4, 2, 16)
        return Z, batch, 2, dict(n_clusters=256)
    if name == "n300_d50_K256_B3":                  # Y in more than 64 KiB of LDS
        Z, batch = _edge(300, 50, 5, 3, 17)
        return Z, batch, 3, dict(n_clusters=256)
    if name == "n2000_d1":
        Z, batch = _edge(2000, 1, 2, 2, 18)
        return Z, batch, 2, dict(n_clusters=4)
    if name == "n2000_d8_K10_B65":                  # four chunks of grouped sums folded in two runs of two
        Z, batch = _edge(2000, 8, 3, 65, 21)
        return Z, batch, 65, dict(n_clusters=10)
    if name == "duplicates_and_zero_row":
        Z, batch = _edge(200, 10, 3, 3, 19)
        Z = Z.copy()
        Z[:10] = Z[10]
        Z[20] = 0.0
        return Z, batch, 3, dict(n_clusters=8)
    if name == "n_dims_5_of_12":
        Z, batch = _edge(120, 12, 3, 2, 20)
        return Z, batch, 2, dict(n_clusters=6, n_dims=5)
    raise KeyError(name)


EDGES = ["n1", "n63_d2_K2_B2", "n64_d31_K63_B7_blocks100", "n65_d50_K64_B64", "n257_d64_K65_B65_theta0_block1",
         "n257_d65_K100_B256_noinit", "n257_d128_K256_B2", "n300_d50_K256_B3", "n2000_d1", "n2000_d8_K10_B65", "duplicates_and_zero_row",
         "n_dims_5_of_12"]

_REF = {}


def reference(name, **kw):
    """(f64 run, gaps against the longdouble run) of a case, computed once and left unchanged."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _REF:
        Z, batch, B, case_kw = _case(name)
        args = dict(case_kw, **kw)
        args["lam"] = args.pop("lambda_", 1.0)
        a = ref.run(Z, batch, B, **args)
        b = ref.run(Z, batch, B, ft=np.longdouble, **args)
        _REF[key] = (a, b, ref.gaps(a, b))
    return _REF[key]


def device(ctx, name, **kw):
    from singlerust_amd.memory.processing import harmony_points
    Z, batch, B, case_kw = _case(name)
    h = harmony_points(ctx, Z, batch, B, **dict(case_kw, **kw))
    out = {"Z_corr": h.fetch("corrected"), "R": h.fetch("R"), "Y": h.fetch("centroids"), "O": h.fetch("observed"),
           "E": h.fetch("expected"), "info": h.info()}
    out["round_objective"] = out["info"]["round_objective"]
    h.free()
    return out


def check_tables(name, dev, a, gaps):
    worst = {}
    for t in ref.TABLES + ("objectives",):
        x = np.asarray(a[t if t != "objectives" else "round_objective"], dtype=np.float64)
        y = np.asarray(dev[t if t != "objectives" else "round_objective"], dtype=np.float64)
        assert x.shape == y.shape, (name, t, x.shape, y.shape)
        dist = float(np.abs(x - y).max(initial=0) / max(np.abs(x).max(initial=0), np.finfo(np.float64).tiny))
        worst[t] = (dist, gaps[t])
    print(name, " ".join("%s: device %.2e gap %.2e" % (t, *worst[t]) for t in worst))
    for t, (dist, gap) in worst.items():
        assert dist <= TOL_FACTOR * gap, (name, t, dist, gap)


@pytest.mark.parametrize("name", ["planted_two", "planted_seven"] + EDGES)
def test_fixed_count_against_the_definition(ctx, name):
    a, _, gaps = reference(name, **FIXED)
    dev = device(ctx, name, **FIXED)
    i = dev["info"]
    assert i["rounds"] == 3 and i["round_iters"] == [5, 5, 5] and i["converged"] == 0 and i["cluster_iters"] == 15
    assert (i["n"], i["d"], i["n_clusters"], i["n_batches"], i["n_blocks"]) == (a["n"], a["d"], a["K"], a["B"], a["n_blocks"])
    check_tables(name, dev, a, gaps)


@pytest.mark.parametrize("name", ["planted_two", "planted_seven"])
def test_stopping_rules(ctx, name):
    a, b, gaps = reference(name)
    for run in (a, b):                                    # of the reference alone: no ratio near its epsilon
        assert all(abs(r - 1e-5) >= 1e-9 for r in run["ratios_cluster"])
        assert all(abs(r - 1e-4) >= 1e-9 for r in run["ratios_harmony"])
    assert a["round_iters"] == b["round_iters"] and a["converged"] == b["converged"]
    dev = device(ctx, name)
    i = dev["info"]
    assert i["rounds"] == a["rounds"] and i["round_iters"] == a["round_iters"] and i["converged"] == a["converged"]
    assert i["cluster_iters"] == a["cluster_iters"]
    check_tables(name, dev, a, gaps)


def test_two_calls_give_the_same_bits(ctx):
    for name in ("planted_seven", "n257_d65_K100_B256_noinit"):
        x, y = device(ctx, name, **FIXED), device(ctx, name, **FIXED)
        for t in ref.TABLES:
            assert np.array_equal(x[t], y[t]), (name, t)
        assert x["round_objective"] == y["round_objective"]
        assert {k: v for k, v in x["info"].items() if k != "ms"} == {k: v for k, v in y["info"].items() if k != "ms"}


def test_default_cluster_count_and_theta_matter(ctx):
    """n_clusters = 0 follows the header's rule, and the diversity penalty is live: theta = 0 gives another R."""
    Z, batch, _ = ref.planted_two()
    from singlerust_amd.memory.processing import harmony_points
    h = harmony_points(ctx, Z, batch, 2, **FIXED)
    assert h.info()["n_clusters"] == ref.default_clusters(600) == 20
    h0 = harmony_points(ctx, Z, batch, 2, theta=0.0, **FIXED)
    assert np.abs(h.fetch("R") - h0.fetch("R")).max() > 1e-3


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _raw_points(ctx, Z, batch, B, opts, out):
    from singlerust_amd import _ffi as F
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    batch = np.ascontiguousarray(batch, dtype=np.uint32)
    return F.lib().srx_harmony_points(ctx.handle, F.ptr(Z), Z.shape[0], Z.shape[1], F.ptr(batch), B,
                                      None if opts is None else C.byref(opts), out, None)


def test_every_refusal_leaves_out_untouched(ctx):
    import scipy.sparse as sp
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing.harmony import _opts
    Z, batch = _edge(100, 8, 3, 3, 30)
    SENTINEL = 0x5A5A5A5A
    h = C.c_void_p(SENTINEL)

    def refused(rc, c=ctx):
        assert rc == F.E_ARG, rc
        assert h.value == SENTINEL
        msg = F.lib().srx_last_error(c.handle)
        assert msg
        return msg.decode()

    for bad in (dict(theta=-1.0), dict(theta=np.nan), dict(sigma=0.0), dict(sigma=-0.1), dict(sigma=np.inf), dict(lambda_=0.0),
                dict(lambda_=-1.0), dict(epsilon_cluster=-1e-9), dict(epsilon_harmony=-1.0), dict(epsilon_harmony=np.nan),
                dict(n_clusters=-1), dict(n_clusters=257), dict(n_clusters=101), dict(n_blocks=-1), dict(n_blocks=65537),
                dict(max_rounds=-1), dict(max_rounds=65), dict(max_cluster_iters=-1), dict(init_iters=-2), dict(n_dims=-1),
                dict(n_dims=9)):
        refused(_raw_points(ctx, Z, batch, 3, _opts(**bad), C.byref(h)))
    refused(_raw_points(ctx, Z, batch, 0, None, C.byref(h)))
    refused(_raw_points(ctx, Z, batch, 257, None, C.byref(h)))
    assert "batch" in refused(_raw_points(ctx, Z, batch, 2, None, C.byref(h)))           # a label >= B
    for v in (np.nan, np.inf, -np.inf):
        y = Z.copy()
        y[17, 3] = v
        assert "NaN" in refused(_raw_points(ctx, y, batch, 3, None, C.byref(h)))
    refused(_raw_points(ctx, np.zeros((100, F.KNN_MAX_DIMS + 1)), batch, 3, None, C.byref(h)))
    refused(_raw_points(ctx, np.zeros((100, 0)), batch, 3, None, C.byref(h)))
    refused(F.lib().srx_harmony_points(ctx.handle, None, 100, 8, F.ptr(batch), 3, None, C.byref(h), None))
    refused(F.lib().srx_harmony_points(ctx.handle, F.ptr(Z), 100, 8, None, 3, None, C.byref(h), None))
    assert F.lib().srx_harmony_points(ctx.handle, F.ptr(Z), 100, 8, F.ptr(batch), 3, None, None, None) == F.E_ARG
    assert F.lib().srx_harmony_points(None, F.ptr(Z), 100, 8, F.ptr(batch), 3, None, C.byref(h), None) == F.E_ARG
    assert F.lib().srx_harmony_result(None, F.ptr(batch), 3, None, C.byref(h), None) == F.E_ARG
    assert h.value == SENTINEL
    # no PCA result on the matrix
    x = sp.random(50, 30, density=0.3, format="csr", random_state=np.random.RandomState(1))
    x.sort_indices()
    dev = sr.DeviceCsr.upload(ctx, 50, 30, x.indptr, x.indices, x.data, 2)
    assert "no PCA result" in refused(F.lib().srx_harmony_result(dev.handle, F.ptr(batch), 3, None, C.byref(h), None))
    # a context with more than one rank
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    assert "sharded" in refused(_raw_points(c2, Z, batch, 3, None, C.byref(h)), c2)
    # the context still works, and an empty input gives an empty handle
    assert _raw_points(ctx, Z, batch, 3, _opts(**FIXED), C.byref(h)) == 0 and h.value != SENTINEL
    i = F.HarmonyInfo()
    assert F.lib().srx_harmony_info_get(h, C.byref(i)) == 0 and i.n == 100 and i.rounds == 3
    assert F.lib().srx_harmony_fetch(h, 5, None) == F.E_ARG
    F.lib().srx_harmony_free(h)
    e = C.c_void_p()
    assert F.lib().srx_harmony_points(ctx.handle, None, 0, 8, None, 3, None, C.byref(e), C.byref(i)) == 0 and e.value
    assert i.n == 0 and i.rounds == 0
    assert F.lib().srx_harmony_fetch(e, F.HARMONY_R, None) == 0
    F.lib().srx_harmony_free(e)


# ---- residency -----------------------------------------------------------------------------------------------------------
def _fitted(ctx, csc):
    import scipy.sparse as sp
    import singlerust_amd as sr
    from singlerust_amd.memory.processing import dim_red
    z = np.load(os.path.join(GOLD, "planted_600x240.npz"))
    x = sp.csr_matrix((z["log_values"], z["indices"].astype(np.int64), z["indptr"].astype(np.int64)),
                      shape=(int(z["n_rows"]), int(z["n_cols"])))
    x = x.tocsc() if csc else x.tocsr()
    x.sort_indices()
    dev = sr.DeviceCsr.upload(ctx, 600, 240, x.indptr, x.indices, x.data, 2, csc=csc)
    a = sr.IMAnnData(dev, x.indptr, x.indices, [f"c{i}" for i in range(600)], [f"g{j}" for j in range(240)])
    dim_red.pca_inplace(a, 20, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    return a


def _scores(a, n_pc=20):
    from singlerust_amd import _ffi as F
    out = np.zeros((a.n_obs(), n_pc))
    F.check(F.lib().srx_result_fetch(a.x().handle, F.ptr(out), None, None, None, None, None), a.x().ctx.handle)
    return out


@pytest.mark.parametrize("csc", [False, True])
def test_resident_scores_and_the_consumers_of_the_handle(ctx, csc):
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import (connectivities_from_knn, harmony_integrate, harmony_points, knn_points, louvain,
                                                  neighbors)
    a = _fitted(ctx, csc)
    before = _scores(a)
    labels = np.array(["s%d" % (i % 3) for i in range(600)])
    info = harmony_integrate(a, labels, n_clusters=12, n_dims=15)
    assert info["n"] == 600 and info["d"] == 15 and info["n_batches"] == 3 and info["batches"] == ["s0", "s1", "s2"]
    assert np.array_equal(_scores(a), before)                                   # the scores on m are unchanged
    hm = a._harmony[1]
    hp = harmony_points(ctx, before, (np.arange(600) % 3).astype(np.uint32), 3, n_clusters=12, n_dims=15)
    for t in ("corrected", "R", "centroids", "observed", "expected"):
        assert np.array_equal(hm.fetch(t), hp.fetch(t)), t                      # bit for bit
    assert {k: v for k, v in hp.info().items() if k != "ms"} == {k: v for k, v in info.items() if k not in ("ms", "batches")}
    zc = a.obsm["X_pca_harmony"]
    assert zc.shape == (600, 15) and np.array_equal(zc, hm.fetch("corrected"))
    # the k-NN entries read the corrected block
    idx, dist, ki = hm.knn(k=15)
    pi, pd, _ = knn_points(ctx, zc, k=15)
    assert np.array_equal(idx, pi) and np.array_equal(dist, pd) and ki["d"] == 15
    idx8, dist8, _ = hm.knn(k=7, n_dims=8)
    pi8, pd8, _ = knn_points(ctx, zc, k=7, n_dims=8)
    assert np.array_equal(idx8, pi8) and np.array_equal(dist8, pd8)
    g, _ = hm.neighbors(k=15)
    g2 = connectivities_from_knn(ctx, pi, pd)
    for which in (F.GRAPH_DISTANCES, F.GRAPH_CONNECTIVITIES):
        for x, y in zip(g.fetch(which), g2.fetch(which)):
            assert np.array_equal(x, y)
    assert g.info() == g2.info()
    # through the adata: the same lists, the same graph, and Louvain runs on it
    u = neighbors(a, n_neighbors=15, use_rep="X_pca_harmony")
    assert np.array_equal(a.obsm["knn_indices"], pi) and np.array_equal(a.obsm["knn_distances"], pd)
    assert u["params"]["use_rep"] == "X_pca_harmony"
    codes = np.arange(600) % 3                       # the device's mixing is the brute-force mixing on the device's embedding
    assert float((codes[a.obsm["knn_indices"]] != codes[:, None]).mean()) == float((codes[ref.knn_brute(zc, 15)] != codes[:, None]).mean())
    neighbors(a, n_neighbors=15, connectivities=True, use_rep="X_pca_harmony")
    for x, y in zip(a._graph.fetch(F.GRAPH_CONNECTIVITIES), g2.fetch(F.GRAPH_CONNECTIVITIES)):
        assert np.array_equal(x, y)
    lv = louvain(a)
    assert lv["n_communities"] >= 1 and a.obs["louvain"].shape == (600,)
    with pytest.raises(F.SrxError):
        neighbors(a, use_rep="X_other")
    neighbors(a, n_neighbors=15)                                                # the default path is what it was
    ri, rd, _ = knn_points(ctx, before, k=15)
    assert np.array_equal(a.obsm["knn_indices"], ri) and np.array_equal(a.obsm["knn_distances"], rd)
    assert np.array_equal(_scores(a), before)


def test_python_planted_set_mixes(ctx):
    """harmony_points then the handle's k-NN on the planted set: the share of other-batch neighbours from the device's lists
    equals the brute-force share on the device's embedding, and it is what the method is for."""
    from singlerust_amd.memory.processing import harmony_points
    Z, batch, typ = ref.planted_two()
    h = harmony_points(ctx, Z, batch, 2, n_clusters=20)
    zc = h.fetch("corrected")
    idx, _, _ = h.knn(k=15)
    mix_dev = float((batch[idx] != batch[:, None]).mean())
    mix_ref, purity = ref.mixing_and_purity(zc, batch, typ)
    before, _ = ref.mixing_and_purity(Z, batch, typ)
    assert mix_dev == mix_ref and before < 0.15 and mix_dev > 0.4 and purity >= 0.99

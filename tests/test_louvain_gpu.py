"""srx_louvain / srx_louvain_csr on the device: the invariants of the definition (include/srx.h) on every case, quality against
networkx's own seed-to-seed range (tests/golden/louvain_nx.json; networkx itself is never imported here), known answers,
resolution, the resident path, refusals and a 200 000-cell run."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import louvain_ref as ref

pytestmark = pytest.mark.gpu


def run(ctx, W, **kw):
    from singlerust_amd.memory.processing import louvain_csr
    return louvain_csr(ctx, W, **kw)


def check_invariants(ctx, W, labels, info, gamma=1.0, rerun=None, first_level=True):
    """Everything the issue asks of every case.  `rerun`: a callable giving (labels, info) of a second identical call."""
    W = sp.csr_matrix(W)
    n = W.shape[0]
    nc = info["n_communities"]
    assert labels.dtype == np.uint32 and labels.shape == (n,) and info["n"] == n
    sizes = np.bincount(labels, minlength=nc)
    assert len(sizes) == nc and (sizes > 0).all()                                  # 0 .. nc - 1, all used
    first = np.full(nc, n, dtype=np.int64)
    np.minimum.at(first, labels, np.arange(n))
    assert (np.diff(sizes) <= 0).all()
    same = np.diff(sizes) == 0
    assert (np.diff(first)[same] > 0).all()                                        # equal sizes: by smallest member
    q_host = ref.modularity(W, labels, gamma)
    print("Q device %.12f host %.12f diff %.3e levels %s %s" % (info["modularity"], q_host, info["modularity"] - q_host,
                                                                info["level_communities"], info["level_modularity"]))
    assert W.nnz * 2.0 ** -53 < 1e-9                                                # the accumulation bound behind the 1e-9
    assert abs(info["modularity"] - q_host) <= 1e-9
    lm, lc = info["level_modularity"], info["level_communities"]
    assert len(lm) == len(lc) == info["n_levels"]
    assert all(b > a for a, b in zip(lm, lm[1:])) and all(b < a for a, b in zip(lc, lc[1:]))
    if lm:
        assert lm[-1] == info["modularity"] and lc[-1] == nc
    else:
        assert nc == n
    if rerun is not None:
        l2, i2 = rerun()
        assert np.array_equal(labels, l2)
        assert {k: v for k, v in info.items() if k != "ms"} == {k: v for k, v in i2.items() if k != "ms"}
    if first_level and W.nnz:
        l0, i0 = run(ctx, W, resolution=gamma, max_levels=1)
        assert i0["n_levels"] <= 1
        if i0["n_levels"] == 1 and i0["sweeps"] < 200:
            ex = ref.max_excess(W, l0, gamma)
            print("first level: %d communities, max g(best) - g(own) = %.3e" % (i0["n_communities"], ex))
            assert ex <= 1e-12


# ---- quality -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["separated_3000", "separated_20011", "overlapping_6000", "karate_stored", "karate_unit"])
def test_quality_against_networkx_range(ctx, name):
    """Q_dev >= q_min - (q_max - q_min) over networkx's five seeds (q - 1e-9 where they agree)."""
    W, planted = ref.fixture_graph(name)
    gold = ref.golden()["fixtures"][name]
    assert gold["n"] == W.shape[0] and gold["nnz"] == W.nnz
    labels, info = run(ctx, W)
    floor = ref.quality_floor(name)
    print(name, "Q", info["modularity"], "floor", floor, "communities", info["n_communities"], "ms", info["ms"])
    check_invariants(ctx, W, labels, info, rerun=lambda: run(ctx, W))
    assert info["modularity"] >= floor
    if name.startswith("separated"):
        assert info["n_communities"] == 12 and ref.ari(labels, planted) == 1.0


# ---- known answers ---------------------------------------------------------------------------------------------------------
def test_ring_of_cliques(ctx):
    W = ref.ring_of_cliques(8, 6)
    labels, info = run(ctx, W)
    check_invariants(ctx, W, labels, info, rerun=lambda: run(ctx, W))
    assert info["n_communities"] == 8 and np.array_equal(np.bincount(labels), [6] * 8)
    assert abs(info["modularity"] - 0.8125) <= 1e-12
    assert all(len(set(labels[c * 6:(c + 1) * 6])) == 1 for c in range(8))


def test_two_cliques(ctx):
    W = ref.two_cliques()
    labels, info = run(ctx, W)
    check_invariants(ctx, W, labels, info, rerun=lambda: run(ctx, W))
    assert np.array_equal(np.bincount(labels), [4, 3]) and abs(info["modularity"] - 4.0 / 9.0) <= 1e-12
    assert np.array_equal(labels, [1, 1, 1, 0, 0, 0, 0])


def test_one_edge_edgeless_and_empty(ctx):
    W = sp.csr_matrix(np.array([[0.0, 0.7], [0.7, 0.0]]))
    labels, info = run(ctx, W)
    check_invariants(ctx, W, labels, info, rerun=lambda: run(ctx, W))
    assert info["n_communities"] == 1 and np.array_equal(labels, [0, 0]) and abs(info["modularity"]) <= 1e-15
    W = sp.csr_matrix((5, 5))
    labels, info = run(ctx, W)
    check_invariants(ctx, W, labels, info, rerun=lambda: run(ctx, W))
    assert info["n_communities"] == 5 and np.array_equal(labels, np.arange(5)) and info["modularity"] == 0.0 and info["n_levels"] == 0
    labels, info = run(ctx, (np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0)))
    assert labels.shape == (0,) and info["n"] == 0 and info["n_communities"] == 0 and info["n_levels"] == 0 and info["modularity"] == 0.0


def test_isolated_vertices_among_clusters(ctx):
    x, planted = ref.planted_clusters(21, 1500, 20, 5, 6.0)
    W = ref.connectivities(x, 10).tolil()
    iso = np.array([0, 7, 333, 1499])
    for i in iso:
        W[i, :] = 0
        W[:, i] = 0
    W = sp.csr_matrix(W)
    W.eliminate_zeros()
    W.sort_indices()
    labels, info = run(ctx, W)
    check_invariants(ctx, W, labels, info, rerun=lambda: run(ctx, W))
    assert info["n_communities"] == 5 + len(iso)
    assert np.array_equal(labels[iso], 5 + np.arange(len(iso)))                      # singletons last, by their cell number
    keep = np.setdiff1d(np.arange(1500), iso)
    assert ref.ari(labels[keep], planted[keep]) == 1.0


def test_hub_rows_of_every_length(ctx):
    """Rows longer than a wave (the workgroup path) beside short ones: stars joined into a ring, hubs of 40 to 3000 spokes, each
    spoke also tied to the next one of its star.  Every star is one community."""
    deg = [40, 65, 200, 700, 3000, 64, 33]
    rows, cols, hubs, start = [], [], [], 0
    for d in deg:
        hub = start
        hubs.append(hub)
        sp_ = np.arange(start + 1, start + 1 + d)
        rows += [np.full(d, hub), sp_[:-1]]
        cols += [sp_, sp_[1:]]
        start += d + 1
    rows += [np.array(hubs)]
    cols += [np.roll(np.array(hubs), -1)]
    r, c = np.concatenate(rows), np.concatenate(cols)
    w = 0.25 + 0.5 * np.random.default_rng(5).random(len(r))
    W = sp.coo_matrix((np.r_[w, w], (np.r_[r, c], np.r_[c, r])), shape=(start, start)).tocsr()
    W.sort_indices()
    labels, info = run(ctx, W)
    check_invariants(ctx, W, labels, info, rerun=lambda: run(ctx, W))
    rl, ri = ref.louvain(W)
    print("hub stars: device", info["n_communities"], info["modularity"], "restatement", ri["n_communities"], ri["modularity"])
    assert info["modularity"] >= ri["modularity"] - 1e-9


# ---- resolution ------------------------------------------------------------------------------------------------------------
def test_resolution(ctx):
    W, _ = ref.fixture_graph("overlapping_6000")
    counts = {}
    for gamma in (0.5, 1.0, 2.0):
        labels, info = run(ctx, W, resolution=gamma)
        check_invariants(ctx, W, labels, info, gamma=gamma, rerun=lambda: run(ctx, W, resolution=gamma))
        counts[gamma] = info["n_communities"]
    print("communities by resolution", counts)
    assert counts[2.0] >= counts[1.0] >= counts[0.5]


# ---- resident path ---------------------------------------------------------------------------------------------------------
def test_resident_path(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import dim_red, graph_labels, louvain, neighbors
    from test_knn_gpu import _planted, _upload
    a = _upload(ctx, _planted())
    with pytest.raises(sr.SrxError):
        louvain(a)                                                                   # no graph yet
    dim_red.pca_inplace(a, 20, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    neighbors(a, n_neighbors=15, connectivities=True)
    before = a._graph.fetch(F.GRAPH_CONNECTIVITIES)
    with pytest.raises(sr.SrxError):
        graph_labels(a._graph)                                                       # no louvain yet
    info = louvain(a)
    after = a._graph.fetch(F.GRAPH_CONNECTIVITIES)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(before, after))      # C untouched
    labels = a.obs["louvain"]
    assert labels.dtype == np.uint32 and a.uns["louvain"]["info"] == info and a.uns["louvain"]["params"]["resolution"] == 1.0
    l2, i2 = run(ctx, before)
    assert np.array_equal(labels, l2)
    assert {k: v for k, v in info.items() if k != "ms"} == {k: v for k, v in i2.items() if k != "ms"}
    assert np.array_equal(graph_labels(a._graph), labels)
    check_invariants(ctx, a.obsp["connectivities"], labels, info)
    info3 = louvain(a, resolution=2.0, key_added="fine")
    assert a.uns["fine"]["params"]["resolution"] == 2.0 and info3["n_communities"] >= info["n_communities"]
    assert np.array_equal(graph_labels(a._graph), a.obs["fine"])


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    lib = F.lib()
    base = ref.ring_of_cliques(4, 5)

    def refused(indptr, indices, data, n=None, opts=None, c=None):
        indptr, indices, data = np.asarray(indptr, np.uint64), np.asarray(indices, np.uint32), np.asarray(data, np.float64)
        n = len(indptr) - 1 if n is None else n
        labels = np.zeros(max(n, 1), np.uint32)
        info = F.LouvainInfo()
        rc = lib.srx_louvain_csr((c or ctx).handle, F.ptr(indptr), F.ptr(indices), F.ptr(data), n,
                                 None if opts is None else C.byref(opts), F.ptr(labels), C.byref(info))
        msg = lib.srx_last_error((c or ctx).handle)
        assert rc == F.E_ARG and msg, (rc, msg)
        return msg.decode()

    ip, ix, w = base.indptr.copy(), base.indices.copy(), base.data.copy()
    bad = ix.copy(); bad[3] = 20
    assert "index" in refused(ip, bad, w)
    bad = ix.copy(); bad[0] = 0                                                      # row 0 names itself
    assert "diagonal" in refused(ip, bad, w)
    bad = ix.copy(); bad[[0, 1]] = bad[[1, 0]]
    assert "ascending" in refused(ip, bad, w)
    bad = ix.copy(); bad[1] = bad[0]                                                 # a duplicate is not strictly ascending
    assert "ascending" in refused(ip, bad, w)
    for v in (0.0, -1.0, np.nan, np.inf):
        bw = w.copy(); bw[2] = v
        assert "weight" in refused(ip, ix, bw)
    bw = w.copy(); bw[0] = np.nextafter(bw[0], 2.0)                                  # W_ij and W_ji differ in the last bit
    assert "symmetric" in refused(ip, ix, bw)
    one = sp.csr_matrix(np.array([[0, 1.0, 0], [0, 0, 0], [0, 0, 0]]))              # W_01 without W_10
    assert "symmetric" in refused(one.indptr, one.indices, one.data)
    for g in (0.0, -1.0, np.nan):
        assert "resolution" in refused(ip, ix, w, opts=F.LouvainOpts(g, 0.0, 0, 0))
    # a context with more than one rank
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    assert "sharded" in refused(ip, ix, w, c=c2)
    # the context is still usable
    labels, info = run(ctx, base)
    assert info["n_communities"] == 4


# ---- a larger run ----------------------------------------------------------------------------------------------------------
def test_larger_run(ctx):
    """200 000 x 50 clustered, k = 15, graph built on the device: invariants and determinism only (the nnz of this graph, about
    5.2e6, keeps nnz 2^-53 < 6e-10 below the 1e-9 bound).  Prints Q, the planted labelling's Q, the levels and the time."""
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import connectivities_from_knn, graph_labels, knn_points
    x, planted = ref.planted_clusters(31, 200_000, 50, 12, 6.0)
    idx, dist, _ = knn_points(ctx, x, k=15)
    g = connectivities_from_knn(ctx, idx, dist)
    Wt = g.fetch(F.GRAPH_CONNECTIVITIES)
    W = g.matrix(F.GRAPH_CONNECTIVITIES)
    n = x.shape[0]

    def on_handle():
        labels, info = np.zeros(n, np.uint32), F.LouvainInfo()
        F.check(F.lib().srx_louvain(g.handle, None, F.ptr(labels), C.byref(info)), ctx.handle)
        from singlerust_amd.memory.processing.louvain import _info_dict
        return labels, _info_dict(info)

    labels, info = on_handle()
    print("200k: nnz", W.nnz, "Q", info["modularity"], "planted Q", ref.modularity(W, planted), "communities", info["n_communities"],
          "levels", info["level_communities"], info["level_modularity"], "sweeps", info["sweeps"], "moves", info["moves"], "ms", info["ms"])
    check_invariants(ctx, W, labels, info, rerun=on_handle)
    assert np.array_equal(graph_labels(g), labels)
    l2, i2 = run(ctx, Wt)
    assert np.array_equal(l2, labels) and i2["modularity"] == info["modularity"]
    g.free()

"""srx_paga / srx_paga_csr / srx_paga_init_positions on the device against the definition in tests/paga_ref.py.  Every comparison
is exact: the six tables bit for bit, every counter equal.  Edge cases of the walk (row lengths around the lane-group widths,
workgroup boundaries, a counter past 16 bits, 4096 groups), regular k-NN patterns, the resident path, the start positions and
every refusal."""
import ctypes as C

import numpy as np
import pytest

import paga_ref as ref

pytestmark = pytest.mark.gpu

COUNTERS = ("n", "nnz", "n_groups", "groups_empty", "edges_inner", "edges_inter", "pairs_connected", "pairs_clipped", "tree_edges",
            "components")
TABLES = ("sizes", "out_edges", "counts", "connectivities", "expected", "tree")
R = ref.ROWS_PER_WORKGROUP


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_result(a, b):
    return all(np.array_equal(bits(a[t]), bits(b[t])) for t in TABLES) and all(a["info"][c] == b["info"][c] for c in COUNTERS)


def run(ctx, indptr, indices, labels, G):
    from singlerust_amd.memory.processing import paga_csr
    return paga_csr(ctx, (np.asarray(indptr), np.asarray(indices)), labels, G)


def check(ctx, indptr, indices, labels, G):
    """The device's result on the pattern equals the reference's, table for table and counter for counter."""
    got = run(ctx, indptr, indices, labels, G)
    E, sizes = ref.counts_of(indptr, indices, labels, G)
    want = ref.from_counts(E, sizes, G)
    assert got["sizes"].tolist() == sizes and got["out_edges"].tolist() == want["out_edges"]
    assert ref.sparse_counts(got["counts"]) == E
    for name, key in (("connectivities", "connectivities"), ("expected", "expected"), ("tree", "tree")):
        assert np.array_equal(bits(got[name]), bits(ref.dense(want[key], G))), name
    for c in COUNTERS:
        assert got["info"][c] == want["info"][c], c
    assert got["info"]["edges_inner"] + got["info"]["edges_inter"] == got["info"]["nnz"] == len(indices)
    assert got["info"]["tree_edges"] == G - got["info"]["components"]
    return got


def rows_of(lengths, n, rng):
    """A pattern with the given row lengths and uniform targets (duplicates and diagonal entries as they fall)."""
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    return indptr, rng.integers(0, n, int(indptr[-1])).astype(np.uint32)


def knn_pattern(rng, n, k, n_clumps):
    """A regular k-NN pattern (k distinct neighbours, no diagonal) of points in planted clumps, and the clumps as labels."""
    lab = rng.integers(0, n_clumps, n)
    x = rng.standard_normal((n, 4)) + 5.0 * rng.standard_normal((n_clumps, 4))[lab]
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    return np.arange(0, n * k + 1, k, dtype=np.uint64), idx.reshape(-1).astype(np.uint32), lab.astype(np.uint32)


# ---- 1. edge cases through srx_paga_csr ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_n(ctx, n):
    lengths = [3, 0][:n]
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    indices = np.array([n - 1, 0, 0][:int(indptr[-1])], np.uint32)           # row 0: (0, n - 1), (0, 0) twice
    labels = np.array([1, 0][:n], np.uint32)
    got = check(ctx, indptr, indices, labels, 3)
    if n == 0:
        assert got["info"]["components"] == 3 and not any(bits(got[t]).any() for t in TABLES)


def test_one_group_and_every_cell_its_own_group(ctx):
    rng = np.random.default_rng(1)
    indptr, indices = rows_of(rng.integers(0, 9, 300), 300, rng)
    got = check(ctx, indptr, indices, np.zeros(300, np.uint32), 1)
    assert got["info"]["pairs_connected"] == 0 and got["counts"][0, 0] == len(indices)
    got = check(ctx, indptr, indices, rng.permutation(300).astype(np.uint32), 300)
    assert got["info"]["groups_empty"] == 0


def test_4096_groups_most_of_them_empty(ctx):
    rng = np.random.default_rng(2)
    n = 5000
    used = rng.choice(4096, 40, replace=False)
    used[:2] = (0, 4095)
    indptr, indices = rows_of(rng.integers(0, 6, n), n, rng)
    got = check(ctx, indptr, indices, used[rng.integers(0, 40, n)].astype(np.uint32), 4096)
    assert got["info"]["groups_empty"] == 4096 - 40


def test_labels_that_skip_values(ctx):
    rng = np.random.default_rng(3)
    indptr, indices = rows_of(rng.integers(0, 20, 700), 700, rng)
    got = check(ctx, indptr, indices, (3 * rng.integers(0, 5, 700) + 1).astype(np.uint32), 17)
    assert got["info"]["groups_empty"] == 12


def test_row_lengths_around_every_width(ctx):
    """Rows of 0, 1, 63, 64, 65, 257 and 1025 entries in one matrix: shorter than, equal to and longer than a lane group."""
    rng = np.random.default_rng(4)
    lengths = np.array([0, 1, 63, 64, 65, 257, 1025] * 3 + [2] * 40)
    rng.shuffle(lengths)
    n = len(lengths)
    indptr, indices = rows_of(lengths, n, rng)
    check(ctx, indptr, indices, rng.integers(0, 7, n).astype(np.uint32), 7)
    # the same rows among many short ones: a mean row length below 4, the narrowest lane group
    lengths = np.concatenate([lengths, np.ones(2000, np.int64)])
    n = len(lengths)
    indptr, indices = rows_of(lengths, n, rng)
    check(ctx, indptr, indices, rng.integers(0, 7, n).astype(np.uint32), 7)


def test_duplicate_and_diagonal_entries(ctx):
    indptr = np.array([0, 4, 6, 9], np.uint64)
    indices = np.array([1, 1, 1, 0, 1, 1, 2, 0, 0], np.uint32)             # (0, 1) three times, (0, 0), (1, 1) twice, (2, 2), (2, 0) twice
    got = check(ctx, indptr, indices, np.array([0, 1, 0], np.uint32), 2)
    assert got["counts"].tolist() == [[4, 3], [0, 2]]


def test_70000_entries_on_one_pair(ctx):
    """70 rows of group 0 in ONE workgroup, 1000 entries each, all into group 1: a 16-bit or per-wave counter would lose some."""
    assert 70 <= R
    n = 80
    labels = np.array([0] * 70 + [1] * 10, np.uint32)
    rng = np.random.default_rng(5)
    indptr = np.concatenate([np.arange(0, 70001, 1000), np.full(10, 70000)]).astype(np.uint64)
    indices = rng.integers(70, 80, 70000).astype(np.uint32)
    got = check(ctx, indptr, indices, labels, 2)
    assert got["counts"].tolist() == [[0, 70000], [0, 0]]


def test_groups_and_workgroup_boundaries(ctx):
    """Group 0 ends exactly on a workgroup's last row, group 1 fills two workgroups and part of a third, group 3 is empty."""
    rng = np.random.default_rng(6)
    labels = np.repeat(np.array([0, 1, 2, 4], np.uint32), [R, 2 * R + 37, 5, R - 1])
    rng.shuffle(labels)
    n = len(labels)
    indptr, indices = rows_of(np.full(n, 3), n, rng)
    got = check(ctx, indptr, indices, labels, 5)
    assert got["sizes"].tolist() == [R, 2 * R + 37, 5, 0, R - 1]


# ---- 2. regular k-NN patterns ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 15, 16, 17, 63, 64])
def test_knn_patterns(ctx, k):
    rng = np.random.default_rng(10 + k)
    n = 1000
    indptr, indices, labels = knn_pattern(rng, n, k, 9)
    got = check(ctx, indptr, indices, labels, 9)
    assert same_result(got, run(ctx, indptr, indices, labels, 9))                          # a second call: the same bits
    p = rng.permutation(n)                                                                 # cell i becomes cell p[i]
    rows = np.empty(n, np.int64)
    rows[p] = np.arange(n)
    ind2 = p[indices.reshape(n, k)[rows]].reshape(-1).astype(np.uint32)
    lab2 = np.empty(n, np.uint32)
    lab2[p] = labels
    assert same_result(got, run(ctx, indptr, ind2, lab2, 9))


# ---- 3. the resident path and the Python layer -----------------------------------------------------------------------------------
def test_resident_path(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import dim_red, graph_labels, louvain, neighbors, paga, paga_init_positions, umap
    from test_knn_gpu import _planted, _upload
    a = _upload(ctx, _planted())
    with pytest.raises(sr.SrxError):
        paga(a)                                                                            # no graph yet
    dim_red.pca_inplace(a, 20, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    neighbors(a, n_neighbors=15, connectivities=True)
    g = a._graph
    t = F.PagaTables()
    info = F.PagaInfo()
    assert F.lib().srx_paga(g.handle, None, 4, C.byref(t), C.byref(info)) == F.E_ARG       # no labels on the handle yet
    assert b"louvain" in F.lib().srx_last_error(ctx.handle)
    li = louvain(a)
    labels = a.obs["louvain"].copy()
    G = li["n_communities"]
    c_before, gi_before = g.fetch(F.GRAPH_CONNECTIVITIES), g.info()
    info = paga(a)                                                                         # labels == NULL: those on the handle
    u = a.uns["paga"]
    assert u["groups"] == "louvain" and u["info"] == info and info["n_groups"] == G and info["ms"] > 0.0
    ip, ix, _ = g.fetch(F.GRAPH_DISTANCES)
    want = check(ctx, ip, ix, labels, G)
    for key, name in (("connectivities", "connectivities"), ("connectivities_tree", "tree"), ("expected_n_edges_random", "expected")):
        assert np.array_equal(bits(np.asarray(u[key].todense())), bits(want[name])), key
    assert u["sizes"].tolist() == want["sizes"].tolist() and all(info[c] == want["info"][c] for c in COUNTERS)
    assert info["nnz"] == a.n_obs() * 15 and info["groups_empty"] == 0
    a.obs["mine"] = labels                                                                 # the same labels from the host
    assert paga(a, groups="mine") == {**info, "ms": a.uns["paga"]["info"]["ms"]} and a.uns["paga"]["groups"] == "mine"
    assert np.array_equal(bits(np.asarray(a.uns["paga"]["connectivities"].todense())), bits(want["connectivities"]))
    more = F.PagaInfo()                                                                    # n_groups above n_communities: empty groups
    F.check(F.lib().srx_paga(g.handle, None, G + 3, None, C.byref(more)), ctx.handle)
    assert more.groups_empty == 3 and more.components == info["components"] + 3 and more.pairs_connected == info["pairs_connected"]
    # C, the labels and the graph's info are as they were
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(c_before, g.fetch(F.GRAPH_CONNECTIVITIES)))
    assert np.array_equal(graph_labels(g), labels) and g.info() == gi_before
    # the start positions: the handle's labels, equal to the reference, accepted by umap
    paga(a)
    pos = np.random.default_rng(0).standard_normal((G, 2)) * 4.0
    y0 = paga_init_positions(a, pos, seed=9)
    assert np.array_equal(bits(y0), bits(ref.init_positions(labels, want["connectivities"], pos, 9)))
    ui = umap(a, init=y0, n_epochs=5, seed=1)
    assert ui["epochs_run"] == 5 and np.isfinite(a.obsm["X_umap"]).all()


# ---- 4. srx_paga_init_positions ---------------------------------------------------------------------------------------------------
def init_positions(ctx, labels, conn, pos, seed, n_groups=None):
    from singlerust_amd import _ffi as F
    labels, conn, pos = np.ascontiguousarray(labels, np.uint32), np.ascontiguousarray(conn, np.float64), np.ascontiguousarray(pos, np.float64)
    out = np.full((len(labels), pos.shape[1]), -7.0)
    rc = F.lib().srx_paga_init_positions(None, ctx.handle, F.ptr(labels), len(labels), n_groups or pos.shape[0], F.ptr(conn), F.ptr(pos),
                                         pos.shape[1], seed, F.ptr(out))
    return rc, out


@pytest.mark.parametrize("dim", [2, 3])
def test_init_positions(ctx, dim):
    from singlerust_amd import _ffi as F
    rng = np.random.default_rng(20 + dim)
    G, n = 6, 1500
    conn = np.triu(rng.random((G, G)) * (rng.random((G, G)) < 0.6), 1)
    conn[0, 1] = conn[0, 2] = 1.0                                  # group 0: a tie, to the lowest h
    conn[:, 4] = conn[4, :] = 0.0                                  # group 4: no neighbour
    conn = conn + conn.T
    pos = rng.standard_normal((G, dim)) * 3.0
    pos[4, 0] = -0.0
    labels = rng.integers(0, G, n)
    for seed in (0, 12345, 2 ** 64 - 1):
        rc, out = init_positions(ctx, labels, conn, pos, seed)
        assert rc == F.OK
        assert np.array_equal(bits(out), bits(ref.init_positions(labels, conn, pos, seed)))
    assert np.array_equal(bits(out[labels == 4]), bits(np.broadcast_to(pos[4], (int((labels == 4).sum()), dim))))
    lo, hi = np.minimum(pos[0], pos[1]), np.maximum(pos[0], pos[1])
    assert np.all((out[labels == 0] >= lo) & (out[labels == 0] <= hi))          # between the group and its neighbour, group 1


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    lib = F.lib()
    indptr, indices, labels = np.array([0, 2, 3, 3], np.uint64), np.array([1, 2, 0], np.uint32), np.array([0, 1, 1], np.uint32)
    conn = np.full((2, 2), 7.0)
    info = F.PagaInfo()
    info.n = 99
    t = F.PagaTables(None, None, None, F.ptr(conn), None, None)

    def refused(ip, ix, lab, G, n=3, c=None):
        h = (c or ctx).handle
        rc = lib.srx_paga_csr(h, None if ip is None else F.ptr(ip), None if ix is None else F.ptr(ix), n,
                              None if lab is None else F.ptr(lab), G, C.byref(t), C.byref(info))
        msg = lib.srx_last_error(h)
        assert rc == F.E_ARG and msg, (rc, msg)
        assert info.n == 99 and np.all(conn == 7.0)                                        # nothing written
        return msg.decode()

    assert "n_groups" in refused(indptr, indices, labels, 0)
    assert "n_groups" in refused(indptr, indices, labels, F.GROUPS_MAX + 1)
    assert "label" in refused(indptr, indices, np.array([0, 2, 1], np.uint32), 2)
    assert "label" in refused(indptr, indices, None, 2)
    assert "index" in refused(indptr, np.array([1, 3, 0], np.uint32), labels, 2)
    assert "indices" in refused(indptr, None, labels, 2)
    assert "indptr" in refused(None, indices, labels, 2)
    assert "indptr" in refused(np.array([1, 2, 3, 3], np.uint64), indices, labels, 2)
    assert "decreases" in refused(np.array([0, 2, 1, 3], np.uint64), indices, labels, 2)
    assert "2^32" in refused(indptr, indices, labels, 2, n=2 ** 32)
    long_row = np.array([0, 1 << 22], np.uint64)                                           # one row of 2^22 entries
    assert "2^22" in refused(long_row, np.zeros(1 << 22, np.uint32), np.zeros(1, np.uint32), 1, n=1)
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    assert "sharded" in refused(indptr, indices, labels, 2, c=c2)
    assert lib.srx_paga_csr(None, F.ptr(indptr), F.ptr(indices), 3, F.ptr(labels), 2, None, None) == F.E_ARG and lib.srx_last_error(None)
    assert lib.srx_paga(None, F.ptr(labels), 2, None, None) == F.E_ARG and lib.srx_last_error(None)

    # a handle: n_groups, a bad host label, a sharded context
    from singlerust_amd.memory.processing import connectivities_from_knn
    rng = np.random.default_rng(8)
    idx = np.array([rng.choice(np.delete(np.arange(40), i), 3, replace=False) for i in range(40)], np.uint32)
    g = connectivities_from_knn(ctx, idx, np.sort(rng.random((40, 3)) + 0.1, axis=1))
    lab40 = rng.integers(0, 3, 40).astype(np.uint32)

    def refused_g(lab, G):
        rc = lib.srx_paga(g.handle, None if lab is None else F.ptr(lab), G, C.byref(t), C.byref(info))
        msg = lib.srx_last_error(ctx.handle)
        assert rc == F.E_ARG and msg and info.n == 99 and np.all(conn == 7.0), (rc, msg)
        return msg.decode()

    assert "louvain" in refused_g(None, 3)                                                 # a handle that holds no labels
    assert "n_groups" in refused_g(lab40, 0) and "n_groups" in refused_g(lab40, F.GROUPS_MAX + 1)
    assert "label" in refused_g(lab40, 2)
    t3 = F.PagaTables()
    i3 = F.PagaInfo()
    F.check(lib.srx_paga(g.handle, F.ptr(lab40), 3, C.byref(t3), C.byref(i3)), ctx.handle)         # host labels on a handle without any
    assert i3.nnz == 120 and i3.n == 40

    # srx_paga_init_positions
    pos, cn, lab = np.zeros((2, 2)), np.array([[0, 0.5], [0.5, 0]]), np.array([0, 1, 1], np.uint32)
    out = np.full((3, 2), -7.0)

    def refused_p(gh, ch, lab, n, G, cn, pos, dim, o):
        rc = lib.srx_paga_init_positions(gh, ch, None if lab is None else F.ptr(lab), n, G, None if cn is None else F.ptr(cn),
                                         None if pos is None else F.ptr(pos), dim, 0, None if o is None else F.ptr(o))
        msg = lib.srx_last_error(ch)
        assert rc == F.E_ARG and msg and np.all(out == -7.0), (rc, msg)
        return msg.decode()

    h = ctx.handle
    assert "null" in refused_p(None, None, lab, 3, 2, cn, pos, 2, out)
    assert "dim" in refused_p(None, h, lab, 3, 2, cn, np.zeros((2, 4)), 4, out)
    assert "dim" in refused_p(None, h, lab, 3, 2, cn, np.zeros((2, 1)), 1, out)
    assert "n_groups" in refused_p(None, h, lab, 3, 0, cn, pos, 2, out)
    for bad in (np.nan, np.inf, -np.inf):
        p2, c2n = pos.copy(), cn.copy()
        p2[1, 0] = bad
        c2n[0, 1] = bad
        assert "pos" in refused_p(None, h, lab, 3, 2, cn, p2, 2, out)
        assert "connectivities" in refused_p(None, h, lab, 3, 2, c2n, pos, 2, out)
    assert "output" in refused_p(None, h, lab, 3, 2, cn, pos, 2, None)
    assert "label" in refused_p(None, h, np.array([0, 2, 1], np.uint32), 3, 2, cn, pos, 2, out)
    assert "labels" in refused_p(None, h, None, 3, 2, cn, pos, 2, out)
    assert "labels" in refused_p(g.handle, h, None, 40, 2, cn, pos, 2, np.zeros((40, 2)))          # the handle holds none
    assert "cells" in refused_p(g.handle, h, lab, 3, 2, cn, pos, 2, out)                          # n is not the handle's
    assert "sharded" in refused_p(None, c2.handle, lab, 3, 2, cn, pos, 2, out)
    # the context is still usable
    check(ctx, indptr, indices, labels, 2)

"""srx_diffmap / srx_diffmap_csr / srx_graph_diffmap_fetch / srx_graph_transitions_fetch / srx_dpt / srx_dpt_from on the
device against the definition of include/srx.h (tests/diffmap_ref.py).

Tolerances.  D is the reference's own max |f64 numpy - longdouble numpy|, computed here for every case, and the device
gets 32 D (the rule of profiles/umap.md; profiles/diffmap.md has the table).  For symmetric T an eigenvalue lies within
|r| of lambda, so eigenvalues are held to tol + 32 D, the host's residual from the fetched T to tol + 32 D, info.max_residual to
tol, |V^T V - I| to 64 n_comps 2^-53, and vectors (Davis-Kahan, gap delta) to 2 (tol + n 2^-53) / delta.

T can be fetched from a handle only.  The graphs that come from k-NN lists (traj500, blobs3, ring257, traj2 .. traj257) are
therefore built on the device from those lists, and the reference works from the C the device returns; traj257k7 and
traj257k8 (k = 7 and 8) bring the rows of G - 1, G, G + 1 and 2 G + 1 entries to that entry-by-entry comparison.  `rows` (the
hub-of-300 graph of the UMAP tests) is no k-NN graph: there the residual is taken against the REFERENCE's T, whose rows differ
from the device's by at most (row length) x 32 D in sum, which is added to the bound."""
import ctypes as C

import numpy as np
import pytest

import diffmap_ref as ref

pytestmark = pytest.mark.gpu

TOL = ref.TOL
U = ref.U
TOL_FACTOR = 32
KNN_GRAPHS = ["traj500", "blobs3", "ring257", "traj2", "traj5", "traj63", "traj64", "traj65", "traj257", "traj257k7", "traj257k8"]


def G():
    from singlerust_amd import _ffi
    return _ffi.DIFFMAP_GROUP


_H = {}


def handle(ctx, name):
    """The device graph of the named points and what the device holds as C: (Graph, (indptr, indices, data))."""
    if name not in _H:
        from singlerust_amd import _ffi as F
        from singlerust_amd.memory.processing import connectivities_from_knn
        x, k = ref.points(name)
        idx, dist = ref.knn_lists(x, k)
        g = connectivities_from_knn(ctx, idx, dist)
        _H[name] = (g, g.fetch(F.GRAPH_CONNECTIVITIES))
    return _H[name]


_REF = {}


def reference(key, csr, density=True):
    """(T values f64, z, D, T as scipy CSR, all eigenvalues descending, eigenvectors of all of them with the sign rule) for a CSR
    triple, computed once per key and left unchanged."""
    key = (key, density)
    if key not in _REF:
        ip, ix, w = csr
        t, z, D = ref.transitions_D(ip, ix, w, density, G())
        T = ref.t_matrix(ip, ix, t)
        w_all, _, v_all = ref.eigen(T, T.shape[0] - 1)
        _REF[key] = (t, z, D, T, w_all, v_all)
    return _REF[key]


def rows_csr():
    return ref.csr_arrays(ref.fixture("rows%d" % G()))


_RUN = {}


def solve_handle(ctx, name, **kw):
    """srx_diffmap on the handle through the ctypes layer: (evals, evecs, info dict, T values fetched)."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _RUN:
        from singlerust_amd import _ffi as F
        import importlib
        D_ = importlib.import_module("singlerust_amd.memory.processing.diffmap")      # (the package exports the function of that name)
        from singlerust_amd.memory.processing import graph_transitions
        g, csr = handle(ctx, name)
        n = len(csr[0]) - 1
        o = D_._opts(kw.get("n_comps", 0), kw.get("ncv", 0), kw.get("tol", 0.0), kw.get("max_matvecs", 0), kw.get("seed", 0),
                     kw.get("density_normalize", True))
        evals, evecs = D_._room(n, kw.get("n_comps", 0))
        info = F.DiffmapInfo()
        F.check(F.lib().srx_diffmap(g.handle, C.byref(o), F.ptr(evals), F.ptr(evecs), C.byref(info)), ctx.handle)
        m = int(info.n_comps)
        _RUN[key] = (evals[:m].copy(), evecs[:n * m].reshape(n, m).copy(), D_._info_dict(info), graph_transitions(g))
    return _RUN[key]


def solve_csr(ctx, csr, **kw):
    from singlerust_amd.memory.processing import diffmap_csr
    return diffmap_csr(ctx, csr, **kw)


def check_contract(name, T, D, evals, evecs, info, tol=TOL, extra=0.0):
    """Section 3: the host's residual, the reported one, orthonormality, the sign rule, the order."""
    n, m = evecs.shape
    assert evals.shape == (m,) and info["n_comps"] == m and info["n"] == n and info["nnz"] == T.nnz
    assert np.isfinite(evecs).all() and np.isfinite(evals).all()
    R = T @ evecs - evecs * evals[None, :]
    host_res = float(np.sqrt((R * R).sum(axis=0)).max())
    ortho = float(np.abs(evecs.T @ evecs - np.eye(m)).max())
    print("%s n_comps %d ncv %d: matvecs %d restarts %d breakdowns %d | residual host %.3e reported %.3e bound %.3e | ortho host %.3e "
          "reported %.3e bound %.3e | D %.3e" % (name, m, info["ncv"], info["matvecs"], info["restarts"], info["breakdowns"], host_res,
                                                   info["max_residual"], tol + TOL_FACTOR * D + extra, ortho, info["max_ortho"], 64 * m * U, D))
    assert info["max_residual"] <= tol
    assert host_res <= tol + TOL_FACTOR * D + extra
    assert ortho <= 64 * m * U and info["max_ortho"] <= 64 * m * U
    assert ref.sign_rule_holds(evecs)
    assert np.all(np.diff(evals) <= 0)


# ---- 1. transitions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [True, False])
@pytest.mark.parametrize("name", KNN_GRAPHS)
def test_transitions(ctx, name, density):
    g, csr = handle(ctx, name)
    ip, ix, w = csr
    t_ref, z, D, T, _, _ = reference(name, csr, density)
    _, _, info, t_dev = solve_handle(ctx, name, n_comps=3, density_normalize=density)
    err = float(np.abs(t_dev - t_ref).max())
    print("%s density %d: n %d nnz %d rows %d..%d | D %.3e 32D %.3e device %.3e" % (name, density, len(ip) - 1, len(w), np.diff(ip.astype(np.int64)).min(),
                                                                                     np.diff(ip.astype(np.int64)).max(), D, TOL_FACTOR * D, err))
    assert t_dev.shape == t_ref.shape and err <= TOL_FACTOR * D
    Td = ref.t_matrix(ip, ix, t_dev)
    Tt = Td.T.tocsr()
    Tt.sort_indices()
    assert np.array_equal(Td.data.view(np.uint64), Tt.data.view(np.uint64))                  # T[i, j] and T[j, i]: equal bits
    if name == "ring257":
        assert np.abs(w - 1.0).max() <= 4 * U and np.abs(t_dev - 0.5).max() <= 8 * U


def test_transitions_cover_the_lane_group_edges(ctx):
    """Rows of G - 1, G, G + 1 and 2 G + 1 entries are among those test_transitions compares entry by entry."""
    g = G()
    lens = set()
    for name in ("traj257k%d" % (g - 1), "traj257k%d" % g):
        lens |= set(np.diff(handle(ctx, name)[1][0].astype(np.int64)).tolist())
    assert {g - 1, g, g + 1, 2 * g + 1} <= lens, sorted(lens)


# ---- 2. eigenvalues -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("traj500", {}), ("traj500", {"n_comps": 6, "ncv": 14}), ("blobs3", {})])
def test_eigenvalues(ctx, name, kw):
    g, csr = handle(ctx, name)
    _, _, D, T, w_all, _ = reference(name, csr)
    evals, evecs, info, _ = solve_handle(ctx, name, **kw)
    m = len(evals)
    err = float(np.abs(evals - w_all[:m]).max())
    print("%s %s: matvecs %d restarts %d | lambda err %.3e bound %.3e" % (name, kw, info["matvecs"], info["restarts"], err, TOL + TOL_FACTOR * D))
    assert m == kw.get("n_comps", 15)
    assert err <= TOL + TOL_FACTOR * D
    if kw:
        assert info["ncv"] == 14 and info["restarts"] >= 1


@pytest.mark.parametrize("m", [1, 3, 5])
def test_ring_is_the_cosine(ctx, m):
    g, csr = handle(ctx, "ring257")
    _, _, D, T, w_all, _ = reference("ring257", csr)
    evals, evecs, info, _ = solve_handle(ctx, "ring257", n_comps=m)
    want = np.cos(2.0 * np.pi * ((np.arange(m) + 1) // 2) / 257.0)
    err = float(np.abs(evals - want).max())
    print("ring257 n_comps %d: matvecs %d restarts %d | err against the cosine %.3e bound %.3e | lambda_min %.6f" %
          (m, info["matvecs"], info["restarts"], err, TOL + TOL_FACTOR * D, w_all[-1]))
    assert err <= TOL + TOL_FACTOR * D
    assert w_all[-1] < -0.9999                                                               # where 'LM' would differ


# ---- 3. the contract ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("traj500", {}), ("traj500", {"n_comps": 6, "ncv": 14}), ("blobs3", {}), ("ring257", {"n_comps": 5}),
                                     ("traj500", {"density_normalize": False})])
def test_contract_on_handles(ctx, name, kw):
    g, csr = handle(ctx, name)
    D = reference(name, csr, kw.get("density_normalize", True))[2]
    evals, evecs, info, t_dev = solve_handle(ctx, name, **kw)
    check_contract(name, ref.t_matrix(csr[0], csr[1], t_dev), D, evals, evecs, info)


def test_contract_on_rows(ctx):
    csr = rows_csr()
    g = G()
    lens = np.diff(csr[0].astype(np.int64))
    assert lens.max() == 300 and {g - 1, g, g + 1, 2 * g + 1} <= set(lens.tolist())
    _, _, D, T, w_all, _ = reference("rows", csr)
    evals, evecs, info = solve_csr(ctx, csr)
    check_contract("rows", T, D, evals, evecs, info, extra=TOL_FACTOR * D * (lens.max() + 1))
    assert np.abs(evals - w_all[:15]).max() <= TOL + TOL_FACTOR * D * (lens.max() + 1)
    assert np.abs(evals[:5] - 1.0).max() <= TOL                                              # five components


# ---- 4. vectors ---------------------------------------------------------------------------------------------------------------
def test_vectors_traj500(ctx):
    g, csr = handle(ctx, "traj500")
    _, _, D, T, w_all, v_all = reference("traj500", csr)
    evals, evecs, info, _ = solve_handle(ctx, "traj500")
    n, m = evecs.shape
    delta = ref.gaps(w_all, m)
    assert delta.min() >= 7.5e-4
    for l in range(m):
        err = min(np.abs(evecs[:, l] - v_all[:, l]).max(), np.abs(evecs[:, l] + v_all[:, l]).max())
        bound = 2.0 * (TOL + n * U) / delta[l]
        print("traj500 vector %d: delta %.3e err %.3e bound %.3e" % (l, delta[l], err, bound))
        assert err <= bound


def test_projector_blobs3(ctx):
    g, csr = handle(ctx, "blobs3")
    _, z, D, T, w_all, v_all = reference("blobs3", csr)
    evals, evecs, info, _ = solve_handle(ctx, "blobs3")
    n = evecs.shape[0]
    delta = w_all[2] - w_all[3]
    assert abs(delta - 0.133) < 1e-3 and np.abs(evals[:3] - 1.0).max() <= TOL + TOL_FACTOR * D
    bound = 2.0 * (TOL + n * U) / delta
    P = evecs[:, :3] @ evecs[:, :3].T
    P_ref = v_all[:, :3] @ v_all[:, :3].T
    ncomp, lab = ref.components(T)
    assert ncomp == 3
    B = np.stack([np.where(lab == c, np.sqrt(z), 0.0) for c in range(3)], axis=1)             # indicator times sqrt(z)
    B /= np.sqrt((B * B).sum(axis=0))[None, :]
    P_closed = B @ B.T
    print("blobs3 projector: against eigh %.3e against the closed form %.3e bound %.3e" %
          (np.abs(P - P_ref).max(), np.abs(P - P_closed).max(), bound))
    assert np.abs(P - P_ref).max() <= bound and np.abs(P - P_closed).max() <= bound


# ---- 5. small and clamped -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,m", [("traj5", {"n_comps": 15}, 4), ("traj2", {"n_comps": 15}, 1), ("traj63", {"n_comps": 3}, 3),
                                       ("traj64", {"n_comps": 3}, 3), ("traj65", {"n_comps": 3}, 3), ("traj257", {"n_comps": 3}, 3),
                                       ("traj63", {"n_comps": 3, "ncv": 63}, 3), ("traj64", {"n_comps": 3, "ncv": 129}, 3),
                                       ("traj65", {"n_comps": 3, "ncv": 65}, 3)])
def test_small_and_clamped(ctx, name, kw, m):
    g, csr = handle(ctx, name)
    n = len(csr[0]) - 1
    _, _, D, T, w_all, _ = reference(name, csr)
    evals, evecs, info, t_dev = solve_handle(ctx, name, **kw)
    check_contract(name, ref.t_matrix(csr[0], csr[1], t_dev), D, evals, evecs, info)
    assert info["n_comps"] == m and evecs.shape == (n, m)
    assert np.abs(evals - w_all[:m]).max() <= TOL + TOL_FACTOR * D
    assert info["ncv"] == min(kw.get("ncv", 0) or max(2 * m + 1, 20), n)
    if info["ncv"] >= n:
        assert info["breakdowns"] >= 1
    if name == "traj2":
        assert abs(evals[0] - 1.0) <= TOL and abs(w_all[1] + 1.0) <= 4 * U


# ---- 6. determinism -----------------------------------------------------------------------------------------------------------
def test_determinism_and_the_csr_route(ctx):
    from singlerust_amd.memory.processing import graph_diffmap
    g, csr = handle(ctx, "traj500")
    _RUN.pop(("traj500", ()), None)
    first = solve_handle(ctx, "traj500")
    for _ in range(4):
        _RUN.pop(("traj500", ()), None)
        again = solve_handle(ctx, "traj500")
        assert np.array_equal(first[0].view(np.uint64), again[0].view(np.uint64))
        assert np.array_equal(first[1].view(np.uint64), again[1].view(np.uint64))
        assert np.array_equal(first[3].view(np.uint64), again[3].view(np.uint64))
        assert {k: v for k, v in first[2].items() if k != "ms"} == {k: v for k, v in again[2].items() if k != "ms"}
    fe, fv = graph_diffmap(g)
    assert np.array_equal(fe.view(np.uint64), first[0].view(np.uint64)) and np.array_equal(fv.view(np.uint64), first[1].view(np.uint64))
    evals, evecs, info = solve_csr(ctx, csr)
    assert np.array_equal(evals.view(np.uint64), first[0].view(np.uint64))
    assert np.array_equal(evecs.view(np.uint64), first[1].view(np.uint64))
    assert {k: v for k, v in info.items() if k != "ms"} == {k: v for k, v in first[2].items() if k != "ms"}
    other = solve_handle(ctx, "traj500", seed=1)
    assert np.abs(other[0] - first[0]).max() <= 2 * TOL and not np.array_equal(other[1], first[1])
    _RUN.pop(("traj500", ()), None)
    solve_handle(ctx, "traj500")                                                              # the handle holds the seed-0 result again


# ---- 7. pseudotime ------------------------------------------------------------------------------------------------------------
def test_dpt(ctx):
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import dpt_from

    def both(name, root, cap):
        g, csr = handle(ctx, name)
        _RUN.pop((name, ()), None)
        evals, evecs, _, _ = solve_handle(ctx, name)                                          # the handle's current eigenpairs
        n = evecs.shape[0]
        want, D = ref.dpt_D(evals, evecs, root, cap or ref.CAP)
        out = np.full(n, -1.0)
        F.check(F.lib().srx_dpt(g.handle, root, cap, F.ptr(out)), ctx.handle)
        out2 = dpt_from(ctx, evals, evecs, root, cap)
        print("dpt %s root %d cap %g: D %.3e 32D %.3e srx_dpt %.3e srx_dpt_from %.3e" %
              (name, root, cap, D, TOL_FACTOR * D, np.abs(out - want).max(), np.abs(out2 - want).max()))
        assert np.abs(out - want).max() <= TOL_FACTOR * D and np.abs(out2 - want).max() <= TOL_FACTOR * D
        assert out.max() == 1.0 and out[root] == 0.0 and out.min() == 0.0
        return evals, out

    evals, p0 = both("traj500", 0, 0.0)
    _, p_end = both("traj500", 499, 0.0)
    _, p_cap1 = both("traj500", 0, 1.0)
    assert evals[0] >= ref.CAP and evals[1] < ref.CAP                  # lambda_0 = 1 has the weight 1 under the default cap
    assert np.array_equal(p0, p_cap1) == bool(evals[0] >= 1.0) and not np.array_equal(p0, p_end)
    lab = ref.components(ref.t_matrix(*handle(ctx, "blobs3")[1]))[1]
    root = int(np.nonzero(lab == lab[200])[0][3])
    both("blobs3", root, 0.0)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import connectivities_from_knn
    lib = F.lib()
    ip, ix, w = ref.csr_arrays(ref.fixture("traj65"))
    n = 65
    SENT = 12345.0

    def opts(**kw):
        d = dict(tol=0.0, seed=0, n_comps=3, ncv=0, max_matvecs=0, density_normalize=1)
        d.update(kw)
        return F.DiffmapOpts(*[d[name] for name, _ in F.DiffmapOpts._fields_])

    def refused(o, c=None, graph=None, arrays=(ip, ix, w), n_=n, code=F.E_ARG):
        evals, evecs = np.full(64, SENT), np.full(n * 64, SENT)
        info = F.DiffmapInfo()
        info.matvecs = 777
        h = (c or ctx).handle
        if graph is not None:
            rc = lib.srx_diffmap(graph, C.byref(o), F.ptr(evals), F.ptr(evecs), C.byref(info))
        else:
            rc = lib.srx_diffmap_csr(h, F.ptr(arrays[0]), F.ptr(arrays[1]), F.ptr(arrays[2]), n_, C.byref(o), F.ptr(evals), F.ptr(evecs),
                                     C.byref(info))
        msg = lib.srx_last_error(h)
        assert rc == code and msg, (rc, msg)
        assert (evals == SENT).all() and (evecs == SENT).all()                               # nothing written
        if code == F.E_ARG:
            assert info.matvecs == 777
        return msg.decode(), info

    x, k = ref.points("traj65")
    gh = connectivities_from_knn(ctx, *ref.knn_lists(x, k))
    for route in (None, gh.handle):
        for v in (-1, 65, 1000):
            assert "n_comps" in refused(opts(n_comps=v), graph=route)[0]
        for v in (4, 2, 130, -3):
            assert "ncv" in refused(opts(ncv=v), graph=route)[0]
        for v in (-1e-10, np.nan):
            assert "tol" in refused(opts(tol=v), graph=route)[0]
        assert "max_matvecs" in refused(opts(max_matvecs=-1), graph=route)[0]
    for n_small in (0, 1):
        assert "at least 2" in refused(opts(), arrays=(np.zeros(n_small + 1, dtype=np.uint64), ix, w), n_=n_small)[0]
    # an empty row: vertex 64 cut out of the graph
    W = ref.fixture("traj65").tolil()
    W[64, :] = 0
    W[:, 64] = 0
    cut = ref.csr_arrays(W.tocsr())
    assert "no entries" in refused(opts(), arrays=cut)[0]
    bw = w.copy()
    bw[0] = np.nextafter(bw[0], 2.0)
    assert "symmetric" in refused(opts(), arrays=(ip, ix, bw))[0]                            # the validation of srx_louvain_csr
    bad = ix.copy()
    bad[0] = 70
    assert "index" in refused(opts(), arrays=(ip, bad, w))[0]
    neg = w.copy()
    neg[3] = -neg[3]
    assert "weight" in refused(opts(), arrays=(ip, ix, neg))[0]
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    assert "sharded" in refused(opts(), c=c2)[0]
    # pseudotime: before a diffmap, a root outside, a cap outside
    out = np.full(n, SENT)

    def dpt_refused(fn, *args):
        rc = fn(*args)
        msg = lib.srx_last_error(ctx.handle)
        assert rc == F.E_ARG and msg and (out == SENT).all()
        return msg.decode()

    assert "no srx_diffmap" in dpt_refused(lib.srx_dpt, gh.handle, 0, 0.0, F.ptr(out))
    with pytest.raises(sr.SrxError):
        from singlerust_amd.memory.processing import graph_diffmap
        graph_diffmap(gh)                                                                    # every call above left the handle as it was
    with pytest.raises(sr.SrxError):
        from singlerust_amd.memory.processing import graph_transitions
        graph_transitions(gh)
    evals, evecs = np.zeros(3), np.zeros((n, 3))
    F.check(lib.srx_diffmap(gh.handle, C.byref(opts()), F.ptr(evals), F.ptr(evecs), None), ctx.handle)
    assert "root" in dpt_refused(lib.srx_dpt, gh.handle, n, 0.0, F.ptr(out))
    assert "root" in dpt_refused(lib.srx_dpt_from, ctx.handle, F.ptr(evals), F.ptr(evecs), n, 3, n + 5, 0.0, F.ptr(out))
    for cap in (-0.5, 1.5, np.nan):
        assert "cap" in dpt_refused(lib.srx_dpt, gh.handle, 0, cap, F.ptr(out))
        assert "cap" in dpt_refused(lib.srx_dpt_from, ctx.handle, F.ptr(evals), F.ptr(evecs), n, 3, 0, cap, F.ptr(out))
    assert lib.srx_dpt_from(c2.handle, F.ptr(evals), F.ptr(evecs), n, 3, 0, 0.0, F.ptr(out)) == F.E_ARG
    assert "sharded" in lib.srx_last_error(c2.handle).decode() and (out == SENT).all()
    # max_matvecs = 5: SRX_E_NOCONV at once, the counters filled in
    g500, _ = handle(ctx, "traj500")
    ev, vec, info = np.full(15, SENT), np.full(500 * 15, SENT), F.DiffmapInfo()
    rc = lib.srx_diffmap(g500.handle, C.byref(opts(n_comps=0, max_matvecs=5)), F.ptr(ev), F.ptr(vec), C.byref(info))
    assert rc == F.E_NOCONV and lib.srx_last_error(ctx.handle)
    assert 1 <= info.matvecs <= 5 + info.ncv and info.ncv == 31 and info.n_comps == 15 and info.n == 500
    assert (ev == SENT).all() and (vec == SENT).all()
    _RUN.pop(("traj500", ()), None)
    # the context is still usable
    evals, evecs, info = solve_csr(ctx, (ip, ix, w), n_comps=3)
    assert info["n_comps"] == 3 and np.isfinite(evecs).all()

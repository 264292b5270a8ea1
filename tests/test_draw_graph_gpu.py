"""srx_draw_graph* on the device against the definition of include/srx.h (tests/draw_graph_ref.py): the forces through
srx_draw_graph_forces (masses, total mass and the four walk counters exactly: the same decisions; rep, grav and attr within
32 D), positions after 1 and 3 iterations with the speed rule's state, determinism, stop_after, the stated start, the handle's
slot, quality over the default run against the reference's own seed-to-seed range (tests/golden/draw_graph_kat.json) and the
refusals.

Tolerances.  Forces and positions: D = max |f64 numpy - longdouble numpy| of the case, computed here on the CPU; the device
gets 32 D, the factor of the UMAP and t-SNE tests (its order of summation differs from numpy's).  swing and traction are sums
of n non-negative terms added in another order than numpy's, so beside 32 times their own D they get n * 2^-53 of their value,
the bound of a reordered sum; the speed follows from them through the rule and gets the same.  speed_efficiency is a product
of the rule's constants: with the same branches (test_draw_graph_cpu.py shows the two references take the same ones) it is the
same bits.  The kernel stages levels 1 .. 4 of the pyramid in LDS and reads deeper cells from memory: levels 4 and 5 stand on
the two sides of that boundary."""
import ctypes as C

import numpy as np
import pytest

import draw_graph_ref as ref

pytestmark = pytest.mark.gpu

TOL_FACTOR = 32
LDS_LEVELS = 4


def P():
    from singlerust_amd.memory import processing
    return processing


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- forces -----------------------------------------------------------------------------------------------------------------------------
def check_forces(ctx, W, Y, theta, levels, name, strong=False, linlog=False, kr=2.0, g=1.0):
    want = ref.forces(W, Y, theta, levels, kr, g, strong, linlog)
    wantl = ref.forces(W, Y, theta, levels, kr, g, strong, linlog, dtype=np.longdouble)
    assert want[4] == wantl[4]                                                                               # the same decisions
    D = float(max(np.abs(a - b).max() for a, b in zip(want[:3], wantl[:3]))) if Y.shape[0] else 0.0
    rep, grav, attr, mass, fi = P().draw_graph_forces(ctx, W, Y, theta, levels, kr, g, strong, linlog)
    err = float(max(np.abs(a - b).max() for a, b in zip((rep, grav, attr), want[:3]))) if Y.shape[0] else 0.0
    print("%s n %d theta %g L %d flags %d%d: accepted %d exact %d pairs %d coincident %d | D %.3e 32D %.3e device %.3e"
          % (name, Y.shape[0], theta, fi["levels"], strong, linlog, fi["cells_accepted"], fi["cells_exact"], fi["pairs_exact"],
             fi["pairs_coincident"], D, TOL_FACTOR * D, err))
    assert fi == want[4], (name, theta, levels, fi, want[4])                  # counters, total mass, levels, side and lo: exactly
    assert np.array_equal(mass, want[3])
    assert err <= TOL_FACTOR * D
    return rep, grav, attr, fi


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257])
def test_forces_exact_sum_at_wave_and_workgroup_edges(ctx, n):
    W, Y = ref.knn_graph(n), ref.generic_layout(n)
    for levels in (0, 2):
        _, _, _, fi = check_forces(ctx, W, Y, 0.0, levels, "generic")
        assert fi["pairs_exact"] == n * (n - 1) and fi["cells_accepted"] == 0 and fi["pairs_coincident"] == 0
    check_forces(ctx, W, Y, 0.0, 0, "generic", strong=True, linlog=True, kr=0.5, g=3.0)


@pytest.mark.parametrize("theta", [0.5, 1.2, 1e9])
def test_forces_theta_and_levels(ctx, theta):
    n = 1500
    W, Y = ref.knn_graph(n), ref.generic_layout(n)
    assert ref.auto_levels(n) == LDS_LEVELS + 1
    for levels in (1, LDS_LEVELS, LDS_LEVELS + 1, 12):
        _, _, _, fi = check_forces(ctx, W, Y, theta, levels, "generic")
        assert fi["cells_accepted"] > 0 or levels == 1                 # a level-1 cell is too wide to accept at theta = 0.5
    check_forces(ctx, W, Y, theta, 0, "generic", strong=True, linlog=True)


@pytest.mark.parametrize("name", ref.EDGE_LAYOUTS)
def test_forces_edge_layouts(ctx, name):
    W, Y, levels = ref.edge_case(name)
    n = Y.shape[0]
    for theta in (0.5, 1.2):
        rep, grav, attr, fi = check_forces(ctx, W, Y, theta, levels, name)
    if name == "coincident":
        assert fi["side"] == 1.0 and not rep.any() and fi["pairs_coincident"] == fi["pairs_exact"] == n * (n - 1)
    if name == "two_coincident":
        assert fi["pairs_coincident"] == 2
    if name == "origin":
        assert not grav[77].any() and grav[76].any()
    if name.startswith("cell"):
        m = int(name[4:])
        assert fi["pairs_exact"] >= m * (m - 1)                                # every member opened its own cell
        check_forces(ctx, W, Y, 0.0, levels, name)
    if name == "two_clumps":
        for lv in (1, 12):
            check_forces(ctx, W, Y, 1.2, lv, name)
    if name == "isolated":
        assert not attr[100:].any() and attr[:100].any()
    if name == "star300":
        check_forces(ctx, W, Y, 1.2, levels, name, linlog=True)


# ---- iterations ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.POSITION_CASES)
def test_positions_after_1_and_3_iterations(ctx, name):
    W, Y0, seed, runs = ref.position_case(name)
    n = int(W[0].size) - 1
    y0 = ref.random_start(n, seed) if Y0 is None else Y0
    for iters, flags in runs:
        for n_iter, stop in ((500, iters), (iters, 0)):
            Y, want, _ = ref.layout(W, y0, n_iter, stop_after=stop, **flags)
            Yl, wantl, _ = ref.layout(W, y0, n_iter, stop_after=stop, dtype=np.longdouble, **flags)
            D = float(np.abs(Y - Yl).max())
            got, info = P().draw_graph_csr(ctx, W, Y0, n_iter=n_iter, seed=seed, stop_after=stop, strong_gravity=flags.get("strong", False),
                                           linlog=flags.get("linlog", False))
            err = float(np.abs(got - Y).max())
            print("%s iterations T %d stop %d flags %s: D %.3e 32D %.3e device %.3e max|y| %.3e | speed %.6e eff %.4f S %.6e Tr %.6e "
                  "(ref %.6e %.4f %.6e %.6e)" % (name, n_iter, stop, flags, D, TOL_FACTOR * D, err, float(np.abs(Y).max()), info["speed"],
                                                 info["speed_efficiency"], info["swing"], info["traction"], want["speed"],
                                                 want["speed_efficiency"], want["swing"], want["traction"]))
            assert err <= TOL_FACTOR * D
            for key in ("n", "nnz", "total_mass", "n_iter", "iters_run", "levels"):
                assert info[key] == want[key], (key, info[key], want[key])
            assert info["speed_efficiency"] == float(want["speed_efficiency"])
            for key in ("swing", "traction", "speed"):
                tol = TOL_FACTOR * abs(float(want[key]) - float(wantl[key])) + n * 2.0 ** -53 * abs(float(want[key]))
                assert abs(info[key] - float(want[key])) <= tol, (key, info[key], want[key], tol)
            # the walk of iteration 1 reads the start itself: the same decisions, exactly
            if iters == 1:
                assert all(info[c] == want[c] for c in ref.COUNTERS) and info["side"] == want["side"]


def test_determinism_stop_after_and_the_first_force(ctx):
    n = 300
    W = ref.knn_graph(n)
    a, ia = P().draw_graph_csr(ctx, W, None, seed=5, stop_after=6)
    b, ib = P().draw_graph_csr(ctx, W, None, seed=5, stop_after=6)
    assert np.array_equal(bits(a), bits(b))
    assert {k: v for k, v in ia.items() if k != "ms"} == {k: v for k, v in ib.items() if k != "ms"}
    full, _ = P().draw_graph_csr(ctx, W, None, seed=5, n_iter=6)
    assert np.array_equal(bits(a), bits(full))                                                              # the first 6 of 500
    other, _ = P().draw_graph_csr(ctx, W, None, seed=6, n_iter=6)
    assert not np.array_equal(a, other)
    # iteration 1 from a given start: F is srx_draw_graph_forces at the start, bit for bit.  With Fprev = 0 the swing is |F|,
    # and every operation from F to the new position is rounded once on both sides, so the position is reproduced exactly.
    y0 = 10.0 * ref.generic_layout(n, 5)
    y1, info = P().draw_graph_csr(ctx, W, y0, n_iter=1)
    rep, grav, attr, mass, _ = P().draw_graph_forces(ctx, W, y0)
    Fv = (rep + grav) + attr
    swing = np.sqrt(Fv[:, 0] * Fv[:, 0] + Fv[:, 1] * Fv[:, 1])
    factor = info["speed"] / (1.0 + np.sqrt(info["speed"] * (mass.astype(np.float64) * swing)))
    assert np.array_equal(bits(y1), bits(y0 + Fv * factor[:, None]))


def test_hashed_start_is_the_stated_hash(ctx):
    """Vertices without edges, no repulsion and no gravity: F = 0, so one iteration returns the start itself."""
    n = 65
    W = (np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0))
    for seed in (0, 9, 2 ** 64 - 1):
        got, info = P().draw_graph_csr(ctx, W, None, n_iter=1, seed=seed, scaling_ratio=0.0, gravity=0.0)
        assert np.array_equal(bits(got), bits(ref.random_start(n, seed))) and info["swing"] == 0.0 and info["total_mass"] == n
        assert (got >= 0).all() and (got < 1).all()


def test_no_point(ctx):
    W = (np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0))
    got, info = P().draw_graph_csr(ctx, W, None)
    assert got.shape == (0, 2) and info["n"] == 0 and info["iters_run"] == 0 and info["n_iter"] == 500
    rep, grav, attr, mass, fi = P().draw_graph_forces(ctx, W, np.zeros((0, 2)))
    assert rep.shape == (0, 2) and mass.size == 0 and fi["pairs_exact"] == 0


# ---- the handle ---------------------------------------------------------------------------------------------------------------------------
def run_on_handle(g, **kw):
    from singlerust_amd import _ffi as F
    d = dict(theta=1.2, scaling_ratio=2.0, gravity=1.0, jitter_tolerance=1.0, seed=0, n_iter=500, stop_after=0, levels=0,
             init=F.FA2_INIT_RANDOM, strong_gravity=0, linlog=0)
    d.update(kw)
    out, info = np.zeros((g.info()["n"], 2)), F.Fa2Info()
    opts = F.Fa2Opts(*[d[name] for name, _ in F.Fa2Opts._fields_])
    F.check(F.lib().srx_draw_graph(g.handle, C.byref(opts), None, F.ptr(out), C.byref(info)), g.ctx.handle)
    return out, info


def test_handle_equals_csr_and_keeps_its_other_results(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import diffmap, dim_red, draw_graph, louvain, neighbors, paga, umap
    from test_knn_gpu import _planted, _upload
    a = _upload(ctx, _planted())
    with pytest.raises(sr.SrxError):
        draw_graph(a)                                                               # no graph yet
    dim_red.pca_inplace(a, 20, None, None, None, sr.FeatureSelection.HighlyVariable(120), None)
    neighbors(a, n_neighbors=15, connectivities=True)
    g = a._graph
    with pytest.raises(sr.SrxError) as ei:
        P().graph_layout(g)                                                         # no layout yet
    assert "no srx_draw_graph has run" in str(ei.value)
    louvain(a)
    umap(a, n_epochs=20)
    diffmap(a, n_comps=5)
    before = (P().graph_labels(g), P().graph_embedding(g), *P().graph_diffmap(g), *g.fetch(F.GRAPH_CONNECTIVITIES), *g.fetch(F.GRAPH_DISTANCES))
    Cm = g.fetch(F.GRAPH_CONNECTIVITIES)
    got, info = run_on_handle(g, n_iter=20, seed=3)
    want, wi = P().draw_graph_csr(ctx, Cm, None, n_iter=20, seed=3)
    assert np.array_equal(bits(got), bits(want)) and np.isfinite(got).all()
    assert all(getattr(info, k) == v for k, v in wi.items() if k != "ms")
    assert info.total_mass == info.n + info.nnz == a.n_obs() + Cm[1].size
    assert np.array_equal(bits(P().graph_layout(g)), bits(got))
    after = (P().graph_labels(g), P().graph_embedding(g), *P().graph_diffmap(g), *g.fetch(F.GRAPH_CONNECTIVITIES), *g.fetch(F.GRAPH_DISTANCES))
    assert all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(before, after))
    # NULL opts: every default
    dflt, di = np.zeros((a.n_obs(), 2)), F.Fa2Info()
    F.check(F.lib().srx_draw_graph(g.handle, None, None, F.ptr(dflt), C.byref(di)), ctx.handle)
    assert di.n_iter == di.iters_run == 500 and np.isfinite(dflt).all() and di.speed > 0
    ref_dflt, _ = P().draw_graph_csr(ctx, Cm, None)
    assert np.array_equal(bits(dflt), bits(ref_dflt))
    # the scanpy chain: paga, a coarse layout of the groups, draw_graph(init_pos="paga")
    with pytest.raises(ValueError, match="paga"):
        draw_graph(a, init_pos="paga")
    paga(a)
    with pytest.raises(ValueError, match="pos"):
        draw_graph(a, init_pos="paga")
    G = a.uns["paga"]["sizes"].size
    ang = 2.0 * np.pi * np.arange(G) / G
    a.uns["paga"]["pos"] = 50.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    d = draw_graph(a, init_pos="paga", n_iter=30)
    Y = a.obsm["X_draw_graph_fa"]
    assert Y.shape == (a.n_obs(), 2) and np.isfinite(Y).all() and d["iters_run"] == 30
    assert a.uns["draw_graph"]["params"]["init_pos"] == "paga" and a.uns["draw_graph"]["info"] == d
    draw_graph(a, init_pos="X_draw_graph_fa", n_iter=2, key_added_ext="again")
    assert "X_draw_graph_again" in a.obsm and a.uns["draw_graph"]["params"]["init_pos"] == "X_draw_graph_fa"
    with pytest.raises(ValueError, match="layout"):
        draw_graph(a, layout="fr")
    with pytest.raises(ValueError, match="init_pos"):
        draw_graph(a, init_pos="X_nothing")


# ---- quality --------------------------------------------------------------------------------------------------------------------------------
def test_quality_over_the_default_run(ctx):
    """600 points in six separated clumps in 10 dimensions, the connectivities of their k = 30 list on a graph handle, the
    default 500 iterations from three hashed seeds: the label purity, recomputed here from the fetched layout, lies inside the
    reference's own seed-to-seed range (five other seeds) widened by that range on both sides."""
    g = ref.golden()["quality"]
    _, labels, idx, dist = ref.quality_graph(g)
    h = P().connectivities_from_knn(ctx, idx, dist)
    lo, hi = g["purity_range"]
    allowed = (lo - (hi - lo), hi + (hi - lo))
    for seed in (1, 2, 3):
        Y, info = run_on_handle(h, seed=seed)
        pur = ref.purity(Y, labels)
        print("quality seed %d: purity %.4f (reference range %s, networkx %s), speed %.4g, side %.6g, %.1f ms"
              % (seed, pur, g["purity_range"], g["networkx_purity"], info.speed, info.side, info.ms))
        assert info.iters_run == 500 and allowed[0] <= pur <= allowed[1]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import singlerust_amd as sr
    from singlerust_amd import _ffi as F
    lib = F.lib()
    n = 50
    W = ref.knn_graph(n)
    y0 = ref.generic_layout(n)

    def opts(**kw):
        d = dict(theta=1.2, scaling_ratio=2.0, gravity=1.0, jitter_tolerance=1.0, seed=0, n_iter=3, stop_after=0, levels=0,
                 init=F.FA2_INIT_GIVEN, strong_gravity=0, linlog=0)
        d.update(kw)
        return F.Fa2Opts(*[d[name] for name, _ in F.Fa2Opts._fields_])

    def refused(o, init=y0, w=W, c=None, nn=None):
        out = np.full((n, 2), 12345.0)
        info = F.Fa2Info()
        info.cells_exact = 777
        h = (c or ctx).handle
        rc = lib.srx_draw_graph_csr(h, F.ptr(w[0]), F.ptr(w[1]), F.ptr(w[2]), n if nn is None else nn, C.byref(o),
                                    None if init is None else F.ptr(init), F.ptr(out), C.byref(info))
        msg = lib.srx_last_error(h)
        assert rc == F.E_ARG and msg, (rc, msg)
        assert (out == 12345.0).all() and info.cells_exact == 777                                             # nothing written
        return msg.decode()

    for v in (-0.5, np.nan, np.inf):
        for key in ("theta", "scaling_ratio", "gravity", "jitter_tolerance"):
            assert key in refused(opts(**{key: v}))
    for v in (-1, 13):
        assert "levels" in refused(opts(levels=v))
    for v in (-1, 2 ** 20 + 1):
        assert "n_iter" in refused(opts(n_iter=v))
    assert "stop_after" in refused(opts(n_iter=3, stop_after=4))
    assert "stop_after" in refused(opts(stop_after=-1))
    assert "unknown start" in refused(opts(init=7))
    assert "start positions" in refused(opts(), init=None)
    for v in (np.nan, np.inf, -np.inf):
        bad = y0.copy()
        bad[7, 1] = v
        assert "NaN or Inf" in refused(opts(), init=bad)
    # what srx_louvain_csr refuses about a graph
    asym = (W[0], W[1], W[2].copy())
    asym[2][0] *= 2.0
    assert "symmetric" in refused(opts(), w=asym)
    neg = (W[0], W[1], -W[2])
    assert "weight" in refused(opts(), w=neg)
    # the total mass: n + nnz must stay below 2^32 (the row offsets alone say so; nothing else is read before the refusal)
    huge = (np.array([0] + [2 ** 32 - 1] * n, dtype=np.uint64), W[1], W[2])
    assert "2^32" in refused(opts(), w=huge)
    c2 = sr.Context(0)
    c2.comm_init_host(2, 0, lambda buf: None)
    assert "sharded" in refused(opts(), c=c2)
    # the forces
    for key, v in (("theta", -1.0), ("theta", np.nan), ("scaling_ratio", np.inf), ("gravity", -2.0), ("levels", -1), ("levels", 13)):
        r = np.full((n, 2), 5.0)
        o = opts(**{key: v})
        assert lib.srx_draw_graph_forces(ctx.handle, F.ptr(W[0]), F.ptr(W[1]), F.ptr(W[2]), n, F.ptr(y0), C.byref(o), F.ptr(r), None, None,
                                         None, None) == F.E_ARG
        assert key in lib.srx_last_error(ctx.handle).decode() and (r == 5.0).all()
    bad = y0.copy()
    bad[0, 0] = np.nan
    r = np.full((n, 2), 5.0)
    assert lib.srx_draw_graph_forces(ctx.handle, F.ptr(W[0]), F.ptr(W[1]), F.ptr(W[2]), n, F.ptr(bad), None, F.ptr(r), None, None, None,
                                     None) == F.E_ARG and (r == 5.0).all()
    for fn, args in (("srx_draw_graph", (None, None, None, None, None)), ("srx_graph_layout_fetch", (None, None)),
                     ("srx_draw_graph_csr", (None, None, None, None, 0, None, None, None, None)),
                     ("srx_draw_graph_forces", (None, None, None, None, 0, None, None, None, None, None, None, None))):
        assert getattr(lib, fn)(*args) == F.E_ARG, fn
    # the context is still usable
    got, info = P().draw_graph_csr(ctx, W, y0, n_iter=3)
    assert info["iters_run"] == 3 and np.isfinite(got).all()

"""graph.hip at the edges of its kernels, on the fixtures of graph_edges.py (test_graph_edges_cpu.py holds their
preconditions), through connectivities_from_knn and the C ABI, against the host restatement graph_ref.graph.

The checks and tolerances are those of test_graph_gpu.py (check_against_restatement: D, rho, both patterns and all
counters exact, directed weights 1e-8, C 2e-8, row sums 1e-9, clamped sigma within 4 ulp of the floor); no row, k or
fixture is exempted.  Two cases carry more than that, both derived in their tests: scaling the distances by a power of two
must leave every stored bit of C unchanged, and subnormal distances get the bound that the width of the last bracket gives.
profiles/graph.md has the errors measured on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import graph_edges as E
import graph_ref
from test_graph_gpu import FIGURES, TOL_A, build, check_against_restatement, check_properties, fetch_all

pytestmark = pytest.mark.gpu


def run(ctx, idx, dist):
    g = build(ctx, idx, dist)
    got = fetch_all(g)
    g.free()
    return got


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def summary(case, labels):
    """One line per case for profiles/graph.md: the worst figures over the comparisons the case made."""
    f = np.array([FIGURES[l] for l in labels])
    print(f"PROFILE {case}: comparisons {len(labels)}, max |a - a_ref| {f[:, 0].max():.1e}, max |sum a - T| {f[:, 1].max():.1e}, "
          f"max |C - C_ref| {f[:, 2].max():.1e}")


# ---- 1. every k ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k0", [1, 17, 33, 49])
def test_every_k(ctx, k0):
    """k = 1 .. 64 (sixteen per case) at n = k + 1, k + 2, 2 k + 3: every lane count of the ballots, of below(p), of the
    counting sort and of the binary searches; n < 4 is one partial workgroup, n = k + 1 has every edge mutual."""
    labels = []
    for k in range(k0, k0 + 16):
        for n in E.every_k_sizes(k):
            idx, dist = E.every_k_list(k, n)
            got = run(ctx, idx, dist)
            labels.append(f"every k: k={k} n={n}")
            want, sc = check_against_restatement(idx, dist, got, labels[-1])
            info = got[0]
            if n == k + 1:
                assert info["n_mutual"] == n * k // 2
                assert info["nnz_connectivities"] == n * k - info["entries_dropped"]
                assert (np.diff(got[2][0].astype(np.int64)) <= k).all()                        # no in-only entry anywhere
            if k == 1:
                assert info["rows_no_root"] == n and info["rows_clamped"] == n and (got[2][2] == 1.0).all()
            else:
                assert info["rows_no_root"] == 0
    if k0 == 1:
        got = run(ctx, *E.every_k_list(1, 2))                                                  # the smallest graph there is
        assert got[0]["nnz_connectivities"] == 2 and got[2][1].tolist() == [1, 0] and got[2][2].tolist() == [1.0, 1.0]
    summary(f"every k {k0}..{k0 + 15}", labels)


# ---- 2. integer T -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", E.INTEGER_T_KS)
def test_integer_T(ctx, k):
    """c == T exactly in the even rows (no root, sigma = the floor), c == T - 1 in the odd ones (a root): the device's
    log2(k + 1) has to be the integer, or rows_no_root and those rows' weights move."""
    idx, dist, c = E.integer_T_list(k)
    n = len(idx)
    got = run(ctx, idx, dist)
    label = f"integer T: k={k}"
    want, sc = check_against_restatement(idx, dist, got, label)
    tied = c == int(np.log2(k + 1.0))
    assert got[0]["rows_no_root"] == int(tied.sum()) == (n if k == 1 else (n + 1) // 2)
    assert got[0]["rows_clamped"] == int(tied.sum())
    floor = 1e-3 * got[1][2].reshape(n, k).sum(axis=1) / (k + 1.0)
    sigma = got[4]
    assert (np.abs(sigma[tied] - floor[tied]) <= 4 * np.spacing(floor[tied])).all()
    assert (sigma[~tied] > floor[~tied]).all()                                                 # a root above the floor
    summary(label, [label])


# ---- 3. upward bracket --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", E.UPWARD_KS)
def test_upward_bracket(ctx, k):
    """Rows with S(max x) < T double hi (all 400 at k = 2, 225 / 56 / 40 at k = 3 / 4 / 5); such a row ends with sigma above
    max x, the others at or below it."""
    idx, dist = E.upward_list(k)
    got = run(ctx, idx, dist)
    label = f"upward bracket: k={k}"
    check_against_restatement(idx, dist, got, label)
    S, c, T = E.s_at_max_x(dist)
    xmax = (dist - got[3][:, None]).max(axis=1)
    up = S < T
    assert up.any() and (got[4][up] > xmax[up]).all() and (got[4][~up] <= xmax[~up]).all()
    print(f"{label}: {int(up.sum())} rows bracket upwards, {int((~up).sum())} downwards")
    summary(label, [label])


# ---- 4. long downward bracket, clamp and drop in one row ----------------------------------------------------------------
def test_long_downward_bracket(ctx):
    idx, dist = E.long_bracket_list()
    n, k = idx.shape
    got = run(ctx, idx, dist)
    want, sc = check_against_restatement(idx, dist, got, "long bracket")
    info = got[0]
    assert (info["rows_clamped"], info["entries_dropped"], info["nnz_connectivities"]) == (20, 400, 800)
    even = np.arange(n) % 2 == 0
    a = graph_ref.weights(got[1][2].reshape(n, k), got[3], got[4])
    assert ((a[even] == 1.0).sum(axis=1) == 5).all() and ((a[even] == 0.0).sum(axis=1) == 10).all()
    assert ((got[4][~even] > 3.9e299) & (got[4][~even] < 4.1e299)).all()
    summary("long bracket", ["long bracket"])


# ---- 5. scale -----------------------------------------------------------------------------------------------------------
def test_powers_of_two_leave_C_unchanged(ctx):
    """Scaling the distances by 2^e is exact, and every step of the definition is homogeneous in them or dimensionless (rho,
    x, doubling and halving, lo + 0.5 (hi - lo), the floor, x / s, the 1e-13 test on S): C keeps its bits, rho and sigma
    scale exactly, the counters stay.  A failure names an operation with an absolute constant or a narrower type."""
    idx, dist = E.scale_list()
    base = run(ctx, idx, dist)
    check_against_restatement(idx, dist, base, "scale e=0")
    labels = ["scale e=0"]
    for e in E.SCALE_EXACT:
        scaled = np.ldexp(dist, e)
        got = run(ctx, idx, scaled)
        labels.append(f"scale e={e}")
        check_against_restatement(idx, scaled, got, labels[-1])
        assert got[0] == base[0], (e, got[0], base[0])
        for a, b in zip(got[2], base[2]):
            assert same_bits(a, b), e
        assert same_bits(got[1][0], base[1][0]) and same_bits(got[1][1], base[1][1])
        assert same_bits(got[1][2], np.ldexp(base[1][2], e)), e
        assert same_bits(got[3], np.ldexp(base[3], e)), e
        bad = np.nonzero(got[4] != np.ldexp(base[4], e))[0]
        assert len(bad) == 0, (e, bad[:5], got[4][bad[:5]], np.ldexp(base[4], e)[bad[:5]])
    summary("scale 2^e, e in 0, -1000, -500, 500, 1000, 1015", labels)


def test_overflowing_row_sums(ctx):
    """e = 1021: sum d is +inf in 224 of the 300 rows; read literally in IEEE f64 the floor and sigma are +inf there, every
    weight of the row is 1 and the row counts as clamped (include/srx.h says so)."""
    idx, dist = E.scale_list()
    n, k = idx.shape
    scaled = np.ldexp(dist, E.SCALE_OVERFLOW)
    got = run(ctx, idx, scaled)
    with np.errstate(over="ignore"):
        want, sc = check_against_restatement(idx, scaled, got, "scale e=1021")
        over = np.isinf(scaled.sum(axis=1))
    assert 150 <= over.sum() < n and got[0]["rows_clamped"] == int(over.sum())
    assert (got[4][over] == np.inf).all() and np.isfinite(got[4][~over]).all()
    assert (graph_ref.weights(got[1][2].reshape(n, k), got[3], got[4])[over] == 1.0).all()
    summary("scale e=1021 (overflowing sums)", ["scale e=1021"])


def check_on_the_coarse_grid(idx, dist, got, label):
    """Subnormal distances: sigma lives on a grid too coarse for |S - T| <= 1e-9 (the restatement's own row sums miss by
    3e-4), so the weights get the bound the grid gives.  Both sides end on adjacent doubles (lo, hi) around the same root and
    a is non-decreasing in sigma: |a_dev - a_ref| <= a(hi) - a(lo) + TOL_A per entry; C = a + b - a b has partial
    derivatives in [0, 1]: the bounds of its two directed entries add.  D, rho, both patterns and the counters are exact."""
    info, d, c, rho, sigma = got
    n, k = idx.shape
    D, Cr, sc, A, want = graph_ref.graph(idx, dist)
    check_properties(info, d, c)
    assert np.array_equal(d[0].astype(np.int64), D.indptr) and np.array_equal(d[1].astype(np.int64), D.indices)
    assert np.array_equal(d[2], D.data) and np.array_equal(rho, sc["rho"])
    assert info == want, (label, info, want)
    assert np.array_equal(c[0].astype(np.int64), Cr.indptr) and np.array_equal(c[1].astype(np.int64), Cr.indices)
    free = sc["has_root"] & ~sc["clamped"]
    lo, hi = np.where(free, sc["lo"], sc["sigma"]), np.where(free, sc["hi"], sc["sigma"])
    dd = d[2].reshape(n, k)
    a_dev, a_ref = graph_ref.weights(dd, rho, sigma), A.data.reshape(n, k)
    bound = graph_ref.weights(dd, rho, hi) - graph_ref.weights(dd, rho, lo) + TOL_A
    assert (bound >= TOL_A).all()
    err_a = np.abs(a_dev - a_ref)
    assert (err_a <= bound).all(), (label, float((err_a - bound).max()))
    assert ((sigma >= lo) & (sigma <= hi))[free].all(), label                 # the device ends inside the same bracket
    both = np.zeros((n, n))
    both[np.repeat(np.arange(n), k), d[1].astype(np.int64)] = bound.ravel()
    both = both + both.T
    rows = np.repeat(np.arange(n), np.diff(Cr.indptr))
    err_c = np.abs(c[2] - Cr.data)
    assert (err_c <= both[rows, Cr.indices]).all(), (label, float(err_c.max()))
    miss = np.abs(a_dev[free].sum(axis=1) - sc["T"]).max()
    print(f"PROFILE {label}: max |a - a_ref| {err_a.max():.1e} (bound {bound.max():.1e}), max |sum a - T| {miss:.1e}, "
          f"max |C - C_ref| {err_c.max():.1e}")
    return sc


def test_subnormal_distances(ctx):
    idx, dist = E.scale_list()
    scaled = np.ldexp(dist, E.SCALE_SUBNORMAL)
    check_on_the_coarse_grid(idx, scaled, run(ctx, idx, scaled), "scale e=-1060 (subnormal)")
    # the lo == 0.0 exit of the downward bracket: distances of one and two units, sigma = one unit on both sides
    idx, dist = E.lo_zero_list()
    got = run(ctx, idx, dist)
    check_on_the_coarse_grid(idx, dist, got, "one-unit distances (lo == 0)")
    assert (got[4] == E.TINY).all() and got[0]["rows_clamped"] == 0 and got[0]["rows_no_root"] == 0


# ---- 6. window edges of the long-list ordering ---------------------------------------------------------------------------
def test_window_edges_of_the_long_lists(ctx):
    """Three hubs at n = 2^17 + 700: a list with nothing in the first window, one across the boundary with 2^17 - 1 and 2^17
    in it, one with nothing in the second window while the hub's own number lies there."""
    idx, dist, sources = E.window_list()
    got = run(ctx, idx, dist)
    check_against_restatement(idx, dist, got, "windows")
    ptr, ind, dat = got[2]
    for h, src in sources.items():
        cols = ind[int(ptr[h]):int(ptr[h + 1])]
        assert np.array_equal(cols, np.sort(np.concatenate([idx[h], src]))), h
        assert np.array_equal(cols[~np.isin(cols, idx[h])], src), h
    summary("windows", ["windows"])


# ---- 7. merge with dropped out-edges -------------------------------------------------------------------------------------
def test_merge_with_holes_in_the_kept_mask(ctx):
    idx, dist, sources = E.merge_holes_list()
    got = run(ctx, idx, dist)
    check_against_restatement(idx, dist, got, "merge holes")
    assert got[0]["entries_dropped"] == 20
    ptr, ind, dat = got[2]
    for (h, src), length in zip(sources.items(), E.MERGE_LENGTHS):
        cols = ind[int(ptr[h]):int(ptr[h + 1])]
        kept = idx[h][dist[h] == 1.0]
        assert len(cols) == length + 3
        assert np.array_equal(cols, np.sort(np.concatenate([kept, src]))), h
        assert not np.isin(idx[h][dist[h] == 3.0], cols).any()
    summary("merge holes", ["merge holes"])


# ---- 8. refusals at the edges --------------------------------------------------------------------------------------------
def test_refusals_at_the_edges(ctx):
    """Every defect in the first lane of the first row, the last lane of the last row and the first row of the partial last
    workgroup; then four kinds at once (the range message wins).  Each refusal is SRX_E_ARG with a null handle, and the
    context builds the right graph straight after it."""
    from singlerust_amd import _ffi as F
    lib = F.lib()
    idx, dist = E.refusal_list()
    n, k = idx.shape
    good = run(ctx, idx, dist)
    check_against_restatement(idx, dist, good, "refusals: the sound list")
    for label, i, d, word in E.defects(idx, dist):
        i, d = np.ascontiguousarray(i), np.ascontiguousarray(d)
        assert i.shape == (n, k) and d.shape == (n, k)
        h = C.c_void_p(1)
        rc = lib.srx_neighbors_from_knn(ctx.handle, F.ptr(i), F.ptr(d), n, k, C.byref(h))
        msg = lib.srx_last_error(ctx.handle).decode()
        assert rc == F.E_ARG and not h.value and word in msg, (label, rc, h.value, msg)
        after = run(ctx, idx, dist)
        assert after[0] == good[0], label
        for a, b in zip(after[1] + after[2] + after[3:], good[1] + good[2] + good[3:]):
            assert same_bits(a, b), label

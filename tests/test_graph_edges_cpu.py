"""Preconditions of the graph-edge fixtures (graph_edges.py), proved on the host restatement alone: each list is valid and
exercises the branch it is named for.  test_graph_edges_gpu.py relies on these figures."""
import numpy as np
import pytest

import graph_edges as E
import graph_ref


def _rows_sum_to_T(sc, a):
    free = sc["has_root"] & ~sc["clamped"]
    return np.abs(a[free].sum(axis=1) - sc["T"]).max() if free.any() else 0.0


# ---- 1. every k ---------------------------------------------------------------------------------------------------------
def test_every_k_lists_are_valid_and_the_restatement_solves_them():
    worst = 0.0
    for k in range(1, 65):
        for n in E.every_k_sizes(k):
            idx, dist = E.every_k_list(k, n)
            assert idx.shape == (n, k) and dist.min() >= 0.5 and dist.max() <= 2.0
            E.assert_valid(idx)
            D, Cm, sc, A, info = graph_ref.graph(idx, dist)
            worst = max(worst, _rows_sum_to_T(sc, A.data.reshape(n, k)))
            if n == k + 1:                                     # every row names all the others
                assert info["n_mutual"] == n * k // 2 and E.in_only_lists(idx).nnz == 0
                assert info["nnz_connectivities"] == n * k - info["entries_dropped"]
            if k == 1:
                assert info["rows_no_root"] == n and (A.data == 1.0).all()
            else:
                assert info["rows_no_root"] == 0
    print("every k: worst |sum a - T| of the restatement", worst)
    assert worst <= 1e-12
    idx, dist = E.every_k_list(1, 2)                           # the smallest graph there is
    assert idx.tolist() == [[1], [0]]


# ---- 2. integer T -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", E.INTEGER_T_KS)
def test_integer_T_classes(k):
    t = np.log2(k + 1.0)
    assert t == int(t)                                         # the host's log2 gives the integer exactly
    idx, dist, c = E.integer_T_list(k)
    n = len(idx)
    E.assert_valid(idx)
    D, Cm, sc, A, info = graph_ref.graph(idx, dist)
    assert np.array_equal(sc["c"], c)
    tied = c == int(t)
    assert np.array_equal(sc["has_root"], ~tied) and np.array_equal(sc["clamped"], tied)
    assert (sc["sigma"][tied] == sc["floor"][tied]).all()
    assert info["rows_no_root"] == int(tied.sum()) == (n if k == 1 else (n + 1) // 2)
    if k > 1:
        assert (c[~tied] == int(t) - 1).all() and (~tied).sum() == n // 2
        assert _rows_sum_to_T(sc, A.data.reshape(n, k)) <= 1e-12


# ---- 3. upward bracket --------------------------------------------------------------------------------------------------
def test_upward_bracket_census():
    census = {}
    for k in E.UPWARD_KS:
        idx, dist = E.upward_list(k)
        E.assert_valid(idx)
        S, c, T = E.s_at_max_x(dist)
        assert (c < T).all()                                   # every row has a root: it takes one branch or the other
        census[k] = (int((S < T).sum()), int((S >= T).sum()))
    print("rows starting (below T: bracket upwards, at or above T: downwards):", census)
    assert census[2] == (E.UPWARD_N, 0)
    for k in (3, 4):
        assert census[k][0] > 0 and census[k][1] > 0
    assert census[5][0] >= 10 and census[5][1] >= 10
    # the same census from the restatement's own first step: a row that starts below T ends above max x, and only such a row
    for k in E.UPWARD_KS:
        idx, dist = E.upward_list(k)
        sc, a = graph_ref.scales(dist)
        S, c, T = E.s_at_max_x(dist)
        xmax = (dist - sc["rho"][:, None]).max(axis=1)
        assert np.array_equal(sc["sigma_star"] > xmax, S < T)


# ---- 4. long downward bracket -------------------------------------------------------------------------------------------
def test_long_bracket_figures():
    idx, dist = E.long_bracket_list()
    n, k = idx.shape
    E.assert_valid(idx)
    D, Cm, sc, A, info = graph_ref.graph(idx, dist)
    assert info["rows_clamped"] == 20 and info["entries_dropped"] == 400 and info["nnz_connectivities"] == 800
    assert info["rows_no_root"] == 0 and info["n_mutual"] == 0
    even = np.arange(n) % 2 == 0
    assert np.array_equal(sc["clamped"], even)
    assert ((sc["sigma_star"][even] > 6e-300) & (sc["sigma_star"][even] < 8e-300)).all()      # ~1990 halvings below 1e300
    assert np.log2(1e300) - np.log2(sc["sigma_star"][even].max()) > 1980
    assert np.allclose(sc["floor"][even], 6.25e296, rtol=1e-12)
    assert ((sc["sigma_star"][~even] > 3.9e299) & (sc["sigma_star"][~even] < 4.1e299)).all()
    a = A.data.reshape(n, k)
    assert set(np.unique(a[even])) == {0.0, 1.0} and ((a[even] == 0).sum(axis=1) == 10).all()
    assert _rows_sum_to_T(sc, a) <= 1e-12


# ---- 5. scale -----------------------------------------------------------------------------------------------------------
def _bits(m):
    return m.indptr.tolist(), m.indices.tolist(), m.data.view(np.uint64).tolist()


def test_restatement_is_bit_invariant_under_powers_of_two():
    idx, dist = E.scale_list()
    E.assert_valid(idx)
    D0, C0, sc0, A0, info0 = graph_ref.graph(idx, dist)
    assert info0["rows_no_root"] == 0 and info0["rows_clamped"] == 0 and info0["entries_dropped"] == 0
    for e in E.SCALE_EXACT:
        scaled = np.ldexp(dist, e)
        assert np.array_equal(np.ldexp(scaled, -e), dist)                  # the scaling itself is exact
        D, Cm, sc, A, info = graph_ref.graph(idx, scaled)
        assert info == info0 and _bits(Cm) == _bits(C0) and _bits(A) == _bits(A0), e
        assert np.array_equal(sc["rho"], np.ldexp(sc0["rho"], e)) and np.array_equal(sc["sigma"], np.ldexp(sc0["sigma"], e)), e


def test_overflowing_row_sums_clamp_to_infinity():
    idx, dist = E.scale_list()
    n, k = idx.shape
    scaled = np.ldexp(dist, E.SCALE_OVERFLOW)
    assert np.isfinite(scaled).all()
    with np.errstate(over="ignore"):
        D, Cm, sc, A, info = graph_ref.graph(idx, scaled)
        over = np.isinf(scaled.sum(axis=1))
    print("rows whose sum of distances overflows:", int(over.sum()), "of", n)
    assert 150 <= over.sum() < n                                             # most rows, and some of the other kind
    assert np.array_equal(np.isinf(sc["floor"]), over) and np.array_equal(sc["clamped"], over)
    assert np.isinf(sc["sigma"][over]).all() and np.isfinite(sc["sigma"][~over]).all()
    assert (A.data.reshape(n, k)[over] == 1.0).all() and info["rows_clamped"] == int(over.sum())
    assert info["rows_no_root"] == 0 and np.isfinite(sc["sigma_star"]).all()


def test_subnormal_distances_leave_a_coarse_grid():
    idx, dist = E.scale_list()
    n, k = idx.shape
    scaled = np.ldexp(dist, E.SCALE_SUBNORMAL)
    assert scaled.max() < 2.0 ** -1022 and scaled.min() >= 8192 * E.TINY
    D, Cm, sc, A, info = graph_ref.graph(idx, scaled)
    assert sc["has_root"].all() and not sc["clamped"].any()
    assert (sc["hi"] - sc["lo"] == E.TINY).all() and ((sc["sigma_star"] == sc["lo"]) | (sc["sigma_star"] == sc["hi"])).all()
    miss = _rows_sum_to_T(sc, A.data.reshape(n, k))
    print("subnormal distances: the restatement's own row sums miss T by", miss)
    assert 1e-9 < miss < 1e-3                                                # why this case has a bound of its own
    # the lo == 0.0 exit of the downward bracket
    idx, dist = E.lo_zero_list()
    E.assert_valid(idx)
    sc, a = graph_ref.scales(dist)
    assert sc["has_root"].all() and (sc["lo"] == 0.0).all() and (sc["hi"] == E.TINY).all() and (sc["sigma"] == E.TINY).all()
    assert (sc["floor"] == 0.0).all() and not sc["clamped"].any()


# ---- 6. window edges ----------------------------------------------------------------------------------------------------
def test_window_hubs_have_the_intended_in_only_lists():
    idx, dist, sources = E.window_list()
    n, k = idx.shape
    assert (n, k) == (E.WINDOW_N, 2)
    E.assert_valid(idx)
    lists = E.in_only_lists(idx)
    lens = np.diff(lists.indptr)
    assert sorted(np.nonzero(lens > 512)[0].tolist()) == sorted(sources)     # three long lists, the hubs'
    for h, src in sources.items():
        assert len(src) > 512 and np.array_equal(lists[h].indices, src)
    a, b, c = (sources[h] for h in sorted(sources))
    ha, hb, hc = sorted(sources)
    W = E.WINDOW
    assert ha < W and a.min() >= W                                           # (a) first window empty
    assert hb < W and b.min() < W <= b.max() and W - 1 in b and W in b       # (b) both sides of the boundary
    assert hc >= W and c.max() < W                                           # (c) second window empty, the hub lies in it
    every = np.concatenate([a, b, c])
    assert len(np.unique(every)) == len(every) and not np.isin(every, list(sources)).any()
    assert not np.isin(idx[list(sources)], every).any()                      # no hub names a source


# ---- 7. merge with dropped out-edges ------------------------------------------------------------------------------------
def test_merge_fixture_drops_two_out_edges_of_every_hub():
    idx, dist, sources = E.merge_holes_list()
    n, k = idx.shape
    E.assert_valid(idx)
    lists = E.in_only_lists(idx)
    D, Cm, sc, A, info = graph_ref.graph(idx, dist)
    assert info["entries_dropped"] == 20
    holes = 0
    for (h, src), length in zip(sources.items(), E.MERGE_LENGTHS):
        assert len(src) == length and np.array_equal(lists[h].indices, src)
        assert sc["c"][h] == 3 and not sc["has_root"][h] and sc["clamped"][h] and abs(sc["sigma"][h] - 1.5e-3) < 1e-18
        kept = np.sort(idx[h][dist[h] == 1.0])
        row = Cm[h].indices
        assert len(row) == length + 3 and np.array_equal(row, np.sort(np.concatenate([kept, src])))
        # a hole: a dropped out-edge with a kept one above it in column order
        holes += int(idx[h][dist[h] == 3.0].min() < kept.max())
    assert holes >= 3


# ---- 8. refusals --------------------------------------------------------------------------------------------------------
def test_refusal_lists_stay_inside_the_arrays():
    idx, dist = E.refusal_list()
    assert idx.shape == (E.REFUSAL_N, E.REFUSAL_K) == dist.shape
    E.assert_valid(idx)
    cases = E.defects(idx, dist)
    assert len(cases) == 13
    for label, i, d, word in cases:
        assert i.shape == idx.shape and d.shape == dist.shape and i.dtype == np.uint32 and d.dtype == np.float64
        changed = int((i != idx).sum()) + int((d != dist).sum())
        assert changed == (4 if label == "all four" else 1), label

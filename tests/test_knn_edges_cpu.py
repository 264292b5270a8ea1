"""Preconditions of the cases of test_knn_edges_gpu.py, without a device: every case is exactly representable, sits at the
dispatch boundary, tile edge or certificate condition it is named for, and the host restatement of eps_row says which rows
are certainly proven or certainly refused.  A case that stops exercising its target fails here."""
import numpy as np
import pytest

import knn_ref as R

CASES = R.all_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_exact_in_f64(name):
    """Coordinates are integers times one power of two, every squared distance stays below 2^53 units^2, and the scaled
    values neither overflow nor go subnormal: the int64 expectation is also what exact f64 arithmetic gives."""
    case = CASES[name]()
    assert case.name == name and case.units.dtype == np.int64
    ref, qry = case.points()
    for x, u in ((ref, case.units), (qry, case.query)):
        if x is None:
            continue
        assert np.array_equal(np.ldexp(x, -case.exp), (u + case.shift).astype(np.float64))
        nz = x[x != 0]
        assert np.isfinite(x).all() and (len(nz) == 0 or np.abs(nz).min() > 2.0 ** -1000)
    dmax = case.max_d2()
    assert 0 <= dmax < 2 ** 53
    scaled = np.ldexp(float(dmax), 2 * case.exp)
    assert np.isfinite(scaled) and (dmax == 0 or scaled > 2.0 ** -1000)
    assert 1 <= case.d <= 128
    for inc in case.selfs:
        adm = R.admissible(len(case.units), case.self_graph, inc)
        assert all(1 <= k <= min(64, adm) for k in R.run_ks(case, inc)), (name, inc)


def test_expectation_breaks_ties_to_the_lower_index():
    case = R.Case("tiny", np.array([[0], [2], [1], [1], [-1]], dtype=np.int64))
    idx, d2, _ = case.expected(False)
    assert idx[0].tolist() == [2, 3, 4, 1] and d2[0].tolist() == [1, 1, 1, 4]
    assert case.expected(True)[0][2].tolist() == [2, 3, 0, 1, 4]
    idx, dist = R.Case("tiny2", np.array([[0, 0], [3, 4]], dtype=np.int64), exp=-3).expected_k(1)
    assert idx.tolist() == [[1], [0]] and dist.tolist() == [[0.625], [0.625]]


def test_widths_and_boundaries():
    assert [R.width(d) for d in R.WIDTH_DIMS] == [8, 8, 20, 20, 36, 36, 52, 52, 68, 68, 132, 132, 132]
    assert {R.width(d) for d in R.WIDTH_DIMS} == set(R.WIDTHS)
    last_slot = [d for d in R.WIDTH_DIMS if d == R.width(d) - 1]           # the norm is the last coordinate of the instance
    assert last_slot == [7, 19, 35, 51, 67]
    assert {d % 2 for d in R.WIDTH_DIMS} == {0, 1} and 1 in R.WIDTH_DIMS
    assert R.BLIND_N % 32 != 0 and R.BLIND_N % 64 != 0 and R.BLIND_N > 8 * 128     # several query blocks, a ragged last tile


@pytest.mark.parametrize("d", R.WIDTH_DIMS)
def test_blind_data_is_below_the_f32_error_bound(d):
    """Inside a cluster the whole window from the nearest to the K'-th neighbour is narrower than eps_row, the honest bound
    on the f32 score's error: the f32 pass cannot order these neighbours, and rounding the centred points to f32 moves them."""
    case = R.blind_case(d)
    ref, _ = case.points()
    eps, Rmax = R.eps_row(ref, None)
    assert 2.0 ** 12 < Rmax < 2.0 ** 14 and np.isfinite(eps).all()
    _, d2, _ = case.expected(False)
    window = np.ldexp((d2[:, -1] - d2[:, 0]).astype(np.float64), 2 * case.exp)           # k = 1 .. K' = 72
    assert (window < 0.01 * eps).all(), (window / eps).max()
    assert (window < 2.0 ** -10 * eps).any()                      # eps / 4096 would still "prove" rows on f32 noise alone
    c = ref - ref.mean(axis=0)
    assert (c.astype(np.float32).astype(np.float64) != c).mean() > 0.5


def test_switches_are_crossed():
    ks = R.SWITCH_KS
    rounds = {k: (k + R.SLACK + 63) // 64 for k in ks}             # 64-candidate rounds of the re-rank
    assert rounds[56] == 1 and rounds[57] == 2
    caps = {k: R.cap(k + R.SLACK) for k in ks}
    assert caps[36] == 2 * 44 + 32 == 120 and 2 * (37 + 8) + 32 > 120 and caps[37] == 120 and caps[35] == 118
    assert caps[64] == 120 and 64 + R.SLACK <= 120 - 32            # K' = 72 fits what a merge keeps
    case = R.switch_case()
    assert case.units.shape == (700, 20) and case.selfs == (False, True)
    for inc in (False, True):
        _, d2, _ = case.expected(inc)
        for k in ks:
            if not (inc and k == 1):           # ties at the cut, so the lower index decides (k = 1 with self: the row itself)
                assert (d2[:, k - 1] == d2[:, k]).sum() >= 30, (k, inc)
            assert R.n_candidates(k, 700, True, inc) == k + 8


def test_point_counts_cover_the_tile_and_partial_sum_edges():
    ns = R.COUNT_NS
    for edge in (32, 64, 128, 256):
        assert {edge - 1, edge, edge + 1} <= set(ns)
    assert {n for n in ns if n <= 64} and {(n + 63) // 64 for n in ns} >= {1, 2, 3, 4, 5}          # one reference tile .. five
    assert {min(1024, (n + 255) // 256) for n in (256, 257)} == {1, 2}                             # n_part goes 1 -> 2
    assert min((n % 128) / 128 for n in ns if n > 128) < 0.01      # a query block that is nearly all padding (n = 129, 257)
    # K' = min(k + 8, admissible) is reached from both sides: clipped to the admissible count, and k + 8 below it
    kp = {(n, inc): R.n_candidates(min(64, n - (not inc)), n, True, inc) for n in ns for inc in (False, True)}
    assert kp[(72, True)] == 72 and kp[(72, False)] == 71 and kp[(73, False)] == 72 and kp[(300, False)] == 72
    assert kp[(2, False)] == 1 and kp[(10, False)] == 9 and kp[(9, True)] == 9
    for d in R.COUNT_DIMS:
        for nr, nq in R.PAIRS:
            case = R.pair_case(nr, nq, d)
            assert (case.query[::2] == case.units[(np.arange(nq)[::2] * 5) % nr]).all()           # exact copies of reference rows
            assert case.expected(False)[1][::2, 0].max() == 0
    assert {nq / nr for nr, nq in R.PAIRS} >= {200.0, 1 / 64, 1 / 300}


@pytest.mark.parametrize("dim", sorted(R.LINE_DIRS))
def test_line_orders_and_merge_pressure(dim):
    """Pairs at +-j tie exactly; in the organ-pipe order every sub-tile is nearer to the middle queries than everything
    before it, so at K' = 72 / CAP = 120 every sub-tile after the first forces a merge."""
    pos = {o: R.line_positions(o) for o in R.LINE_ORDERS}
    for o, v in pos.items():
        assert sorted(v.tolist()) == list(range(R.LINE_N)), o
    assert pos["organ_pipe"][:4].tolist() == [0, R.LINE_N - 1, 1, R.LINE_N - 2]
    scale = sum(c * c for c in R.LINE_DIRS[dim])
    case = R.line_case(dim, "organ_pipe")
    idx, d2, _ = case.expected(False)
    v = pos["organ_pipe"]
    mid = int(np.nonzero(v == R.LINE_N // 2)[0][0])
    assert d2[mid, :6].tolist() == [scale * j * j for j in (1, 1, 2, 2, 3, 3)]
    assert idx[mid, 0] < idx[mid, 1] and {int(v[idx[mid, 0]]), int(v[idx[mid, 1]])} == {R.LINE_N // 2 - 1, R.LINE_N // 2 + 1}
    row = scale * (v - v[mid]) ** 2
    n_sub = (R.LINE_N + 31) // 32
    added, merges = R.merge_walk(row, 72, self_index=mid)
    assert len(added) == n_sub and min(added[:-1]) == 32 and merges >= n_sub - 3, (added, merges)
    asc = R.line_case(dim, "ascending")
    a_added, a_merges = R.merge_walk(scale * (pos["ascending"] - (R.LINE_N - 1)) ** 2, 72, self_index=R.LINE_N - 1)
    assert a_merges >= n_sub - 3                                   # the last point of the ascending order sees the same
    assert asc.expected(False)[1][R.LINE_N // 2, :2].tolist() == [scale, scale]


@pytest.mark.parametrize("d,k", R.CLUSTER_DK)
def test_isolated_clusters_are_certainly_proven(d, k):
    case = R.clusters_case(d, k)
    assert len(case.units) == 12 * (k + 1)
    ref, _ = case.points()
    eps, _ = R.eps_row(ref, None)
    gap = R.cut_gap(case, k)
    idx, d2, _ = case.expected(False)
    assert d2[:, k - 1].max() <= d * 36 and d2[:, k].min() > d * 36        # exactly k neighbours inside the own cluster
    ratio = gap / eps
    print(f"clusters d={d} k={k}: min (t_K' - t_k) / eps_row = {ratio.min():.3g}")
    assert ratio.min() >= 4.0, ratio.min()


@pytest.mark.parametrize("d,k", R.DUPLICATE_DK)
def test_duplicates_are_certainly_refused(d, k):
    case = R.duplicates_case(d, k)
    assert len(case.units) == 10 * (k + 10)
    assert (R.cut_gap(case, k) == 0).all()                         # t_K' == t_k on every row
    _, d2, _ = case.expected(False)
    assert (d2[:, :k + 8] == 0).all()
    eps, _ = R.eps_row(case.points()[0], None)
    assert np.isfinite(eps).all()                                  # refused by the certificate, not by the range guard


def test_identical_points_have_zero_radius():
    ref, _ = R.identical_case().points()
    assert ref.shape == (300, 20) and (ref == ref[0]).all() and (ref[0] != 0).all()
    assert (ref.sum(axis=0) / 300 == ref[0]).all()                 # the column mean is the point itself: R is exactly 0
    eps, Rmax = R.eps_row(ref, None)
    assert Rmax == 0.0 and np.isinf(eps).all()


def test_scales_against_the_range_guard():
    base, _ = R.blind_case(20).points()
    for e in R.SCALES_OUTSIDE + R.SCALES_INSIDE:
        ref, _ = R.scaled_case(e).points()
        assert np.array_equal(ref, np.ldexp(base, e))
        eps, Rmax = R.eps_row(ref, None)
        if e in R.SCALES_OUTSIDE:
            assert np.isinf(eps).all() and (Rmax < 2.0 ** -42 or Rmax > 2.0 ** 62)          # outside by far more than 2 x
        else:
            assert np.isfinite(eps).all() and 2.0 ** -38 < Rmax < 2.0 ** 58
    assert min(R.SCALES_OUTSIDE) < 0 < max(R.SCALES_OUTSIDE) and min(R.SCALES_INSIDE) < 0 < max(R.SCALES_INSIDE)
    off, _ = R.offset_case().points()
    assert np.array_equal(off - 2.0 ** 30, base) and np.array_equal(off, base + 2.0 ** 30)
    assert np.array_equal(R.offset_case().expected(False)[1], R.blind_case(20).expected(False)[1])


def test_certificate_bounds_of_the_named_cases():
    """What the device file may require of rows_certified / rows_recomputed, from the header's conditions alone."""
    sw = R.switch_case()
    proven, refused = R.certificate_bounds(sw, 64)
    assert proven + refused == 700 and refused > 0 and proven > 0  # integer gaps against eps << 1: every row is settled
    for e in R.SCALES_INSIDE:
        c = R.clusters_scaled_case(e)
        assert R.certificate_bounds(c, 15) == (len(c.units), 0)
        eps, Rmax = R.eps_row(c.points()[0], None)
        assert (R.cut_gap(c, 15) / eps).min() >= 4.0 and 2.0 ** -38 < Rmax < 2.0 ** 58
    assert R.certificate_bounds(R.blind_case(20), 15) == (0, 0)    # inside the f32 error: settled only on the device
    assert R.certificate_bounds(R.identical_case(), 15) == (0, 300)
    assert R.certificate_bounds(R.count_case(9, 5), 8, False) == (9, 0) and R.certificate_bounds(R.count_case(10, 5), 1, False) == (10, 0)
    assert R.certificate_bounds(R.pair_case(1, 200, 5), 1) == (0, 200)


def test_eps_row_restates_the_header_formula():
    """One hand-computed row: two references at +-3 on one axis (d = 1, K = 8), the query at the centre's right."""
    ref = np.array([[-3.0], [3.0]])
    eps, Rmax = R.eps_row(ref, np.array([[1.0]]))
    assert Rmax == 3.0 and eps[0] == 1.01 * 12 * 2.0 ** -24 * (2 * 1.0 * 3.0 + 9.0)
    assert np.isinf(R.eps_row(ref * 2.0 ** -45, None)[0]).all() and np.isinf(R.eps_row(ref * 2.0 ** 61, None)[0]).all()
    assert R.eps_row(np.zeros((4, 60)), None, d=60)[1] == 0.0 and R.width(60) == 68

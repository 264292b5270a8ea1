"""The device k-NN search at every kernel width, tile edge and certificate path, against the integer expectation of
knn_ref.py: indices equal, distances bit-identical to sqrt(exact d2), no row exempted.  test_knn_edges_cpu.py holds the
preconditions that make each case exercise what it is named for.

Every call is also held to what the header comment of knn.hip settles without a device (knn_ref.certificate_bounds): a row
with t_K' - t_k > 2 eps_row must be certified, a row with t_K' == t_k (or eps = +inf) must be recomputed.

Measured on an MI355X (profiles/knn.md has the table): the f32-blind data of case 1 certifies no row at any width, at any
in-range scale or offset; the isolated clusters, the line and the small point counts certify every row; duplicates,
identical points, a single reference point and out-of-range scales recompute every row; the tie-heavy switch data
recomputes exactly its rows that tie from k to K' (k >= 55: 1 to 6 of 700) and certifies the rest."""
import numpy as np
import pytest

import knn_ref as R

pytestmark = pytest.mark.gpu


def knn(ctx, ref, query=None, **kw):
    from singlerust_amd.memory.processing import knn_points
    return knn_points(ctx, ref, query, **kw)


def assert_exact(case, k, include_self, idx, dist, info, want=None):
    """Indices equal and distances bit-identical on every row; the message names the first row that differs."""
    want_i, want_d = case.expected_k(k, include_self) if want is None else want
    label = f"{case.name} k={k} include_self={include_self}"
    print(f"{label}: certified {info['rows_certified']} recomputed {info['rows_recomputed']} K'={info['n_candidates']}")
    assert idx.dtype == np.uint32 and dist.dtype == np.float64 and idx.shape == want_i.shape == dist.shape, label
    bad = np.nonzero((idx.astype(np.int64) != want_i).any(axis=1))[0]
    if len(bad):
        r = int(bad[0])
        raise AssertionError(f"{label}: {len(bad)} rows with wrong indices, first row {r}:\n device   {idx[r].tolist()}\n"
                             f" expected {want_i[r].tolist()}\n device d {dist[r].tolist()}\n expect d {want_d[r].tolist()}\n {info}")
    bad = np.nonzero((dist != want_d).any(axis=1))[0]
    if len(bad):
        r = int(bad[0])
        raise AssertionError(f"{label}: {len(bad)} rows with wrong distances, first row {r}:\n device   {dist[r].tolist()}\n"
                             f" expected {want_d[r].tolist()}\n {info}")
    n_q = len(want_i)
    kp = R.n_candidates(k, case.units.shape[0], case.self_graph, include_self)
    assert (info["n_ref"], info["n_query"], info["d"], info["k"]) == (case.units.shape[0], n_q, case.d, k), (label, info)
    assert info["n_candidates"] == kp, (label, info)
    assert info["rows_certified"] + info["rows_recomputed"] == n_q, (label, info)
    proven, refused = R.certificate_bounds(case, k, include_self)  # what the header's conditions settle without a device
    assert info["rows_certified"] >= proven and info["rows_recomputed"] >= refused, (label, info, proven, refused)


def run_case(ctx, case, ks=None, selfs=None):
    """Every (k, include_self) of the case; returns {(k, include_self): info}."""
    ref, qry = case.points()
    out = {}
    for inc in (case.selfs if selfs is None else selfs):
        for k in (R.run_ks(case, inc) if ks is None else ks):
            idx, dist, info = knn(ctx, ref, qry, k=k, include_self=inc)
            assert_exact(case, k, inc, idx, dist, info)
            out[(k, inc)] = info
    return out


# ---- 1. every width, at its boundaries ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", R.WIDTH_DIMS)
def test_every_width_f32_blind(ctx, d):
    case = R.blind_case(d)
    infos = run_case(ctx, case)
    for (k, _), info in infos.items():
        assert info["d"] == d and info["n_candidates"] == k + 8
        assert info["rows_certified"] + info["rows_recomputed"] == R.BLIND_N


# ---- 2. k, K' and CAP switches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("include_self", [False, True])
@pytest.mark.parametrize("k", R.SWITCH_KS)
def test_k_switches_with_ties(ctx, k, include_self):
    run_case(ctx, R.switch_case(), ks=(k,), selfs=(include_self,))


# ---- 3. point counts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", R.COUNT_DIMS)
@pytest.mark.parametrize("n", R.COUNT_NS)
def test_point_counts_self_graph(ctx, n, d):
    case = R.count_case(n, d)
    for (k, inc), info in run_case(ctx, case).items():
        assert info["n_candidates"] == min(k + 8, n - (not inc)), (n, d, k, inc, info)


@pytest.mark.parametrize("d", R.COUNT_DIMS)
@pytest.mark.parametrize("n_ref,n_query", R.PAIRS)
def test_point_counts_query_against_reference(ctx, n_ref, n_query, d):
    case = R.pair_case(n_ref, n_query, d)
    ref, qry = case.points()
    for k in case.ks:
        idx, dist, info = knn(ctx, ref, qry, k=k)
        assert_exact(case, k, False, idx, dist, info)
        assert info["n_candidates"] == min(k + 8, n_ref)
        assert (dist[::2, 0] == 0.0).all()                         # the copies find their originals (or an equal row) first


# ---- 4. merge pressure --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", R.LINE_ORDERS)
@pytest.mark.parametrize("dim", sorted(R.LINE_DIRS))
def test_merge_pressure_on_a_line(ctx, dim, order):
    run_case(ctx, R.line_case(dim, order))


# ---- 5. both certificate paths, by construction -------------------------------------------------------------------------
@pytest.mark.parametrize("d,k", R.CLUSTER_DK)
def test_isolated_clusters_are_all_certified(ctx, d, k):
    case = R.clusters_case(d, k)
    info = run_case(ctx, case)[(k, False)]
    assert info["rows_recomputed"] == 0 and info["rows_certified"] == len(case.units), info


@pytest.mark.parametrize("d,k", R.DUPLICATE_DK)
def test_blocks_of_duplicates_are_all_recomputed(ctx, d, k):
    case = R.duplicates_case(d, k)
    info = run_case(ctx, case)[(k, False)]
    assert info["rows_recomputed"] == len(case.units), info


def test_identical_points_take_the_f64_pass(ctx):
    case = R.identical_case()
    ref, _ = case.points()
    n = len(ref)
    for inc in (False, True):
        for k in (1, 15, 64):
            idx, dist, info = knn(ctx, ref, k=k, include_self=inc)
            assert_exact(case, k, inc, idx, dist, info)
            assert info["rows_recomputed"] == n, info               # R = 0: eps is +inf
            want = np.array([[j for j in range(k + 1) if inc or j != i][:k] for i in range(n)])      # lowest admissible indices
            assert np.array_equal(idx, want) and (dist == 0.0).all()


def test_both_certificate_paths_run_on_generic_and_blind_data(ctx):
    """The clustered data of test_knn_gpu.py is certified (its rows have real gaps at the cut), the f32-blind data of case 1
    is refused; the tie-heavy switch data at k = 64 takes both paths in one call (six rows tie from k to K')."""
    rng = np.random.default_rng(102)
    centres = rng.standard_normal((12, 50)) * 6.0
    x = centres[rng.integers(0, 12, 3000)] + rng.standard_normal((3000, 50))
    _, _, generic = knn(ctx, x, k=15)
    ref, _ = R.blind_case(20).points()
    _, _, blind = knn(ctx, ref, k=15)
    ref, _ = R.switch_case().points()
    _, _, ties = knn(ctx, ref, k=64)
    print("generic", generic, "\nblind", blind, "\nties", ties)
    assert generic["rows_certified"] > 0
    assert blind["rows_recomputed"] > 0
    assert ties["rows_certified"] > 0 and ties["rows_recomputed"] > 0


# ---- 6. range guard and offsets ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", R.SCALES_OUTSIDE + R.SCALES_INSIDE)
def test_power_of_two_scales(ctx, e):
    case, base = R.scaled_case(e), R.blind_case(20)
    ref, _ = case.points()
    for k in case.ks:
        want_i, want_d = base.expected_k(k)
        idx, dist, info = knn(ctx, ref, k=k)
        assert_exact(case, k, False, idx, dist, info, want=(want_i, np.ldexp(want_d, e)))        # the unscaled answer, scaled
        if e in R.SCALES_OUTSIDE:
            assert info["rows_recomputed"] == len(ref), info       # R outside [2^-40, 2^60]: eps is +inf


@pytest.mark.parametrize("e", R.SCALES_INSIDE)
def test_certificate_holds_at_scales_inside_the_guard(ctx, e):
    case = R.clusters_scaled_case(e)
    info = run_case(ctx, case)[(15, False)]
    assert info["rows_recomputed"] == 0, info


def test_offset_of_2_to_30(ctx):
    case, base = R.offset_case(), R.blind_case(20)
    ref, _ = case.points()
    assert np.array_equal(ref, base.points()[0] + 2.0 ** 30)
    for k in case.ks:
        idx, dist, info = knn(ctx, ref, k=k)
        assert_exact(case, k, False, idx, dist, info, want=base.expected_k(k))


# ---- 7. determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["switch_k37", "line_d3_organ_pipe_k64"])
def test_two_calls_bit_identical(ctx, which):
    case, k = (R.switch_case(), 37) if which == "switch_k37" else (R.line_case(3, "organ_pipe"), 64)
    ref, _ = case.points()
    i1, d1, f1 = knn(ctx, ref, k=k)
    i2, d2, f2 = knn(ctx, ref, k=k)
    assert np.array_equal(i1, i2) and np.array_equal(d1.view(np.uint64), d2.view(np.uint64)) and f1 == f2
    assert_exact(case, k, False, i1, d1, f1)

"""The numpy restatements of the dense solver's kernels (tests/iterate_ref.py) against numpy.linalg and longdouble products, on
the very matrices tests/test_iterate_gpu.py hands to the device — and the conditions those inputs must meet, so that a bad input
shows here and not on the GPU."""
import numpy as np
import pytest

import iterate_ref as ref
from iterate_ref import EPS, L, gamma, ld

CASES = ref.eig_cases()


def test_round_robin_meets_every_pair_once():
    seen = set()
    for pairs in ref.ROUNDS:
        players = [x for pq in pairs for x in pq]
        assert sorted(players) == list(range(L))                  # 32 disjoint pairs
        seen |= {(min(p, q), max(p, q)) for p, q in pairs}
    assert len(ref.ROUNDS) == L - 1 and len(seen) == L * (L - 1) // 2


def test_rotation_annihilates_and_keeps_dead_pairs():
    rng = ref.rng_of(10)
    app, aqq, apq = rng.standard_normal(100), rng.standard_normal(100), rng.standard_normal(100)
    t, c = ref.rotation(app, aqq, apq)
    s = t * c
    new_pq = c * s * (app - aqq) + (c * c - s * s) * apq           # (J^T A J)_pq for new_p = c p - s q, new_q = s p + c q
    assert np.all(np.abs(new_pq) <= 8 * EPS * (np.abs(app) + np.abs(aqq) + np.abs(apq)))
    assert np.all(np.abs(t) <= 1.0)                                # the inner rotation
    t, c = ref.rotation(np.array([1.0, 1.0, 0.0]), np.array([2.0, 1.0, 0.0]), np.array([0.0, 1e-150, 1e-150]))
    assert t[0] == 0 and c[0] == 1                                 # b == 0
    assert t[1] == 0 and c[1] == 1 and t[2] == 0 and c[2] == 1     # b^2 + d^2 <= 1e-290


@pytest.mark.parametrize("case", CASES, ids=str)
def test_jacobi_restatement_meets_every_bound(case):
    """eigh and the bounds of the device test, on the restatement; at most 20 sweeps, so that the device keeps 10 in hand."""
    res, _ = ref.eig_reference(case)
    fig = ref.eig_checks(case, res.U, res.theta, res.sweeps, res.status)
    assert res.sweeps <= 20, f"{case}: the restatement needs {res.sweeps} sweeps"
    assert fig["orth"] <= 2e-14


@pytest.mark.parametrize("case", [c for c in CASES if c.family in ("block", "ritz")], ids=str)
def test_block_like_wanted_set_is_settled_after_the_first_sweep(case):
    """The leading n_want diagonal ranks must not move after the first sweep, or "ranked one sweep earlier" is ambiguous."""
    res, _ = ref.eig_reference(case)
    # want_history[s]: the set sweep s is measured over — all at 0, ranked inside sweep s - 1's first round afterwards; [2] is the
    # first one ranked with a whole sweep done
    for later in res.want_history[3:]:
        assert np.array_equal(later, res.want_history[2])
    lam = ref.eig_reference(case)[1]
    if case.family == "block":
        assert lam[L - 1] / lam[49] == pytest.approx(0.97, rel=1e-9)
        assert (lam[50] - lam[L - 1]) / lam[50] < 0.03


def test_early_stop_is_exercised():
    """Asking for fewer pairs never costs the restatement a sweep, and on the simulated Ritz steps — ten crowded guard columns
    apart from the 54 wanted pairs — asking for 54 of the 64 saves one: the cases that tell an early stop from none."""
    by = {c.name: ref.eig_reference(c)[0].sweeps for c in CASES if c.family in ("block", "ritz")}
    for fam in ("block0.1", "block0.01", "ritz1", "ritz2"):
        for tol in ("1e-06", "1e-22", "1e-30"):
            assert by[f"{fam}-want14-tol{tol}"] <= by[f"{fam}-want54-tol{tol}"] <= by[f"{fam}-want64-tol{tol}"]
    for name in ref.EARLY_STOP_SAVES:
        assert by[name.replace("want64", "want54")] < by[name]


@pytest.mark.parametrize("n", ref.CHOL_N)
@pytest.mark.parametrize("ill", [False, True])
def test_cholesky_inputs_and_inverted_blocks(n, ill):
    g = ref.chol_matrix(n, ill)
    if n > 1:
        cond = np.linalg.cond(g[:n, :n])
        assert (cond < 100) if not ill else (1e7 < cond < 1e9)
    r, dinv, xi = ref.chol_factor_ref(n, ill)
    ref.chol_checks(g, n, r, dinv, xi)


@pytest.mark.parametrize("n", [1, 17, 48, 64])
@pytest.mark.parametrize("ill", [False, True])
def test_substitutions_solve_the_system(n, ill):
    r, dinv, xi = ref.chol_factor_ref(n, ill)
    wp = ref.rng_of(3, n).standard_normal((37, L))
    for w in (ref.trsm_rows_ref(wp, r, dinv), ref.trsm_blocked_ref(wp, r, xi)):
        assert np.all(w[:, n:] == 0)
        # backward stable up to the condition of a 16 x 16 diagonal block of R (<= 1e4 here)
        assert ref.trsm_residual(w, r, wp, n) <= gamma(L) * (1e4 if ill else 20)


def test_chebyshev_recurrence_is_the_polynomial():
    """The three-term recurrence with the kernels' scalars reproduces T_d((2 C - b I) / b) on a diagonal C."""
    rng = ref.rng_of(4)
    theta = np.sort(rng.uniform(0.5, 3.0, L))[::-1].copy()
    lam = rng.uniform(0.0, 3.0, 40)
    v = rng.standard_normal((40, L))
    l_act, d = 60, 5
    y_prev, y = v, ref.cheb_first(lam[:, None] * v, v, theta, l_act)
    for _ in range(d - 1):
        y_prev, y = y, ref.cheb_step(lam[:, None] * y, y, y_prev, theta, l_act)
    b = ref.cheb_b(theta, l_act)
    x = (2.0 * lam - b) / b
    want = np.polynomial.chebyshev.Chebyshev.basis(d)(x)[:, None] * v
    assert np.allclose(y, want, rtol=1e-11, atol=1e-11 * np.abs(want).max())
    t = ref.cheb_t(theta, l_act)
    td = ref.cheb_td(t, d)
    assert np.allclose(td[t > 1], np.polynomial.chebyshev.Chebyshev.basis(d)(t[t > 1]), rtol=1e-12)
    assert np.all(td[t <= 1] == 1)


def test_chebyshev_floors():
    th = np.zeros(L)
    assert ref.cheb_b(th, 10) == 1.0
    th[0] = 4.0
    assert ref.cheb_b(th, 10) == 4e-10
    th[:10] = np.linspace(4.0, 1.0, 10)
    assert ref.cheb_b(th, 10) == 1.0 and ref.cheb_b(th, 11) == 4e-10


def test_resid_scalars():
    theta = np.array([2.0, 1.0, 1e-6, 0.0])
    rho = np.array([2e-3, 3e-3, 1e-7, 5e-8])
    r, ratio, spread = ref.resid_final_ref(rho, theta, 3, 4)
    assert r == max(1e-3, 3e-3, 1e-7 / 2e-5) and ratio == 0.0 and spread == 1.0        # theta[l_act - 1] = 0
    r, ratio, spread = ref.resid_final_ref(rho, theta, 2, 3)
    assert ratio == 1e-6 and spread == 2e6
    assert ref.resid_final_ref(rho, theta, 4, 4)[1] == 1.0                               # theta[n_pc - 1] = 0
    assert np.isnan(ref.resid_final_ref(np.array([1.0, np.nan]), theta, 2, 4)[0])
    assert ref.resid_final_ref(rho, np.zeros(4), 2, 4)[0] == 3e-3                        # all-zero spectrum: rho itself


def test_colmax_rule():
    a = np.array([[1.0, -2.0, 0.0], [-3.0, 2.0, 0.0], [3.0, -2.0, 0.0]])
    v, rows = ref.colmax_ref(a)
    assert list(v) == [-3.0, -2.0, 0.0] and list(rows) == [1, 0, 0]

"""Every kernel of the dense k x 64 subspace iteration (csrc/iterate.inl, csrc/jacobi.inl) alone, through srx_iterate_op — which
launches each one exactly as the solver does — against its definition: longdouble products with Higham's bounds, the numpy
restatements of tests/iterate_ref.py, numpy.linalg.  Shapes are tiny; every block is allocated with 8 sentinel rows behind it,
and `run` asserts that none was touched.

The three allowances that are measured, not derived, and what an MI355X reached (run with -s: every case prints its figures):
  orthogonality of U, max |U^T U - I| <= max(4 x the restatement's on the same case, 64 eps = 1.4e-14): 8.8e-15 at most
      (geometric spectrum, n = 64, 15 sweeps: restatement 5.0e-15; the restatement's own worst is 1.4e-14, repeated eigenvalues)
  substitutions, |W R - Wp| / (|W| |R|) <= 4 x the restatement's + gamma_64: k_trsm_rows 4.1e-16 (restatement 2.5e-16),
      k_trsm_mfma 5.6e-16 (3.1e-16), against gamma_64 = 1.4e-14
  k_cheb_scale, relative <= 4 x (numpy's f64 cosh(d acosh t) against longdouble) + 4 eps: 4.9e-14 (numpy 4.9e-14, t ~ 2e10, d = 12)
Sweeps of the eigen-solve: the device took the restatement's count in every case but two (repeated eigenvalues 17 against 19, rank
5: 7 against 6)."""
import ctypes as C

import numpy as np
import pytest

import iterate_ref as ref
from iterate_ref import EPS, L, gamma, ld

pytestmark = pytest.mark.gpu


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64).copy()


def run(ctx, op, *, k=1, n=0, l_act=0, n_pc=0, n_want=0, d=0, variant=0, flags=0, off_tol2=0.0, c=None, blk=(), sm=(), vec=(),
        xi=None, expect=0):
    """One srx_iterate_op call on the given arrays (written in place); returns the argument block."""
    from singlerust_amd import _ffi
    a = _ffi.IterateArgs()
    a.k, a.n, a.l_act, a.n_pc, a.n_want, a.d, a.variant, a.flags, a.off_tol2 = k, n, l_act, n_pc, n_want, d, variant, flags, off_tol2
    keep = []

    def addr(x, shape):
        if x is None:
            return None
        assert x.dtype == np.float64 and x.flags.c_contiguous and x.shape == shape, (x.shape, shape)
        keep.append(x)
        return x.ctypes.data

    a.c = addr(c, (k, k))
    for i, x in enumerate(blk):
        a.blk[i] = addr(x, (k, L))
    for i, x in enumerate(sm):
        a.sm[i] = addr(x, (L, L))
    for i, x in enumerate(vec):
        a.vec[i] = addr(x, (L,))
    a.xi = addr(xi, (4, 16, 16))
    rc = _ffi.lib().srx_iterate_op(ctx.handle, op, C.byref(a))
    if expect:
        assert rc == expect
        return a
    _ffi.check(rc, ctx.handle)
    assert a.tail_touched == 0, "a sentinel row behind a k x 64 block was written"
    return a


def ops():
    from singlerust_amd import _ffi
    return _ffi


# ---- apply ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 31, 32, 33, 65, 127, 128, 129, 500, 1000])
def test_dense_apply(ctx, k):
    rng = ref.rng_of(20, k)
    cm = rng.standard_normal((k, k))
    cm = 0.5 * (cm + cm.T)
    w, wp0 = rng.standard_normal((k, L)), rng.standard_normal((k, L))
    wp = wp0.copy()
    run(ctx, ops().IT_APPLY, k=k, c=cm, blk=[w, wp])
    want = ld(wp0) + ld(cm).T @ ld(w)
    bound = gamma(k + 8) * (np.abs(ld(wp0)) + np.abs(ld(cm)).T @ np.abs(ld(w)))
    assert np.all(np.abs(ld(wp) - want) <= bound), float((np.abs(ld(wp) - want) / bound).max())


def test_dense_apply_reads_c_transposed(ctx):
    """The documented transposed read: Wp += C^T W for a C that is not symmetric."""
    k = 129
    rng = ref.rng_of(21)
    cm, w, wp0 = rng.standard_normal((k, k)), rng.standard_normal((k, L)), rng.standard_normal((k, L))
    wp = wp0.copy()
    run(ctx, ops().IT_APPLY, k=k, c=cm, blk=[w, wp])
    want = ld(wp0) + ld(cm).T @ ld(w)
    bound = gamma(k + 8) * (np.abs(ld(wp0)) + np.abs(ld(cm)).T @ np.abs(ld(w)))
    assert np.all(np.abs(ld(wp) - want) <= bound)
    assert not np.allclose(wp, wp0 + cm @ w)


# ---- the Gram products ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("same", [False, True], ids=["AB", "AA"])
@pytest.mark.parametrize("k", [1, 3, 31, 32, 33, 64, 511, 512, 513, 1000])
def test_gram_products(ctx, k, same):
    rng = ref.rng_of(22, k, int(same))
    a = rng.standard_normal((k, L))
    b = a if same else rng.standard_normal((k, L))
    flags = ops().IT_ALIAS_B if same else 0
    blk = [a.copy()] if same else [a.copy(), b.copy()]
    ab = np.abs(ld(a)).T @ np.abs(ld(b))
    h0 = rng.standard_normal((L, L))
    h = h0.copy()
    run(ctx, ops().IT_GRAM1, k=k, flags=flags, blk=blk, sm=[h])
    assert np.all(np.abs(ld(h) - (ld(h0) + ld(a).T @ ld(b))) <= gamma(k + 16) * (np.abs(ld(h0)) + ab))
    h2, g2 = np.full((L, L), 7.0), np.full((L, L), 7.0)
    run(ctx, ops().IT_GRAM2, k=k, flags=flags, blk=blk, sm=[h2, g2])
    assert np.all(np.abs(ld(h2) - ld(a).T @ ld(b)) <= gamma(k + 16) * ab)
    assert np.all(np.abs(ld(g2) - ld(b).T @ ld(b)) <= gamma(k + 16) * (np.abs(ld(b)).T @ np.abs(ld(b))))
    assert np.array_equal(blk[0], a)


# ---- the Cholesky factorisations --------------------------------------------------------------------------------------------------
def _chol(ctx, g, n, variant):
    g = _f64(g)
    r, dinv, xi = np.full((L, L), 5.0), np.full(L, 5.0), np.full((4, 16, 16), 5.0)
    a = run(ctx, ops().IT_CHOL, n=n, variant=variant, sm=[g, r], vec=[dinv], xi=xi if variant == 2 else None)
    return r, dinv, xi, g, a.status[0]


@pytest.mark.parametrize("ill", [False, True], ids=["well", "cond1e8"])
@pytest.mark.parametrize("n", ref.CHOL_N)
def test_cholesky(ctx, n, ill):
    g = ref.chol_matrix(n, ill)
    got = {}
    for variant in (0, 1, 2):
        r, dinv, xi, g_left, status = _chol(ctx, g, n, variant)
        assert status == 0
        ref.chol_checks(g, n, r, dinv, xi if variant == 2 else None)
        if variant == 2:
            assert np.all(g_left == 0), "k_chol_factor_mfma leaves G zeroed"
        else:
            assert np.array_equal(g_left, g)
        got[variant] = (r, dinv)
    assert np.array_equal(got[1][0], got[0][0]) and np.array_equal(got[1][1], got[0][1])     # a clean G: the shift does nothing
    # the panelled factor against the plain one: each is the exact factor of G + E_i, |E_i| <= 2 gamma_(n+1) |R_i^T| |R_i|, so the two
    # products differ by at most the sum of the bounds, and the factors by the first-order perturbation bound of the Cholesky
    # factor (Sun 1991): || dR ||_F <= kappa_2(G) || R ||_2 || E ||_F / (sqrt(2) || G ||_2)
    r0, r2 = got[0][0][:n, :n], got[2][0][:n, :n]
    e0 = 2 * gamma(n + 1) * (np.abs(ld(r0)).T @ np.abs(ld(r0)))
    e2 = 2 * gamma(n + 1) * (np.abs(ld(r2)).T @ np.abs(ld(r2)))
    assert np.all(np.abs(ld(r0).T @ ld(r0) - ld(r2).T @ ld(r2)) <= e0 + e2)
    gn = g[:n, :n]
    e_f = float(np.linalg.norm(e0.astype(np.float64)) + np.linalg.norm(e2.astype(np.float64)))
    fwd = np.linalg.cond(gn) * np.linalg.norm(r0, 2) * e_f / (np.sqrt(2) * np.linalg.norm(gn, 2))
    assert np.linalg.norm(r0 - r2) <= 2 * fwd                      # (2: the bound is first order)


@pytest.mark.parametrize("pivot", [0.0, -1.0], ids=["zero", "negative"])
@pytest.mark.parametrize("pos", [0, 7, 8, 63])
def test_cholesky_reports_a_lost_pivot(ctx, pos, pivot):
    """A pivot that is exactly zero (an empty column) or negative: the plain kernels set kStatChol; every call returns."""
    g = _f64(ref.chol_matrix(L, False))
    g[pos, :] = 0.0
    g[:, pos] = 0.0
    g[pos, pos] = pivot
    for variant in (0, 2):
        assert _chol(ctx, g, L, variant)[4] & ref.STAT_CHOL
    r, dinv, _, _, status = _chol(ctx, g, L, 1)                 # shifted: the column is dropped instead
    assert status == 0 and dinv[pos] == 0 and r[pos, pos] == 1 and np.count_nonzero(r[pos]) == 1


def test_cholesky_shifted(ctx):
    rng = ref.rng_of(23)
    b = rng.standard_normal((200, L))
    b[:, 40] = b[:, 11]                                          # a duplicated column: dropped
    b[:, 50] = 1e-8 * rng.standard_normal(200)                   # independent but tiny: lifted to the floor
    g = b.T @ b
    g = 0.5 * (g + g.T)
    r, dinv, _, _, status = _chol(ctx, g, L, 1)
    assert status == 0
    assert dinv[40] == 0 and r[40, 40] == 1 and np.count_nonzero(r[40]) == 1
    floor_ = 1e-13 * np.diag(g).max()
    assert 0 < g[50, 50] < floor_
    assert abs(dinv[50] * np.sqrt(floor_) - 1.0) <= 4 * EPS
    assert abs(r[50, 50] * dinv[50] - 1.0) <= 4 * EPS
    keep = [j for j in range(L) if j not in (40, 50)]
    assert np.all(np.isfinite(r)) and np.all(dinv[keep] > 0)
    # the columns before the first special one are factored as the plain kernel factors them
    r0, dinv0, _, _, _ = _chol(ctx, g, 40, 0)
    assert np.array_equal(r[:40, :40], r0[:40, :40]) and np.array_equal(dinv[:40], dinv0[:40])


# ---- the triangular substitutions -----------------------------------------------------------------------------------------------
def _trsm(ctx, route, k, n, ill, flags, seed=0):
    it = ops()
    r, dinv, xi = ref.chol_factor_ref(n, ill)
    rng = ref.rng_of(24, k, n, seed)
    wp = rng.standard_normal((k, L))
    src, w = wp.copy(), np.full((k, L), 3.0)
    z = [rng.standard_normal((k, L)) for _ in range(3)]
    z0 = [x.copy() for x in z]
    run(ctx, it.IT_TRSM, k=k, variant=route, flags=flags, blk=[src, w] + z, sm=[None, _f64(r)],
        vec=[_f64(dinv)] if route == 0 else [], xi=_f64(xi) if route == 1 else None)
    want = ref.trsm_rows_ref(wp, r, dinv) if route == 0 else ref.trsm_blocked_ref(wp, r, xi)
    assert np.all(np.isfinite(w)) and np.all(w[:, n:] == 0)
    res_ref, res_dev = ref.trsm_residual(want, r, wp, n), ref.trsm_residual(w, r, wp, n)
    allow = 4 * res_ref + gamma(L)
    print(f"trsm route {route} k {k} n {n} ill {ill}: residual {res_dev:.3e} (restatement {res_ref:.3e}, allowance {allow:.3e})")
    assert res_dev <= allow
    for i in range(3):
        passed = bool(flags & (it.IT_Z0 << i)) and not (i == 0 and flags & it.IT_Z0_IS_SRC)
        assert np.all(z[i] == 0) if passed else np.array_equal(z[i], z0[i])
    if flags & (it.IT_Z0_IS_SRC | it.IT_SRC_IS_W):
        assert np.array_equal(src, w) if flags & it.IT_SRC_IS_W else np.all(src == 0)
    else:
        assert np.array_equal(src, wp)
    return w


@pytest.mark.parametrize("route", [0, 1], ids=["rows", "mfma"])
@pytest.mark.parametrize("n", [1, 17, 48, 64])
@pytest.mark.parametrize("k", [1, 15, 16, 17, 63, 64, 65, 100, 257])
def test_substitution(ctx, k, n, route):
    _trsm(ctx, route, k, n, False, 7)             # z0 .. z2 all given and distinct


@pytest.mark.parametrize("route", [0, 1], ids=["rows", "mfma"])
def test_substitution_flags_and_conditioning(ctx, route):
    it = ops()
    base = _trsm(ctx, route, 100, 48, False, 0)                                   # all null
    assert np.array_equal(_trsm(ctx, route, 100, 48, False, 7), base)             # all given
    assert np.array_equal(_trsm(ctx, route, 100, 48, False, it.IT_Z0_IS_SRC | 6), base)     # one z is the source
    assert np.array_equal(_trsm(ctx, route, 100, 48, False, it.IT_SRC_IS_W), base)          # in place
    _trsm(ctx, route, 100, 64, True, 7)                                           # cond(G) = 1e8


# ---- the eigen-solve ------------------------------------------------------------------------------------------------------------
def _eig(ctx, h, n, off_tol2, n_want):
    hh, u, theta = _f64(h), np.full((L, L), 9.0), np.full(L, 9.0)
    a = run(ctx, ops().IT_EIG, n=n, off_tol2=off_tol2, n_want=n_want, sm=[hh, u], vec=[theta])
    return u, theta, a.status[0], a.status[1], hh


_EIG_SWEEPS = {}


@pytest.mark.parametrize("case", ref.eig_cases(), ids=str)
def test_eig(ctx, case):
    res, _ = ref.eig_reference(case)
    u, theta, status, sweeps, h_left = _eig(ctx, ref.eig_input(case), case.n, case.off_tol2, case.n_want)
    _EIG_SWEEPS[case.name] = sweeps
    assert np.all(h_left == 0), "k_jacobi_eig2 leaves H zeroed"
    orth_allow = max(4 * ref.eig_orthogonality(res.U, case.n), 64 * EPS)
    orth = ref.eig_orthogonality(u, case.n)
    print(f"eig {case.name}: sweeps {sweeps} (restatement {res.sweeps}), |U^T U - I| {orth:.3e} (restatement "
          f"{ref.eig_orthogonality(res.U, case.n):.3e}, allowance {orth_allow:.3e})")
    fig = ref.eig_checks(case, u, theta, sweeps, status, orth_allow=orth_allow, sweeps_allow=res.sweeps + 2)
    print(f"eig {case.name}: wanted residual {fig['resid']:.3e}, |theta - lambda| {fig['dlam']:.3e}, bound {fig['bound']:.3e}")


def test_eig_early_stop_is_exercised(ctx):
    """Asking for n_pc + 4 = 54 of the 64 pairs never costs the device a sweep, and saves one where it saves the restatement one."""
    by = {}
    for case in ref.eig_cases():
        if case.family in ("block", "ritz"):
            by[case.name] = _EIG_SWEEPS.get(case.name)
            if by[case.name] is None:
                by[case.name] = _eig(ctx, ref.eig_input(case), case.n, case.off_tol2, case.n_want)[3]
    for name, sweeps in by.items():
        if "want64" in name:
            assert by[name.replace("want64", "want54")] <= sweeps and by[name.replace("want64", "want14")] <= sweeps
    saved = [name for name in ref.EARLY_STOP_SAVES if by[name.replace("want64", "want54")] < by[name]]
    print("early stop: sweeps", by)
    assert saved, "asking for 54 pairs took as many sweeps as asking for 64 in every case"


def test_nan_reaches_the_residual(ctx):
    """The guard the driver relies on: a NaN in the projected matrix comes out of the Ritz tail as a NaN residual (the sweep loop
    is bounded: nothing hangs)."""
    h = _f64(ref.eig_input(ref.EigCase("geom", "geom", L, L, 1e-22)))
    h[3, 5] = np.nan
    u, theta, _, sweeps, _ = _eig(ctx, h, L, 1e-22, L)
    assert sweeps <= ref.MAX_SWEEPS
    k = 40
    rng = ref.rng_of(25)
    w, wp = rng.standard_normal((k, L)), rng.standard_normal((k, L))
    a1, a2 = np.zeros((k, L)), np.zeros((k, L))
    rho, colmax = np.zeros(L), np.zeros(L)
    a = run(ctx, ops().IT_RITZ, k=k, n_pc=50, l_act=L, blk=[w, wp, a1, a2], sm=[None, u], vec=[theta, rho, colmax])
    assert np.isnan(a.out[0])


# ---- the Ritz tail --------------------------------------------------------------------------------------------------------------
def _ritz(ctx, w, wp, u, theta, n_pc, l_act, zero_wp):
    k = w.shape[0]
    wp_io, a1, a2 = wp.copy(), np.full((k, L), 2.0), np.full((k, L), 2.0)
    rho, colmax = np.full(L, 2.0), np.full(L, 2.0)
    a = run(ctx, ops().IT_RITZ, k=k, n_pc=n_pc, l_act=l_act, flags=ops().IT_ZERO_WP if zero_wp else 0,
            blk=[_f64(w), wp_io, a1, a2], sm=[None, _f64(u)], vec=[_f64(theta), rho, colmax])
    return a1, a2, wp_io, rho, colmax, list(a.out)


def _check_scalars(out, rho, theta, n_pc, l_act):
    r, ratio, spread = ref.resid_final_ref(rho, theta, n_pc, l_act)
    for got, want in ((out[0], r), (out[2], ratio), (out[4], spread)):
        assert abs(got - want) <= 4 * EPS * abs(want), (got, want)
    assert out[1] == 0 and out[3] == 0 and out[5] == 0


@pytest.mark.parametrize("zero_wp", [0, 1])
@pytest.mark.parametrize("k", [1, 4, 511, 512, 513, 1000])
def test_ritz_tail(ctx, k, zero_wp):
    rng = ref.rng_of(26, k)
    w, wp = rng.standard_normal((k, L)), rng.standard_normal((k, L))
    u = ref.random_orthogonal(L, rng)
    theta = np.sort(rng.uniform(0.5, 4.0, L))[::-1].copy()
    a1, a2, wp_left, rho, colmax, out = _ritz(ctx, w, wp, u, theta, 50, L, zero_wp)
    g = gamma(L)
    e1, e2 = g * (np.abs(ld(wp)) @ np.abs(ld(u))), g * (np.abs(ld(w)) @ np.abs(ld(u)))
    assert np.all(np.abs(ld(a1) - ld(wp) @ ld(u)) <= e1)
    assert np.all(np.abs(ld(a2) - ld(w) @ ld(u)) <= e2)
    assert np.all(wp_left == 0) if zero_wp else np.array_equal(wp_left, wp)
    # rho_c = || A1[:, c] - theta_c A2[:, c] ||: every entry of the difference carries the two products' errors and two
    # roundings of its own, the sum of k squares and the root gamma_(k + 8) more
    r = ld(wp) @ ld(u) - ld(theta)[None, :] * (ld(w) @ ld(u))
    rho_ref = np.sqrt((r * r).sum(axis=0))
    e = e1 + np.abs(ld(theta))[None, :] * e2 + 2 * EPS * (np.abs(ld(wp) @ ld(u)) + np.abs(ld(theta))[None, :] * np.abs(ld(w) @ ld(u)))
    assert np.all(np.abs(ld(rho) - rho_ref) <= np.sqrt((e * e).sum(axis=0)) + gamma(k + 8) * rho_ref)
    want_v, _ = ref.colmax_ref(a2)
    assert np.array_equal(colmax, want_v)
    _check_scalars(out, rho, theta, 50, L)


@pytest.mark.parametrize("k", [530, 1000])
def test_ritz_largest_entry_takes_the_smallest_row(ctx, k):
    """Columns of A2 = W U that attain their largest magnitude in several rows, with both signs, in rows of one block's different
    `sub` lanes (the later pass first), of different blocks and of different slices of k_resid_final — small integers, so that A2
    is exact.  The value at the smallest such row is the one returned."""
    rng = ref.rng_of(27, k)
    w = rng.integers(-5, 6, size=(k, L)).astype(np.float64)
    # rows j -> block (j / 4) % 128, lane j % 4 of k_ritz_post; block b -> slice b % 16 of k_resid_final
    plant = {
        0: [(512 + 4 * 3, +7), (4 * 3 + 1, -7)],                 # block 3: lane 0 holds the LATER row, lane 1 the earlier one
        1: [(4 * 3 + 1, +7), (512 + 4 * 3, -7)],
        2: [(4 * 9 + 2, -7), (4 * 9 + 3, +7), (4 * 9 + 1, +7)],  # three lanes of block 9
        3: [(4 * 20, +7), (4 * 4 + 3, -7)],                      # blocks 20 and 4: slices 4 and 4 of the final reduction
        4: [(4 * 17 + 1, -7), (4 * 2, +7)],                      # blocks 17 and 2: slices 1 and 2
        5: [(k - 1, +7), (0, -7)],
        6: [(k - 1, -7), (k - 2, +7), (2, +7)],
        7: [(300, +7)],
    }
    for col, rows in plant.items():
        for j, v in rows:
            w[j, col] = v
    perm = rng.permutation(L)
    sgn = rng.choice([-1.0, 1.0], size=L)
    u = np.zeros((L, L))
    u[perm, np.arange(L)] = sgn                                   # A2[:, c] = sgn_c W[:, perm_c]
    inv = np.argsort(perm)
    theta = np.linspace(2.0, 1.0, L)
    _, a2, _, _, colmax, _ = _ritz(ctx, w, np.zeros((k, L)), u, theta, 50, L, 1)
    assert np.array_equal(a2, w @ u)
    want_v, want_rows = ref.colmax_ref(w @ u)
    assert np.array_equal(colmax, want_v)
    for col, rows in plant.items():
        c = inv[col]
        assert want_rows[c] == min(j for j, _ in rows)
        assert colmax[c] == sgn[c] * dict(rows)[want_rows[c]]


@pytest.mark.parametrize("which", ["small", "npc_zero", "last_zero", "all_zero"])
def test_ritz_scalars_at_the_floors(ctx, which):
    k, n_pc, l_act = 33, 5, 8
    rng = ref.rng_of(28)
    w, wp = rng.standard_normal((k, L)), rng.standard_normal((k, L))
    u = ref.random_orthogonal(L, rng)
    theta = np.zeros(L)
    theta[:l_act] = {"small": [4, 3, 2, 1e-6, 1e-7, 1e-8, 1e-9, 1e-10], "npc_zero": [4, 3, 2, 1, 0, 0, 0, 0],
                     "last_zero": [4, 3, 2, 1, 0.5, 0.25, 0.125, 0], "all_zero": [0] * 8}[which]
    _, _, _, rho, _, out = _ritz(ctx, w, wp, u, theta, n_pc, l_act, 0)
    _check_scalars(out, rho, theta, n_pc, l_act)
    if which == "npc_zero":
        assert out[2] == 1.0
    if which in ("last_zero", "all_zero", "npc_zero"):
        assert out[4] == 1.0


# ---- the Chebyshev filter ---------------------------------------------------------------------------------------------------------
def _theta_case(which):
    theta = np.zeros(L)
    if which == "plain":
        theta[:] = np.geomspace(8.0, 0.5, L)
    elif which == "l_act40":
        theta[:40] = np.geomspace(8.0, 0.5, 40)
        theta[40:] = 123.0                                       # beyond l_act: never read
    elif which == "last_zero":
        theta[:39] = np.geomspace(8.0, 0.5, 39)                  # theta[l_act - 1] = 0: b = 1e-10 theta_0
    l_act = 64 if which == "plain" else 40
    return theta, l_act


@pytest.mark.parametrize("which", ["plain", "l_act40", "last_zero", "all_zero"])
def test_chebyshev_kernels(ctx, which):
    it = ops()
    k = 70
    theta, l_act = _theta_case(which)
    rng = ref.rng_of(29)
    x, y, z = (rng.standard_normal((k, L)) for _ in range(3))
    a = 2.0 / ref.cheb_b(theta, l_act)
    two_ulp = 2 * EPS                      # of the largest term: the compiler may contract a x - y into one FMA or round twice

    a1 = x.copy()
    run(ctx, it.IT_CHEB, k=k, variant=0, l_act=l_act, blk=[a1, y.copy()], vec=[_f64(theta)])
    assert np.all(np.abs(a1 - ref.cheb_first(x, y, theta, l_act)) <= two_ulp * np.maximum(np.abs(a * x), np.abs(y)))

    zz, cur, prev = z.copy(), np.full((k, L), 4.0), np.full((k, L), 4.0)
    run(ctx, it.IT_CHEB, k=k, variant=1, l_act=l_act, blk=[zz, x.copy(), cur, prev], vec=[_f64(theta)])
    want_cur, want_prev = ref.cheb_first2(z, x, theta, l_act)
    assert np.all(np.abs(cur - want_cur) <= two_ulp * np.maximum(np.abs(a * z), np.abs(x)))
    assert np.array_equal(prev, want_prev) and np.all(zz == 0)

    zz, prev = z.copy(), y.copy()
    run(ctx, it.IT_CHEB, k=k, variant=2, l_act=l_act, blk=[zz, x.copy(), prev], vec=[_f64(theta)])
    scale = np.maximum(np.maximum(np.abs(2 * a * z), np.abs(2 * x)), np.abs(y))
    assert np.all(np.abs(prev - ref.cheb_step(z, x, y, theta, l_act)) <= 2 * two_ulp * scale)      # (two dependent operations)
    assert np.all(zz == 0)

    for d in (2, 5, 12):
        yy = y.copy()
        run(ctx, it.IT_CHEB, k=k, variant=3, l_act=l_act, d=d, blk=[yy], vec=[_f64(theta)])
        t = ref.cheb_t(theta, l_act)
        td_ld = ref.cheb_td(t, d, dtype=np.longdouble)
        e_np = float(np.abs(ld(ref.cheb_td(t, d)) / td_ld - 1).max())
        allow = 4 * e_np + 4 * EPS
        rel = np.abs(ld(yy[:, :l_act]) * td_ld[None, :] / ld(y[:, :l_act]) - 1)
        print(f"cheb_scale {which} d {d}: relative error {float(rel.max()):.3e} (numpy {e_np:.3e}, allowance {allow:.3e})")
        assert np.all(rel <= allow)
        assert np.array_equal(yy[:, l_act:], y[:, l_act:])                       # columns at or beyond l_act: untouched
        if which == "all_zero":
            assert np.array_equal(yy, y)                                         # b = 1, t = -1: no scaling
        assert np.array_equal(yy[:, :l_act][:, t <= 1], y[:, :l_act][:, t <= 1])


def test_chebyshev_filter_chained_with_apply(ctx):
    """A degree-5 filter at k = 70 through the operations, as the solver chains them, against the longdouble recurrence with a
    running a-priori bound: every application of C adds gamma_(k+8) |C| |Y| to what the recurrence has carried so far."""
    it = ops()
    k, d, l_act = 70, 5, 60
    rng = ref.rng_of(30)
    q = ref.random_orthogonal(k, rng)
    cm = (q * np.geomspace(8.0, 0.05, k)) @ q.T
    cm = 0.5 * (cm + cm.T)
    theta = np.zeros(L)
    theta[:l_act] = np.geomspace(8.0, 0.6, l_act)
    v = rng.standard_normal((k, L))
    th = [_f64(theta)]

    def apply(y):
        z = np.zeros((k, L))
        run(ctx, it.IT_APPLY, k=k, c=cm, blk=[y.copy(), z])
        return z

    a1, a2 = apply(v), v.copy()
    run(ctx, it.IT_CHEB, k=k, variant=0, l_act=l_act, blk=[a1, a2], vec=th)
    cur, prev = a1, a2
    for _ in range(d - 1):
        z = apply(cur)
        run(ctx, it.IT_CHEB, k=k, variant=2, l_act=l_act, blk=[z, cur, prev], vec=th)
        assert np.all(z == 0)
        cur, prev = prev, cur
    run(ctx, it.IT_CHEB, k=k, variant=3, l_act=l_act, d=d, blk=[cur], vec=th)

    a = np.longdouble(2.0 / ref.cheb_b(theta, l_act))
    cl, ca, g = ld(cm), np.abs(ld(cm)), gamma(k + 8)
    y_prev, e_prev = ld(v), np.zeros((k, L), dtype=np.longdouble)
    y = a * (cl @ y_prev) - y_prev
    e = a * g * (ca @ np.abs(y_prev)) + 2 * EPS * (np.abs(a * (cl @ y_prev)) + np.abs(y_prev))
    for _ in range(d - 1):
        y_next = 2 * (a * (cl @ y) - y) - y_prev
        e_next = (2 * (a * (ca @ e + g * (ca @ (np.abs(y) + e))) + e) + e_prev
                  + 4 * EPS * (np.abs(2 * a * (cl @ y)) + 2 * np.abs(y) + np.abs(y_prev)))
        y_prev, e_prev, y, e = y, e, y_next, e_next
    t = ref.cheb_t(theta, l_act)
    td = np.ones(L, dtype=np.longdouble)
    td[:l_act] = ref.cheb_td(t, d, dtype=np.longdouble)
    e_np = float(np.abs(ld(ref.cheb_td(t, d)) / td[:l_act] - 1).max())
    want = y / td[None, :]
    bound = e / td[None, :] + (4 * e_np + 4 * EPS) * np.abs(want)
    assert np.all(np.abs(ld(cur) - want) <= bound), float((np.abs(ld(cur) - want) / bound).max())
    # the bound is not vacuous: it stays far below the result
    assert float((bound / np.abs(want).max()).max()) < 1e-9


# ---- the entry's own refusals ---------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments(ctx):
    it = ops()
    k = 5
    blk = [np.zeros((k, L)) for _ in range(4)]
    sm = [np.eye(L), np.eye(L)]
    vec = [np.ones(L), np.ones(L), np.ones(L)]
    bad = it.E_ARG
    assert it.lib().srx_iterate_op(ctx.handle, it.IT_APPLY, None) == bad
    run(ctx, it.IT_APPLY, k=k, c=None, blk=blk[:2], expect=bad)
    run(ctx, it.IT_APPLY, k=k, c=np.zeros((k, k)), blk=blk[:1], expect=bad)
    run(ctx, it.IT_APPLY, k=0, c=np.zeros((0, 0)), blk=[np.zeros((0, L))] * 2, expect=bad)
    run(ctx, it.IT_GRAM1, k=k, blk=blk[:2], expect=bad)
    for n in (0, 65, -1):
        run(ctx, it.IT_EIG, n=n, n_want=1, off_tol2=1e-22, sm=sm, vec=vec[:1], expect=bad)
        run(ctx, it.IT_CHOL, n=n, sm=sm, vec=vec[:1], expect=bad)
    run(ctx, it.IT_CHOL, n=8, variant=2, sm=sm, vec=vec[:1], expect=bad)                  # no xi
    run(ctx, it.IT_CHOL, n=8, variant=3, sm=sm, vec=vec[:1], expect=bad)
    for l_act in (0, 65):
        run(ctx, it.IT_RITZ, k=k, n_pc=1, l_act=l_act, blk=blk, sm=sm, vec=vec, expect=bad)
        run(ctx, it.IT_CHEB, k=k, variant=3, l_act=l_act, d=3, blk=blk[:1], vec=vec[:1], expect=bad)
    for n_pc in (0, 9):
        run(ctx, it.IT_RITZ, k=k, n_pc=n_pc, l_act=8, blk=blk, sm=sm, vec=vec, expect=bad)
    run(ctx, it.IT_RITZ, k=k, n_pc=2, l_act=8, blk=blk[:3], sm=sm, vec=vec, expect=bad)
    run(ctx, it.IT_TRSM, k=k, variant=1, blk=blk[:2], sm=[None, sm[1]], expect=bad)      # no xi
    run(ctx, it.IT_TRSM, k=k, variant=0, flags=it.IT_Z0 << 2, blk=blk[:2], sm=[None, sm[1]], vec=vec[:1], expect=bad)
    run(ctx, 99, k=k, expect=bad)
    # the context is still usable
    wp = np.ones((k, L))
    run(ctx, it.IT_APPLY, k=k, c=np.eye(k), blk=[np.ones((k, L)), wp])
    assert np.all(wp == 2.0)

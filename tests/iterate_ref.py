"""Host side of the kernel-level tests of the dense k x 64 subspace iteration (csrc/iterate.inl, csrc/jacobi.inl), independent
of the device code: numpy restatements of what each kernel is defined to compute, the seeded inputs the CPU and the GPU tests
share, the rounding bounds, and the checks of an eigen-solve's output (run on the restatement by test_iterate_cpu.py and on the
device by test_iterate_gpu.py: one statement of every bound).

numpy only; numpy.longdouble where a higher-precision sum is wanted."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

L = 64
EPS = float(np.finfo(np.float64).eps)              # 2^-52
LD = np.longdouble
MAX_SWEEPS = 30
STAT_CHOL, STAT_EIG = 1, 2


def gamma(m):
    """Higham's gamma_m = m eps / (1 - m eps)."""
    return m * EPS / (1.0 - m * EPS)


def ld(a):
    return np.asarray(a, dtype=LD)


def rng_of(*key):
    return np.random.default_rng([20240611, *[int(x) for x in key]])


def random_orthogonal(n, rng):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def expm_antisym(n, size, rng):
    """exp(K) of a random antisymmetric K with ||K||_2 = size: an orthogonal matrix that close to the identity."""
    k = rng.standard_normal((n, n))
    k = k - k.T
    k *= size / np.linalg.norm(k, 2)
    w, v = np.linalg.eigh(1j * k)                  # K = V diag(-i w) V^H
    return np.real((v * np.exp(-1j * w)) @ v.conj().T)


# ---- the largest-|.| entry, the smallest row on a tie ----------------------------------------------------------------------------
def colmax_ref(a2):
    """Per column: the entry of largest magnitude, the one in the smallest row where several rows attain it (0 for a zero column)."""
    a2 = np.asarray(a2)
    rows = np.argmax(np.abs(a2), axis=0)           # argmax returns the first maximum
    return a2[rows, np.arange(a2.shape[1])], rows


# ---- k_resid_final's scalars -----------------------------------------------------------------------------------------------------
def resid_final_ref(rho, theta, n_pc, l_act):
    """out[0], out[2], out[4] of k_resid_final from the residual norms and the Ritz values, as its header states them."""
    resid = 0.0
    for i in range(n_pc):
        den = theta[i] if theta[i] > 1e-5 * theta[0] else 1e-5 * theta[0]
        q = rho[i] / den if den > 0 else rho[i]
        if not (q <= resid):                       # NaN-propagating maximum
            resid = q
    ratio = theta[l_act - 1] / theta[n_pc - 1] if theta[n_pc - 1] > 0 else 1.0
    spread = theta[0] / theta[l_act - 1] if theta[l_act - 1] > 0 else 1.0
    return resid, ratio, spread


# ---- the Chebyshev filter ---------------------------------------------------------------------------------------------------------
def cheb_b(theta, l_act):
    """The filter's bound: theta[l_act - 1], floored at 1e-10 theta[0]; 1 when both are zero."""
    b, floor_ = theta[l_act - 1], 1e-10 * theta[0]
    return b if b > floor_ else (floor_ if floor_ > 0 else 1.0)


def cheb_first(a1, a2, theta, l_act):
    a = 2.0 / cheb_b(theta, l_act)
    return a * a1 - a2


def cheb_first2(z, w, theta, l_act):
    """-> cur, prev (Z is left zero)"""
    a = 2.0 / cheb_b(theta, l_act)
    return a * z - w, w.copy()


def cheb_step(z, cur, prev, theta, l_act):
    a = 2.0 / cheb_b(theta, l_act)
    return 2.0 * (a * z - cur) - prev


def cheb_t(theta, l_act):
    b = cheb_b(theta, l_act)
    return (2.0 * np.asarray(theta[:l_act]) - b) / b


def cheb_td(t, d, dtype=np.float64):
    """T_d(t) = cosh(d acosh t) for t > 1, else 1 (no scaling), evaluated in `dtype`."""
    t = np.asarray(t, dtype=dtype)
    safe = np.where(t > 1, t, dtype(2))
    return np.where(t > 1, np.cosh(dtype(d) * np.arccosh(safe)), dtype(1))


# ---- the triangular substitutions -----------------------------------------------------------------------------------------------
def trsm_rows_ref(wp, r, dinv):
    """w_j = (wp_j - sum_{i<j} w_i R[i][j]) dinv[j], every row of Wp on its own, in plain f64."""
    w = np.zeros_like(wp)
    for j in range(L):
        w[:, j] = (wp[:, j] - w[:, :j] @ r[:j, j]) * dinv[j]
    return w


def xi_ref(r, dinv):
    """The four inverted 16 x 16 diagonal blocks of R by back substitution, column by column (a column with dinv = 0 is zero)."""
    xi = np.zeros((4, 16, 16))
    for J in range(4):
        o = 16 * J
        for c in range(16):
            x = np.zeros(16)
            for i in range(c, -1, -1):
                if i == c:
                    x[i] = dinv[o + i]
                else:
                    x[i] = -(r[o + i, o + i + 1:o + 16] @ x[i + 1:]) * dinv[o + i]
            xi[J, :, c] = x
    return xi


def trsm_blocked_ref(wp, r, xi):
    """X_J = (Wp_J - sum_{I<J} W_I R_IJ) Xi_J over the four 16-column blocks."""
    w = np.zeros_like(wp)
    for J in range(4):
        t = wp[:, 16 * J:16 * J + 16].copy()
        for I in range(J):
            t -= w[:, 16 * I:16 * I + 16] @ r[16 * I:16 * I + 16, 16 * J:16 * J + 16]
        w[:, 16 * J:16 * J + 16] = t @ xi[J]
    return w


def trsm_residual(w, r, wp, n):
    """max over the entries of the leading n columns of |W R - Wp| / (|W| |R|), in longdouble (0 / 0 counts as 0)."""
    num = np.abs(ld(w) @ ld(r) - ld(wp))[:, :n]
    den = (np.abs(ld(w)) @ np.abs(ld(r)))[:, :n]
    q = np.where(den > 0, num / np.where(den > 0, den, 1), np.where(num > 0, np.inf, 0))
    return float(q.max()) if q.size else 0.0


# ---- the Jacobi eigen-solve -------------------------------------------------------------------------------------------------------
def _slot_of_c(i):
    return 1 if i == 0 else (2 * i if i <= L // 2 - 1 else 2 * ((L - 1) - i) + 1)


def round_pairs(r):
    """The 32 disjoint pairs (p, q) of round r of the round-robin tournament on 64 players: player 0 stays, the others move one
    step round the circle every round."""
    m1 = L - 1
    out = [(0, _slot_of_c((-r) % m1))]
    for m in range(1, L // 2):
        out.append((_slot_of_c((m - r) % m1), _slot_of_c((m1 - m - r) % m1)))
    return out


ROUNDS = [round_pairs(r) for r in range(L - 1)]


def rotation(app, aqq, apq):
    """t, c of the rotation that annihilates a_pq (rows / columns combined as new_p = c p - s q, new_q = s p + c q), vectorised;
    nothing to rotate (t = 0, c = 1) unless b^2 + d^2 > 1e-290 and b != 0, b = 2 a_pq, d = a_qq - a_pp."""
    b, d = 2.0 * apq, aqq - app
    x = b * b + d * d
    live = (x > 1e-290) & (b != 0.0)
    xs = np.where(live, x, 1.0)
    u = np.abs(d) + np.sqrt(xs)
    ab = np.where((d >= 0) == (b >= 0), np.abs(b), -np.abs(b))
    t = np.where(live, ab / u, 0.0)
    c = np.where(live, u / np.sqrt(u * u + b * b), 1.0)
    return t, c


@dataclass
class EigResult:
    U: np.ndarray
    theta: np.ndarray
    sweeps: int                  # full sweeps before the measurement that stopped the solve
    status: int
    want_history: list           # the wanted index set of every sweep's measurement
    off_history: list            # sqrt(off / diag) of every measurement


def jacobi_ref(h, n, off_tol2, n_want):
    """The eigen-solve as jacobi.inl's header defines it, on the 64 x 64 padded matrix: symmetrise the leading n x n block (the rest
    is zero), round-robin sweeps of 63 rounds of 32 disjoint rotations; before a sweep's first round the off-diagonal sum over
    the pairs with a wanted index is measured — wanted: the n_want largest diagonal entries as ranked at the measurement one
    sweep earlier (all of them at the first) — and compared with off_tol2 x the sum of the squared diagonal (taken, like the ranks,
    once that first round is applied); the solve leaves after that round.  30 sweeps at most.  Eigenvalues descending, ties by
    index, padded indices last; eigenvector c in column c of U."""
    a = np.zeros((L, L))
    a[:n, :n] = 0.5 * (h[:n, :n] + h[:n, :n].T)
    u = np.eye(L)
    want = np.ones(L, dtype=bool)
    status, sweeps = 0, 0
    wants, offs = [], []
    iu = np.triu_indices(L, 1)
    for sweep in range(MAX_SWEEPS + 1):
        sweeps = sweep
        pair_wanted = (want[:, None] | want[None, :])[iu]
        off = float(np.sum(np.where(pair_wanted, a[iu] ** 2, 0.0)))
        wants.append(np.flatnonzero(want))
        stop = False
        for r in range(L - 1):
            pq = ROUNDS[r]
            p = np.array([x[0] for x in pq])
            q = np.array([x[1] for x in pq])
            app, aqq, apq = a[p, p], a[q, q], a[p, q]
            t, c = rotation(app, aqq, apq)
            s = t * c
            ap, aq = a[p, :].copy(), a[q, :].copy()
            a[p, :] = c[:, None] * ap - s[:, None] * aq
            a[q, :] = s[:, None] * ap + c[:, None] * aq
            ap, aq = a[:, p].copy(), a[:, q].copy()
            a[:, p] = c[None, :] * ap - s[None, :] * aq
            a[:, q] = s[None, :] * ap + c[None, :] * aq
            a[p, p] = app - t * apq                # the diagonal and the annihilated pivot as the rotation gives them
            a[q, q] = aqq + t * apq
            a[p, q] = 0.0
            a[q, p] = 0.0
            up, uq = u[:, p].copy(), u[:, q].copy()
            u[:, p] = c[None, :] * up - s[None, :] * uq
            u[:, q] = s[None, :] * up + c[None, :] * uq
            if r == 0:
                dg = np.diag(a)
                diag2 = float(np.sum(dg ** 2))
                offs.append(np.sqrt(off / diag2) if diag2 > 0 else np.inf)
                if not (off > off_tol2 * diag2):
                    stop = True
                elif sweep >= MAX_SWEEPS:
                    stop = True
                    status = STAT_EIG
                # rank of every diagonal entry among the 64 (descending, ties by index): who is wanted one sweep later
                order = np.lexsort((np.arange(L), -dg))
                rank = np.empty(L, dtype=int)
                rank[order] = np.arange(L)
                want = rank < n_want
                if stop:
                    break
        if stop:
            break
    dg = np.diag(a).copy()
    idx = np.arange(L)
    real = idx < n
    order = np.lexsort((idx, np.where(real, -dg, 0.0), ~real))       # real indices first, descending, ties by index
    theta = np.where(real[order], dg[order], 0.0)
    uo = u[:, order].copy()
    uo[n:, :] = 0.0
    uo[:, n:] = 0.0
    return EigResult(uo, theta, sweeps, status, wants, offs)


# ---- the eigen-solve's cases ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class EigCase:
    name: str
    family: str
    n: int
    n_want: int
    off_tol2: float
    arg: float = 0.0

    def __str__(self):
        return self.name


GEOM_N = (1, 2, 3, 31, 32, 33, 63, 64)
SPECIAL = ("diag3", "cluster", "repeated", "rank5", "indefinite", "scaled_up", "scaled_down", "antisym")
TOLS = (1e-6, 1e-22, 1e-30)
# the cases (named by their all-pairs member) in which asking for 54 of the 64 pairs saves the restatement a sweep
EARLY_STOP_SAVES = ("ritz1-want64-tol1e-22", "ritz2-want64-tol1e-22", "ritz2-want64-tol1e-30")


def eig_cases():
    cs = []
    for tol in TOLS:
        for n in GEOM_N:
            cs.append(EigCase(f"geom-n{n}-tol{tol:g}", "geom", n, n, tol))
    for fam in SPECIAL:
        cs.append(EigCase(f"{fam}-tol1e-22", fam, L, L, 1e-22))
    for size in (0.1, 0.01):
        for n_want in (14, 54, 64):
            for tol in TOLS:
                cs.append(EigCase(f"block{size:g}-want{n_want}-tol{tol:g}", "block", L, n_want, tol, size))
    for step in (1, 2):
        for n_want in (14, 54, 64):
            for tol in TOLS:
                cs.append(EigCase(f"ritz{step}-want{n_want}-tol{tol:g}", "ritz", L, n_want, tol, float(step)))
    return cs


@lru_cache(maxsize=None)
def ritz_step_matrices():
    """The projected matrices of two consecutive Rayleigh-Ritz steps of the solver's own schedule, simulated in numpy on a
    300 x 300 operator: 50 eigenvalues geomspace(100, 1), four guards 0.9 .. 0.75 and a crowd of 246 within 1 % of each other at
    0.5.  The ten unwanted guard columns of a 64-column block then span a dense perturbation of a multiple of the identity that
    is well separated from the 54 wanted pairs: the situation the early stop of the eigen-solve is written for."""
    rng = rng_of(5)
    k = 300
    lam = np.concatenate([np.geomspace(100.0, 1.0, 50), [0.9, 0.85, 0.8, 0.75], np.sort(0.5 + 0.005 * rng.random(k - 54))[::-1]])
    q = random_orthogonal(k, rng)
    c = (q * lam) @ q.T
    c = 0.5 * (c + c.T)
    w = rng.standard_normal((k, L))
    for _ in range(4):                              # sweeps of three applications and an orthonormalisation
        w = np.linalg.qr(c @ (c @ (c @ w)))[0]
    h1 = w.T @ c @ w
    _, u = np.linalg.eigh(0.5 * (h1 + h1.T))
    w2 = np.linalg.qr(c @ (c @ (c @ (w @ u[:, ::-1]))))[0]
    h2 = w2.T @ c @ w2
    return h1, h2


@lru_cache(maxsize=None)
def eig_matrix(family, n, arg=0.0):
    """The 64 x 64 input of a case (what lies outside the leading n x n block is finite garbage), read-only."""
    rng = rng_of(1, SPECIAL.index(family) if family in SPECIAL else (90 if family == "geom" else 91), n, int(arg * 1000))
    if family == "ritz":
        h = ritz_step_matrices()[int(arg) - 1].copy()          # (not symmetrised: the products leave it symmetric to rounding)
        h.setflags(write=False)
        return h
    h = rng.standard_normal((L, L)) * 3.0 + 0.5     # the garbage
    if family == "geom":
        lam = np.geomspace(1.0, 1e-12, n) if n > 1 else np.array([1.0])
        q = random_orthogonal(n, rng)
        m = (q * lam) @ q.T
    elif family == "diag3":
        m = 3.0 * np.eye(n)
    elif family == "cluster":
        s = rng.standard_normal((n, n))
        m = np.eye(n) + 1e-9 * 0.5 * (s + s.T)
    elif family == "repeated":
        lam = np.concatenate([np.full(20, 1.0), np.full(20, 0.5), np.zeros(24)])
        q = random_orthogonal(n, rng)
        m = (q * lam) @ q.T
    elif family == "rank5":
        b = rng.standard_normal((n, 5))
        m = b @ b.T
    elif family == "indefinite":
        q = random_orthogonal(n, rng)
        m = (q * np.linspace(-1.0, 1.0, n)) @ q.T
    elif family in ("scaled_up", "scaled_down"):
        q = random_orthogonal(n, rng)
        m = ((q * np.geomspace(1.0, 1e-6, n)) @ q.T) * (2.0 ** (100 if family == "scaled_up" else -100))
    elif family == "antisym":
        q = random_orthogonal(n, rng)
        m = (q * np.geomspace(1.0, 1e-4, n)) @ q.T
        m = 0.5 * (m + m.T)
        k = rng.standard_normal((n, n))
        k = k - k.T
        m = m + k * (1e-8 * np.linalg.norm(m) / np.linalg.norm(k))
    elif family == "block":
        top = np.geomspace(100.0, 1.0, 50)
        # 14 within 3 % of each other, theta_64 / theta_50 = 0.97: the four guards n_pc + 4 reaches stand apart from the other ten, so
        # that the wanted set does not depend on the order rounding gives a crowd
        tail = top[-1] * np.concatenate([[0.999, 0.995, 0.99, 0.985], 0.97 + 1e-6 * np.arange(9, -1, -1.0)])
        q = expm_antisym(n, arg, rng)
        m = (q * np.concatenate([top, tail])) @ q.T
    else:
        raise ValueError(family)
    if family != "antisym":
        m = 0.5 * (m + m.T)
    h[:n, :n] = m
    h.setflags(write=False)
    return h


def eig_input(case):
    return eig_matrix(case.family, case.n, case.arg)


def symmetrised(h, n):
    hs = np.zeros((L, L))
    hs[:n, :n] = 0.5 * (h[:n, :n] + h[:n, :n].T)
    return hs


@lru_cache(maxsize=None)
def eig_reference(case):
    """The restatement's solve of a case and numpy's eigenvalues of the symmetrised block (descending, padded with zeros)."""
    h = eig_input(case)
    res = jacobi_ref(h, case.n, case.off_tol2, case.n_want)
    lam = np.zeros(L)
    lam[:case.n] = np.linalg.eigvalsh(symmetrised(h, case.n)[:case.n, :case.n])[::-1]
    return res, lam


def clusters_of(lam, n, hs_norm):
    """Groups of eigenvalues closer together than 1e-6 ||Hs||_F, as (first, last + 1, gap to the rest of the spectrum)."""
    cuts = [0] + [i for i in range(1, n) if lam[i - 1] - lam[i] > 1e-6 * hs_norm] + [n]
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        gap = min(lam[a - 1] - lam[a] if a > 0 else np.inf, lam[b - 1] - lam[b] if b < n else np.inf)
        out.append((a, b, gap))
    return out


def eig_orthogonality(U, n):
    return float(np.abs(U[:n, :n].T @ U[:n, :n] - np.eye(n)).max())


def eig_checks(case, U, theta, sweeps, status, orth_allow=None, sweeps_allow=None):
    """Everything an eigen-solve of `case` must satisfy, for the restatement and for the device alike; returns the reached figures.
    orth_allow / sweeps_allow: the measured allowances the device is held to (None: not checked)."""
    n, h = case.n, eig_input(case)
    hs = symmetrised(h, n)
    _, lam = eig_reference(case)
    hs_norm = float(np.linalg.norm(hs))
    floor_ = 64 * EPS * hs_norm
    assert status == 0, f"{case}: status {status}"
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(theta))
    assert np.all(np.diff(theta[:n]) <= 0), f"{case}: theta is not descending"
    assert np.all(theta[n:] == 0)
    assert np.all(U[n:, :] == 0) and np.all(U[:, n:] == 0)
    n_w = min(case.n_want, n)
    # wanted pairs: the kernel's own stop rule (the off-diagonal row of a wanted index is inside the measured sum) + the rounding floor
    bound = np.sqrt(case.off_tol2) * float(np.linalg.norm(theta)) + floor_
    resid = np.linalg.norm(ld(hs) @ ld(U) - ld(U) * ld(theta)[None, :], axis=0).astype(np.float64)
    assert np.all(resid[:n_w] <= bound), f"{case}: wanted residual {resid[:n_w].max():.3e} > {bound:.3e}"
    dlam = np.abs(theta - lam)
    assert np.all(dlam[:n_w] <= bound), f"{case}: wanted |theta - lambda| {dlam[:n_w].max():.3e} > {bound:.3e}"
    # every diagonal entry of U^T Hs U is a Rayleigh quotient: none lies below the smallest eigenvalue ("errs upward")
    assert theta[:n].min() >= lam[n - 1] - floor_, f"{case}: theta_min {theta[:n].min():.17g} < lambda_min {lam[n - 1]:.17g}"
    orth = eig_orthogonality(U, n)
    if orth_allow is not None:
        assert orth <= orth_allow, f"{case}: |U^T U - I| {orth:.3e} > {orth_allow:.3e}"
    if sweeps_allow is not None:
        assert sweeps <= sweeps_allow, f"{case}: {sweeps} sweeps > {sweeps_allow}"
    # repeated eigenvalues: the spectral projector of every cluster that lies wholly among the wanted columns.  Davis-Kahan:
    # || sin Theta ||_F <= || R ||_F / gap with R the cluster's residual block, and || P - P' ||_F = sqrt(2) || sin Theta ||_F;
    # the columns' own departure from orthonormality (<= 64 x the entrywise figure) comes on top
    w, v = np.linalg.eigh(hs[:n, :n])
    v = v[:, ::-1]
    proj = 0.0
    for a, b, gap in clusters_of(lam, n, hs_norm):
        if b > n_w or not np.isfinite(gap):
            continue
        p_ref = v[:, a:b] @ v[:, a:b].T
        p_got = U[:n, a:b] @ U[:n, a:b].T
        err = float(np.linalg.norm(p_got - p_ref))
        allow = 2.0 * np.sqrt(b - a) * bound / gap + 64 * max(orth, 64 * EPS)
        assert err <= allow, f"{case}: projector of eigenvalues {a}..{b - 1}: {err:.3e} > {allow:.3e}"
        proj = max(proj, err / allow)
    if n_w == n:                                    # the whole basis: U U^T = I is the projector of the one cluster of 3 I too
        err = float(np.abs(U[:n, :n] @ U[:n, :n].T - np.eye(n)).max())
        assert err <= 64 * max(orth, 64 * EPS)
    return {"resid": float(resid[:n_w].max()), "bound": bound, "dlam": float(dlam[:n_w].max()), "orth": orth, "sweeps": sweeps,
            "proj": proj}


# ---- the CholeskyQR's cases ----------------------------------------------------------------------------------------------------
CHOL_N = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 48, 63, 64)


@lru_cache(maxsize=None)
def chol_matrix(n, ill):
    """G = B^T B of a random 200 x n block in the leading n x n block of a 64 x 64 matrix of finite garbage; `ill`: the columns of B
    scaled so that cond(G) ~ 1e8."""
    rng = rng_of(2, n, int(ill))
    b = rng.standard_normal((200, n))
    if ill and n > 1:
        q, _ = np.linalg.qr(b)
        b = (q * np.geomspace(1.0, 1e-4, n)) @ random_orthogonal(n, rng)      # singular values 1 .. 1e-4: cond(G) = 1e8
    g = rng.standard_normal((L, L)) * 2.0 - 1.0
    g[:n, :n] = b.T @ b
    g[:n, :n] = 0.5 * (g[:n, :n] + g[:n, :n].T)
    g.setflags(write=False)
    return g


@lru_cache(maxsize=None)
def chol_factor_ref(n, ill):
    """numpy's factor of chol_matrix(n, ill) as the kernels' outputs: R (64 x 64, zero outside the leading block's upper triangle),
    dinv, Xi."""
    g = chol_matrix(n, ill)
    r = np.zeros((L, L))
    r[:n, :n] = np.linalg.cholesky(g[:n, :n]).T
    dinv = np.zeros(L)
    dinv[:n] = 1.0 / np.diag(r)[:n]
    return r, dinv, xi_ref(r, dinv)


def chol_checks(g, n, r, dinv, xi=None):
    """The factor of the leading n x n block of g: shape, Higham's backward bound (doubled: a reciprocal square root and a multiply
    in the place of a square root and a divide), the reciprocal diagonal, and the inverted diagonal blocks.  Returns the largest
    ratio of |G - R^T R| to its bound."""
    assert np.all(np.isfinite(r)) and np.all(np.isfinite(dinv))
    assert np.all(np.tril(r, -1) == 0), "R is not upper triangular"
    assert np.all(r[n:, :] == 0) and np.all(r[:, n:] == 0), "R is not zero outside the leading block"
    num = np.abs(ld(g[:n, :n]) - ld(r[:n, :n]).T @ ld(r[:n, :n]))
    den = 2.0 * gamma(n + 1) * (np.abs(ld(r[:n, :n])).T @ np.abs(ld(r[:n, :n])))
    assert np.all(num <= den), f"|G - R^T R| exceeds Higham's bound by {float((num / den).max()):.3f}x"
    assert np.all(np.abs(dinv[:n] * np.diag(r)[:n] - 1.0) <= 4 * EPS)
    assert np.all(dinv[n:] == 0)
    if xi is not None:
        for J in range(4):
            o = 16 * J
            rjj, x = r[o:o + 16, o:o + 16], xi[J]
            cols = max(0, min(16, n - o))
            eye = np.zeros((16, 16))
            eye[:cols, :cols] = np.eye(cols)
            assert np.all(x[:, cols:] == 0), "Xi has a non-zero column at or beyond n"
            err = np.abs(ld(x) @ ld(rjj) - eye)
            assert np.all(err <= gamma(16) * (np.abs(ld(x)) @ np.abs(ld(rjj)))), "Xi_J R_JJ - I exceeds gamma_16 |Xi_J| |R_JJ|"
    return float((num / den).max())

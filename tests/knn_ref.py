"""Host side of the k-NN edge tests, independent of the device code: seeded case builders whose coordinates are integers
(`units`) times one power of two, the exact expectation from int64 arithmetic, and the restatement of the certificate's
eps_row from the header comment of knn.hip (with the dispatch constants K, K', CAP the cases are aimed at).

Every squared distance of a case is an integer below 2^53 times 4^exp, so the device's f64 difference form is exact too:
indices must be equal and distances bit-identical, with no near-tie allowance."""
from dataclasses import dataclass, field

import numpy as np

SLACK = 8                                   # K' = k + 8
CAP_MAX = 120
WIDTHS = (8, 20, 36, 52, 68, 132)           # instantiated widths of k_knn_candidates
U = 2.0 ** -24


def width(d):
    """Padded coordinate count of the candidate pass: the first instantiated width above d (d + 1 with the norm)."""
    return next(w for w in WIDTHS if d < w)


def admissible(n_ref, self_graph, include_self):
    return n_ref - (1 if self_graph and not include_self else 0)


def n_candidates(k, n_ref, self_graph, include_self):
    return min(k + SLACK, max(admissible(n_ref, self_graph, include_self), 1))


def cap(kp):
    return min(2 * kp + 32, CAP_MAX)


@dataclass
class Case:
    name: str
    units: np.ndarray                       # int64, n_ref x d
    exp: int = 0                            # x = (units + shift) * 2^exp
    query: np.ndarray = None                # int64 units of the query rows; None: the self graph
    shift: int = 0                          # added to every coordinate, in units
    ks: tuple = (1, 15, 64)
    selfs: tuple = (False,)                 # include_self settings the case runs with
    _cache: dict = field(default_factory=dict, repr=False)

    @property
    def self_graph(self):
        return self.query is None

    @property
    def d(self):
        return self.units.shape[1]

    def points(self):
        """(ref, query or None) as f64, exactly units * 2^exp."""
        def f(u):
            v = u + self.shift
            assert np.abs(v).max(initial=0) < 2 ** 53
            return np.ldexp(v.astype(np.float64), self.exp)
        return f(self.units), None if self.query is None else f(self.query)

    def expected(self, include_self=False):
        """(indices, int64 squared distances in units^2, largest distance) of the min(64 + 8, admissible) nearest
        references of every query row: the stable argsort of the exact distances, so ties go to the lower index."""
        key = bool(include_self)
        if key not in self._cache:
            q = self.units if self.self_graph else self.query
            d2 = np.zeros((q.shape[0], self.units.shape[0]), dtype=np.int64)
            for j in range(self.d):                                    # one coordinate at a time: n x n, not n x n x d
                t = q[:, j][:, None] - self.units[None, :, j]
                d2 += t * t
            dmax = int(d2.max())
            if self.self_graph and not include_self:
                d2[np.arange(len(q)), np.arange(len(q))] = np.iinfo(np.int64).max
            kmax = min(64 + SLACK, admissible(self.units.shape[0], self.self_graph, include_self))
            order = np.argsort(d2, axis=1, kind="stable")[:, :kmax]
            self._cache[key] = (order, np.take_along_axis(d2, order, axis=1), dmax)
        return self._cache[key]

    def expected_k(self, k, include_self=False):
        """(indices n x k, distances n x k as the device must report them: sqrt(exact d2), bit for bit)."""
        idx, d2, _ = self.expected(include_self)
        assert k <= idx.shape[1]
        return idx[:, :k], np.ldexp(np.sqrt(d2[:, :k].astype(np.float64)), self.exp)

    def max_d2(self):
        return self.expected(True)[2]


def eps_row(ref, qry, d=None):
    """eps_row of every query row as knn.hip states it: 1.01 (K + 4) u (2 |q| R + R^2) on points centred at the column
    means of the reference, +inf when R = max |r| is 0 or outside [2^-40, 2^60].  Returns (eps, R)."""
    qry = ref if qry is None else qry
    d = ref.shape[1] if d is None else d
    c = ref.mean(axis=0)
    R2 = float((((ref - c) ** 2).sum(axis=1)).max())
    R = np.sqrt(R2)
    qn = ((qry - c) ** 2).sum(axis=1)
    eps = 1.01 * (width(d) + 4) * U * (2.0 * np.sqrt(qn) * R + R2)
    if not (2.0 ** -40 <= R <= 2.0 ** 60):
        eps = np.full(len(qry), np.inf)
    return eps, R


def cut_gap(case, k, include_self=False):
    """t_K' - t_k of every row in the case's real units (|q|^2 cancels): what the certificate has to work with."""
    kp = n_candidates(k, case.units.shape[0], case.self_graph, include_self)
    _, d2, _ = case.expected(include_self)
    assert kp <= d2.shape[1]
    return np.ldexp((d2[:, kp - 1] - d2[:, k - 1]).astype(np.float64), 2 * case.exp)


def certificate_bounds(case, k, include_self=False):
    """(rows the certificate must prove, rows it must refuse) from the conditions of the header comment: with eps = +inf
    every row is refused; when no more than K' references are admissible nothing is dropped, the bound stays +inf and every
    row is proven; otherwise a row with t_K' - t_k > 2 eps_row is proven and one with t_K' == t_k is refused."""
    ref, qry = case.points()
    eps, _ = eps_row(ref, qry)
    n_q = len(eps)
    if np.isinf(eps).all():
        return 0, n_q
    if admissible(len(ref), case.self_graph, include_self) <= n_candidates(k, len(ref), case.self_graph, include_self):
        return n_q, 0
    gap = cut_gap(case, k, include_self)
    return int((gap > 2.0 * eps).sum()), int((gap == 0).sum())


# ---- 1. every width: differences f32 cannot see ----------------------------------------------------------------------
WIDTH_DIMS = (1, 7, 8, 19, 20, 35, 36, 51, 52, 67, 68, 127, 128)
BLIND_N = 1100


def blind_units(d, n=BLIND_N):
    rng = np.random.default_rng(1000 + d)
    units = rng.integers(-40, 41, (n, d)).astype(np.int64)
    units[:, 0] += (np.arange(n) % 2) * (1 << 24)                 # every second point 2^24 units (2^14) away on axis 0
    return units


def blind_case(d):
    return Case(f"blind_d{d}", blind_units(d), exp=-10)


# ---- 2. k, K' and CAP switches ------------------------------------------------------------------------------------------
SWITCH_KS = (1, 2, 23, 24, 25, 35, 36, 37, 55, 56, 57, 63, 64)
_SWITCH = []


def switch_case():
    if not _SWITCH:
        rng = np.random.default_rng(2020)
        _SWITCH.append(Case("switch_700x20", rng.integers(-3, 4, (700, 20)).astype(np.int64), ks=SWITCH_KS, selfs=(False, True)))
    return _SWITCH[0]


# ---- 3. point counts ----------------------------------------------------------------------------------------------------
COUNT_NS = (2, 9, 10, 31, 32, 33, 63, 64, 65, 72, 73, 127, 128, 129, 255, 256, 257, 300)
COUNT_DIMS = (5, 50)
PAIRS = ((1, 1), (1, 200), (64, 1), (65, 129), (300, 1), (129, 257))


def _ks_upto(adm):
    return tuple(sorted({1, min(64, adm)}))


def count_case(n, d):
    rng = np.random.default_rng(3000 + 7 * n + d)
    return Case(f"count_n{n}_d{d}", rng.integers(-60, 61, (n, d)).astype(np.int64), exp=-4, selfs=(False, True))


def pair_case(n_ref, n_query, d):
    rng = np.random.default_rng(3500 + 11 * n_ref + 3 * n_query + d)
    ref = rng.integers(-60, 61, (n_ref, d)).astype(np.int64)
    qry = rng.integers(-60, 61, (n_query, d)).astype(np.int64)
    qry[::2] = ref[(np.arange(n_query)[::2] * 5) % n_ref]         # every second query is an exact copy of a reference row
    return Case(f"pair_{n_ref}x{n_query}_d{d}", ref, exp=-4, query=qry, ks=_ks_upto(n_ref))


# ---- 4. merge pressure --------------------------------------------------------------------------------------------------
LINE_N = 2000
LINE_ORDERS = ("ascending", "descending", "organ_pipe", "shuffled")
LINE_DIRS = {1: (1,), 3: (1, 2, 2)}


def line_positions(order, n=LINE_N):
    v = np.arange(n, dtype=np.int64)
    if order == "descending":
        v = v[::-1].copy()
    elif order == "organ_pipe":                                   # 0, n-1, 1, n-2, ...: far from the middle first
        w = np.empty(n, dtype=np.int64)
        w[0::2], w[1::2] = v[:(n + 1) // 2], v[::-1][:n // 2]
        v = w
    elif order == "shuffled":
        v = np.random.default_rng(4004).permutation(n).astype(np.int64)
    else:
        assert order == "ascending"
    return v


def line_case(dim, order):
    v = line_positions(order)
    return Case(f"line_d{dim}_{order}", v[:, None] * np.array(LINE_DIRS[dim], dtype=np.int64)[None, :], ks=(1, 64))


def merge_walk(d2_row, kp, self_index=None):
    """The candidate pass of one query restated with exact scores: per 32-reference sub-tile the entries appended (those
    strictly below the bound), a merge to the K' lowest by (score, index) whenever more than CAP - 32 are held, the bound
    falling to the K'-th score.  Returns (entries appended per sub-tile, merges)."""
    full = cap(kp) - 32
    held, added, merges, tau = [], [], 0, None
    for s in range(0, len(d2_row), 32):
        new = [(int(d2_row[i]), i) for i in range(s, min(s + 32, len(d2_row)))
               if i != self_index and (tau is None or d2_row[i] < tau)]
        added.append(len(new))
        held += new
        if len(held) > full:
            held = sorted(held)[:kp]
            tau = held[kp - 1][0]
            merges += 1
    return added, merges


# ---- 5. certificate paths by construction ------------------------------------------------------------------------------
CLUSTER_DK = ((7, 15), (50, 15), (68, 64), (128, 36))
DUPLICATE_DK = ((8, 15), (36, 64))


def clusters_case(d, k):
    rng = np.random.default_rng(5000 + d)
    centres = 8 * rng.integers(-2000, 2001, (12, d)).astype(np.int64)
    units = np.repeat(centres, k + 1, axis=0) + rng.integers(-3, 4, (12 * (k + 1), d))
    return Case(f"clusters_d{d}_k{k}", units[rng.permutation(len(units))].astype(np.int64), ks=(k,))


def clusters_scaled_case(e):
    """The isolated clusters at a power-of-two scale inside the range guard: still all proven (the margin is scale-free)."""
    c = clusters_case(7, 15)
    return Case(f"clusters_d7_k15_scaled_2^{e}", c.units, exp=e, ks=(15,))


def duplicates_case(d, k):
    rng = np.random.default_rng(5500 + d)
    pts = rng.integers(-100, 101, (10, d)).astype(np.int64)
    assert len(np.unique(pts, axis=0)) == 10
    units = np.repeat(pts, k + 10, axis=0)
    return Case(f"duplicates_d{d}_k{k}", units[rng.permutation(len(units))], ks=(k,))


def identical_case():
    rng = np.random.default_rng(5900)
    return Case("identical_300x20", np.repeat(rng.integers(-500, 501, (1, 20)).astype(np.int64), 300, axis=0), exp=-10,
                selfs=(False, True))


# ---- 6. range guard and offsets ----------------------------------------------------------------------------------------
SCALES_OUTSIDE = (-80, 70)
SCALES_INSIDE = (-30, 40)


def scaled_case(e):
    return Case(f"blind_d20_scaled_2^{e}", blind_units(20), exp=-10 + e)


def offset_case():
    return Case("blind_d20_offset_2^30", blind_units(20), exp=-10, shift=1 << 40)          # 2^40 units = 2^30


# ---- every case, for the preconditions ---------------------------------------------------------------------------------
def all_cases():
    """name -> builder of every case of the device file."""
    b = {}
    for d in WIDTH_DIMS:
        b[f"blind_d{d}"] = lambda d=d: blind_case(d)
    b["switch_700x20"] = switch_case
    for d in COUNT_DIMS:
        for n in COUNT_NS:
            b[f"count_n{n}_d{d}"] = lambda n=n, d=d: count_case(n, d)
        for nr, nq in PAIRS:
            b[f"pair_{nr}x{nq}_d{d}"] = lambda nr=nr, nq=nq, d=d: pair_case(nr, nq, d)
    for dim in LINE_DIRS:
        for o in LINE_ORDERS:
            b[f"line_d{dim}_{o}"] = lambda dim=dim, o=o: line_case(dim, o)
    for d, k in CLUSTER_DK:
        b[f"clusters_d{d}_k{k}"] = lambda d=d, k=k: clusters_case(d, k)
    for d, k in DUPLICATE_DK:
        b[f"duplicates_d{d}_k{k}"] = lambda d=d, k=k: duplicates_case(d, k)
    b["identical_300x20"] = identical_case
    for e in SCALES_OUTSIDE + SCALES_INSIDE:
        b[f"blind_d20_scaled_2^{e}"] = lambda e=e: scaled_case(e)
        if e in SCALES_INSIDE:
            b[f"clusters_d7_k15_scaled_2^{e}"] = lambda e=e: clusters_scaled_case(e)
    b["blind_d20_offset_2^30"] = offset_case
    return b


def run_ks(case, include_self):
    """The k values a case runs with under one include_self setting (count cases: 1 and min(64, admissible))."""
    if case.name.startswith("count_"):
        return _ks_upto(admissible(case.units.shape[0], True, include_self))
    return case.ks

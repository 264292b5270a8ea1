"""The inverted-file search of include/srx.h restated in numpy, independent of the device code.  On integer-valued inputs
(int64 arrays) every squared distance is an exact integer, so assignments, probe order, results and counters are exact; on
float arrays the same code runs in f64 (used for the recall floor and the k-means of the training restatement).

    search(ref, cent, k, n_probe, query=None, include_self=False) -> dict with
        assign, offsets, members        the index
        probes                          n_query x n_probe centroid indices by (distance, centroid index)
        idx, d2                         n_query x k neighbours ascending by (distance, point index) and their squared distances
        exhaustive                      bool per row: its probed lists hold fewer than k admissible points
        pairs, points_scanned, rows_exhaustive
"""
import numpy as np

GOLD = np.uint64(0x9E3779B97F4A7C15)


def _big(dtype):
    return np.iinfo(np.int64).max if np.issubdtype(dtype, np.integer) else np.inf


def dist2(a, b):
    """Pairwise squared distances, difference form, summed in coordinate order (int64 exact for integer input)."""
    out = np.zeros((a.shape[0], b.shape[0]), dtype=np.result_type(a.dtype, b.dtype))
    for j in range(a.shape[1]):
        t = a[:, j][:, None] - b[None, :, j]
        out += t * t
    return out


def assign_points(ref, cent):
    """Nearest centroid of every point, ties to the lower centroid index (argmin returns the first minimum)."""
    return np.argmin(dist2(ref, cent), axis=1)


def build_lists(assign, n_lists):
    """(offsets n_lists + 1, members ascending by point index within a list)."""
    members = np.argsort(assign, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=n_lists))])
    return offsets.astype(np.int64), members.astype(np.int64)


def probe_sets(query, cent, n_probe):
    return np.argsort(dist2(query, cent), axis=1, kind="stable")[:, :n_probe]


def search(ref, cent, k, n_probe, query=None, include_self=False):
    self_form = query is None
    q = ref if self_form else query
    nq, n_ref, n_lists = q.shape[0], ref.shape[0], cent.shape[0]
    assign = assign_points(ref, cent)
    offsets, members = build_lists(assign, n_lists)
    probes = probe_sets(q, cent, n_probe)
    probed = np.zeros((nq, n_lists), dtype=bool)
    probed[np.arange(nq)[:, None], probes] = True
    allowed = probed[:, assign]                                    # nq x n_ref: the reference lies in a probed list
    admissible = np.ones((nq, n_ref), dtype=bool)
    if self_form and not include_self:
        admissible[np.arange(nq), np.arange(nq)] = False
    allowed &= admissible
    exhaustive = allowed.sum(axis=1) < k
    allowed[exhaustive] = admissible[exhaustive]
    d2 = dist2(q, ref)
    masked = np.where(allowed, d2, _big(d2.dtype))
    idx = np.argsort(masked, axis=1, kind="stable")[:, :k]         # stable: ties go to the lower point index
    lengths = np.diff(offsets)
    return {"assign": assign, "offsets": offsets, "members": members, "probes": probes, "idx": idx,
            "d2": np.take_along_axis(d2, idx, axis=1), "exhaustive": exhaustive, "pairs": nq * n_probe,
            "points_scanned": int(lengths[probes].sum()), "rows_exhaustive": int(exhaustive.sum())}


def brute(ref, k, query=None, include_self=False):
    """The exact search: (idx, d2), ascending by (distance, point index)."""
    q = ref if query is None else query
    d2 = dist2(q, ref)
    if query is None and not include_self:
        d2[np.arange(len(q)), np.arange(len(q))] = _big(d2.dtype)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return idx, np.take_along_axis(d2, idx, axis=1)


# ---- training ------------------------------------------------------------------------------------------------------------
def mix64(z):
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def splitmix64(x):
    with np.errstate(over="ignore"):
        return mix64(np.asarray(x, dtype=np.uint64) + GOLD)


def sample_order(n_ref, n_train, seed):
    """The training sample: the n_train points with the smallest (h_i, i), h_i = splitmix64(splitmix64(seed) ^ i)."""
    h = splitmix64(splitmix64(np.uint64(seed)) ^ np.arange(n_ref, dtype=np.uint64))
    return np.lexsort((np.arange(n_ref), h))[:n_train]


def default_n_lists(n_ref):
    return int(min(n_ref, max(1, round(4.0 * np.sqrt(n_ref)))))


def train(ref, n_lists=0, train_iters=10, seed=0, max_train_points=0):
    """Lloyd's iterations on the hashed sample, in f64 (numpy's summation order, not the device's)."""
    n_ref = ref.shape[0]
    n_lists = n_lists or default_n_lists(n_ref)
    n_train = min(n_ref, max(max_train_points or 64 * n_lists, n_lists))
    s = ref[sample_order(n_ref, n_train, seed)].astype(np.float64)
    cent = s[:n_lists].copy()
    for _ in range(train_iters):
        a = assign_points(s, cent)
        cnt = np.bincount(a, minlength=n_lists)
        sums = np.zeros_like(cent)
        np.add.at(sums, a, s)
        cent[cnt > 0] = sums[cnt > 0] / cnt[cnt > 0][:, None]
    return cent


def recall(idx, true_idx):
    """Per-row count of true neighbours found."""
    return np.array([len(np.intersect1d(a, b)) for a, b in zip(idx, true_idx)])


# ---- the integer cases of the device tests ---------------------------------------------------------------------------------
EXP = -3                                    # coordinates are units * 2^-3
LATTICE_POS = (100, 100, 200, 300, 400, 500, 600, 700, 800, 900, 1000)      # centroid 1 repeats centroid 0: list 1 stays empty
LATTICE_SIZES = {0: 1, 2: 31, 3: 32, 4: 33, 5: 63, 6: 64, 7: 65, 8: 127, 9: 200, 10: 0}
LATTICE_EDGES = (0, 1, 31, 32, 33, 63, 64, 65, 129)
DUP = 25                                    # k + 10 duplicates for k = 15


def lattice_case(d=5):
    """(ref units, centroid units, query units).  Centroids on a line, 100 apart on axis 0; points within 20 of theirs, so the
    list lengths are as LATTICE_SIZES plans them: every tile edge of LATTICE_EDGES, two points midway between centroids 8 and 9
    (equidistant: they go to 8, which then holds 129), two blocks of DUP duplicates in list 10, 200 points in list 9 (more than
    one query block on one list).  Queries: on the centroids (the 2nd and 3rd nearest tie), midway between them (1st / 2nd and
    5th / 6th tie), far right (the repeated centroids tie at the last two places), copies of points, and random ones."""
    rng = np.random.default_rng(7100 + d)
    cent = np.zeros((len(LATTICE_POS), d), dtype=np.int64)
    cent[:, 0] = LATTICE_POS
    parts = []
    for l, size in LATTICE_SIZES.items():
        p = rng.integers(-20, 21, (size, d)).astype(np.int64)
        p[:, 0] += LATTICE_POS[l]
        parts.append(p)
    mid = rng.integers(-20, 21, (2, d)).astype(np.int64)
    mid[:, 0] = 850
    dup = rng.integers(-20, 21, (2, d)).astype(np.int64)
    dup[:, 0] += 1000
    parts += [mid, np.repeat(dup, DUP, axis=0)]
    ref = np.concatenate(parts)
    ref = ref[rng.permutation(len(ref))]
    qs = []
    for x0 in list(range(100, 1001, 100)) + list(range(150, 1000, 100)) + [1000, 1400, 2000]:
        p = rng.integers(-20, 21, (2, d)).astype(np.int64)
        p[:, 0] = x0
        qs.append(p)
    near9 = rng.integers(-20, 21, (150, d)).astype(np.int64)
    near9[:, 0] += 900
    anywhere = rng.integers(-20, 21, (40, d)).astype(np.int64)
    anywhere[:, 0] = rng.integers(0, 1200, 40)
    qry = np.concatenate(qs + [near9, anywhere, ref[::17]])
    return ref, cent, qry


def blind_case():
    """knn_ref's f32-blind points (every second one 2^24 units away on axis 0) with one centroid per half: inside a list f32
    cannot tell any two points apart, so no row can be certified."""
    from knn_ref import blind_units
    units = blind_units(20)
    cent = np.zeros((2, 20), dtype=np.int64)
    cent[1, 0] = 1 << 24
    return units, cent


def to_f64(units, exp=EXP):
    return np.ldexp(units.astype(np.float64), exp)

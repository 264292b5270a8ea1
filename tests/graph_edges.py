"""Fixtures for the edges of graph.hip (pure numpy, deterministic seeds, no device): k-NN lists built by hand so that a
named branch of a named kernel runs.  test_graph_edges_cpu.py proves on the host restatement (graph_ref.py) that each
fixture exercises what it is named for; test_graph_edges_gpu.py runs the device on them.

Every list is valid unless a test breaks it on purpose: k distinct neighbours per row, none the row itself."""
import numpy as np
import scipy.sparse as sp

TINY = 2.0 ** -1074                        # the smallest subnormal double


def random_list(n, k, seed):
    """Each row a random k-subset of the other n - 1 cells in random order, distances uniform in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    pick = np.argsort(rng.random((n, n - 1)), axis=1)[:, :k]                 # numbers 0 .. n - 2
    idx = (pick + (pick >= np.arange(n)[:, None])).astype(np.uint32)         # ... with the row itself skipped
    return idx, rng.uniform(0.5, 2.0, (n, k))


def pattern(idx):
    """The k-NN edges as a boolean CSR pattern."""
    n, k = idx.shape
    return sp.csr_matrix((np.ones(n * k, bool), idx.ravel().astype(np.int64), np.arange(0, n * k + 1, k)), shape=(n, n))


def in_only_lists(idx):
    """CSR pattern of the in-only entries: row i holds every j that names i and is not named by i (columns ascending)."""
    B = pattern(idx)
    out = (B.T > B).tocsr()
    out.sort_indices()
    return out


def assert_valid(idx):
    n, k = idx.shape
    assert idx.dtype == np.uint32 and idx.max() < n and (idx != np.arange(n)[:, None]).all()
    assert (np.diff(np.sort(idx, axis=1), axis=1) > 0).all()


# ---- 1. every k ---------------------------------------------------------------------------------------------------------
def every_k_sizes(k):
    return (k + 1, k + 2, 2 * k + 3)        # every edge mutual | one spare cell | more than one workgroup's worth of choice


def every_k_list(k, n):
    return random_list(n, k, seed=1000 * k + n)


# ---- 2. integer T -------------------------------------------------------------------------------------------------------
INTEGER_T_KS = (1, 3, 7, 15, 31, 63)


def keep_off_the_underflow_edge(dist, rows):
    """Rows that will be clamped to the floor: an entry whose exponent (d - rho) / floor lies near 745 has a subnormal weight
    of one or two units, and whether it is stored would rest on the last bit of exp.  Such entries are moved inwards (their
    offset halved) until no exponent of these rows lies in [700, 800], as test_graph_gpu.underflow_list keeps its own."""
    d = dist.copy()
    k = d.shape[1]
    for _ in range(20):
        rho = d[rows].min(axis=1, keepdims=True)
        ratio = (d[rows] - rho) / (1e-3 * d[rows].sum(axis=1, keepdims=True) / (k + 1.0))
        near = (ratio > 650) & (ratio < 850)
        if not near.any():
            break
        d[rows] = np.where(near, rho + 0.5 * (d[rows] - rho), d[rows])
    rho = d[rows].min(axis=1, keepdims=True)
    ratio = (d[rows] - rho) / (1e-3 * d[rows].sum(axis=1, keepdims=True) / (k + 1.0))
    assert ((ratio < 700) | (ratio > 800)).all()
    return d


def integer_T_list(k):
    """n = k + 30 (never a multiple of 4), t = log2(k + 1) an integer.  Even rows: the t smallest distances are equal, so
    c = t = T and the row has no root.  Odd rows: the t - 1 smallest are equal, c = max(t - 1, 1).  For k = 1 that is 1 = T
    again (a row always has one neighbour at its own minimum), so every row of that list is without a root.
    Returns (idx, dist, c per row)."""
    assert k in INTEGER_T_KS
    t = int(np.log2(k + 1.0))
    assert 2 ** t == k + 1
    n = k + 30
    assert n % 4 != 0
    idx, dist = random_list(n, k, seed=200 + k)
    order = np.argsort(dist, axis=1)
    c = np.where(np.arange(n) % 2 == 0, t, max(t - 1, 1))
    smallest = dist.min(axis=1)
    for i in range(n):
        dist[i, order[i, :c[i]]] = smallest[i]
    dist = keep_off_the_underflow_edge(dist, np.nonzero(c >= t)[0])
    return idx, dist, c


# ---- 3. upward bracket --------------------------------------------------------------------------------------------------
UPWARD_KS = (2, 3, 4, 5)
UPWARD_N = 400


def upward_list(k):
    """Random lists; at k = 5, where a uniform row almost never starts below T, every tenth row has one near neighbour and
    four far ones at about the same distance: S(max x) = 1 + 3 exp(-~0.99) + exp(-1) = 2.49 < log2 6 = 2.585."""
    idx, dist = random_list(UPWARD_N, k, seed=300 + k)
    if k == 5:
        rng = np.random.default_rng(355)
        for i in range(0, UPWARD_N, 10):
            dist[i] = rng.permutation(np.array([0.5, 1.97, 1.98, 1.99, 2.0]))
    return idx, dist


def s_at_max_x(dist):
    """S(max x), c and T of every row, straight from the definition (rows with a positive distance)."""
    d = np.asarray(dist, dtype=np.float64)
    k = d.shape[1]
    rho = np.where(d > 0, d, np.inf).min(axis=1, keepdims=True)
    one = d <= rho
    x = np.where(one, 0.0, d - rho)
    s = x.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        S = one.sum(axis=1) + np.where(one, 0.0, np.exp(-x / s)).sum(axis=1)
    return S, one.sum(axis=1), np.log2(k + 1.0)


# ---- 4. long downward bracket, clamp and drop in one row -----------------------------------------------------------------
def long_bracket_list(n=40, k=15, seed=41):
    """Ring lists (row i names i + 1 .. i + 15 mod n: no edge has a reverse).  Even rows (class A): one distance 1e-300, four
    3e-300, ten 1e300: the plateau 1 + 4 >= T = 4 puts the root near 7e-300, about 2000 halvings below max x = 1e300, and the
    floor 6.25e296 clamps the row; the small weights are exactly 1, the ten far ones underflow.  Odd rows (class B): two of
    the four at 1e300 instead: the plateau is 3 < T, the root near 4e299, no clamp.  Positions within a row are shuffled."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    idx = ((i[:, None] + np.arange(1, k + 1)[None, :]) % n).astype(np.uint32)
    a = np.array([1e-300] + [3e-300] * 4 + [1e300] * 10)
    b = np.array([1e-300] + [3e-300] * 2 + [1e300] * 12)
    dist = np.array([rng.permutation(a if r % 2 == 0 else b) for r in range(n)])
    return idx, dist


# ---- 5. scale -----------------------------------------------------------------------------------------------------------
SCALE_EXACT = (-1000, -500, 500, 1000, 1015)     # powers of two at which every step of the definition scales exactly
SCALE_OVERFLOW = 1021                            # sum d overflows in most rows
SCALE_SUBNORMAL = -1060                          # distances of 8192 .. 32768 units of 2^-1074


def scale_list():
    return random_list(300, 7, seed=500)


def lo_zero_list(n=20, k=7):
    """Distances of one and two units of 2^-1074 on ring lists: c = 2 < T = 3, x = one unit for the other five, and
    S(one unit) = 2 + 5 / e >= T, so the downward bracket halves one unit to 0.0 and stops there: sigma = one unit."""
    i = np.arange(n)
    idx = ((i[:, None] + np.arange(1, k + 1)[None, :]) % n).astype(np.uint32)
    rng = np.random.default_rng(510)
    row = np.array([1.0, 1.0, 2.0, 2.0, 2.0, 2.0, 2.0]) * TINY
    return idx, np.array([rng.permutation(row) for _ in range(n)])


# ---- 6. window edges of the long-list ordering ---------------------------------------------------------------------------
WINDOW = 1 << 17
WINDOW_N = WINDOW + 700


def window_list(seed=61):
    """k = 2, three hubs with more than 512 in-only entries each:
      (a) hub 1000 (window 0), sources WINDOW + 150 .. WINDOW + 669: nothing of it in window 0
      (b) hub 70001 (window 0), sources WINDOW - 400 .. WINDOW + 129: both sides, with WINDOW - 1 and WINDOW
      (c) hub WINDOW + 690 (window 1), sources 5000 .. 5599: nothing of it in its own window
    Every other cell names the next two cells of a shuffled ring of the non-hubs; a source names its hub in place of the
    first of them; a hub names two cells of the ring that are no sources.  Returns (idx, dist, {hub: sorted sources})."""
    n, k = WINDOW_N, 2
    rng = np.random.default_rng(seed)
    sources = {1000: np.arange(WINDOW + 150, WINDOW + 670), 70001: np.arange(WINDOW - 400, WINDOW + 130),
               WINDOW + 690: np.arange(5000, 5600)}
    hubs = np.array(sorted(sources))
    is_hub = np.zeros(n, bool)
    is_hub[hubs] = True
    ring = rng.permutation(np.nonzero(~is_hub)[0])
    m = len(ring)
    idx = np.zeros((n, k), dtype=np.uint32)
    idx[ring] = ring[(np.arange(m)[:, None] + np.arange(1, k + 1)[None, :]) % m]
    is_source = np.zeros(n, bool)
    for h, src in sources.items():
        idx[src, 0] = h
        is_source[src] = True
    plain = np.nonzero(~is_hub & ~is_source)[0]
    for t, h in enumerate(hubs):
        idx[h] = plain[[7 + 2 * t, n // 2 + 2 * t]]
    return idx, rng.uniform(0.5, 2.0, (n, k)), {int(h): s.astype(np.uint32) for h, s in sources.items()}


# ---- 7. merge with dropped out-edges -------------------------------------------------------------------------------------
MERGE_LENGTHS = (3, 64, 512, 513, 900)


def merge_holes_list(n=3000, k=5, seed=71):
    """test_graph_gpu.hub_list's construction with in-only lists of MERGE_LENGTHS entries; every hub's own row has distances
    [1, 1, 1, 3, 3] in shuffled positions: c = 3 >= log2 6, sigma = the floor 1.5e-3, the two far weights exp(-1333) are
    zero and have no reverse, so each hub drops two of its out-edges and keeps three, with its in-only list merged in
    between.  Returns (idx, dist, {hub: sorted sources})."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(n).astype(np.uint32)
    hubs, ring = ids[:len(MERGE_LENGTHS)], ids[len(MERGE_LENGTHS):]
    m = len(ring)
    assert sum(MERGE_LENGTHS) + k <= m
    idx = np.zeros((n, k), dtype=np.uint32)
    idx[ring] = ring[(np.arange(m)[:, None] + np.arange(1, k + 1)[None, :]) % m]
    sources, at = {}, 0
    for h, length in zip(hubs, MERGE_LENGTHS):
        sources[int(h)] = np.sort(ring[at:at + length])
        idx[ring[at:at + length], 0] = h
        at += length
    dist = rng.uniform(0.5, 2.0, (n, k))
    for t, h in enumerate(hubs):
        idx[h] = ring[at + t * k:at + (t + 1) * k]               # cells that name no hub
        dist[h] = rng.permutation(np.array([1.0, 1.0, 1.0, 3.0, 3.0]))
    return idx, dist, sources


# ---- 8. refusals at the edges --------------------------------------------------------------------------------------------
REFUSAL_N, REFUSAL_K = 67, 64
REFUSAL_SPOTS = ((0, 0), (66, 63), (64, 31))       # first lane of all | last lane of all | first row of the partial workgroup


def refusal_list():
    return random_list(REFUSAL_N, REFUSAL_K, seed=800)


def defects(idx, dist):
    """[(label, idx, dist, word of the message)]: one defect per list, at each of REFUSAL_SPOTS (the duplicate is always lane
    0's neighbour repeated in lane 63 of that row), then one list with all four kinds in different rows."""
    n = len(idx)
    out = []

    def put(arr, r, c, v):
        new = arr.copy()
        new[r, c] = v
        return new

    for r, c in REFUSAL_SPOTS:
        out.append((f"index n at ({r}, {c})", put(idx, r, c, n), dist, "not below n"))
        out.append((f"self at ({r}, {c})", put(idx, r, c, r), dist, "names itself"))
        out.append((f"lane 0 repeated in lane 63 of row {r}", put(idx, r, 63, idx[r, 0]), dist, "twice"))
        out.append((f"NaN at ({r}, {c})", idx, put(dist, r, c, np.nan), "negative, NaN or Inf"))
    four = put(put(put(idx, 66, 63, n), 0, 0, 0), 64, 63, idx[64, 0])
    out.append(("all four", four, put(dist, 33, 17, np.nan), "not below n"))
    return out

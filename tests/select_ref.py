"""The device feature selection (csrc/select.hip) restated in numpy, with no device: the variance of k_gene_var in its operation
order, the true rank under (variance descending, gene index ascending), the sampled threshold and the decision of
k_hvg_candidates, the selection (list, bit mask, prefix counts, slots) and the vectors and trace of k_sel_finish in its order.
Also the shapes and value patterns that tests/test_select_gpu.py runs: tests/test_select_cpu.py checks, without a device, that
every pattern takes the route its GPU test names and that no (G, take) puts kq next to an integer."""
import math

import numpy as np

NONE = 0xffffffff            # rank of a gene outside the candidates / the fallback mark of `counter`
UNUSED = 0x7ffffffe          # SRX_SEL_COUNTER_UNUSED: the full ranking was launched directly
SAMPLE = 512                 # kRankSample
MAX_K = 8192                 # kDevSelMaxK
MAX_G = 65536
ROUTES = (0, 1, 2)           # as the pipeline decides / every gene ranked / the threshold nothing reaches
FULL, FALLBACK, CANDIDATES = "full", "fallback", "candidates"


def rng_of(*key):
    return np.random.default_rng([7919, *[int(k) for k in key]])


# ---- k_gene_var -----------------------------------------------------------------------------------------------------------------
def variance(cnt, s, q):
    """sum / c, sq / c - mean * mean with c = (double)(uint32_t)cnt, every operation rounded on its own; 0 where cnt == 0."""
    cnt = np.asarray(cnt, np.uint64)
    c = (cnt & np.uint64(0xffffffff)).astype(np.float64)
    with np.errstate(all="ignore"):
        mean = np.asarray(s, np.float64) / c
        v = np.asarray(q, np.float64) / c - mean * mean
    return np.where(cnt > 0, v, 0.0)


def plant(var):
    """Moments whose variance is `var` exactly: cnt = 1, sum = 0, sq = v (v / 1 - 0 * 0 = v, and -0.0 - 0.0 = -0.0)."""
    var = np.asarray(var, np.float64)
    return np.ones(len(var), np.uint64), np.zeros(len(var)), var.copy()


# ---- ranks ----------------------------------------------------------------------------------------------------------------------
def order_of(var):
    """Gene ids under (variance descending, index ascending); -0.0 equals +0.0; no NaN."""
    var = np.asarray(var, np.float64)
    assert not np.isnan(var).any()
    return np.lexsort((np.arange(len(var)), -var))          # lexsort is stable and compares floats with <: -0.0 == 0.0


def true_rank(var):
    o = order_of(var)
    r = np.empty(len(o), np.int64)
    r[o] = np.arange(len(o))
    return r


def brute_order(var):
    """The same order by the comparator, O(G^2 log G): the check of order_of."""
    import functools

    def cmp(a, b):
        if var[a] > var[b]:
            return -1
        if var[a] < var[b]:
            return 1
        return -1 if a < b else 1 if a > b else 0
    return np.array(sorted(range(len(var)), key=functools.cmp_to_key(cmp)), np.int64)


# ---- k_hvg_candidates -----------------------------------------------------------------------------------------------------------
def sample_positions(G):
    S = min(G, SAMPLE)
    return np.arange(S, dtype=np.int64) * G // S


def kq_of(G, take):
    S = min(G, SAMPLE)
    q = float(take) / float(G)
    return (q + 4.0 * math.sqrt(q * (1.0 - q) / float(S))) * float(S) + 1.0


def cap_of(G, take):
    return min(G, max(4 * take, 4096))


def threshold(var, take):
    """(thr, M): the value at int(kq) of the sample in descending order (-inf when kq >= S - 1 or G < 512) and the number of
    genes at or above it.  `take` is min(n, G)."""
    var = np.asarray(var, np.float64)
    G = len(var)
    S = min(G, SAMPLE)
    thr = -np.inf
    if S == SAMPLE:
        kq = kq_of(G, take)
        if kq < S - 1:
            thr = np.sort(var[sample_positions(G)])[::-1][int(kq)]
    return thr, int(np.count_nonzero(var >= thr))


def predict(var, n, route):
    """(kind, counter, thr): which ranking runs and what `counter` holds after it."""
    G = len(var)
    take = min(n, G)
    if route == 1 or G < SAMPLE:
        return FULL, UNUSED, -np.inf
    if route == 2:
        return FALLBACK, NONE, np.inf
    thr, M = threshold(var, take)
    if take <= M <= cap_of(G, take):
        return CANDIDATES, M, thr
    return FALLBACK, NONE, thr


def expected_rank(var, n, route):
    """The rank table k_sel_finish reads: the true rank of every gene, or on the candidate route the true rank of the genes
    at or above the threshold (they precede every other gene, so their rank among themselves is their true rank) and NONE for
    the rest."""
    kind, _, thr = predict(var, n, route)
    r = true_rank(var)
    if kind == CANDIDATES:
        r = np.where(np.asarray(var) >= thr, r, NONE)
    return r.astype(np.uint32)


# ---- k_sel_finish: the selection ------------------------------------------------------------------------------------------------
def popcount32(w):
    w = np.asarray(w, np.uint32).astype(np.uint64)
    return np.array([bin(int(x)).count("1") for x in w.ravel()], np.int64).reshape(w.shape)


def mask_of(genes, G):
    """(bits, prefix): the selection's bit mask (gene g = bit g & 31 of word g >> 5) and the exclusive prefix popcounts."""
    n_words = (G + 31) // 32
    flag = np.zeros(n_words * 32, np.uint8)
    flag[np.asarray(genes, np.int64)] = 1
    bits = np.packbits(flag.reshape(n_words, 32), axis=1, bitorder="little").view("<u4").ravel().astype(np.uint32)
    per = flag.reshape(n_words, 32).sum(axis=1, dtype=np.int64)
    prefix = (np.cumsum(per) - per).astype(np.uint32)
    return bits, prefix


def genes_of_bits(bits):
    flag = np.unpackbits(np.asarray(bits, "<u4").view(np.uint8), bitorder="little")
    return np.flatnonzero(flag)


def selection(var, n):
    """(sel_rank, bits, prefix) of HighlyVariable(n)."""
    G = len(var)
    sel = order_of(var)[:min(n, G)]
    return (sel.astype(np.int32),) + mask_of(sel, G)


def slots(genes):
    """The selected genes in ascending order: slot s holds gene slots(genes)[s]."""
    return np.sort(np.asarray(genes, np.int64))


# ---- k_sel_finish: the vectors --------------------------------------------------------------------------------------------------
def vectors(genes, s, q, n_cells, center, scale, G):
    """(mu, sd, dinv, terms): per slot, in the kernel's operation order (no contraction); terms[g] is gene g's term of the
    trace, 0 for a gene outside the selection (a term is never negative, so adding +0.0 changes nothing)."""
    g = slots(genes)
    n = float(n_cells)
    sg, qg = np.asarray(s, np.float64)[g], np.asarray(q, np.float64)[g]
    with np.errstate(all="ignore"):
        mean = sg / n
        var = qg / n - mean * mean
        var = np.where(var < 0, 0.0, var)
        std = np.sqrt(var)
        mu = mean if (center or scale) else np.zeros(len(g))
        sd = std if scale else np.ones(len(g))
        di = np.where(std > 0, 1.0 / std, 1.0) if scale else np.ones(len(g))
        ss = (qg - n * mean * mean) if center else qg.copy()
        ss = np.where(ss < 0, 0.0, ss)
        term = di * di * ss
    terms = np.zeros(G)
    terms[g] = term
    return mu, sd, di, terms


def trace_tree(terms):
    """The sum in k_sel_finish's tree: thread t adds genes t, t + 1024, ... in ascending order, then halving by 512 .. 1."""
    G = len(terms)
    rows = (G + 1023) // 1024
    pad = np.zeros(rows * 1024)
    pad[:G] = terms
    acc = np.zeros(1024)
    for r in pad.reshape(rows, 1024):
        acc = acc + r
    half = 512
    while half > 0:
        acc[:half] = acc[:half] + acc[half:2 * half]
        half >>= 1
    return float(acc[0])


def trace_ld(terms):
    """The longdouble sum of the f64 terms.  (The terms themselves are pinned bit for bit by `vectors`; a longdouble evaluation
    of a term is no reference for it: sq / n - mean^2 cancels.)"""
    return np.sum(np.asarray(terms, np.longdouble))


def trace_bound(terms, k):
    """(ceil(k / 1024) + 16) 2^-53 sum |term|: at most 6 roundings in a term, a sum of depth ceil(k / 1024) + 10."""
    return ((k + 1023) // 1024 + 16) * 2.0 ** -53 * float(np.sum(np.abs(np.asarray(terms, np.longdouble))))


def moments_of(x):
    """cnt, sum, sq of the columns of a dense non-negative matrix (the zeros are not stored)."""
    x = np.asarray(x, np.float64)
    return np.count_nonzero(x, axis=0).astype(np.uint64), x.sum(axis=0), (x * x).sum(axis=0)


def negative_variance_constant(n_cells):
    """A value c whose constant column has sq / n - mean * mean < 0 in f64 (it exists for every n tried; asserted by the caller)."""
    n = float(n_cells)
    for i in range(1, 2000):
        c = 0.1 * i + 0.013
        _, s, q = moments_of(np.full((n_cells, 2), c))        # (summed as realistic_moments sums its columns)
        s, q = s[0], q[0]
        mean = s / n
        if q / n - mean * mean < 0:
            return c
    return None


def realistic_moments(G, n_cells, seed):
    """Random non-negative sparse columns, with gene 3 constant (variance 0 or a rounding away from it), gene 5 empty and
    gene 7 a constant column whose variance rounds below zero."""
    rng = rng_of(31, G, n_cells, seed)
    x = rng.gamma(0.7, 2.0, (n_cells, G)) * (rng.random((n_cells, G)) < 0.3)
    x[:, 3] = 2.5
    x[:, 5] = 0.0
    x[:, 7] = negative_variance_constant(n_cells)
    return moments_of(x)


# ---- the shapes of test_select_gpu.py -------------------------------------------------------------------------------------------
SHAPE_G = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 8191, 8192, 8193,
           16385, 65535, 65536)


def takes_of(G):
    """take in {1, 2, min(G, 151), G - 1, G, G + 5} where the envelope allows it, {1024, 1025, 8192} at the large G."""
    t = {1, 2, min(G, 151), G - 1, G, G + 5}
    if G >= 8191:
        t |= {1024, 1025, 8192}
    return sorted(x for x in t if x >= 1 and min(x, G) <= MAX_K)


def distinct(G, seed=0):
    """Distinct positive variances in random order."""
    rng = rng_of(1, G, seed)
    return rng.permutation(G).astype(np.float64) * 0.37 + rng.random() + 0.5


# ---- the value patterns ---------------------------------------------------------------------------------------------------------
def twice_adjacent(G, shift):
    """Every value twice at g, g + 1; `shift` = 1 starts the pairs at gene 1, so that a pair straddles every even edge (255 | 256,
    2047 | 2048)."""
    rng = rng_of(2, G, shift)
    v = rng.permutation((G + 2) // 2 + 1).astype(np.float64) + 1.0
    return np.ascontiguousarray(np.repeat(v, 2)[shift:][:G])


def twice_half(G):
    """Every value twice at g and g + G // 2."""
    h = G // 2
    v = rng_of(3, G).permutation(h + 1).astype(np.float64) + 1.0
    return np.concatenate([v[:h], v[:h], v[h:h + 1]])[:G] if G % 2 else np.concatenate([v[:h], v[:h]])


def tie_group(G, above, size, seed=0):
    """`above` distinct high values, `size` equal values, the rest distinct and lower, in random places."""
    rng = rng_of(4, G, above, size, seed)
    low = G - above - size
    v = np.concatenate([1000.0 + np.arange(above), np.full(size, 500.0), rng.permutation(low) * (400.0 / low) + 1.0])
    return v[rng.permutation(G)]


def all_equal(G):
    return np.full(G, 3.25)


def zeros_block(G):
    """A third of the genes positive and distinct, the rest zeros of both signs."""
    rng = rng_of(5, G)
    v = np.where(rng.random(G) < 0.5, 0.0, -0.0)
    pos = rng.permutation(G)[:G // 3]
    v[pos] = rng.permutation(len(pos)) + 1.0
    return v


def ramp(G, ascending):
    v = np.arange(G, dtype=np.float64) + 1.0
    return v if ascending else v[::-1].copy()


def too_few(G):
    """High variances only at the sampled positions: the sample promises what the genes do not hold."""
    v = rng_of(6, G).permutation(G) * 1e-3 + 1.0
    p = sample_positions(G)
    v[p] = 1e6 + np.arange(len(p))
    return v


def too_many_ties(G, n_max):
    """n_max genes tied at the largest value (the first n_max genes, so the sample sees them), the rest distinct."""
    v = rng_of(7, G).permutation(G) * 1e-3 + 1.0
    v[:n_max] = 1e6
    return v


def too_many_zero(G, n_pos):
    """n_pos positive genes in random places, the rest 0: the threshold falls on 0."""
    rng = rng_of(8, G)
    v = np.zeros(G)
    pos = rng.permutation(G)[:n_pos]
    v[pos] = rng.permutation(n_pos) + 1.0
    return v


def pattern_cases():
    """(name, variances, n, kind on route 0): every named pattern at the shapes where it bites.  The kinds are what
    test_select_cpu.py proves from this file alone and test_select_gpu.py then holds the device's counter to."""
    c = []
    for G in (300, 513, 2049, 4608):
        for shift in (0, 1):
            c.append(("twice_adjacent%d_%d" % (shift, G), twice_adjacent(G, shift), 151, FULL if G < SAMPLE else CANDIDATES))
    for G in (600, 4100, 8193):
        c.append(("twice_half_%d" % G, twice_half(G), 151, CANDIDATES))
    for G in (300, 700, 4500):
        for size in (3, 64, 300):
            if size + 40 < G:
                c.append(("tie_group%d_%d" % (size, G), tie_group(G, 40, size), 40 + (size + 1) // 2, FULL if G < SAMPLE else CANDIDATES))
    c.append(("tie_group300_first_4500", tie_group(4500, 40, 300, 1), 41, CANDIDATES))
    c.append(("tie_group300_last_4500", tie_group(4500, 40, 300, 2), 339, CANDIDATES))
    for G, n, kind in ((64, 10, FULL), (513, 100, CANDIDATES), (2049, 2048, CANDIDATES), (8193, 100, FALLBACK)):
        c.append(("all_equal_%d" % G, all_equal(G), n, kind))
    for G, n in ((300, 151), (700, 151), (700, 400), (4097, 2000)):
        c.append(("zeros_%d_%d" % (G, n), zeros_block(G), n, FULL if G < SAMPLE else CANDIDATES))
    for G in (257, 2049, 4608):
        for asc in (True, False):
            c.append(("ramp_%s_%d" % ("up" if asc else "down", G), ramp(G, asc), 151, FULL if G < SAMPLE else CANDIDATES))
    c.append(("too_few_5120", too_few(5120), 1000, FALLBACK))
    c.append(("too_many_ties_65536", too_many_ties(65536, 5000), 100, FALLBACK))
    c.append(("too_many_zero_20000", too_many_zero(20000, 5000), 4500, FALLBACK))
    c.append(("every_gene_600", distinct(600, 9), 599, CANDIDATES))
    c.append(("every_gene_4096", distinct(4096, 9), 4090, CANDIDATES))
    return c


def nan_cases():
    """(name, variances with NaN, n): G >= 512, NaN inside the sample, outside it, 600 of them, in the last gene."""
    G = 5120                                   # sampled positions: the multiples of 10
    out = []
    for name, where in (("sampled", [2560]), ("unsampled", [2561]), ("many", list(range(7, 7 + 600 * 8, 8))), ("last", [G - 1]),
                        ("sampled_many", list(range(0, 3000, 10)))):
        v = distinct(G, 11)
        v[where] = np.nan
        out.append((name, v, 100))
    return out

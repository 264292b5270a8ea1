"""Numpy and Python-int restatement of the gene-list section of include/srx.h (srx_gene_list_sums, srx_score_genes_controls,
srx_score_genes) and the inputs of its tests.

The fixed point goes through Python integers and ``fractions`` (round() of a Fraction rounds ties to even), the hash through
Python ints; nothing here calls the library.  A matrix is a ``Csr``: canonical rows, values AS STORED (an explicit 0 is an entry).
The gene means of the score are an INPUT: the definition takes them from srx_compute_sum, bit for bit."""
import math
import os
from fractions import Fraction

import numpy as np

M64 = (1 << 64) - 1
GOLD64 = 0x9E3779B97F4A7C15
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NOT_IN_POOL = 0xFFFFFFFF


class Refused(Exception):
    """What the definition refuses: ``args[0]`` names the reason."""


class Csr:
    def __init__(self, n, G, indptr, indices, values):
        self.n, self.G = int(n), int(G)
        self.indptr = np.asarray(indptr, dtype=np.uint64)
        self.indices = np.asarray(indices, dtype=np.uint64)
        self.values = np.asarray(values)

    @classmethod
    def from_rows(cls, G, rows, dtype):
        """rows: per cell a list of (gene, value), any order; stored sorted by gene, zeros kept"""
        indptr, idx, val = [0], [], []
        for r in rows:
            r = sorted(r)
            assert len({g for g, _ in r}) == len(r)
            idx += [g for g, _ in r]
            val += [v for _, v in r]
            indptr.append(len(idx))
        return cls(len(rows), G, indptr, idx, np.asarray(val, dtype=np.float64).astype(dtype))

    @classmethod
    def from_dense(cls, X, dtype):
        return cls.from_rows(X.shape[1], [[(int(j), X[i, j]) for j in np.flatnonzero(X[i])] for i in range(X.shape[0])], dtype)

    def dense(self):
        X = np.zeros((self.n, self.G), dtype=np.float64)
        ip = self.indptr.astype(np.int64)
        X[np.repeat(np.arange(self.n), np.diff(ip)), self.indices.astype(np.int64)] = self.values.astype(np.float64)
        return X

    def upload(self, ctx):
        import singlerust_amd as sr
        return sr.DeviceCsr.upload(ctx, self.n, self.G, self.indptr, self.indices, self.values)


# ---- the hash --------------------------------------------------------------------------------------------------------------------
def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, j):
    return mix64(seed + GOLD64 * (j + 1))


# ---- 1. sums over gene lists -------------------------------------------------------------------------------------------------------
def scale_log2(max_abs, longest):
    """62 - e - L"""
    e = max(math.frexp(max_abs)[1], -30)             # max_abs = f 2^e, 0.5 <= f < 1; 0 for 0
    L = 0
    while (1 << L) < max(longest, 1):
        L += 1
    return 62 - e - L


def list_sums(csr, lists):
    """(SUM f64 n x T, cnt u32 n x T, sum_scale_log2, S_int as Python ints)"""
    vals = csr.values.astype(np.float64)
    if not np.all(np.isfinite(vals)):
        raise Refused("nan")
    max_abs = float(np.abs(vals).max()) if vals.size else 0.0
    s = scale_log2(max_abs, max(len(l) for l in lists))
    two = Fraction(2) ** s
    member = [set(int(g) for g in l) for l in lists]
    S = [[0] * len(lists) for _ in range(csr.n)]
    cnt = np.zeros((csr.n, len(lists)), dtype=np.uint32)
    ip = csr.indptr.astype(np.int64)
    for i in range(csr.n):
        for p in range(ip[i], ip[i + 1]):
            g = int(csr.indices[p])
            q = None
            for t, mem in enumerate(member):
                if g in mem:
                    if q is None:
                        q = round(Fraction(float(vals[p])) * two)           # ties to even
                    S[i][t] += q
                    cnt[i, t] += 1
    out = np.array([[math.ldexp(float(v), -s) for v in row] for row in S], dtype=np.float64).reshape(csr.n, len(lists))
    assert all(abs(v) < (1 << 62) for row in S for v in row)
    return out, cnt, s, S


# ---- 2. control genes ----------------------------------------------------------------------------------------------------------------
def n_items_of(P, n_bins):
    return int(np.round(P / (n_bins - 1)))


def cuts(mean, pool, n_bins):
    """(cut per gene, NOT_IN_POOL outside the pool; n_items)"""
    mean = np.asarray(mean, dtype=np.float64)
    pool = np.arange(mean.size) if pool is None else np.asarray(pool, dtype=np.int64)
    n_items = n_items_of(pool.size, n_bins)
    if n_items == 0:
        raise Refused("n_items")
    cut = np.full(mean.size, NOT_IN_POOL, dtype=np.uint32)
    ordered = np.sort(mean[pool] + 0.0)                           # -0.0 + 0.0 = +0.0: the two zeros are one value
    rank = 1 + np.searchsorted(ordered, mean[pool] + 0.0, side="left")          # 1 + the number of strictly smaller means
    cut[pool] = rank // n_items
    return cut, n_items


def controls(mean, sets, pool=None, ctrl_size=50, n_bins=25, seed=0, ctrl_as_ref=True):
    """the control list of every set, ascending gene order"""
    cut, _ = cuts(mean, pool, n_bins)
    in_pool = [j for j in range(len(mean)) if cut[j] != NOT_IN_POOL]
    out = []
    for s, genes in enumerate(sets):
        own = set(int(g) for g in genes)
        picked = set()
        for c in sorted({int(cut[g]) for g in own}):
            cand = [j for j in in_pool if cut[j] == c and (ctrl_as_ref or j not in own)]
            if len(cand) > ctrl_size:
                cand = sorted(cand, key=lambda j: (key(seed, j), j))[:ctrl_size]
            picked |= set(cand)
        picked -= own
        if not picked:
            raise Refused("empty", s)
        out.append(np.array(sorted(picked), dtype=np.uint64))
    return out


# ---- 3. the score ----------------------------------------------------------------------------------------------------------------------
def score(csr, gene_mean, sets, pool=None, ctrl_size=50, n_bins=25, seed=0, ctrl_as_ref=True):
    """(score n x n_sets f64, control lists, sum_scale_log2): the sets, then their controls, summed in ONE call (one scale)"""
    ctrl = controls(gene_mean, sets, pool, ctrl_size, n_bins, seed, ctrl_as_ref)
    lists = [np.asarray(s, dtype=np.uint64) for s in sets] + ctrl
    SUM, _, s, _ = list_sums(csr, lists)
    k = len(sets)
    size = np.array([float(len(l)) for l in lists])
    return SUM[:, :k] / size[:k] - SUM[:, k:] / size[k:], ctrl, s


def phase(s_score, g2m_score):
    out = []
    for s, g in zip(s_score, g2m_score):
        p = "S"
        if g > s:
            p = "G2M"
        if s < 0 and g < 0:
            p = "G1"
        out.append(p)
    return np.array(out, dtype=object)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def hashed_counts(n, G, seed, density=0.3, top=9):
    """dense integer counts from the hash: entry (i, j) is kept with probability `density`, its value 1 .. top"""
    X = np.zeros((n, G), dtype=np.float64)
    for i in range(n):
        for j in range(G):
            h = mix64((seed << 40) + i * 1000003 + j)
            if (h >> 11) / 2.0 ** 53 < density:
                X[i, j] = 1 + (h & 0xFF) % top
    return X


def planted(values="log_values"):
    """the fixture as a Csr at f64 (600 x 240): its log1p values (made at f32 precision), or the raw counts with "values" """
    z = np.load(os.path.join(GOLD, "planted_600x240.npz"))
    return Csr(int(z["n_rows"]), int(z["n_cols"]), z["indptr"], z["indices"], np.asarray(z[values], dtype=np.float64))

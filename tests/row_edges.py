"""Fixtures and references for the row kernels of singlerust_amd/csrc/rows.hip, shared by test_row_edges_cpu.py and
test_row_edges_gpu.py (a plain helper module).

`edges()` is one CSR matrix that places a row of every edge length of the kernels' loops at every alignment of its first
entry: the register cache of k_row_pass / k_row_qc covers 2048 entries from the 16-byte boundary at or before the row's start,
so a row starting at `indptr[r] % 4 == a` has `2048 - a` cached entries (f64 storage: `2048 - a % 2`), and the first and last
vector of a row are shared with its neighbours.  `cycle()` is 40 000 short rows, more than any launch has waves, for the
grid-stride loops.  All values are integers 1..49 (exact in f32, every row sum below 2^19 and so the same in any order); a
second value array on the same pattern plants each row's minimum and maximum at its two ends.

The references are numpy from the definitions (csr.rs:87-93, :158-171, :200-210, scale/mod.rs:9-15,66-83): integer sums,
mean = fl64(sum / L), variance = sum((v - mean)^2) / L in np.longdouble, normalised values fl64(v * fl64(target / sum)) cast
to the storage type, logarithms np.log1p in np.longdouble of that exact argument."""
import functools

import numpy as np

N_COLS = 8192
TARGET = 1e4
CACHE = 2048                      # kRowCache * 64
ALIGNMENTS = (0, 1, 2, 3)
EDGE_LENGTHS = ([0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193] + list(range(255, 262)) + list(range(511, 518)) +
                [767, 768, 769, 1023, 1024, 1025] + list(range(2044, 2053)) + [2111, 2112, 2113] +
                [4095, 4096, 4097, 6143, 7000])
CONST_LENGTH, CONST_VALUE = 2049, 7.0
CYCLE_ROWS = 40_000

# bars of the logarithms: the ones tests/test_log1p_gpu.py asserts for the same routines
LOG_F32_REL = 3e-7                # apply_log1p<float>: relative, against the longdouble log1p of the f32 argument
FAST_REL = 2.7e-16                # log1p_f64_fast, what the pipeline stores at f64 storage
# apply_log1p<double> and the pipeline's f32 store: one ulp (of f64 / of f32) — see log_err_in_bars


class RowFixture:
    """indptr / indices (u64), values and minmax_values (f64 holding f32-exact numbers), per row: lens, align = indptr % 4,
    is_edge; pairs[(L, a)] = the edge row of that length and alignment; const_row (or None)."""

    def __init__(self, name, lens, is_edge, indices, values, pairs, const_row):
        self.name = name
        self.n_rows, self.n_cols = len(lens), N_COLS
        self.lens = np.asarray(lens, dtype=np.int64)
        self.indptr = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint64)
        self.align = (self.indptr[:-1] % 4).astype(np.int64)
        self.is_edge = np.asarray(is_edge, dtype=bool)
        self.indices = np.asarray(indices, dtype=np.uint64)
        self.values = np.asarray(values, dtype=np.float64)
        self.rows = np.repeat(np.arange(self.n_rows), self.lens)
        self.pairs, self.const_row = pairs, const_row
        self.nnz = int(self.indptr[-1])
        self.minmax_values = self._plant()
        for a in (self.lens, self.indptr, self.align, self.is_edge, self.indices, self.values, self.rows, self.minmax_values):
            a.setflags(write=False)

    def _plant(self):
        """Edge rows: the unique minimum 0.5 at the first entry, the unique maximum 100 at the last (a row of one entry holds
        100).  Filler rows: 0.25 first and 200 last (one entry: 0.25 in an even row, 200 in an odd one).  A kernel that reads
        one entry across a row boundary sees a value outside its own row's range."""
        mm = self.values.copy()
        ip = self.indptr.astype(np.int64)
        some = self.lens > 0
        first, last = ip[:-1][some], ip[1:][some] - 1
        edge = self.is_edge[some]
        one = (self.lens[some] == 1) & ~edge
        even = np.nonzero(some)[0] % 2 == 0
        mm[first] = np.where(edge, 0.5, 0.25)
        mm[last] = np.where(edge, 100.0, np.where(one & even, 0.25, 200.0))
        return mm

    def typed(self, values, store):
        return values.astype(np.float32 if store == 1 else np.float64)

    def where(self, r):
        r = int(r)
        return f"row {r} of {self.name} (L = {int(self.lens[r])}, a = {int(self.align[r])}, {'edge' if self.is_edge[r] else 'filler'} row)"

    def first_bad_row(self, bad):
        """Message for a per-row failure mask (None if the mask is empty)."""
        bad = np.asarray(bad, dtype=bool)
        if not bad.any():
            return None
        return f"{self.where(np.argmax(bad))}; {int(bad.sum())} of {self.n_rows} rows fail"

    def first_bad_value(self, bad):
        """Message for a per-value failure mask: the row, its L and a, and the first offending position within the row."""
        bad = np.asarray(bad, dtype=bool)
        if not bad.any():
            return None
        p = int(np.argmax(bad))
        r = int(self.rows[p])
        return (f"{self.where(r)}, position {p - int(self.indptr[r])} of the row; {int(bad.sum())} values in "
                f"{len(np.unique(self.rows[bad]))} rows fail")


def _sorted_columns(rng, n):
    return np.sort(rng.choice(N_COLS, size=int(n), replace=False))


@functools.lru_cache(maxsize=None)
def edges():
    """Every (L, a) of EDGE_LENGTHS x ALIGNMENTS once, in a shuffled order, plus one constant row of 2049 entries.  A filler
    row of (a - nnz so far) mod 4 entries before each edge row makes its offset; where that is 0 entries the filler is left
    out or kept empty by a coin, so edge rows also follow each other directly and land on all four wave slots of a workgroup."""
    rng = np.random.default_rng(20480)
    order = [(L, a) for L in EDGE_LENGTHS for a in ALIGNMENTS] + [(CONST_LENGTH, None)]
    order = [order[i] for i in rng.permutation(len(order))]
    lens, is_edge, idx, val, pairs, const_row, pos = [], [], [], [], {}, None, 0
    for L, a in order:
        const = a is None
        if const:
            a = 3
        f = (a - pos) % 4
        if f or rng.random() < 0.5:
            lens.append(f); is_edge.append(False)
            idx.append(_sorted_columns(rng, f)); val.append(rng.integers(1, 50, f).astype(np.float64))
            pos += f
        if const:
            const_row = len(lens)
        else:
            pairs[(L, a)] = len(lens)
        lens.append(L); is_edge.append(True)
        idx.append(_sorted_columns(rng, L))
        val.append(np.full(L, CONST_VALUE) if const else rng.integers(1, 50, L).astype(np.float64))
        pos += L
    return RowFixture("edges", lens, is_edge, np.concatenate(idx), np.concatenate(val), pairs, const_row)


@functools.lru_cache(maxsize=None)
def cycle():
    """40 000 rows of 0, 1, .. 9, 0, 1, .. entries: row_grid caps a launch at 8 workgroups of four rows per CU, so every wave
    walks several rows whatever the CU count."""
    rng = np.random.default_rng(40000)
    lens = np.arange(CYCLE_ROWS) % 10
    nnz = int(lens.sum())
    rows = np.repeat(np.arange(CYCLE_ROWS), lens)
    start = np.concatenate([[0], np.cumsum(lens)])[:-1]
    gaps = rng.integers(1, 800, nnz)                       # 9 gaps of at most 799 stay below 8192
    c = np.cumsum(gaps)
    before = np.concatenate([[0], c])[start]               # the running sum in front of each row
    idx = c - before[rows] - 1
    val = rng.integers(1, 50, nnz).astype(np.float64)
    return RowFixture("cycle", lens, np.ones(CYCLE_ROWS, bool), idx, val, {}, None)


FIXTURES = {"edges": edges, "cycle": cycle}


# ---- references ------------------------------------------------------------------------------------------------------------

def _ld(x):
    assert np.finfo(np.longdouble).nmant >= 63
    return np.asarray(x, dtype=np.float64).astype(np.longdouble)


@functools.lru_cache(maxsize=None)
def row_sums(name):
    fx = FIXTURES[name]()
    s = np.zeros(fx.n_rows, dtype=np.int64)
    np.add.at(s, fx.rows, fx.values.astype(np.int64))
    assert s.max() < 2 ** 19
    out = s.astype(np.float64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def row_variance(name):
    """longdouble sum((v - mean)^2) / L with mean = fl64(sum / L); NaN for an empty row."""
    fx = FIXTURES[name]()
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = row_sums(name) / fx.lens.astype(np.float64)
        d = _ld(fx.values) - _ld(mean)[fx.rows]
        acc = np.zeros(fx.n_rows, dtype=np.longdouble)
        np.add.at(acc, fx.rows, d * d)
        out = acc / fx.lens.astype(np.longdouble)
    out.setflags(write=False)
    return out


def variance_bound(lens):
    """Relative bound of an f64 two-pass row variance against row_variance: the sum is exact, so both use the same mean;
    d = v - mean and d * d are one rounding each (3 * 2^-53 on a term), a sum of L non-negative terms in any order adds
    (L - 1) * 2^-53, the division one more: (L + 3) * 2^-53.  The bar is twice that, rounded up to 2 (L + 4) 2^-53."""
    return 2.0 * (np.asarray(lens, dtype=np.float64) + 4.0) * 2.0 ** -53


def variance_in_bounds(fx, got):
    """(message or None, largest error in units of the bound) of a device / oracle row variance: NaN exactly on the empty rows,
    the constant row exactly 0.0, every other row within variance_bound."""
    want = row_variance(fx.name)
    got = np.asarray(got, dtype=np.float64)
    empty = fx.lens == 0
    msg = fx.first_bad_row(np.isnan(got) != empty)
    if msg:
        return "NaN where a variance is due, or a variance on an empty row: " + msg, np.inf
    if fx.const_row is not None and got[fx.const_row] != 0.0:
        return f"the constant row's variance is {got[fx.const_row]!r}: " + fx.where(fx.const_row), np.inf
    ok = ~empty
    err = np.zeros(fx.n_rows)
    err[ok] = np.abs(got[ok].astype(np.longdouble) - want[ok]).astype(np.float64)
    lim = variance_bound(fx.lens) * np.abs(want.astype(np.float64))
    bad = ok & (err > lim)
    units = float(np.max(err[ok & (lim > 0)] / lim[ok & (lim > 0)], initial=0.0))
    return (("variance outside 2 (L + 4) 2^-53: " + fx.first_bad_row(bad)) if bad.any() else None), units


@functools.lru_cache(maxsize=None)
def min_max(name):
    fx = FIXTURES[name]()
    mn, mx = np.full(fx.n_rows, np.inf), np.full(fx.n_rows, -np.inf)
    np.minimum.at(mn, fx.rows, fx.minmax_values)
    np.maximum.at(mx, fx.rows, fx.minmax_values)
    mn.setflags(write=False); mx.setflags(write=False)
    return mn, mx


@functools.lru_cache(maxsize=None)
def normalized(name):
    """fl64(v * fl64(target / sum)), scale 0 for a zero sum (scale/mod.rs:9-15): the f64 values; cast them with fx.typed."""
    fx = FIXTURES[name]()
    s = row_sums(name)
    scale = np.where(s == 0.0, 0.0, np.float64(TARGET) / np.where(s == 0.0, 1.0, s))
    out = fx.values * scale[fx.rows]
    out.setflags(write=False)
    return out


def ld_log1p(x):
    return np.log1p(_ld(x))


def log_err_in_bars(got, arg, kind):
    """Per-value error of stored logarithms `got` of the exact arguments `arg` in units of the bar of `kind`:
    "f32": apply_log1p<float>, relative error / 3e-7 (got and arg are f32);
    "f64": apply_log1p<double> (ocml log1p), error / ulp of the f64 result;
    "fast": log1p_f64_fast, relative error / 2.7e-16;
    "f32_of_f64": the pipeline's f32 store of an f64 logarithm, distance to the correctly rounded f32 / its ulp."""
    want = ld_log1p(arg)
    assert np.all(want > 0)
    g = np.asarray(got, dtype=np.float64).astype(np.longdouble)
    if kind == "f32":
        return (np.abs(g - want) / want).astype(np.float64) / LOG_F32_REL
    if kind == "f64":
        return np.abs(g - want).astype(np.float64) / np.spacing(np.abs(want.astype(np.float64)))
    if kind == "fast":
        return (np.abs(g - want) / want).astype(np.float64) / FAST_REL
    assert kind == "f32_of_f64"
    want32 = want.astype(np.float32)
    return np.abs(np.asarray(got, dtype=np.float64) - want32.astype(np.float64)) / np.spacing(want32).astype(np.float64)

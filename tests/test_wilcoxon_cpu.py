"""CPU tests of the Wilcoxon rank-sum definition (include/srx.h): the host reference (tests/wilcoxon_ref.py) against scipy's
rankdata and mannwhitneyu and against the hand-sized known answer, and the layout of the two new ABI structs."""
import ctypes as C
import json
import os
from fractions import Fraction

import numpy as np
import scipy.sparse as sp
import scipy.stats

import wilcoxon_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Largest relative deviation |2 norm.sf(|score|) - p_scipy| / p_scipy over the 156 tie-corrected scores of the case below,
# measured where this was written: 9.905e-16 (profiles/markers.md).  Both sides evaluate the same z through a handful of
# differently ordered f64 operations and the same survival function, whose relative condition number |z| pdf(z) / sf(z) is about
# z^2 + 1 (at most 7 at the largest |z| = 2.42 of the case), so the deviation is a few ulp of z carried through sf.  The bound is 100
# times the measured figure.
SCIPY_P_REL_MEASURED = 9.905e-16
SCIPY_P_REL_BOUND = 100 * SCIPY_P_REL_MEASURED


def wilcoxon_case():
    """300 x 40, 4 groups: log-normalised-looking values with many ties; gene 3 all zero, gene 5 one distinct non-zero value,
    gene 7 with negative entries, gene 9 without a zero."""
    rng = np.random.default_rng(20240611)
    X = np.log1p(rng.poisson(1.2, size=(300, 40)) * rng.choice([0.5, 1.0, 2.0], size=(300, 1)))
    X[rng.random(X.shape) < 0.3] = 0.0
    X[:, 3] = 0.0
    X[:, 5] = np.where(rng.random(300) < 0.4, 1.25, 0.0)
    X[:, 7] = rng.integers(-3, 4, 300) * 0.5
    X[:, 9] = 1.0 + rng.integers(0, 5, 300)
    labels = rng.integers(0, 4, 300)
    return X, labels, 4


def test_reference_rank_sums_are_scipys():
    X, labels, k = wilcoxon_case()
    N = X.shape[0]
    constant = [j for j in range(X.shape[1]) if np.unique(X[:, j]).size == 1]
    assert constant == [3] and (X[:, 9] != 0).all() and (X[:, 7] < 0).any() and np.unique(X[:, 5]).size == 2
    assert min(np.unique(X[:, j]).size for j in range(40) if j != 3) >= 2 and max(np.unique(X[:, j]).size for j in range(40)) < 40
    R2, T = ref.rank_sums(X, labels, k)
    sizes = np.bincount(labels, minlength=k)
    assert np.array_equal(R2.sum(axis=0), np.full(40, N * (N + 1), np.uint64))
    ranks = scipy.stats.rankdata(X, axis=0)                    # average ranks: halves, exact in f64
    for g in range(k):
        assert np.array_equal(R2[g].astype(np.float64), 2.0 * ranks[labels == g].sum(axis=0))
        u = scipy.stats.mannwhitneyu(X[labels == g], X[labels != g], axis=0, use_continuity=False, method="asymptotic").statistic
        assert np.array_equal(R2[g].astype(np.float64) / 2 - sizes[g] * (sizes[g] + 1) / 2, u)
    # the tie term against the multiplicities scipy's tie correction uses
    for j in range(40):
        t = np.unique(X[:, j], return_counts=True)[1].astype(np.int64)
        assert int(T[j]) == int((t ** 3 - t).sum())


def test_reference_tie_corrected_scores_give_scipys_p_value():
    X, labels, k = wilcoxon_case()
    R2, T = ref.rank_sums(X, labels, k)
    sizes = np.bincount(labels, minlength=k)
    z, deg = ref.score(R2, T, sizes, X.shape[0], tie_correct=True)
    assert deg == 0
    worst, skipped = 0.0, set()
    for g in range(k):
        p = scipy.stats.mannwhitneyu(X[labels == g], X[labels != g], axis=0, use_continuity=False, method="asymptotic").pvalue
        for j in range(40):
            if np.unique(X[:, j]).size == 1:                   # a constant column: scipy gives NaN, the definition score 0
                assert np.isnan(p[j]) and z[g, j] == 0.0
                skipped.add(j)
                continue
            mine = 2.0 * scipy.stats.norm.sf(abs(z[g, j]))
            worst = max(worst, abs(mine - p[j]) / p[j])
    assert skipped == {3}
    print("largest relative deviation of 2 norm.sf(|score|) from scipy.stats.mannwhitneyu's p-value: %.3e (bound %.3e), largest |z| %.3f"
          % (worst, SCIPY_P_REL_BOUND, np.abs(z).max()))
    assert worst <= SCIPY_P_REL_BOUND
    # without the correction the variance is the untied one: the score of a tied column is smaller in magnitude
    z0, _ = ref.score(R2, None, sizes, X.shape[0], tie_correct=False)
    tied = T > 0
    assert np.all(np.abs(z0[:, tied]) <= np.abs(z[:, tied])) and np.array_equal(z0[:, ~tied], z[:, ~tied])


def load_kat():
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_wilcoxon.json")))
    X = sp.csr_matrix((np.array(kat["data"], np.float64), kat["indices"], kat["indptr"]), shape=(kat["n_rows"], kat["n_cols"]))
    return kat, X


def test_known_answer_against_reference():
    kat, X = load_kat()
    assert X.nnz == 15 and np.signbit(X.data).sum() == 3       # the stored 0.0 and -0.0 are entries (two -1.0 and one -0.0 carry a sign)
    for store in (1, 2):
        for tie_correct, key in ((False, "score"), (True, "score_tie_correct")):
            r = ref.reference(X, kat["labels"], kat["n_groups"], store, tie_correct)
            assert np.array_equal(r["ranksum2"], np.array(kat["ranksum2"], np.uint64)) and np.array_equal(r["ties"], np.array(kat["ties"], np.uint64))
            assert r["groups_degenerate"] == kat["groups_degenerate"]
            # the rational's square root against num / sqrt(d) with d from up to four rounded operations: a few ulp
            assert np.allclose(r["score"], kat[key], rtol=1e-15, atol=0)
            sq = np.array([[float(Fraction(v)) for v in row] for row in kat[key.replace("score", "score_squared")]])
            assert np.allclose(r["score"] ** 2, sq, rtol=2e-15, atol=0)
            order = np.stack([np.lexsort((np.arange(X.shape[1]), -row)) for row in r["score"]])
            assert np.array_equal(order, kat[key.replace("score", "ranked")])


def test_wilcoxon_struct_layouts_match_header():
    """sizeof() of the ctypes mirrors of srx_wilcoxon_opts and srx_wilcoxon_info equals what gcc lays out."""
    import subprocess
    import tempfile
    from singlerust_amd import _ffi
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "srx.h"
int main(void){printf("%zu %zu %zu %zu %d\n", sizeof(srx_wilcoxon_opts), sizeof(srx_wilcoxon_info), offsetof(srx_wilcoxon_opts, scratch_bytes),
                      offsetof(srx_wilcoxon_info, ms_stage), SRX_MARKERS_RANKSUM2); return 0;}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [C.sizeof(_ffi.WilcoxonOpts), C.sizeof(_ffi.WilcoxonInfo), _ffi.WilcoxonOpts.scratch_bytes.offset,
                   _ffi.WilcoxonInfo.ms_stage.offset, _ffi.MARKERS_RANKSUM2]
    assert _ffi.lib().srx_abi_version() == 6                                   # additive: no version bump
    for name in ("srx_rank_genes_wilcoxon", "srx_rank_genes_wilcoxon_graph", "srx_markers_fetch_ties", "srx_markers_wilcoxon_info_get"):
        assert name in _ffi.EXPORTS and getattr(_ffi.lib(), name)

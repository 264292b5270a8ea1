"""CPU tests of the marker-gene definition (include/srx.h): the host reference (tests/markers_ref.py) against scipy's Welch
t-test and against the hand-sized known answer, and the layout of the two new ABI structs."""
import ctypes as C
import json
import os
from fractions import Fraction

import numpy as np
import scipy.sparse as sp
import scipy.stats

import markers_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Largest relative deviation |ref - scipy| / |scipy| of the 160 scores below measured where this was written: 1.008e-13
# (profiles/markers.md).  The reference's variance is the cancelling form Q / n - mean^2, scipy's is two-pass: they differ by
# rounding, amplified by mean^2 / var (and, relative to t, by a small mean difference).  The bound is that deviation with a margin of two orders for other libm / BLAS builds.
SCIPY_REL_BOUND = 1.008e-11


def welch_case():
    rng = np.random.default_rng(20240607)
    X = np.log1p(rng.poisson(1.2, size=(300, 40)) * rng.uniform(0.5, 3.0, size=(300, 1)))
    X[rng.random(X.shape) < 0.3] = 0.0
    labels = rng.integers(0, 4, 300)
    return X, labels, 4


def test_reference_scores_are_welch_t():
    X, labels, n_groups = welch_case()
    Xs = sp.csr_matrix(X)
    cnt, s, q = ref.exact_moments_fsum(Xs, labels, n_groups)
    st = ref.statistics(ref.sizes_of(labels, n_groups), cnt, s, q, X.shape[0], logged=True)
    assert (st["var"] > 0).all() and (st["var_rest"] > 0).all() and st["groups_degenerate"] == 0
    worst = 0.0
    for g in range(n_groups):
        t = scipy.stats.ttest_ind(X[labels == g], X[labels != g], axis=0, equal_var=False).statistic
        worst = max(worst, float(np.max(np.abs(st["score"][g] - t) / np.abs(t))))
    print("largest relative deviation from scipy.stats.ttest_ind: %.3e (bound %.1e)" % (worst, SCIPY_REL_BOUND))
    assert worst <= SCIPY_REL_BOUND


def test_known_answer_against_reference():
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_markers.json")))
    base = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_4x5.json")))
    X = sp.csr_matrix((np.array(base["data"], np.float64), base["indices"], base["indptr"]), shape=(base["n_rows"], base["n_cols"]))
    labels, n_groups = kat["labels"], kat["n_groups"]
    cnt, s, q = ref.exact_moments_int(X, labels, n_groups)
    frac = lambda key: np.array([[float(Fraction(v)) for v in row] for row in kat[key]])
    assert np.array_equal(ref.sizes_of(labels, n_groups), kat["n_cells"])
    assert np.array_equal(cnt, kat["cnt"]) and np.array_equal(s, frac("sum")) and np.array_equal(q, frac("sumsq"))
    st = ref.statistics(kat["n_cells"], cnt, s, q, X.shape[0], logged=False)
    # halves and quarters: the f64 evaluation of these rationals is exact
    for key in ("mean", "var", "mean_rest", "var_rest", "pct", "pct_rest"):
        assert np.array_equal(st[key], frac(key)), key
    assert np.allclose(st["score"], kat["score"], rtol=4e-16, atol=0)          # one division and one square root: 2 ulp
    assert np.allclose(st["lfc"], kat["lfc_unlogged"], rtol=1e-12, atol=1e-12)
    assert st["groups_degenerate"] == kat["groups_degenerate"]
    assert np.array_equal(ref.order(st["score"]), kat["ranked"])
    assert ref.scales(4.0, 4) == (62 - 3 - 2, 62 - 6 - 2) and ref.scales(0.0, 0) == (62, 62) and ref.scales(3.9, 5) == (62 - 2 - 3, 62 - 4 - 3)


def test_markers_struct_layouts_match_header():
    """sizeof() of the ctypes mirrors of srx_rank_genes_opts and srx_markers_info equals what gcc lays out."""
    import subprocess
    import tempfile
    from singlerust_amd import _ffi
    prog = r'''
#include <stdio.h>
#include "srx.h"
int main(void){printf("%zu %zu %d\n", sizeof(srx_rank_genes_opts), sizeof(srx_markers_info), SRX_GROUPS_MAX); return 0;}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        sizes = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert sizes == [C.sizeof(_ffi.RankGenesOpts), C.sizeof(_ffi.MarkersInfo), _ffi.GROUPS_MAX]
    assert _ffi.K_GRAPH == 12 and _ffi.lib().srx_abi_version() == 6          # no new kernel class, no version bump

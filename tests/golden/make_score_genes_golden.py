"""Writes kat_score_genes.json: the worked example of include/srx.h's control-gene bins and a 6-cell x 8-gene score, derived
with `fractions` alone (no numpy, no reference module, no library).  The matrix holds dyadic values, a stored 0 and a negative
value; its column means are the worked example's means, so the bins of the score are the example's.  ctrl_size exceeds every
bin, so no hash takes part: the control list of a set is every gene of its bins but its own.

    python tests/golden/make_score_genes_golden.py
"""
import json
import os
from fractions import Fraction as Fr

N_BINS = 5
MEANS = [0, 0, 1, 2, 3, 5, 8, 13]
# per cell: (gene, value as a string), as stored
ROWS = [
    [(1, "1"), (2, "1.5"), (3, "2"), (4, "0.5"), (5, "5"), (6, "8"), (7, "13")],
    [(1, "-1"), (3, "2"), (4, "3.5"), (5, "5"), (7, "13")],
    [(1, "0"), (2, "2.25"), (3, "2"), (4, "4"), (6, "16"), (7, "13")],
    [(3, "2"), (5, "7.75"), (6, "0.25"), (7, "13")],
    [(2, "2.25"), (3, "2"), (4, "10"), (5, "2.25"), (6, "7.75"), (7, "13")],
    [(3, "2"), (5, "10"), (6, "16"), (7, "13")],
]
SETS = {"a": [3, 5], "b": [4]}


def rint_half_even(q):
    f = q.numerator // q.denominator
    r = q - f
    if r > Fr(1, 2) or (r == Fr(1, 2) and f % 2 == 1):
        f += 1
    return f


def main():
    n, G = len(ROWS), len(MEANS)
    col = [Fr(0)] * G
    for r in ROWS:
        for g, v in r:
            col[g] += Fr(v)
    means = [c / n for c in col]
    assert means == [Fr(m) for m in MEANS]
    n_items = rint_half_even(Fr(G, N_BINS - 1))
    ranks = [1 + sum(1 for o in means if o < m) for m in means]
    cuts = [r // n_items for r in ranks]
    controls, scores = {}, {}
    for name, genes in SETS.items():
        bins = {cuts[g] for g in genes}
        ctrl = [j for j in range(G) if cuts[j] in bins and j not in genes]
        controls[name] = ctrl
        out = []
        for r in ROWS:
            x = {g: Fr(v) for g, v in r}
            s_set = sum((x.get(g, Fr(0)) for g in genes), Fr(0))
            s_ctrl = sum((x.get(g, Fr(0)) for g in ctrl), Fr(0))
            # the sums are dyadic and small: exact in f64; the definition's two divisions and the subtraction in f64
            out.append(float(s_set) / float(len(genes)) - float(s_ctrl) / float(len(ctrl)))
        scores[name] = [repr(v) for v in out]
    doc = {"n_bins": N_BINS, "means": MEANS, "n_items": n_items, "ranks": ranks, "cuts": cuts,
           "n_items_ties": [{"P": 10, "n_bins": 5, "n_items": rint_half_even(Fr(10, 4))}, {"P": 14, "n_bins": 5, "n_items": rint_half_even(Fr(14, 4))},
                            {"P": 12, "n_bins": 25, "n_items": rint_half_even(Fr(12, 24))}, {"P": 36, "n_bins": 25, "n_items": rint_half_even(Fr(36, 24))}],
           "n_genes": G, "rows": [[[g, v] for g, v in r] for r in ROWS], "sets": SETS, "ctrl_size": 50, "controls": controls, "scores": scores}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat_score_genes.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Write tests/golden/kat_paga.json: a PAGA case small enough to check by hand, its tables as exact fractions.

8 cells, k = 2, labels 0 0 0 1 1 1 2 2.  E = [[3, 3, 0], [3, 3, 0], [1, 1, 2]], so es = (6, 6, 4) and N - 1 = 7.
  (0, 1): V = 6, num = 6 * 3 + 6 * 3 = 36, expected 36 / 7, r = 7 / 6 > 1: clipped to 1.
  (0, 2): V = 1, num = 6 * 2 + 4 * 3 = 24, expected 24 / 7, r = 7 / 24.
  (1, 2): the same numbers, so the two pairs TIE: Kruskal takes (0, 1), then (0, 2) before (1, 2), which closes a cycle.

    python tests/golden/make_paga_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import paga_ref as ref  # noqa: E402

K = 2
INDICES = [3, 2, 0, 3, 0, 3, 4, 0, 0, 5, 0, 4, 7, 3, 6, 0]
LABELS = [0, 0, 0, 1, 1, 1, 2, 2]
G = 3


def frac_table(t):
    return {"%d,%d" % k: "%d/%d" % (v.numerator, v.denominator) for k, v in sorted(t.items())}


def main():
    n = len(LABELS)
    indptr = list(range(0, K * n + 1, K))
    E, sizes = ref.counts_of(indptr, INDICES, LABELS, G)
    r = ref.from_counts(E, sizes, G, exact=True)
    doc = {"n": n, "k": K, "n_groups": G, "indices": INDICES, "labels": LABELS, "sizes": sizes,
           "counts": ref.dense_counts(E, G).tolist(), "out_edges": r["out_edges"],
           "expected": frac_table(r["expected_exact"]), "ratio": frac_table(r["ratio_exact"]),
           "tree_pairs": sorted([list(p) for p in r["tree"]]), "info": r["info"]}
    with open(os.path.join(HERE, "kat_paga.json"), "w") as f:
        f.write("{\n" + ",\n".join(' %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in doc.items()) + "\n}\n")     # one key per line


if __name__ == "__main__":
    main()

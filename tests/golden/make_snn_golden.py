"""Writes tests/golden/snn_kat.json: a 6-cell, k = 2 list worked by hand, both `pairs` modes and both include_self values at
prune = 0, from the Python-set restatement in tests/snn_ref.py.

The list: cells 0, 1, 2 name each other; 3 and 4 name each other and 5; 5 names 3 and 2.
With self, N(0) = N(1) = N(2) = {0, 1, 2}: s = 3 of K = 3, J = 3 / (6 - 3) = 1.  N(5) = {2, 3, 5} meets N(2) in {2} alone:
s = 1, J = 1 / 5; the pair (2, 5) is joined by the list (5 names 2), the pairs (0, 5) and (1, 5), which share cell 2 with 5 as
well, are not, and PhenoGraph's restriction drops them.  Without self, N(0) = {1, 2} and N(1) = {0, 2} share cell 2: s = 1 of
K = 2, J = 1 / 3, and N(3) = {4, 5}, N(5) = {2, 3} share nothing although 3 and 5 name each other.

    python tests/golden/make_snn_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import snn_ref as ref  # noqa: E402

IDX = [[1, 2], [0, 2], [0, 1], [4, 5], [3, 5], [3, 2]]


def make():
    cases = []
    for include_self in (1, 0):
        for pairs in (ref.SHARED, ref.KNN):
            got, considered = ref.by_sets(IDX, bool(include_self), pairs, 0.0, ref.JACCARD)
            cases.append({"include_self": include_self, "pairs": pairs, "pairs_considered": considered,
                          "entries": [[i, j, s, str(J)] for (i, j), (s, J, _) in sorted(got.items())]})
    return {"n": 6, "k": 2, "indices": IDX, "cases": cases}


if __name__ == "__main__":
    with open(os.path.join(HERE, "snn_kat.json"), "w") as f:
        json.dump(make(), f, indent=1)
        f.write("\n")

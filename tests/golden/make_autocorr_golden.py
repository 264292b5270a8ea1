#!/usr/bin/env python3
"""Write tests/golden/kat_autocorr.json: Moran's I and Geary's C of a case small enough to check by hand, as exact fractions.

6 cells on a path 0 - 1 - 2 - 3 - 4 - 5 with one chord (1, 4); weights in eighths:
  (0,1) 4/8   (1,2) 2/8   (2,3) 8/8   (3,4) 4/8   (4,5) 2/8   (1,4) 8/8        W = 2 * 28/8 = 7
4 genes of small counts (zeros are not stored):
  gene 0   1 1 1 0 0 0     smooth along the path
  gene 1   2 0 2 0 2 0     alternating
  gene 2   0 0 3 0 0 0     one cell
  gene 3   0 0 0 0 0 0     constant: NaN, counted in genes_constant
Gene 0 by hand: m = 1/2, den = 6/4 = 3/2; sum_ij w z_i z_j = 2 (1/4)(4/8 + 2/8 - 8/8 + 4/8 + 2/8 - 8/8) = -1/4;
  I = (6/7)(-1/4)/(3/2) = -1/7.  sum_ij w (x_i - x_j)^2 = 2 (8/8 + 8/8) = 4;  C = 5 * 4 / (2 * 7 * 3/2) = 20/21.
The values come from the literal double sums in fractions (autocorr_ref.literal_fraction), not from the tables; z is stored as
its exact square, (stat - E)^2 / Var, and its sign.

    python tests/golden/make_autocorr_golden.py
"""
import json
import os
import sys
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import autocorr_ref as ref  # noqa: E402

N = 6
EDGES = [[0, 1, 4], [1, 2, 2], [2, 3, 8], [3, 4, 4], [4, 5, 2], [1, 4, 8]]          # (i, j, eighths)
GENES = [[1, 1, 1, 0, 0, 0], [2, 0, 2, 0, 2, 0], [0, 0, 3, 0, 0, 0], [0, 0, 0, 0, 0, 0]]


def fr(v):
    return None if v is None else "%d/%d" % (v.numerator, v.denominator)


def text():
    """The file's text, one key per line."""
    Wd = [[Fraction(0)] * N for _ in range(N)]
    for i, j, e in EDGES:
        Wd[i][j] = Wd[j][i] = Fraction(e, 8)
    Xd = [[GENES[g][i] for g in range(len(GENES))] for i in range(N)]
    lit = ref.literal_fraction(Xd, Wd)
    s0 = sum(sum(r) for r in Wd)
    s1 = 2 * sum(v * v for r in Wd for v in r)
    s2 = 4 * sum(sum(r) ** 2 for r in Wd)
    n = Fraction(N)
    e_i = Fraction(-1) / (n - 1)
    var_i = (n * n * s1 - n * s2 + 3 * s0 * s0) / ((n * n - 1) * s0 * s0) - e_i * e_i
    var_c = ((2 * s1 + s2) * (n - 1) - 4 * s0 * s0) / (2 * (n + 1) * s0 * s0)

    def z2(stat, e, var):
        return None if stat is None else [fr((stat - e) ** 2 / var), 1 if stat >= e else -1]

    doc = {"n": N, "edges_eighths": EDGES, "genes": GENES, "s0": fr(s0), "s1": fr(s1), "s2": fr(s2), "e_i": fr(e_i), "var_i": fr(var_i),
           "e_c": "1/1", "var_c": fr(var_c), "morans_i": [fr(i) for i, _ in lit], "gearys_c": [fr(c) for _, c in lit],
           "z_i_squared_and_sign": [z2(i, e_i, var_i) for i, _ in lit], "z_c_squared_and_sign": [z2(c, Fraction(1), var_c) for _, c in lit],
           "genes_constant": sum(1 for i, _ in lit if i is None)}
    return "{\n" + ",\n".join(' %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in doc.items()) + "\n}\n"


def main():
    with open(os.path.join(HERE, "kat_autocorr.json"), "w") as f:
        f.write(text())


if __name__ == "__main__":
    main()

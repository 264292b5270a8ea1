"""Writes kat_markers.json: the marker-gene statistics (include/srx.h) of the 4 x 5 matrix of kat_4x5.json with the labels
[0, 1, 0, 1], derived with exact rational arithmetic (fractions) straight from the definition; only the square root of the
score and the logarithm of the fold change are taken in floating point, from the exact rationals."""
import json
import math
import os
from fractions import Fraction as Fr

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    kat = json.load(open(os.path.join(HERE, "kat_4x5.json")))
    n, G = kat["n_rows"], kat["n_cols"]
    labels, n_groups = [0, 1, 0, 1], 2
    rows = [[(kat["indices"][p], Fr(kat["data"][p])) for p in range(kat["indptr"][r], kat["indptr"][r + 1])] for r in range(n)]
    sizes = [labels.count(g) for g in range(n_groups)]
    out = {k: [[None] * G for _ in range(n_groups)] for k in
           ("cnt", "sum", "sumsq", "mean", "var", "mean_rest", "var_rest", "pct", "pct_rest", "score_squared", "score", "lfc_unlogged")}

    def side(member):
        n_s = sum(1 for r in range(n) if member(r))
        c, S, Q = [0] * G, [Fr(0)] * G, [Fr(0)] * G
        for r in range(n):
            if member(r):
                for j, x in rows[r]:
                    c[j] += 1
                    S[j] += x
                    Q[j] += x * x
        mean = [S[j] / n_s for j in range(G)]
        var = [max(Fr(0), (Q[j] / n_s - mean[j] ** 2) * Fr(n_s, n_s - 1)) for j in range(G)]
        return n_s, c, S, Q, mean, var

    for g in range(n_groups):
        ng, c, S, Q, mean, var = side(lambda r: labels[r] == g)
        nr, cr, _, _, mean_r, var_r = side(lambda r: labels[r] != g)
        for j in range(G):
            d = var[j] / ng + var_r[j] / nr
            s2 = (mean[j] - mean_r[j]) ** 2 / d if d > 0 else Fr(0)
            sign = -1.0 if mean[j] < mean_r[j] else 1.0
            out["cnt"][g][j] = c[j]
            out["sum"][g][j] = str(S[j])
            out["sumsq"][g][j] = str(Q[j])
            out["mean"][g][j] = str(mean[j])
            out["var"][g][j] = str(var[j])
            out["mean_rest"][g][j] = str(mean_r[j])
            out["var_rest"][g][j] = str(var_r[j])
            out["pct"][g][j] = str(Fr(c[j], ng))
            out["pct_rest"][g][j] = str(Fr(cr[j], nr))
            out["score_squared"][g][j] = str(s2)
            out["score"][g][j] = sign * math.sqrt(s2) if s2 else 0.0
            out["lfc_unlogged"][g][j] = math.log2((mean[j] + Fr(1, 10 ** 9)) / (mean_r[j] + Fr(1, 10 ** 9)))
    ranked = [sorted(range(G), key=lambda j: (-out["score"][g][j], j)) for g in range(n_groups)]
    doc = {"note": "kat_4x5.json's matrix, labels [0, 1, 0, 1] (group 0 = rows 0 and 2, group 1 = rows 1 and 3; every group and its rest has "
                   "2 cells).  Per (group, gene): c, S = sum x, Q = sum x^2 over the stored entries; mean = S / n; var = max(0, (Q / n - "
                   "mean^2) n / (n - 1)); d = var_g / n_g + var_r / n_r; score^2 = (mean_g - mean_r)^2 / d (0 when d = 0), all as exact "
                   "fractions (python fractions); score = sign(mean_g - mean_r) sqrt(score^2) and lfc_unlogged = log2((mean_g + 1e-9) / "
                   "(mean_r + 1e-9)) with 1e-9 = 1/10^9 are rounded from the exact rationals.  E.g. gene 1, group 0: x = 3, 0 -> mean 3/2, "
                   "Q/n = 9/2, var = (9/2 - 9/4) 2 = 9/2; rest: x = 0, 1 -> mean 1/2, var 1/2; d = 9/4 + 1/4 = 5/2, score^2 = 1 / (5/2) = "
                   "2/5.  ranked = genes by (score descending, index ascending).  Written by make_markers_golden.py.",
           "labels": labels, "n_groups": n_groups, "n_cells": sizes, "groups_degenerate": 0, "ranked": ranked}
    doc.update(out)
    with open(os.path.join(HERE, "kat_markers.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

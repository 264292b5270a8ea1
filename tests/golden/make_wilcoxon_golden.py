"""Writes kat_wilcoxon.json: the Wilcoxon rank-sum tables (include/srx.h) of a 6 x 4 matrix small enough to rank by hand,
derived straight from the definition with integers and exact fractions; only the square root of the score is taken in
floating point, from the exact rational."""
import json
import math
import os
from fractions import Fraction as Fr

HERE = os.path.dirname(os.path.abspath(__file__))

# per row the stored (gene, value) pairs; a stored 0.0 and a stored -0.0 are entries like any other
ROWS = [[(0, 1.5), (1, -1.0), (3, 2.0)],
        [(1, 0.0), (3, 1.0)],
        [(0, 1.5), (3, 4.0)],
        [(0, 2.0), (1, 3.0), (3, 3.0)],
        [(1, -0.0), (3, 6.0)],
        [(0, 0.5), (1, -1.0), (3, 5.0)]]
G = 4
LABELS = [0, 1, 0, 1, 2, 0]
N_GROUPS = 3


def main():
    N = len(ROWS)
    sizes = [LABELS.count(g) for g in range(N_GROUPS)]
    cols = [[Fr(0)] * N for _ in range(G)]
    for r, row in enumerate(ROWS):
        for j, x in row:
            cols[j][r] = Fr(x)                                  # Fr(-0.0) == Fr(0.0): the stored zeros tie with the implicit ones
    R2 = [[0] * G for _ in range(N_GROUPS)]
    T = [0] * G
    for j in range(G):
        col = cols[j]
        for r in range(N):
            b = sum(1 for y in col if y < col[r])
            t = sum(1 for y in col if y == col[r])
            R2[LABELS[r]][j] += 2 * b + t + 1
        for v in set(col):
            t = col.count(v)
            T[j] += t ** 3 - t
        assert sum(R2[g][j] for g in range(N_GROUPS)) == N * (N + 1)

    def scores(tie_correct):
        sq, val = [[None] * G for _ in range(N_GROUPS)], [[None] * G for _ in range(N_GROUPS)]
        for g in range(N_GROUPS):
            ng, nr = sizes[g], N - sizes[g]
            for j in range(G):
                num = Fr(R2[g][j] - ng * (N + 1), 2)
                tc = 1 - Fr(T[j], N ** 3 - N) if tie_correct else Fr(1)
                d = Fr(ng * nr * (N + 1), 12) * tc
                s2 = num * num / d if d > 0 else Fr(0)
                sq[g][j] = str(s2)
                val[g][j] = math.copysign(math.sqrt(s2), num) if s2 else 0.0
        return sq, val

    sq0, s0 = scores(False)
    sq1, s1 = scores(True)
    indptr, indices, data = [0], [], []
    for row in ROWS:
        for j, x in row:
            indices.append(j)
            data.append(x)
        indptr.append(len(indices))
    doc = {"note": "6 cells x 4 genes, labels [0, 1, 0, 1, 2, 0].  Gene 0 = (1.5, ., 1.5, 2, ., 0.5): two implicit zeros tie at "
                   "doubled rank 3, 0.5 has 6, the two 1.5 share 9, 2.0 has 12; group 0 = cells 0, 2, 5 -> R2 = 9 + 9 + 6 = 24; "
                   "T = (8 - 2) + (8 - 2) = 12.  Gene 1 = (-1, 0.0, ., 3, -0.0, -1): the two -1 share 3, the stored 0.0, the "
                   "stored -0.0 and the implicit zero are ONE run of three at 8, 3.0 has 12; T = 6 + 24 = 30.  Gene 2 is "
                   "empty: six zeros at 7, T = 210 = N^3 - N, so the tie-corrected variance is 0 and the score 0.  Gene 3 "
                   "has no zeros and no ties: doubled ranks 2 r.  r2 = 2 b + t + 1 (b smaller values, t members of the tie "
                   "run); R2 = sums per group; num = (R2 - n_g (N + 1)) / 2; d = n_g n_r (N + 1) / 12 (times 1 - T / (N^3 - N) "
                   "when tie-corrected); score^2 = num^2 / d as exact fractions, score = sign(num) sqrt(score^2) rounded "
                   "from the exact rational.  ranked = genes by (score descending, index ascending).  Written by "
                   "make_wilcoxon_golden.py.",
           "n_rows": N, "n_cols": G, "indptr": indptr, "indices": indices, "data": data,
           "labels": LABELS, "n_groups": N_GROUPS, "n_cells": sizes, "groups_degenerate": 0,
           "ranksum2": R2, "ties": T,
           "score_squared": sq0, "score": s0, "ranked": [sorted(range(G), key=lambda j: (-s0[g][j], j)) for g in range(N_GROUPS)],
           "score_squared_tie_correct": sq1, "score_tie_correct": s1,
           "ranked_tie_correct": [sorted(range(G), key=lambda j: (-s1[g][j], j)) for g in range(N_GROUPS)]}
    with open(os.path.join(HERE, "kat_wilcoxon.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

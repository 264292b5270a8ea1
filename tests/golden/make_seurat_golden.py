#!/usr/bin/env python3
"""Known answer of the Seurat v3 gene selection as include/srx.h states it: 9 cells x 6 genes in two batches of 6 and 3 (an empty cell, a gene that is constant in one batch, one clipped entry), every step in
`decimal` at 60 digits (integers stay exact), written as decimal strings into kat_seurat_v3.json.

Independent of tests/hvg_seurat_ref.py in what can differ: the window is found by sorting the distances, the degree of a fit
is min(2, distinct weighted abscissae - 1) counted on the sorted abscissae (the header's rule on the weighted moments must give
the same), and the least-squares intercept comes from a Gaussian elimination of the normal equations in decimal.

    python tests/golden/make_seurat_golden.py
"""
import json
import os
from decimal import Decimal as D
from decimal import getcontext

getcontext().prec = 60

X = [[0, 0, 0, 0, 0, 0],
     [4, 0, 1, 0, 0, 0],
     [3, 0, 0, 0, 0, 1],
     [2, 0, 0, 40, 0, 2],
     [0, 0, 1, 0, 8, 9],
     [5, 7, 0, 0, 0, 0],
     [6, 0, 6, 0, 0, 7],
     [2, 1, 0, 4, 0, 3],
     [0, 0, 7, 2, 0, 0]]
BATCH = [0, 0, 0, 0, 0, 0, 1, 1, 1]
N_BATCHES = 2
SPAN = D(1)
N_TOP = 4


def solve(A, b):
    n = len(b)
    A = [row[:] + [b[i]] for i, row in enumerate(A)]
    for c in range(n):
        p = max(range(c, n), key=lambda r: abs(A[r][c]))
        A[c], A[p] = A[p], A[c]
        for r in range(c + 1, n):
            f = A[r][c] / A[c][c]
            for k in range(c, n + 1):
                A[r][k] -= f * A[c][k]
    x = [D(0)] * n
    for r in range(n - 1, -1, -1):
        x[r] = (A[r][n] - sum(A[r][k] * x[k] for k in range(r + 1, n))) / A[r][r]
    return x


def loess(xs, ys, span):
    m = len(xs)
    q = min(m, max(1, int((span * m + D("0.00001")).to_integral_value(rounding="ROUND_FLOOR"))))
    out = []
    for j in range(m):
        d = sorted(abs(x - xs[j]) for x in xs)
        h = d[q - 1]
        if h == 0:
            pts = [(D(0), D(1), ys[i]) for i in range(m) if xs[i] == xs[j]]
        else:
            pts = []
            for i in range(m):
                if abs(xs[i] - xs[j]) < h:
                    t = (xs[i] - xs[j]) / h
                    pts.append((t, (1 - abs(t) ** 3) ** 3, ys[i]))
        deg = min(2, len({p[0] for p in pts}) - 1)
        pw = lambda t, k: D(1) if k == 0 else t ** k                       # (decimal refuses 0 ** 0)
        A = [[sum(w * pw(t, r + c) for t, w, _ in pts) for c in range(deg + 1)] for r in range(deg + 1)]
        b = [sum(w * pw(t, r) * y for t, w, y in pts) for r in range(deg + 1)]
        out.append(solve(A, b)[0])
    return out


def main():
    n, G = len(X), len(X[0])
    tab = {k: [[None] * G for _ in range(N_BATCHES)] for k in ("mean", "var", "fitted", "clip", "clip_sum", "clip_sumsq", "nv")}
    rank = [[0] * G for _ in range(N_BATCHES)]
    clipped = 0
    for b in range(N_BATCHES):
        rows = [X[i] for i in range(n) if BATCH[i] == b]
        nb = D(len(rows))
        mean = [sum(D(r[j]) for r in rows) / nb for j in range(G)]
        var = [(sum(D(r[j]) ** 2 for r in rows) / nb - mean[j] ** 2) * (nb / (nb - 1)) for j in range(G)]
        ok = [j for j in range(G) if var[j] > 0]
        fit = [D(0)] * G
        for j, e in zip(ok, loess([mean[j].log10() for j in ok], [var[j].log10() for j in ok], SPAN)):
            fit[j] = e
        for j in range(G):
            reg_var = D(10) ** fit[j]
            clip = reg_var.sqrt() * nb.sqrt() + mean[j]
            vals = [min(D(r[j]), clip) for r in rows if r[j]]
            clipped += sum(1 for r in rows if D(r[j]) > clip)
            sc, qc = sum(vals, D(0)), sum((v * v for v in vals), D(0))
            nv = ((nb * mean[j] ** 2 + qc) - 2 * sc * mean[j]) / ((nb - 1) * reg_var)
            for k, v in (("mean", mean[j]), ("var", var[j]), ("fitted", fit[j]), ("clip", clip), ("clip_sum", sc), ("clip_sumsq", qc), ("nv", nv)):
                tab[k][b][j] = v
        order = sorted(range(G), key=lambda j: (-tab["nv"][b][j], j))
        for place, j in enumerate(order):
            rank[b][j] = place
        gaps = [tab["nv"][b][order[i]] - tab["nv"][b][order[i + 1]] for i in range(G - 1)]
        assert all(g > D("1e-6") or g == 0 for g in gaps), gaps          # no order that an f64 rounding could flip
    assert clipped >= 1, "the example must clip a value"
    nbatches = [sum(1 for b in range(N_BATCHES) if rank[b][j] < N_TOP) for j in range(G)]
    median = []
    for j in range(G):
        r = sorted(rank[b][j] for b in range(N_BATCHES) if rank[b][j] < N_TOP)
        median.append(None if not r else (r[(len(r) - 1) // 2] + r[len(r) // 2]) / 2)
    inf = float("inf")
    v3 = sorted(range(G), key=lambda j: (inf if median[j] is None else median[j], -nbatches[j], j))[:N_TOP]
    paper = sorted(range(G), key=lambda j: (-nbatches[j], inf if median[j] is None else median[j], j))[:N_TOP]
    nall = D(n)
    means = [sum(D(r[j]) for r in X) / nall for j in range(G)]
    variances = [(sum(D(r[j]) ** 2 for r in X) / nall - means[j] ** 2) * (nall / (nall - 1)) for j in range(G)]
    vnorm = [sum(tab["nv"][b][j] for b in range(N_BATCHES)) / N_BATCHES for j in range(G)]
    s = lambda v: format(v, ".40e")
    out = {"X": X, "batch": BATCH, "n_batches": N_BATCHES, "span": float(SPAN), "n_top": N_TOP, "clipped_entries": clipped,
           "rank": rank, "nbatches": nbatches, "median": median, "selected": v3, "selected_paper": paper,
           "means": [s(v) for v in means], "variances": [s(v) for v in variances], "variances_norm": [s(v) for v in vnorm]}
    out.update({k: [[s(v) for v in row] for row in t] for k, t in tab.items()})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat_seurat_v3.json")
    json.dump(out, open(path, "w"), indent=1)
    print("wrote", path, "clipped entries:", clipped, "selected:", v3, "paper:", paper)


if __name__ == "__main__":
    main()

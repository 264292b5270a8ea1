"""Writes draw_graph_kat.json: known answers of the ForceAtlas2 definition (include/srx.h) worked out on the CPU.

  pair      two joined points at theta = 0: the three forces and one full iteration (speed rule, positions) in closed form,
            in `decimal` at 60 digits, rounded once to f64 at the end
  triangle  a weighted triangle: rep, grav (both forms) and attr (linear and linlog) of every vertex, the same way
  speed     a table of speed-rule inputs that takes every branch (S == 0 and Tr == 0 included); the outputs are worked out
            in `fractions` (exact +, -, *, /; sqrt in `decimal` at 80 digits), each operation of the header's order rounded to
            f64 by Python's correctly rounded int / int division: an independent model of the IEEE arithmetic, so the library
            is compared with it bit for bit
  quality   600 points in six separated clumps in 10 dimensions (the t-SNE quality input), the connectivities of their k = 30
            list (tests/graph_ref.py): the label purity (the share of points whose 10 nearest layout neighbours all carry
            their label) after the default 500 iterations of the f64 reference at theta = 1.2 from five hashed seeds
            (11 .. 15; the device test runs three others), and their range.  networkx.forceatlas2_layout's purity on the same
            graph is recorded beside it when networkx imports: for the documents, not a bound.

    python tests/golden/make_draw_graph_golden.py
"""
import json
import os
import sys
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import draw_graph_ref as ref  # noqa: E402

getcontext().prec = 80
N, DIM, K, DATA_SEED = 600, 10, 30, 0
SEEDS = [11, 12, 13, 14, 15]
D = Decimal


def dec(x):
    return D(float(x))            # exact: a double is a dyadic rational


def norm(a, b):
    return (a * a + b * b).sqrt()


def forces_dec(Y, W, m, kr, g, strong, linlog):
    """rep, grav, attr of every vertex of a small dense graph, exactly as the header's expressions, in Decimal."""
    n = len(Y)
    rep, grav, attr = [], [], []
    for i in range(n):
        r0 = r1 = D(0)
        a0 = a1 = D(0)
        for j in range(n):
            if j == i:
                continue
            e0, e1 = Y[i][0] - Y[j][0], Y[i][1] - Y[j][1]
            e2 = e0 * e0 + e1 * e1
            f = kr * m[i] * m[j] / e2
            r0, r1 = r0 + f * e0, r1 + f * e1
            w = W[i][j]
            if w:
                if linlog:
                    d = e2.sqrt()
                    w = w * ((1 + d).ln() / d)
                a0, a1 = a0 + w * e0, a1 + w * e1
        rad = norm(*Y[i])
        c = g * m[i] if strong else g * m[i] / rad
        rep.append((r0, r1))
        grav.append((-c * Y[i][0], -c * Y[i][1]))
        attr.append((-a0, -a1))
    return rep, grav, attr


def fl(rows):
    return [[float(a), float(b)] for a, b in rows]


def pair_kat():
    y = [[0.25, 0.5], [-1.0, 0.125]]
    w, kr, g, jtol = 0.7, 2.0, 1.0, 1.0
    Y = [[dec(v) for v in p] for p in y]
    W = [[D(0), dec(w)], [dec(w), D(0)]]
    m = [D(2), D(2)]
    rep, grav, attr = forces_dec(Y, W, m, dec(kr), dec(g), False, False)
    F = [((rep[i][0] + grav[i][0]) + attr[i][0], (rep[i][1] + grav[i][1]) + attr[i][1]) for i in range(2)]
    swing = [norm(*f) for f in F]                       # Fprev = 0
    S = sum(m[i] * swing[i] for i in range(2))
    Tr = S / 2
    # the speed rule at n = 2, speed = eff = 1: opt = 0.05 sqrt 2; S / Tr = 2 is not above 2; S > jt * Tr decides the rest
    opt = dec(0.05) * D(2).sqrt()
    jt = dec(jtol) * max(opt.sqrt(), min(D(10), opt * Tr / 4))
    eff = D(1)
    target = jt * eff * Tr / S
    eff = eff * dec(0.7) if S > jt * Tr else eff * dec(1.3)
    speed = D(1) + min(target - 1, D("0.5"))
    y1 = []
    for i in range(2):
        factor = speed / (1 + (speed * m[i] * swing[i]).sqrt())
        y1.append((Y[i][0] + F[i][0] * factor, Y[i][1] + F[i][1] * factor))
    return {"y": y, "w": w, "scaling_ratio": kr, "gravity": g, "jitter_tolerance": jtol, "mass": [2, 2], "rep": fl(rep), "grav": fl(grav),
            "attr": fl(attr), "F": fl(F), "swing": float(S), "traction": float(Tr), "speed": float(speed), "speed_efficiency": float(eff),
            "y1": fl(y1)}


def triangle_kat():
    y = [[1.0, 0.5], [-0.75, 2.0], [0.375, -1.25]]
    w = [[0.0, 0.5, 1.25], [0.5, 0.0, 2.0], [1.25, 2.0, 0.0]]
    kr, g = 2.0, 1.5
    Y = [[dec(v) for v in p] for p in y]
    W = [[dec(v) for v in r] for r in w]
    m = [D(3), D(3), D(3)]
    out = {"y": y, "w": w, "scaling_ratio": kr, "gravity": g, "mass": [3, 3, 3]}
    rep, grav, attr = forces_dec(Y, W, m, dec(kr), dec(g), False, False)
    _, grav_s, attr_l = forces_dec(Y, W, m, dec(kr), dec(g), True, True)
    out.update(rep=fl(rep), grav=fl(grav), attr=fl(attr), grav_strong=fl(grav_s), attr_linlog=fl(attr_l))
    return out


# ---- the speed rule in exactly rounded steps ---------------------------------------------------------------------------------------------
def R(x):
    """A Fraction rounded to the nearest f64 (int / int true division is correctly rounded), as a Fraction again."""
    return Fraction(float(x))


def rsqrt(x):
    return Fraction(float((D(x.numerator) / D(x.denominator)).sqrt()))


def speed_exact(n, S, Tr, jtol, speed, eff):
    S, Tr, jtol, speed, eff = (Fraction(float(v)) for v in (S, Tr, jtol, speed, eff))
    c = lambda v: Fraction(float(v))      # noqa: E731  (an f64 constant)
    nn = Fraction(n)
    opt = R(c(0.05) * rsqrt(nn))
    a = rsqrt(opt)
    b = R(R(opt * Tr) / R(nn * nn))
    b = b if b < 10 else Fraction(10)
    jt = R(jtol * (a if a > b else b))
    if Tr > 0 and R(S / Tr) > 2:
        if eff > c(0.05):
            eff = R(eff * c(0.5))
        jt = jt if jt > jtol else jtol
    target = None if S == 0 else R(R(R(jt * eff) * Tr) / S)
    if S > R(jt * Tr):
        if eff > c(0.05):
            eff = R(eff * c(0.7))
    elif speed < 1000:
        eff = R(eff * c(1.3))
    cap = R(c(0.5) * speed)
    rise = None if target is None else R(target - speed)
    speed = R(speed + (rise if rise is not None and rise < cap else cap))
    return float(speed), float(eff)


SPEED_INPUTS = [
    # n, S, Tr, jtol, speed, eff
    (1, 0.0, 0.0, 1.0, 1.0, 1.0),                  # S == 0 and Tr == 0
    (10, 0.0, 3.5, 1.0, 2.0, 0.4),                 # S == 0 < Tr: the target is +inf, the rise is capped
    (10, 2.5, 0.0, 1.0, 2.0, 0.4),                 # Tr == 0 < S: the target is 0
    (2, 7.0, 3.5, 1.0, 1.0, 1.0),                  # S / Tr == 2 exactly: not above
    (300, 90.0, 30.0, 1.0, 1.0, 1.0),              # S / Tr > 2, eff halved, jt raised to jtol, then S > jt Tr: eff * 0.7
    (300, 90.0, 30.0, 1.0, 1.0, 0.04),             # the same with eff <= 0.05: neither factor
    (300, 90.0, 30.0, 1.0, 1.0, 0.08),             # halved to 0.04, then not reduced again
    (1000000, 90.0, 30.0, 0.1, 3.0, 1.0),          # S / Tr > 2 with jt already above jtol
    (300, 10.0, 30.0, 1.0, 1.0, 1.0),              # S <= jt Tr, speed < 1000: eff * 1.3; the rise below the cap
    (300, 10.0, 30.0, 1.0, 1500.0, 1.0),           # speed >= 1000: eff unchanged; the target below the speed
    (100, 5000.0, 1.0e6, 1.0, 1.0, 1.0),           # opt Tr / n^2 above 10: the cap of 10
    (100, 200.0, 1.0e4, 1.0, 1.0, 1.0),            # b between sqrt(opt) and 10
    (300, 31.0, 30.0, 0.5, 40.0, 0.06),            # jtol != 1; S > jt Tr with eff just above 0.05
    (50000, 1.0e7, 2.0e7, 1.0, 0.001, 1.0),        # a tiny speed: capped rise
    (7, 1e-300, 1e-300, 1.0, 1.0, 1.0),            # tiny sums
    (1, 3.0, 4.0, 0.0, 1.0, 1.0),                  # jitter_tolerance = 0
]


def speed_kat():
    rows = []
    seen = set()
    for n, S, Tr, jtol, speed, eff in SPEED_INPUTS:
        s1, e1 = speed_exact(n, S, Tr, jtol, speed, eff)
        s2, e2, taken = ref.speed_rule(n, S, Tr, jtol, speed, eff)
        assert (float(s2), float(e2)) == (s1, e1), (n, S, Tr, jtol, speed, eff, s1, float(s2), e1, float(e2))
        seen.add(taken)
        rows.append({"n": n, "S": S, "Tr": Tr, "jitter_tolerance": jtol, "speed": speed, "eff": eff, "speed_out": s1, "eff_out": e1,
                     "speed_out_hex": s1.hex(), "eff_out_hex": e1.hex()})
    # every branch of the rule, both ways
    for pos in range(3):
        assert {t[pos] for t in seen} == {True, False}, pos
    return rows


def quality():
    g = {"n": N, "dim": DIM, "k": K, "data_seed": DATA_SEED, "theta": 1.2, "n_iter": 500}
    W, labels, _, _ = ref.quality_graph(g)
    runs = []
    for seed in SEEDS:
        Y, info, _ = ref.layout(W, ref.random_start(N, seed))
        runs.append({"seed": seed, "purity": ref.purity(Y, labels), "speed": float(info["speed"]), "side": float(info["side"])})
        print(runs[-1], flush=True)
    g.update(runs=runs, nnz=int(W[0][-1]), purity_range=[min(r["purity"] for r in runs), max(r["purity"] for r in runs)])
    try:
        import networkx as nx
        import scipy.sparse as sp
        G = nx.from_scipy_sparse_array(sp.csr_matrix((W[2], W[1].astype(np.int64), W[0].astype(np.int64)), shape=(N, N)))
        pos = nx.forceatlas2_layout(G, max_iter=500, scaling_ratio=2.0, gravity=1.0, jitter_tolerance=1.0, weight="weight", seed=0)
        g["networkx_purity"] = ref.purity(np.array([pos[i] for i in range(N)]), labels)
        g["networkx_version"] = nx.__version__
        print("networkx %s forceatlas2_layout: purity %.4f" % (nx.__version__, g["networkx_purity"]))
    except ImportError:
        g["networkx_purity"] = None
    return g


if __name__ == "__main__":
    kat = {"pair": pair_kat(), "triangle": triangle_kat(), "speed": speed_kat(), "quality": quality()}
    with open(os.path.join(HERE, "draw_graph_kat.json"), "w") as f:
        json.dump(kat, f, indent=1)
        f.write("\n")

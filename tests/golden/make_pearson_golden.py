"""Writes kat_pearson.json: hand-checkable known answers of the Pearson-residual definition (include/srx.h), computed with
``decimal`` at 50 digits, independent of numpy.

The first matrix is X = [[1, 0], [0, 1]]: mu = 0.5 everywhere, so with theta = 100 every |z| = 0.5 / sqrt(0.5 + 0.0025) and
v = z^2 = 100 / 201 for both genes; with theta = inf, v = 0.5.  The generator asserts both.

    python tests/golden/make_pearson_golden.py
"""
import json
import math
import os
from decimal import Decimal, getcontext

getcontext().prec = 50

CASES = [
    {"name": "identity_theta100", "X": [[1, 0], [0, 1]], "theta": 100, "clip": None},
    {"name": "identity_poisson", "X": [[1, 0], [0, 1]], "theta": "inf", "clip": None},
    {"name": "small_default", "X": [[3, 0, 1, 0], [0, 2, 0, 0], [7, 1, 0, 0], [0, 0, 0, 0], [1, 1, 25, 0]], "theta": 100, "clip": None},
    {"name": "small_clip1_theta10", "X": [[3, 0, 1, 0], [0, 2, 0, 0], [7, 1, 0, 0], [0, 0, 0, 0], [1, 1, 25, 0]], "theta": 10, "clip": 1},
    {"name": "small_noclip_poisson", "X": [[3, 0, 1, 0], [0, 2, 0, 0], [7, 1, 0, 0], [0, 0, 0, 0], [1, 1, 25, 0]], "theta": "inf", "clip": "inf"},
]


def solve(X, theta, clip):
    n, G = len(X), len(X[0])
    r = [sum(Decimal(x) for x in row) for row in X]
    g = [sum(Decimal(X[i][j]) for i in range(n)) for j in range(G)]
    T = sum(r)
    # the default clip is an f64 option value, sqrt(n) rounded to f64: the definition clips at THAT number
    c = Decimal(math.sqrt(n)) if clip is None else (None if clip == "inf" else Decimal(clip))
    z = [[Decimal(0)] * G for _ in range(n)]
    for i in range(n):
        for j in range(G):
            mu = r[i] * g[j] / T if T else Decimal(0)
            if mu == 0:
                continue
            s = mu.sqrt() if theta == "inf" else (mu + mu * mu / Decimal(theta)).sqrt()
            v = (Decimal(X[i][j]) - mu) / s
            if c is not None:
                v = min(max(v, -c), c)
            z[i][j] = v
    var = [sum(z[i][j] * z[i][j] for i in range(n)) / n - (sum(z[i][j] for i in range(n)) / n) ** 2 for j in range(G)]
    return z, var


def main():
    out = []
    for case in CASES:
        z, var = solve(case["X"], case["theta"], case["clip"])
        out.append(dict(case, z=[[format(v, ".40e") for v in row] for row in z], v=[format(v, ".40e") for v in var]))
    ident = {c["name"]: c for c in out}
    assert all(abs(Decimal(v) - Decimal(100) / Decimal(201)) < Decimal("1e-38") for v in ident["identity_theta100"]["v"])
    assert all(abs(Decimal(v) - Decimal("0.5")) < Decimal("1e-38") for v in ident["identity_poisson"]["v"])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat_pearson.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()

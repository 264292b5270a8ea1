#!/usr/bin/env python3
"""Writes kat_regress.json: the regression / scale / clip definition of include/srx.h (srx_regress_*) evaluated in 60-digit
`decimal` arithmetic on a 5 x 3 block with one covariate, nothing shared with numpy.  tests/test_regress_cpu.py holds the numpy
restatement (tests/regress_ref.py) against these numbers.

    python tests/golden/make_regress_golden.py
"""
import decimal
import json
import os

D = decimal.Decimal
X = [["0.5", "0", "2.25"], ["0", "1.5", "2.25"], ["1.75", "0", "2.25"], ["0.25", "0.125", "2.25"], ["0", "3", "2.25"]]     # gene 2 is constant
COV = ["1200", "800", "2100", "950", "1600"]
MAX_VALUE = "1.25"


def evaluate():
    with decimal.localcontext() as c:
        c.prec = 60
        x = [[D(v) for v in row] for row in X]
        cov = [D(v) for v in COV]
        n, k = len(x), len(x[0])
        cbar = sum(cov) / n
        ct = [v - cbar for v in cov]
        A = sum(v * v for v in ct)
        out = {"cbar": str(cbar), "A": str(A), "xbar": [], "W": [], "beta": [], "r": [[None] * k for _ in range(n)], "s": [],
               "z": [[None] * k for _ in range(n)]}
        for j in range(k):
            col = [x[i][j] for i in range(n)]
            xbar = sum(col) / n
            W = sum(ct[i] * col[i] for i in range(n))
            beta = W / A
            const = all(v == col[0] for v in col)
            r = [D(0) if const else (col[i] - xbar) - ct[i] * beta for i in range(n)]
            v = sum(e * e for e in r) / (n - 1)
            s = D(1) if v == 0 else v.sqrt()
            mv = D(MAX_VALUE)
            z = [min(max(e / s, -mv), mv) for e in r]
            out["xbar"].append(str(xbar))
            out["W"].append(str(W))
            out["beta"].append(str(beta))
            out["s"].append(str(s))
            for i in range(n):
                out["r"][i][j] = str(r[i])
                out["z"][i][j] = str(z[i])
        return out


if __name__ == "__main__":
    doc = {"x": X, "cov": COV, "max_value": MAX_VALUE, "digits": 60, "expected": evaluate()}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat_regress.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", path)

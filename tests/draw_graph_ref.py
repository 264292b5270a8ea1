"""Host restatement of the ForceAtlas2 definition of include/srx.h in numpy, written from the header text and independent
of the device code: the masses, the pyramid with Python-integer cell sums, the walk (as a frontier of (point, cell) pairs,
level by level) with its four counters, gravity, attraction, the speed rule, the iteration and the hashed start.  Every
DECISION of the walk is taken in f64 (the cell of a point, the accept test, e2 > 0); ``dtype=np.longdouble`` widens only the
arithmetic of the terms, their sums and the updates, so that D = max |f64 - longdouble| measures rounding and not flipped
decisions.  The speed rule branches on the values of its own dtype and reports the branches it took: the tests compare them
between the two evaluations (tests/test_draw_graph_cpu.py)."""
import json
import os

import numpy as np

from tsne_ref import auto_levels, clumps, host_knn, mix_int, purity  # noqa: F401  (the pyramid's default L and the fixtures are t-SNE's)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = 0x9E3779B97F4A7C15
COUNTERS = ("cells_accepted", "cells_exact", "pairs_exact", "pairs_coincident")


def golden():
    return json.load(open(os.path.join(GOLD, "draw_graph_kat.json")))


# ---- starts ------------------------------------------------------------------------------------------------------------------------
def random_start(n, seed):
    c = np.array([(mix_int(seed + G * (c + 1)) >> 11) * 2.0 ** -53 for c in range(2 * n)], dtype=np.float64)
    return c.reshape(n, 2)


# ---- masses and the pyramid ----------------------------------------------------------------------------------------------------------
def masses(indptr):
    return 1 + np.diff(np.asarray(indptr).astype(np.int64))


def _spread(v):
    out = np.zeros_like(v)
    for b in range(16):
        out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(2 * b)
    return out


def pyramid(Y, m, L):
    """lo, side, U (n x 2 uint64), and per level l = 1..L: the sorted codes of the cells that hold a point, their mass M (f64
    of a Python integer) and com (f64, from Python-integer sums)."""
    Y = np.asarray(Y, dtype=np.float64)
    lo = Y.min(axis=0)
    ext = np.float64((Y.max(axis=0) - lo).max())
    side = ext * (1.0 + 2.0 ** -20) if ext != 0.0 else np.float64(1.0)
    U = np.minimum(np.floor(((Y - lo) / side) * 2.0 ** 32), 2.0 ** 32 - 1).astype(np.uint64)
    levels = {}
    for l in range(1, L + 1):
        cx, cy = U[:, 0] >> np.uint64(32 - l), U[:, 1] >> np.uint64(32 - l)
        code = _spread(cx) | (_spread(cy) << np.uint64(1))
        codes, inv = np.unique(code, return_inverse=True)
        M, SX, SY = [0] * codes.size, [0] * codes.size, [0] * codes.size
        for i, c in enumerate(inv):
            M[c] += int(m[i])
            SX[c] += int(m[i]) * int(U[i, 0])
            SY[c] += int(m[i]) * int(U[i, 1])
        assert max(SX + SY) < 2 ** 64
        mf = np.array([float(v) for v in M])
        unit = side * 2.0 ** -32
        com = np.stack([lo[0] + (np.array([float(v) for v in SX]) / mf) * unit,
                        lo[1] + (np.array([float(v) for v in SY]) / mf) * unit], axis=1)
        levels[l] = {"codes": codes, "M": mf, "com": com, "code_of": code}
    return lo, side, U, levels


# ---- the three forces ------------------------------------------------------------------------------------------------------------------
def repulsion(Y, m, theta, L, kr=2.0, dtype=np.float64):
    """rep (n x 2) and the info (the four counters, levels, side, lo) at Y (positions in `dtype`; the decisions use their f64
    values)."""
    Yt = np.asarray(Y, dtype=dtype)
    Y64 = Yt.astype(np.float64)
    n = Y64.shape[0]
    mt = np.asarray(m).astype(dtype)
    lo, side, U, lev = pyramid(Y64, m, L)
    theta2 = np.float64(theta) * np.float64(theta)
    krt = dtype(kr)
    rep = np.zeros((n, 2), dtype=dtype)
    ctr = dict.fromkeys(COUNTERS, 0)
    fin = lev[L]
    order = np.argsort(fin["code_of"], kind="stable")                 # the members of the finest cells in ascending index
    first = np.searchsorted(fin["code_of"][order], fin["codes"], side="left")
    last = np.searchsorted(fin["code_of"][order], fin["codes"], side="right")
    pi = np.repeat(np.arange(n), 4)
    code = np.tile(np.arange(4, dtype=np.uint64), n)
    for l in range(1, L + 1):
        cell = lev[l]
        at = np.minimum(np.searchsorted(cell["codes"], code), cell["codes"].size - 1)
        full = cell["codes"][at] == code                                # a cell without points is skipped
        pi, code, at = pi[full], code[full], at[full]
        d64 = Y64[pi] - cell["com"][at]
        d2_64 = d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1]
        sl = side * 2.0 ** -l
        acc = sl * sl < theta2 * d2_64
        a = np.flatnonzero(acc)
        ctr["cells_accepted"] += int(a.size)
        d = Yt[pi[a]] - cell["com"][at[a]].astype(dtype)
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        f = (krt * (mt[pi[a]] * cell["M"][at[a]].astype(dtype))) / d2
        np.add.at(rep, pi[a], f[:, None] * d)
        rest = np.flatnonzero(~acc)
        if l == L:
            ctr["cells_exact"] += int(rest.size)
            cnt = (last - first)[at[rest]]
            pp = np.repeat(pi[rest], cnt)
            start = np.repeat(first[at[rest]], cnt)
            within = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            jj = order[start + within]
            ok = jj != pp
            pp, jj = pp[ok], jj[ok]
            ctr["pairs_exact"] += int(pp.size)
            e64 = Y64[pp] - Y64[jj]
            pos = (e64[:, 0] * e64[:, 0] + e64[:, 1] * e64[:, 1]) > 0.0
            ctr["pairs_coincident"] += int((~pos).sum())
            pp, jj = pp[pos], jj[pos]
            e = Yt[pp] - Yt[jj]
            e2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
            f = (krt * (mt[pp] * mt[jj])) / e2
            np.add.at(rep, pp, f[:, None] * e)
        else:
            pi = np.repeat(pi[rest], 4)
            code = (np.repeat(code[rest], 4) << np.uint64(2)) + np.tile(np.arange(4, dtype=np.uint64), rest.size)
    return rep, dict(ctr, levels=L, side=float(side), lo=(float(lo[0]), float(lo[1])))


def gravity(Y, m, g=1.0, strong=False, dtype=np.float64):
    Yt = np.asarray(Y, dtype=dtype)
    mt = np.asarray(m).astype(dtype)
    r = np.sqrt(Yt[:, 0] * Yt[:, 0] + Yt[:, 1] * Yt[:, 1])
    gm = dtype(g) * mt
    with np.errstate(divide="ignore", invalid="ignore"):
        c = gm if strong else gm / r
        out = -(c[:, None] * Yt)
    out[r == 0] = 0
    return out


def attraction(W, Y, linlog=False, dtype=np.float64):
    indptr, indices, data = W
    Yt = np.asarray(Y, dtype=dtype)
    n = Yt.shape[0]
    rows = np.repeat(np.arange(n), np.diff(np.asarray(indptr).astype(np.int64)))
    e = Yt[rows] - Yt[np.asarray(indices).astype(np.int64)]
    f = np.asarray(data).astype(dtype)
    if linlog:
        d = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(d > 0, f * (np.log1p(d) / d), dtype(0))
    attr = np.zeros((n, 2), dtype=dtype)
    np.add.at(attr, rows, f[:, None] * e)
    return -attr


def forces(W, Y, theta=1.2, levels=0, kr=2.0, g=1.0, strong=False, linlog=False, dtype=np.float64):
    """(rep, grav, attr, m, info)."""
    m = masses(W[0])
    L = levels or auto_levels(len(m))
    rep, info = repulsion(Y, m, theta, L, kr, dtype)
    info["total_mass"] = int(m.sum())
    return rep, gravity(Y, m, g, strong, dtype), attraction(W, Y, linlog, dtype), m, info


# ---- the speed rule ------------------------------------------------------------------------------------------------------------------
def speed_rule(n, S, Tr, jtol, speed, eff, dtype=np.float64):
    """(speed, eff, the branches taken) in the order of operations of the header; the constants are the f64 ones."""
    t = dtype
    S, Tr, jtol, speed, eff = t(S), t(Tr), t(jtol), t(speed), t(eff)
    nn = t(n)
    taken = []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        opt = t(0.05) * np.sqrt(nn)
        a = np.sqrt(opt)
        b = (opt * Tr) / (nn * nn)
        taken.append(bool(b < t(10.0)))
        b = b if b < t(10.0) else t(10.0)
        taken.append(bool(a > b))
        jt = jtol * (a if a > b else b)
        big = bool(Tr > 0 and S / Tr > t(2.0))
        taken.append(big)
        if big:
            taken.append(bool(eff > t(0.05)))
            if eff > t(0.05):
                eff = eff * t(0.5)
            taken.append(bool(jt > jtol))
            jt = jt if jt > jtol else jtol
        taken.append(bool(S == 0))
        target = t(np.inf) if S == 0 else ((jt * eff) * Tr) / S
        over = bool(S > jt * Tr)
        taken.append(over)
        if over:
            taken.append(bool(eff > t(0.05)))
            if eff > t(0.05):
                eff = eff * t(0.7)
        else:
            taken.append(bool(speed < t(1000.0)))
            if speed < t(1000.0):
                eff = eff * t(1.3)
        rise, cap = target - speed, t(0.5) * speed
        taken.append(bool(rise < cap))
        speed = speed + (rise if rise < cap else cap)
    return speed, eff, tuple(taken)


# ---- the iteration ---------------------------------------------------------------------------------------------------------------------
def layout(W, Y0, n_iter=500, theta=1.2, levels=0, kr=2.0, g=1.0, jtol=1.0, strong=False, linlog=False, stop_after=0,
           dtype=np.float64, keep=()):
    """Iterations 1 .. (stop_after or n_iter).  Returns (Y, info, trace): info as srx_fa2_info; trace[t] = {"Y", "F", the
    counters, "branches"} for t in keep, and trace["branches"] / trace["counters"] the lists over all iterations."""
    Y = np.array(Y0, dtype=dtype)
    n = Y.shape[0]
    m = masses(W[0])
    mt = m.astype(dtype)
    L = levels or auto_levels(n)
    Fprev = np.zeros((n, 2), dtype=dtype)
    speed, eff = dtype(1.0), dtype(1.0)
    run = stop_after or n_iter
    trace = {"branches": [], "counters": []}
    info = {"n": n, "nnz": int(np.asarray(W[0])[-1]), "total_mass": int(m.sum()), "n_iter": n_iter, "iters_run": run, "levels": L,
            "speed": 1.0, "speed_efficiency": 1.0, "swing": 0.0, "traction": 0.0, "side": 0.0}
    info.update(dict.fromkeys(COUNTERS, 0))
    for t in range(1, run + 1):
        rep, ri = repulsion(Y, m, theta, L, kr, dtype)
        F = (rep + gravity(Y, m, g, strong, dtype)) + attraction(W, Y, linlog, dtype)
        dm, dp = Fprev - F, Fprev + F
        swing = np.sqrt(dm[:, 0] * dm[:, 0] + dm[:, 1] * dm[:, 1])
        tract = dtype(0.5) * np.sqrt(dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1])
        S, Tr = (mt * swing).sum(), (mt * tract).sum()
        speed, eff, taken = speed_rule(n, S, Tr, jtol, speed, eff, dtype)
        factor = speed / (dtype(1.0) + np.sqrt(speed * (mt * swing)))
        Y = Y + F * factor[:, None]
        Fprev = F
        trace["branches"].append(taken)
        trace["counters"].append(tuple(ri[c] for c in COUNTERS))
        if t in keep:
            trace[t] = {"Y": Y.copy(), "F": F.copy()}
        info.update({c: ri[c] for c in COUNTERS})
        info.update(speed=speed, speed_efficiency=eff, swing=S, traction=Tr, side=ri["side"])
    return Y, info, trace


# ---- fixtures: graphs and the named inputs of the GPU tests (checked on the CPU by test_draw_graph_cpu.py) ---------------------------------
def csr_of(A):
    """(indptr uint64, indices uint32, data f64) of a dense symmetric matrix, zeros dropped."""
    A = np.asarray(A, dtype=np.float64)
    keep = A != 0.0
    indptr = np.zeros(A.shape[0] + 1, dtype=np.uint64)
    indptr[1:] = np.cumsum(keep.sum(axis=1))
    ii, jj = np.nonzero(keep)
    return indptr, jj.astype(np.uint32), A[ii, jj]


def knn_graph(n, k=5, seed=0):
    """A symmetric weighted k-NN graph of n generic points in 3 dimensions: W = max(A, A^T), A_ij = 1 / (1 + d_ij)."""
    if n == 1:
        return csr_of(np.zeros((1, 1)))
    k = min(k, n - 1)
    idx, dist = host_knn(np.random.default_rng(1000 + seed + n).standard_normal((n, 3)), k)
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), k), idx.ravel().astype(np.int64)] = (1.0 / (1.0 + dist)).ravel()
    return csr_of(np.maximum(A, A.T))


def star_graph(leaves):
    A = np.zeros((leaves + 1, leaves + 1))
    A[0, 1:] = A[1:, 0] = 0.5 + np.arange(leaves) / (2.0 * leaves)
    return csr_of(A)


def generic_layout(n, seed=17):
    return np.random.default_rng(seed).standard_normal((n, 2))


EDGE_LAYOUTS = ("coincident", "two_coincident", "origin", "line", "cell63", "cell64", "cell65", "cell600", "two_clumps", "isolated",
                "star300")


def edge_case(name):
    """(W, Y, levels) of a named edge layout.  cellNN: one finest cell (levels = 3: the cell is side / 8 wide) holding NN points
    beside five outliers.  two_clumps: 64 points, the even ones in one clump and the odd ones in a far one, so that with
    levels = 1 one wave holds both and every other level splits them.  isolated: a third of the vertices have no edge."""
    rng = np.random.default_rng(23)
    if name == "coincident":
        n = 130
        return knn_graph(n), np.tile(np.array([[0.25, -1.5]]), (n, 1)), 0
    if name == "two_coincident":
        Y = generic_layout(200)
        Y[150] = Y[20]
        return knn_graph(200), Y, 0
    if name == "origin":
        Y = generic_layout(200)
        Y[77] = 0.0
        return knn_graph(200), Y, 0
    if name == "line":
        Y = generic_layout(200)
        Y[:, 1] = -0.75
        return knn_graph(200), Y, 0
    if name.startswith("cell"):
        m = int(name[4:])
        out = np.array([[0.0, 0.0], [8.0, 8.0], [8.0, 0.0], [0.0, 8.0], [5.0, 3.0]])
        Y = np.concatenate([out, 2.1 + 0.8 * rng.random((m, 2))])                # inside the cell [2, 3) x [2, 3) of level 3
        return knn_graph(m + 5), Y, 3
    if name == "two_clumps":
        Y = 0.01 * rng.standard_normal((64, 2))
        Y[1::2] += 100.0
        return knn_graph(64), Y, 4
    if name == "isolated":
        n = 150
        W = knn_graph(100)
        indptr = np.concatenate([W[0], np.full(n - 100, W[0][-1], dtype=np.uint64)])
        return (indptr, W[1], W[2]), generic_layout(n), 0
    assert name == "star300", name
    return star_graph(300), generic_layout(301), 0


POSITION_CASES = ("n1", "n2", "n300_given", "n300_random")
FLAGS = {"strong": True, "linlog": True}


def position_case(name):
    """(W, Y0 or None for the hashed start, seed, the compared runs as (iterations, flags)).  At n = 1 the linear gravity has
    the same magnitude wherever the point is, so from iteration 2 on swing is zero up to rounding and S == 0 is a decision
    that rounding takes: three iterations are compared with strong gravity alone, where the force follows the point."""
    runs = ((1, {}), (3, {}), (3, FLAGS))
    if name == "n1":
        return knn_graph(1), np.array([[0.75, -0.5]]), 0, ((1, {}), (3, {"strong": True}))
    if name == "n2":
        return csr_of(np.array([[0.0, 0.7], [0.7, 0.0]])), np.array([[0.25, 0.5], [-1.0, 0.125]]), 0, runs
    if name == "n300_given":
        return knn_graph(300), 10.0 * generic_layout(300, 5), 0, runs
    assert name == "n300_random", name
    return knn_graph(300), None, 4242, runs


def quality_graph(g):
    """The quality input of the golden file: (C as a CSR triple, labels, idx, dist) of the t-SNE quality points' k-NN list."""
    import graph_ref
    x, labels = clumps(g["n"], g["dim"], seed=g["data_seed"])
    idx, dist = host_knn(x, g["k"])
    C = graph_ref.graph(idx, dist)[1]
    return (C.indptr.astype(np.uint64), C.indices.astype(np.uint32), C.data.astype(np.float64)), labels, idx, dist

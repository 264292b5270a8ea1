"""CPU tests of the ForceAtlas2 definition (include/srx.h) as tests/draw_graph_ref.py restates it, and of the one entry point
that needs no GPU, srx_fa2_speed.

  the reference against the known answers of tests/golden/draw_graph_kat.json (decimal / fractions, make_draw_graph_golden.py);
  the reference's forces at theta = 0 against the dense expressions -(diff * A), kr m m^T / d^2 and -g m y / |y|, written out
  here without any pyramid;
  srx_fa2_speed through the library against the table and the reference, bit for bit;
  for every named input of tests/test_draw_graph_gpu.py: the f64 and the long-double reference take the same speed-rule
  branches and give the same walk counters in every compared iteration: the condition the device's position tests rest on.

Tolerance against the known answers: they are exact values rounded once, the reference rounds every operation; a force
component here is the result of fewer than 40 operations on terms of one sign pattern without cancellation below 1e-2 of
the terms, so 40 * 2^-53 / 1e-2 < 1e-12 relative to the largest component of the case."""
import ctypes as C

import numpy as np
import pytest

import draw_graph_ref as ref

KAT_RTOL = 1e-12


def close(got, want, scale=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    s = np.abs(want).max() if scale is None else scale
    return float(np.abs(got - want).max()) <= KAT_RTOL * s


def dense_of(W, n):
    A = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(W[0].astype(np.int64)))
    A[rows, W[1]] = W[2]
    return A


# ---- the known answers ------------------------------------------------------------------------------------------------------------------
def test_pair_known_answer():
    k = ref.golden()["pair"]
    W = ref.csr_of(np.array([[0.0, k["w"]], [k["w"], 0.0]]))
    Y = np.array(k["y"])
    rep, grav, attr, m, info = ref.forces(W, Y, theta=0.0, kr=k["scaling_ratio"], g=k["gravity"])
    assert m.tolist() == k["mass"] and info["total_mass"] == 4 and info["pairs_exact"] == 2 and info["cells_accepted"] == 0
    assert close(rep, k["rep"]) and close(grav, k["grav"]) and close(attr, k["attr"])
    Y1, li, tr = ref.layout(W, Y, n_iter=1, theta=0.0, kr=k["scaling_ratio"], g=k["gravity"], jtol=k["jitter_tolerance"], keep=(1,))
    assert close(tr[1]["F"], k["F"]) and close(Y1, k["y1"])
    for key in ("swing", "traction", "speed", "speed_efficiency"):
        assert abs(float(li[key]) - k[key]) <= KAT_RTOL * abs(k[key]), key
    assert li["traction"] * 2.0 == li["swing"]                       # Fprev = 0: S / Tr is exactly 2, not above it


def test_triangle_known_answer():
    k = ref.golden()["triangle"]
    W = ref.csr_of(np.array(k["w"]))
    Y = np.array(k["y"])
    rep, grav, attr, m, _ = ref.forces(W, Y, theta=0.0, kr=k["scaling_ratio"], g=k["gravity"])
    _, grav_s, attr_l, _, _ = ref.forces(W, Y, theta=0.0, kr=k["scaling_ratio"], g=k["gravity"], strong=True, linlog=True)
    assert m.tolist() == k["mass"]
    for got, key in ((rep, "rep"), (grav, "grav"), (attr, "attr"), (grav_s, "grav_strong"), (attr_l, "attr_linlog")):
        assert close(got, k[key]), key


def test_speed_table_reference():
    for row in ref.golden()["speed"]:
        s, e, _ = ref.speed_rule(row["n"], row["S"], row["Tr"], row["jitter_tolerance"], row["speed"], row["eff"])
        assert float(s).hex() == row["speed_out_hex"] and float(e).hex() == row["eff_out_hex"], row
        assert float(s) == row["speed_out"] and float(e) == row["eff_out"]


def test_fa2_speed_library_bit_for_bit():
    """srx_fa2_speed needs no GPU: the same statement the device's one thread runs, compiled for the host."""
    from singlerust_amd import _ffi as F
    from singlerust_amd.memory.processing import fa2_speed
    rows = ref.golden()["speed"]
    assert len(rows) >= 12
    for row in rows:
        s, e = fa2_speed(row["n"], row["S"], row["Tr"], row["jitter_tolerance"], row["speed"], row["eff"])
        assert s.hex() == row["speed_out_hex"] and e.hex() == row["eff_out_hex"], (row, s, e)
    # a chain of calls against the reference: the state is carried from call to call
    rng = np.random.default_rng(3)
    s, e = 1.0, 1.0
    rs, re = np.float64(1.0), np.float64(1.0)
    for _ in range(200):
        n = int(rng.integers(1, 10 ** 6))
        Tr = float(rng.random() * 10.0 ** rng.integers(-3, 6))
        S = float(Tr * rng.random() * 4.0)
        s, e = fa2_speed(n, S, Tr, 1.0, s, e)
        rs, re, _ = ref.speed_rule(n, S, Tr, 1.0, rs, re)
        assert (s.hex(), e.hex()) == (float(rs).hex(), float(re).hex())
    # the refusals
    lib = F.lib()
    sp, ef = C.c_double(1.0), C.c_double(1.0)
    for args in ((0, 1.0, 1.0, 1.0), (5, -1.0, 1.0, 1.0), (5, np.nan, 1.0, 1.0), (5, 1.0, np.inf, 1.0), (5, 1.0, 1.0, -0.5),
                 (5, 1.0, 1.0, np.nan)):
        assert lib.srx_fa2_speed(*args, C.byref(sp), C.byref(ef)) == F.E_ARG and (sp.value, ef.value) == (1.0, 1.0), args
    assert lib.srx_fa2_speed(5, 1.0, 1.0, 1.0, None, C.byref(ef)) == F.E_ARG
    bad = C.c_double(np.nan)
    assert lib.srx_fa2_speed(5, 1.0, 1.0, 1.0, C.byref(bad), C.byref(ef)) == F.E_ARG


# ---- the forces against the dense expressions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 65, 300])
def test_forces_against_dense_expressions(n):
    W = ref.knn_graph(n)
    Y = ref.generic_layout(n)
    kr, g = 2.0, 1.5
    rep, grav, attr, m, info = ref.forces(W, Y, theta=0.0, levels=2, kr=kr, g=g)
    assert info["pairs_exact"] == n * (n - 1) and info["cells_accepted"] == 0 and info["pairs_coincident"] == 0
    A = dense_of(W, n)
    mf = m.astype(np.float64)
    assert m.tolist() == (1 + (A != 0).sum(axis=1)).tolist()
    diff = Y[:, None, :] - Y[None, :, :]
    d2 = (diff ** 2).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    want_attr = -(diff * A[:, :, None]).sum(axis=1)
    want_rep = (diff * (kr * np.outer(mf, mf) / d2)[:, :, None]).sum(axis=1)
    want_grav = -g * mf[:, None] * Y / np.linalg.norm(Y, axis=1)[:, None]
    # the dense sums add n terms in another order: n * 2^-53 of the sum of the terms' magnitudes
    scale_rep = (np.abs(diff) * (kr * np.outer(mf, mf) / d2)[:, :, None]).sum(axis=1).max()
    assert np.abs(rep - want_rep).max() <= 4 * n * 2.0 ** -53 * scale_rep
    assert np.abs(attr - want_attr).max() <= 4 * 64 * 2.0 ** -53 * np.abs(want_attr).max()
    assert np.abs(grav - want_grav).max() <= 8 * 2.0 ** -53 * np.abs(want_grav).max()
    # both flags
    _, grav_s, attr_l, _, _ = ref.forces(W, Y, theta=0.0, levels=2, kr=kr, g=g, strong=True, linlog=True)
    d = np.sqrt(np.where(np.isinf(d2), 1.0, d2))
    want_l = -(diff * (A * np.log1p(d) / d)[:, :, None]).sum(axis=1)
    assert np.abs(attr_l - want_l).max() <= 4 * 64 * 2.0 ** -53 * np.abs(want_l).max()
    assert np.abs(grav_s - (-g * mf[:, None] * Y)).max() <= 8 * 2.0 ** -53 * np.abs(grav_s).max()


def test_theta_walk_agrees_with_the_exact_sum():
    """Barnes-Hut at theta = 0.5 is an approximation of the exact sum, and a huge theta accepts every cell that is not at a
    point: both evaluate through the same code as theta = 0, so this guards the frontier bookkeeping of the reference."""
    n = 300
    W, Y = ref.knn_graph(n), ref.generic_layout(n)
    m = ref.masses(W[0])
    exact, _ = ref.repulsion(Y, m, 0.0, 4)
    near, info = ref.repulsion(Y, m, 0.5, 4)
    assert info["cells_accepted"] > 0 and info["pairs_exact"] < n * (n - 1)
    assert np.abs(near - exact).max() <= 0.05 * np.abs(exact).max()
    far, info = ref.repulsion(Y, m, 1e9, 4)
    assert info["cells_accepted"] >= 3 * n and info["pairs_exact"] <= n


# ---- the condition the device's position tests rest on ------------------------------------------------------------------------------------
def check_same_decisions(W, Y0, iters, **kw):
    _, i64, t64 = ref.layout(W, Y0, n_iter=iters, **kw)
    _, ild, tld = ref.layout(W, Y0, n_iter=iters, dtype=np.longdouble, **kw)
    assert t64["branches"] == tld["branches"], (t64["branches"], tld["branches"])
    assert t64["counters"] == tld["counters"], (t64["counters"], tld["counters"])


@pytest.mark.parametrize("name", ref.POSITION_CASES)
def test_position_inputs_take_the_same_decisions(name):
    W, Y0, seed, runs = ref.position_case(name)
    if Y0 is None:
        Y0 = ref.random_start(int(W[0].size) - 1, seed)
    for iters, flags in runs:
        check_same_decisions(W, Y0, iters, **flags)


@pytest.mark.parametrize("name", ref.EDGE_LAYOUTS)
def test_edge_inputs_give_the_same_counters(name):
    W, Y, levels = ref.edge_case(name)
    for theta in (0.5, 1.2):
        a = ref.forces(W, Y, theta, levels)[4]
        b = ref.forces(W, Y, theta, levels, dtype=np.longdouble)[4]
        assert a == b
    n = Y.shape[0]
    if name == "coincident":
        assert a["side"] == 1.0 and a["pairs_coincident"] == a["pairs_exact"] == n * (n - 1) and not ref.forces(W, Y)[0].any()
    if name == "two_coincident":
        assert a["pairs_coincident"] == 2
    if name.startswith("cell"):
        code = ref.pyramid(Y, ref.masses(W[0]), levels)[3][levels]["code_of"]
        assert (code[5:] == code[5]).all() and (code[:5] != code[5]).all()
    if name == "isolated":
        m = ref.masses(W[0])
        assert (m[100:] == 1).all() and not ref.forces(W, Y)[2][100:].any()
    if name == "star300":
        assert ref.masses(W[0])[0] == 301


def test_hashed_start_is_in_the_unit_square():
    for n, seed in ((1, 0), (300, 4242), (3, 2 ** 64 - 1)):
        y = ref.random_start(n, seed)
        assert y.shape == (n, 2) and (y >= 0).all() and (y < 1).all()
    assert ref.random_start(2, 7)[1, 0] == (ref.mix_int(7 + ref.G * 3) >> 11) * 2.0 ** -53

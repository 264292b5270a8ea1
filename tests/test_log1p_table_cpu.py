"""The table-driven f64 logarithms of singlerust_amd/csrc/log1p64.hpp, checked on the host (no GPU).

The 128 {inv, lg} entries are parsed out of the header and checked against exact arithmetic.  The straight-line arithmetic
of `log1p_f64_fast` and of `log1p_f64_moment` (= `log1p_f64_lite`) is then RESTATED here, operation by operation: every fma
rounded once (exact products through `fractions.Fraction`), the hardware f32 reciprocal taken as the correctly rounded f32
one.  This checks the ALGORITHM — the table, the constants and the polynomial — against the accuracy the header states, not
the compiled code: a wrong table entry or an edited constant fails here without a GPU; tests/test_log1p_gpu.py checks what the
device computes.
"""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "singlerust_amd", "csrc", "log1p64.hpp")

# the bounds log1p64.hpp states
FAST_REL = 2.7e-16                  # log1p_f64_fast: relative, every x >= 0
MOMENT_ABS, MOMENT_REL = 4e-14, 5e-12   # log1p_f64_moment / _lite for x >= 2^-10 (smaller x take log1p_f64_fast)


def _hexfloat(s):
    return float.fromhex(s)


def _source():
    return open(HDR).read()


def _table():
    body = _source().split("kLog1pTab[128] = {", 1)[1].split("};", 1)[0]
    ent = re.findall(r"\{\s*(0x[0-9a-fA-Fp.+-]+)\s*,\s*(0x[0-9a-fA-Fp.+-]+)\s*\}", body)
    return [(_hexfloat(a), _hexfloat(b)) for a, b in ent]


def _function_body(name):
    src = _source()
    start = src.index(f"double {name}(")
    return src[start:src.index("\n}", start)]


def _constants(name):
    """The hex-float constants of a routine, in source order (the ln 2 pieces)."""
    return [_hexfloat(c) for c in re.findall(r"0x1\.[0-9a-f]+p[+-]\d+", _function_body(name))]


def _poly(name):
    """The fma coefficients of a routine's Horner chain, in source order: `fma(r, A, B)` then `fma(r, p, C)`..."""
    body = _function_body(name)
    first = re.search(r"p = __builtin_fma\(r, (-?1\.0 / \d+|-?0\.5), (-?1\.0 / \d+|-?0\.5)\)", body)
    rest = re.findall(r"p = __builtin_fma\(r, p, (-?1\.0 / \d+|-?0\.5)\)", body)
    ev = lambda s: float(eval(s))      # the literals are C doubles: "1.0 / 7" is fl(1/7) as in Python
    return [ev(first.group(1)), ev(first.group(2))] + [ev(s) for s in rest]


TAB = _table()


def fma(a, b, c):
    """a * b + c rounded once (Fraction -> float is correctly rounded)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _split(x):
    u = 1.0 + x
    b = int(np.float64(u).view(np.uint64))
    e = (b >> 52) - 1023
    i = (b >> 45) & 127
    m = float(np.uint64((b & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000).view(np.float64))
    return u, e, i, m


def _horner(r, coef):
    p = fma(r, coef[0], coef[1])
    for c in coef[2:]:
        p = fma(r, p, c)
    return fma(r * r, p, r)


FAST_COEF, FAST_K = _poly("log1p_f64_fast"), _constants("log1p_f64_fast")
MOM_COEF, MOM_K = _poly("log1p_f64_moment"), _constants("log1p_f64_moment")


def emu_fast(x):
    """log1p_f64_fast for 0 <= x < inf."""
    u, e, i, m = _split(x)
    inv, lg = TAB[i]
    r = fma(m, inv, -1.0)
    lr = _horner(r, FAST_COEF)
    rcp = float(np.float32(1.0) / np.float32(u))            # v_rcp_f32 of (float)u
    c = (x - (u - 1.0)) * rcp
    de = float(e)
    y = fma(de, FAST_K[0], lg)
    return y + (lr + fma(de, FAST_K[1], c))


def emu_moment(x):
    """log1p_f64_moment (= log1p_f64_lite) for 0 <= x < inf: x >= 2^-10 the degree-5 chain, else the full routine."""
    if x == 0.0:
        return 0.0
    if not (x >= 2.0 ** -10):
        return emu_fast(x)
    u, e, i, m = _split(x)
    inv, lg = TAB[i]
    r = fma(m, inv, -1.0)
    lr = _horner(r, MOM_COEF)
    return fma(float(e), MOM_K[0], lg) + lr


def _arguments():
    rng = np.random.default_rng(20261015)
    x = list(2.0 ** rng.uniform(-40, 40, 16000))
    # both edges of every table slot, at several binades of 1 + x: u = 2^e (1 + i/128) and the double below it
    for e in (0, 1, 5, 17, 40):
        for i in range(128):
            u = math.ldexp(1.0 + i / 128, e)
            for uu in (u, math.nextafter(u, 0.0), math.nextafter(u, math.inf)):
                if uu - 1.0 > 0:
                    x.append(uu - 1.0)
    x += [2.0 ** -10, math.nextafter(2.0 ** -10, 0), 2.0 ** -53, 2.0 ** -60, 5e-324, 2.2250738585072014e-308, 1.0, 63.0, 64.0]
    return np.array(x, dtype=np.float64)


def _ref(x):
    assert np.finfo(np.longdouble).nmant >= 63
    return np.log1p(x.astype(np.longdouble))


def test_table_entries_are_the_rounded_reciprocals_and_their_logs():
    import mpmath
    assert len(TAB) == 128
    mpmath.mp.prec = 200
    for i, (inv, lg) in enumerate(TAB):
        assert inv == float(Fraction(128, 128 + i)), i                    # fl(1 / (1 + i/128))
        want = -mpmath.log(mpmath.mpf(inv))
        err = abs(mpmath.mpf(lg) - want)
        half_ulp = mpmath.mpf(math.ulp(lg) if lg else 0.0) / 2
        assert err <= half_ulp, (i, float(err))


def test_routine_constants_are_what_the_emulation_reads():
    # ln 2 split in two for the full routine (hi has 20 trailing zero bits: e * hi is exact), one double for the degree-5 one
    assert len(FAST_K) == 2 and len(MOM_K) == 1
    assert (int(np.float64(FAST_K[0]).view(np.uint64)) & 0xFFFFF) == 0
    import mpmath
    mpmath.mp.prec = 200
    assert abs(mpmath.mpf(FAST_K[0]) + mpmath.mpf(FAST_K[1]) - mpmath.log(2)) < mpmath.mpf(2) ** -80
    assert MOM_K[0] == math.log(2)
    assert FAST_COEF == [-1.0 / 8, 1.0 / 7, -1.0 / 6, 1.0 / 5, -1.0 / 4, 1.0 / 3, -0.5]
    assert MOM_COEF == [1.0 / 5, -1.0 / 4, 1.0 / 3, -0.5]


@pytest.fixture(scope="module")
def args_and_ref():
    x = _arguments()
    return x, _ref(x)


def test_log1p_f64_fast_emulated_meets_its_bound(args_and_ref):
    x, want = args_and_ref
    got = np.array([emu_fast(float(v)) for v in x], dtype=np.longdouble)
    rel = np.abs(got - want) / want
    assert float(rel.max()) <= FAST_REL, (float(rel.max()), float(x[int(np.argmax(rel))]))


def test_log1p_f64_moment_emulated_meets_its_bound(args_and_ref):
    x, want = args_and_ref
    got = np.array([emu_moment(float(v)) for v in x], dtype=np.longdouble)
    err = np.abs(got - want)
    big = x >= 2.0 ** -10
    assert float(err[big].max()) <= MOMENT_ABS, float(err[big].max())
    assert float((err[big] / want[big]).max()) <= MOMENT_REL, float((err[big] / want[big]).max())
    assert float((err[~big] / want[~big]).max()) <= FAST_REL          # below 2^-10: the full routine
    # the bound is not loose by orders of magnitude: the dropped r^6/6 term shows near 2^-7 (table slot 1)
    assert float((err[big] / want[big]).max()) > 1e-12


def test_mpmath_spot_checks_agree_with_longdouble():
    import mpmath
    mpmath.mp.prec = 200
    for v in (2.0 ** -40, 0.0078125, 0.3, 1.0, 63.0, 1e4, 2.0 ** 40):
        want = mpmath.log1p(mpmath.mpf(v))
        assert abs(float((mpmath.mpf(emu_fast(v)) - want) / want)) <= FAST_REL
        assert abs(float(mpmath.mpf(float(np.log1p(np.longdouble(v)))) - want)) <= abs(float(want)) * 2.0 ** -52

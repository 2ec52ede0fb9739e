"""auv_sim_amd/csrc/auvp_math.h (host build, through the portable checker library): < 1 ulp vs mpmath,
and last-bit agreement rate with this machine's libm."""
import math

import numpy as np


def _ulp_err(got, want_mp, mp):
    want = float(want_mp)
    u = math.ulp(want) if want != 0 else 5e-324
    return abs(float((mp.mpf(got) - want_mp) / u))


def test_sincos_under_one_ulp(orc):
    import mpmath as mp
    mp.mp.prec = 200
    L = orc.lib("portable")
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.uniform(-70, 70, 3000), rng.uniform(-1e5, 1e5, 500), rng.uniform(-1e-4, 1e-4, 100),
                         np.array([k * math.pi / 2 for k in range(-40, 41)]),
                         np.array([k * math.pi / 4 for k in range(-40, 41)])])
    worst = 0.0
    for x in xs:
        x = float(x)
        worst = max(worst, _ulp_err(L.orc_sin(x), mp.sin(mp.mpf(x)), mp), _ulp_err(L.orc_cos(x), mp.cos(mp.mpf(x)), mp))
    assert worst < 1.0, worst


def test_sincos_mostly_equal_to_libm(orc):
    L = orc.lib("portable")
    rng = np.random.default_rng(1)
    xs = rng.uniform(-60, 60, 20000)
    s = np.array([L.orc_sin(float(x)) for x in xs])
    c = np.array([L.orc_cos(float(x)) for x in xs])
    ds = np.abs(s - np.sin(xs)) / np.spacing(np.abs(np.sin(xs)))
    dc = np.abs(c - np.cos(xs)) / np.spacing(np.abs(np.cos(xs)))
    assert ds.max() <= 1.0 and dc.max() <= 1.0
    # informational bound: the two agree bit-for-bit on the vast majority of inputs
    assert (ds == 0).mean() > 0.9 and (dc == 0).mean() > 0.9


def test_pow_e_half_ulp_and_equal_to_libm(orc):
    """auvp_exp.h pow(math.e, z): the particle-filter weights (particleFilter.py:103-116)"""
    import mpmath as mp
    from oracle import orc_pf
    mp.mp.prec = 200
    rng = np.random.default_rng(2)
    zs = np.concatenate([-rng.uniform(0, 20, 3000) ** 2 / 0.5, -rng.uniform(0, 800, 3000) ** 2 / 20000,
                         -rng.uniform(0, 1e-3, 200), rng.uniform(-740, 700, 500), [0.0, -0.0, -1.0, 1.0, -745.0, -800.0]])
    got = orc_pf.pow_e(zs, kind="portable")
    libm = orc_pf.pow_e(zs, kind="libm")
    E = mp.mpf(math.e)
    worst = 0.0
    for z, g in zip(zs[::7], got[::7]):
        want = mp.power(E, mp.mpf(float(z)))
        if want > mp.mpf(2) ** -1020:
            worst = max(worst, _ulp_err(float(g), want, mp))
    assert worst < 0.52, worst
    assert np.array_equal(libm, np.array([math.e ** float(z) for z in zs]))
    assert (got == libm).mean() > 0.98
    big = np.abs(libm) > 1e-300
    assert (np.abs(got - libm)[big] <= np.spacing(np.abs(libm))[big]).all()


def test_atan2_special_cases_and_accuracy(orc):
    """atan2 of auvp_atan_body.h (regular case behind one test, the rare cases in a side branch): every special operand
    combination like math.atan2 (signed zeros, infinities, nan), <= 1.2 ulp vs mpmath elsewhere"""
    import itertools
    import mpmath as mp
    mp.mp.prec = 200
    L = orc.lib("portable")
    inf, nan = float("inf"), float("nan")
    vals = [0.0, -0.0, 1.0, -1.0, inf, -inf, nan, 1e-300, -1e-300, 1e300, -1e300, 2.5, -3.75, 5e-324]
    for y, x in itertools.product(vals, vals):
        a, b = L.orc_atan2(y, x), math.atan2(y, x)
        if b != b:
            assert a != a, (y, x, a)
        elif x == 0.0 or y == 0.0:  # a zero operand: exactly libm's value and sign (infinite operands go through atan's limits: 1 ulp)
            assert a == b and math.copysign(1.0, a) == math.copysign(1.0, b), (y, x, a, b)
        else:
            assert abs(a - b) <= 2 * math.ulp(b), (y, x, a, b)
    rng = np.random.default_rng(4)
    worst = 0.0
    for y, x in zip(rng.uniform(-300, 300, 3000), rng.uniform(-300, 300, 3000)):
        worst = max(worst, _ulp_err(L.orc_atan2(float(y), float(x)), mp.atan2(mp.mpf(float(y)), mp.mpf(float(x))), mp))
    assert worst <= 1.2, worst


def test_hypot_equals_libm(orc):
    """Borges' fused hypot with the short square root / division: equal to glibc's on every sampled input, zero operands included"""
    L = orc.lib("portable")
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.uniform(-300, 300, 20000), np.zeros(100), rng.uniform(-1e-9, 1e-9, 500), np.zeros(3)])
    ys = np.concatenate([rng.uniform(-300, 300, 20000), rng.uniform(-5, 5, 100), np.zeros(500), np.array([0.0, -0.0, 2.0])])
    got = np.array([L.orc_hypot(float(x), float(y)) for x, y in zip(xs, ys)])
    # (math.hypot is CPython's own vector_norm, not glibc's hypot -- round 6; both it and Borges' form are correctly rounded on
    # these samples, which glibc's is not on ~0.4 % of them)
    assert np.array_equal(got, np.array([math.hypot(float(x), float(y)) for x, y in zip(xs, ys)]))
    # a square that underflows (|x| < ~2^-511) with a zero partner: the correction would be 0 / 0; the operand comes back
    for x in (1e-200, -3e-180, 5e-324):
        assert L.orc_hypot(x, 0.0) == abs(x) and L.orc_hypot(0.0, x) == abs(x)


def test_checker_libm_build_restates_cpythons_hypot(orc):
    """the libm build of the checker stands for "what the reference's interpreter computes": CPython >= 3.10's math.hypot is its
    own algorithm (Modules/mathmodule.c vector_norm), and glibc's hypot differs from it in the last bit on ~0.4 % of arguments --
    the restatement (oracle/orc_math.h orc_cpython_hypot) must agree with THIS interpreter on every sample, glibc's must not"""
    import ctypes
    L = orc.lib("libm")
    rng = np.random.default_rng(11)
    xs = np.concatenate([rng.uniform(-300, 300, 150000), rng.uniform(-300, 300, 50000) * 10.0 ** rng.uniform(-8, 8, 50000), np.array([0.0, -0.0, 3.0, np.inf])])
    ys = np.concatenate([rng.uniform(-300, 300, 150000), rng.uniform(-300, 300, 50000), np.array([0.0, 5.0, -0.0, 1.0])])
    want = np.array([math.hypot(float(x), float(y)) for x, y in zip(xs, ys)])
    got = np.array([L.orc_hypot(float(x), float(y)) for x, y in zip(xs, ys)])
    assert np.array_equal(got, want)
    libm = ctypes.CDLL("libm.so.6")
    libm.hypot.restype = ctypes.c_double
    libm.hypot.argtypes = [ctypes.c_double, ctypes.c_double]
    glibc = np.array([libm.hypot(float(x), float(y)) for x, y in zip(xs[:150000], ys[:150000])])
    n_diff = int((glibc != want[:150000]).sum())
    assert 0 < n_diff < 3000, n_diff   # (measured 0.4 %: were it 0, this interpreter would be calling glibc and the restatement moot)


# ---- the edges of the documented domains (operand families: tests/math_edge_cases.py) -------------------------------------------

def test_sincos_up_to_1e9_and_special_operands(orc):
    """the ~100-bit reduction holds its < 1 ulp up to 1e9 (auvp_sincos_body.h), measured 0.7397 ulp on the 20 000 of 1e6 .. 1e9;
    beyond 1e9 the header promises only determinism, so that family is printed, not asserted (measured 3 488 ulp on the 5 000 of
    1e9 .. 3.5e15: the arguments next to a multiple of pi/2).  sin(-0) is -0; an infinite or NaN argument gives NaN"""
    import mpmath as mp
    import math_edge_cases as M
    L = orc.lib("portable")
    x, blocks = M.sincos()
    worst = {}
    with mp.workprec(300):
        for name, step in (("mid", 1), ("high", 1)):
            w = 0.0
            for v in x[blocks[name]][::step]:
                v = float(v)
                w = max(w, _ulp_err(L.orc_sin(v), mp.sin(mp.mpf(v)), mp), _ulp_err(L.orc_cos(v), mp.cos(mp.mpf(v)), mp))
            worst[name] = w
    print("sin/cos worst error [ulp]: 1e6..1e9 %.4f, 1e9..3.5e15 %.4f (not asserted)" % (worst["mid"], worst["high"]))
    assert worst["mid"] < 1.0, worst
    assert L.orc_sin(-0.0) == 0.0 and math.copysign(1.0, L.orc_sin(-0.0)) == -1.0
    assert L.orc_sin(0.0) == 0.0 and math.copysign(1.0, L.orc_sin(0.0)) == 1.0 and L.orc_cos(-0.0) == 1.0
    for v in (float("inf"), -float("inf"), float("nan")):
        assert math.isnan(L.orc_sin(v)) and math.isnan(L.orc_cos(v)), v
    # |x| < 2^-27 down to the subnormals: sin x is x or its neighbour towards zero, cos x is 1 (or 1 - 2^-53)
    for v in x[blocks["tiny"]]:
        v = float(v)
        assert L.orc_sin(v) in (v, math.nextafter(v, 0.0)) and L.orc_cos(v) in (1.0, math.nextafter(1.0, 0.0)), v


def test_pow_e_subnormal_results_and_special_operands(orc):
    """auvp_exp_hl_t hands a value within 0.51 ulp to ldexp, whose ONE rounding into the subnormals adds at most half a unit of
    2^-1074: below 1.01 units there (measured 0.7500 on the family's 19 562 subnormal results; the normal results of the same sweep
    0.4989 ulp, held to the working range's 0.52).  The special operands give exactly 0, inf, NaN and 1.0"""
    import mpmath as mp
    import math_edge_cases as M
    from oracle import orc_pf
    z, blocks = M.pow_e()
    lo = np.concatenate([z[blocks["low"]], [v for v in z[blocks["thresholds"]] if v < 0]])
    got = orc_pf.pow_e(lo, kind="portable")
    tiny = mp.mpf(2) ** -1022
    worst_sub = worst_norm = 0.0
    n_sub = 0
    with mp.workprec(300):
        E = mp.mpf(math.e)
        for v, g in zip(lo, got):
            want = mp.power(E, mp.mpf(float(v)))
            if want < tiny:  # a subnormal result (or 0): units of 2^-1074
                worst_sub = max(worst_sub, abs(float((mp.mpf(float(g)) - want) * mp.mpf(2) ** 1074)))
                n_sub += 1
            else:
                worst_norm = max(worst_norm, _ulp_err(float(g), want, mp))
    print("pow_e worst error: %d subnormal results %.4f units of 2^-1074, normal results %.4f ulp" % (n_sub, worst_sub, worst_norm))
    assert n_sub > 3000
    assert worst_sub < 1.01, worst_sub
    assert worst_norm < 0.52, worst_norm
    inf = float("inf")
    for v, want in ((0.0, 1.0), (-0.0, 1.0), (inf, inf), (-inf, 0.0), (1e300, inf), (-1e300, 0.0), (710.0, inf), (709.79, inf),
                    (-746.0, 0.0), (math.nextafter(M.POW_E_LOW, -inf), 0.0), (math.nextafter(M.POW_E_HIGH, inf), inf)):
        g = float(orc_pf.pow_e([v], kind="portable")[0])
        assert g == want and math.copysign(1.0, g) == 1.0, (v, g)
    assert math.isnan(orc_pf.pow_e([float("nan")], kind="portable")[0])
    # +-5e-324: z * AUVP_LN_E_M1 underflows, exp(+-tiny) rounds to 1.0; the thresholds themselves are still in range
    assert orc_pf.pow_e([5e-324], kind="portable")[0] == 1.0 and orc_pf.pow_e([-5e-324], kind="portable")[0] == 1.0
    # (e ** -745.2 is 0.47 units of 2^-1074: 0; the last z that gives 5e-324 lies just above -745.14)
    top = float(orc_pf.pow_e([M.POW_E_HIGH], kind="portable")[0])
    assert 1.79e308 < top < inf and orc_pf.pow_e([M.POW_E_LOW], kind="portable")[0] == 0.0 and orc_pf.pow_e([-745.13], kind="portable")[0] == 5e-324


def test_hypot_correctly_rounded_on_its_documented_domain(orc):
    """the larger operand on [1e-140, 1e140], the other up to 60 binades below, all signs: at most 0.5 ulp against mpmath, i.e.
    correctly rounded (measured 0.4998 on every fifth pair); a zero partner returns the operand; and where exactness ends
    below the domain (auvp_hypot's comment): exact at 2^-508, not at 2^-512"""
    import mpmath as mp
    import math_edge_cases as M
    L = orc.lib("portable")
    (x, y), blocks = M.hypot()
    d = blocks["domain"]
    worst = 0.0
    with mp.workprec(300):
        for p, q in zip(x[d][::5], y[d][::5]):
            p, q = float(p), float(q)
            worst = max(worst, _ulp_err(L.orc_hypot(p, q), mp.sqrt(mp.mpf(p) ** 2 + mp.mpf(q) ** 2), mp))
    print("hypot worst error on the documented domain: %.4f ulp" % worst)
    assert worst <= 0.5, worst
    for name in ("zero_partner", "both_zero", "underflow"):
        for p, q in zip(x[blocks[name]], y[blocks[name]]):
            p, q = float(p), float(q)
            g = L.orc_hypot(p, q)
            assert g == max(abs(p), abs(q)) and math.copysign(1.0, g) == 1.0, (name, p, q, g)
    # below the domain, down to 2^-508, the host build is still correctly rounded (auvp_hypot's comment says where that ends:
    # below it the squares lose bits to the subnormals -- hypot(1e-160, 0) is off by 5.6e-6 of itself); nothing is promised there
    rng = np.random.default_rng(6)
    below = 0.0
    with mp.workprec(300):
        for p, g in zip(2.0 ** rng.uniform(-508, -465, 500), rng.uniform(0, 60, 500)):
            p, q = float(p), float(p * 2.0 ** -g)
            below = max(below, _ulp_err(L.orc_hypot(q, -p), mp.sqrt(mp.mpf(p) ** 2 + mp.mpf(q) ** 2), mp))
    print("hypot worst error, larger operand on 2^-508 .. 2^-465: %.4f ulp; hypot(1e-160, 0) / 1e-160 - 1 = %.3g" %
          (below, L.orc_hypot(1e-160, 0.0) / 1e-160 - 1.0))
    assert below <= 0.5, below


def test_atan_under_one_ulp_and_its_rare_branches(orc):
    """auvp_atan on its own (atan2 never passes it |x| >= 2^64): < 1 ulp on the breakpoints, 2^-27, 2^66 and 2^-40 .. 2^80
    (measured 0.6511); exactly +-(hi3 + lo3) = +-pi/2 from 2^66 on; x itself, sign of zero included, below 2^-27"""
    import mpmath as mp
    import math_edge_cases as M
    L = orc.lib("portable")
    x, blocks = M.atan()
    worst = 0.0
    with mp.workprec(200):
        for v in np.concatenate([x[blocks["edges"]], x[blocks["log"]]]):
            v = float(v)
            worst = max(worst, _ulp_err(L.orc_atan(v), mp.atan(mp.mpf(v)), mp))
    print("atan worst error: %.4f ulp" % worst)
    assert worst < 1.0, worst
    pio2 = 1.57079632679489655800e+00 + 6.12323399573676603587e-17
    for v in (2.0 ** 66, math.nextafter(2.0 ** 66, math.inf), 2.0 ** 80, 1e300, float("inf")):
        assert L.orc_atan(v) == pio2 and L.orc_atan(-v) == -pio2, v
    assert math.isnan(L.orc_atan(float("nan")))
    for v in (0.0, 5e-324, 1e-300, 2.0 ** -28, math.nextafter(2.0 ** -27, 0.0)):
        for s in (v, -v):
            g = L.orc_atan(s)
            assert g == s and math.copysign(1.0, g) == math.copysign(1.0, s), s
    assert L.orc_atan(2.0 ** -27) == float(mp.atan(mp.mpf(2.0 ** -27)))


BEARING_PROGRAM = r"""
#include <cstdio>
#include "auvp_math.h"
#include "replan_measure.h"
int main() {
  double y, x;
  while (std::scanf("%la %la", &y, &x) == 2) std::printf("%a %a %a\n", y, x, auvp::replan_atan2_round(y, x, auvp_atan2(y, x)));
  return 0;
}
"""


def test_bearing_composition_rounds_to_the_nearest_double(tmp_path):
    """replan_measure_kernel's bearing as the host compiles it from the real headers, replan_atan2_round(y, x, auvp_atan2(y, x))
    (on the host auvp_atan2_late IS auvp_atan2): the double nearest to mpmath's atan2 (200 bits) on every pair of the bearing
    family, 0 of 3 249 off -- so a mismatch of the device's `bearing` op (tests/test_gpu_math_edges.py) on these same inputs is
    the device's fault, not the method's"""
    import os
    import shutil
    import subprocess
    import mpmath as mp
    import pytest
    import math_edge_cases as M
    from conftest import REPO
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    (ys, xs), _ = M.bearing()
    src, exe = os.path.join(tmp_path, "bearing.cpp"), os.path.join(tmp_path, "bearing")
    open(src, "w").write(BEARING_PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(REPO, "auv_sim_amd", "csrc"), src, "-o", exe],
                   check=True, capture_output=True, text=True)
    text = "".join("%s %s\n" % (float(y).hex(), float(x).hex()) for y, x in zip(ys, xs))
    lines = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(ys)
    off_libm = 0
    for line, y0, x0 in zip(lines, ys, xs):
        y, x, r = (float.fromhex(t) for t in line.split())
        assert (y, x) == (float(y0), float(x0)) and math.copysign(1.0, y) == math.copysign(1.0, float(y0)), line
        off_libm += r != math.atan2(y, x)
        assert M.bearing_is_nearest(y, x, r), line
    print("bearing: %d of %d differ from math.atan2" % (off_libm, len(lines)))

"""The device build of csrc/auvp_math.h / auvp_exp.h at the edges of the documented domains and in the rare branches, and the
variants that exist on the device alone (auvp_sincos_sk, auvp_atan2_late, auvp_pow_e_t on a table in LDS, the bearing of
replan_measure_kernel), through auvp_math_dev.  Operand families: tests/math_edge_cases.py; the host build is held to mpmath
on the same families by tests/test_portable_math.py.

Every comparison is on the bit patterns (the sign of zero counts); a NaN only has to be a NaN on both sides.

  device == host build, bit for bit          sincos, atan2, atan, pow_e, hypot on every family
  device == the IEEE operation               div_plain, sqrt_plain on 2^+-500
  device variant == device plain function    sincos_sk, atan2_late, pow_e_lds on the full families
  device bearing == nearest double (mpmath)  the bearing family, 0 mismatches
"""
import math

import numpy as np
import pytest

import math_edge_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    c = _lib.Context(0)  # raises when the HIP extension or the GPU is missing: no fallback
    yield c
    c.close()


def _assert_same(got, want, *operands, what=""):
    bad = M.same_bits(got, want)
    assert len(bad) == 0, (what, len(bad), "operands / got / want:", M.show(bad, *operands, got, want))


def test_sincos_device_equals_host(ctx, orc):
    """a host sub-sample of 18 491: 6 000 of [-60, 60] and of 1e6 .. 1e9, 3 000 of 1e9 .. 3.5e15, and all of m 2^e (e up to
    1023: garbage values, but the same garbage), |x| < 2^-27, the multiples of pi/4 and +-0, +-inf, nan"""
    x, blocks = M.sincos()
    take = dict(working=6000, mid=6000, high=3000)
    idx = np.concatenate([np.arange(s.start, s.stop)[:take.get(name, s.stop - s.start)] for name, s in blocks.items()])
    assert len(idx) <= 20000 and all(min(2000, s.stop - s.start) <= np.count_nonzero((idx >= s.start) & (idx < s.stop)) for s in blocks.values())
    L = orc.lib("portable")
    s, c = ctx.math("sincos", x)
    _assert_same(s[idx], np.array([L.orc_sin(float(v)) for v in x[idx]]), x[idx], what="sin")
    _assert_same(c[idx], np.array([L.orc_cos(float(v)) for v in x[idx]]), x[idx], what="cos")
    # the stand-alone probe of the same function
    s1, c1 = ctx.sincos(x)
    _assert_same(s1, s, x, what="auvp_sincos_dev sin")
    _assert_same(c1, c, x, what="auvp_sincos_dev cos")


def test_atan2_and_atan_device_equal_host(ctx, orc):
    """every block of the atan2 family (33 196 pairs: the q >= 2^64 and x < 0 && q < 2^-64 branches, the side branch for zero,
    infinite and NaN operands, subnormal operands and quotients) and of the atan family (|x| < 2^-27, |x| >= 2^66, nan)"""
    L = orc.lib("portable")
    (y, x), _ = M.atan2()
    _assert_same(ctx.math("atan2", y, x), np.array([L.orc_atan2(float(p), float(q)) for p, q in zip(y, x)]), y, x, what="atan2")
    a, _ = M.atan()
    _assert_same(ctx.math("atan", a), np.array([L.orc_atan(float(v)) for v in a]), a, what="atan")


def test_pow_e_device_equals_host(ctx):
    """31 725 exponents: results rounded ONCE into the subnormals (one v_ldexp_f64 on the device, glibc's ldexp on the host),
    the largest finite results, both thresholds of auvp_exp_hl_t's out-of-range test with their neighbours, +-0, +-5e-324,
    +-inf, nan, +-1e300"""
    from oracle import orc_pf
    z, _ = M.pow_e()
    _assert_same(ctx.math("pow_e", z), orc_pf.pow_e(z, kind="portable"), z, what="pow_e")


def test_hypot_device_equals_host(ctx, orc):
    """the documented domain: the larger operand on [1e-140, 1e140] (auvp_sqrt_plain gets squares down to 2^-930, far outside
    ITS documented 2^+-500), a zero partner, both zero, full underflow"""
    L = orc.lib("portable")
    (x, y), _ = M.hypot()
    _assert_same(ctx.math("hypot", x, y), np.array([L.orc_hypot(float(p), float(q)) for p, q in zip(x, y)]), x, y, what="hypot")


def test_div_and_sqrt_plain_equal_ieee_on_their_whole_domain(ctx):
    """|a|, |b|, |a / b| within 2^+-500 and x within 2^+-500: the limits auvp_math.h documents, exact powers of two on them"""
    (a, b), _ = M.div_plain()
    _assert_same(ctx.math("div_plain", a, b), a / b, a, b, what="div_plain")
    _assert_same(ctx.math("div", a, b), a / b, a, b, what="div")
    x, _ = M.sqrt_plain()
    _assert_same(ctx.math("sqrt_plain", x), np.sqrt(x), x, what="sqrt_plain")
    _assert_same(ctx.math("sqrt", x), np.sqrt(x), x, what="sqrt")


def test_device_only_variants_equal_the_plain_functions(ctx):
    """what the hot kernels call against what the probes above hold to the host build, on the full families: auvp_sincos_sk
    (every Horner step an inline-assembly fma through a fixed scalar pair), auvp_atan2_late (constants through a volatile
    asm), auvp_pow_e_t on the table's copy in LDS"""
    x, _ = M.sincos()
    s, c = ctx.math("sincos", x)
    s_sk, c_sk = ctx.math("sincos_sk", x)
    _assert_same(s_sk, s, x, what="sincos_sk sin")
    _assert_same(c_sk, c, x, what="sincos_sk cos")
    (y, xx), _ = M.atan2()
    _assert_same(ctx.math("atan2_late", y, xx), ctx.math("atan2", y, xx), y, xx, what="atan2_late")
    (y, xx), _ = M.bearing()
    _assert_same(ctx.math("atan2_late", y, xx), ctx.math("atan2", y, xx), y, xx, what="atan2_late (bearing family)")
    z, _ = M.pow_e()
    _assert_same(ctx.math("pow_e_lds", z), ctx.math("pow_e", z), z, what="pow_e_lds")


def test_bearing_is_the_nearest_double(ctx):
    """replan_measure_kernel's expression without the heading, replan_atan2_round(y, x, auvp_atan2_late(y, x)), on the device:
    the double nearest to mpmath's atan2 on all 3 249 pairs of the bearing family (y == +-0: math.atan2's value and sign) --
    as the host composition is (tests/test_portable_math.py), so 0 mismatches"""
    (y, x), _ = M.bearing()
    got = ctx.math("bearing", y, x)
    bad = [i for i in range(len(y)) if not M.bearing_is_nearest(float(y[i]), float(x[i]), float(got[i]))]
    print("bearing: %d of %d differ from math.atan2" % (sum(float(g) != math.atan2(float(p), float(q)) for g, p, q in zip(got, y, x)), len(y)))
    assert not bad, (len(bad), M.show(bad, y, x, got))


def test_math_dev_argument_check_and_partial_workgroups(ctx):
    """an op one past the last is AUVP_ERR_ARG; n = 1 and every n that is no multiple of the 256-thread workgroup work -- with
    the LDS op, whose barrier every thread of a partial last workgroup must reach"""
    import ctypes as C
    AUVP_ERR_ARG = -1  # include/auvplan.h
    one = np.ones(1)
    out0, out1 = np.zeros(1), np.zeros(1)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    last = max(ctx.MATH_OPS.values())
    assert ctx.L.auvp_math_dev(ctx.h, last + 1, 1, p(one), p(one), p(out0), p(out1)) == AUVP_ERR_ARG
    assert ctx.L.auvp_math_dev(ctx.h, -1, 1, p(one), p(one), p(out0), p(out1)) == AUVP_ERR_ARG
    assert ctx.L.auvp_math_dev(ctx.h, last, 1, p(one), p(one), p(out0), p(out1)) == 0 and abs(out0[0] - math.pi / 4) <= math.ulp(0.5)
    z, _ = M.pow_e()
    want = ctx.math("pow_e", z[:1024])
    for n in (1, 63, 64, 127, 129, 255, 257, 511, 1000):
        _assert_same(ctx.math("pow_e_lds", z[:n]), want[:n], z[:n], what="pow_e_lds n = %d" % n)
        _assert_same(ctx.math("pow_e", z[:n]), want[:n], z[:n], what="pow_e n = %d" % n)
    assert abs(ctx.math("atan", [1.0])[0] - math.pi / 4) <= math.ulp(0.5) and [float(v[0]) for v in ctx.math("sincos_sk", [0.0])] == [0.0, 1.0]

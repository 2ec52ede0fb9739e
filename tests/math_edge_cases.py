"""Operand families of tests/test_portable_math.py (the host build of csrc/auvp_math.h / auvp_exp.h against mpmath) and of
tests/test_gpu_math_edges.py (the device build against the host build, the device-only variants against the plain ones).  Not a
test module.

Every family reaches the rare branches and the ends of the documented domains of one function:

  sincos      [-60, 60]; 1e6 .. 1e9 (the ~100-bit reduction's documented end); 1e9 .. 3.5e15 (n mod 4 still exact); m 2^e up to
              2^1023 ("the same bits on host and device"); |x| < 2^-27 and subnormals; k pi/2, k pi/4 and their neighbours; +-0,
              +-inf, nan
  atan2       every special operand pair; |y/x| >= 2^64 and < 2^-64 in all four quadrants, quotients that overflow and underflow
              among them; |y/x| < 2^-27 (atan returns its argument); subnormal operands; generic pairs; quotients within 2^-40 of
              atan's reduction breakpoints and exactly on them
  atan        the breakpoints, 2^-27 and 2^66 with their neighbours; +-inf, nan, +-0; 2^-40 .. 2^80 log-uniform
  pow_e       subnormal and just-normal results; the top of the range; both thresholds of auvp_exp_hl_t with their neighbours;
              +-0, +-5e-324, +-inf, nan, +-1e300; the working range
  div_plain   |a|, |b|, |a / b| within 2^+-500, exponents uniform; a = +0; exact powers of two at all three limits
  sqrt_plain  2^+-500; every power of two in it; +0
  hypot       the larger operand on [1e-140, 1e140], exponent gap 0 .. 60, all signs; a zero partner across that range; both
              zero; the full-underflow operands
  bearing     the families of tests/test_replan_bearing_host.py; |y/x| < 2^-64 with x < 0 (a0 is exactly +-pi); its special grid

Every function returns read-only arrays, computed once (fixed seeds).  `blocks` dictionaries map a block's name to its slice of
the family, so that a test can sub-sample per block.
"""
import functools
import itertools
import math

import numpy as np

INF, NAN = float("inf"), float("nan")
ATAN_BREAKS = (0.4375, 0.6875, 1.1875, 2.4375)   # auvp_atan_body.h: where the argument reduction changes
POW_E_LOW, POW_E_HIGH = -745.2, 709.782712893384  # auvp_exp_hl_t: below -> 0, above -> inf
ATAN2_SPECIAL = (0.0, -0.0, 1.0, -1.0, INF, -INF, NAN, 1e-300, -1e-300, 1e300, -1e300, 2.5, -3.75, 5e-324)
BEARING_SPECIAL = (0.0, -0.0, 25.0, -25.0, 1e-9, -1e-9, 30.0)


def _ro(*arrays):
    out = []
    for a in arrays:
        a = np.ascontiguousarray(a, dtype=np.float64)
        a.setflags(write=False)
        out.append(a)
    return out[0] if len(out) == 1 else tuple(out)


def _join(named):
    """[(name, array or tuple of arrays)] -> the concatenated array(s) and {name: slice}"""
    blocks, pos, cols = {}, 0, None
    for name, v in named:
        v = v if isinstance(v, tuple) else (v,)
        v = tuple(np.asarray(c, dtype=np.float64).ravel() for c in v)
        assert len({len(c) for c in v}) == 1
        cols = [[] for _ in v] if cols is None else cols
        for lst, c in zip(cols, v):
            lst.append(c)
        blocks[name] = slice(pos, pos + len(v[0]))
        pos += len(v[0])
    arrays = tuple(_ro(np.concatenate(c)) for c in cols)
    return (arrays[0] if len(arrays) == 1 else arrays), blocks


def neighbours(v, k=1):
    """every value of v with its k neighbouring doubles on either side"""
    v = np.atleast_1d(np.asarray(v, dtype=np.float64))
    out, lo, hi = [v], v, v
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def _signs(rng, n):
    return rng.choice([-1.0, 1.0], n)


def _pow2_mant(rng, e):
    """m 2^e, m uniform on [1, 2) (below 2^-1022 the result is the nearest subnormal)"""
    return np.ldexp(rng.uniform(1.0, 2.0, len(e)), e.astype(np.int64))


def _subnormals(rng, n):
    return rng.integers(1, 2 ** 52, n, dtype=np.uint64).view(np.float64)


@functools.lru_cache(None)
def sincos():
    """-> x, blocks"""
    rng = np.random.default_rng(101)
    tiny = np.concatenate([_pow2_mant(rng, rng.integers(-1074, -27, 990)) * 0.999 * _signs(rng, 990),
                           [5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 2.225073858507201e-308,
                            -2.225073858507201e-308, math.nextafter(2.0 ** -27, 0.0), -math.nextafter(2.0 ** -27, 0.0), 1e-310, -1e-310]])
    return _join([
        ("working", rng.uniform(-60, 60, 20000)),
        ("mid", 10.0 ** rng.uniform(6, 9, 20000) * _signs(rng, 20000)),                      # 1e6 .. 1e9
        ("high", np.minimum(10.0 ** rng.uniform(9, math.log10(3.5e15), 5000), 3.5e15) * _signs(rng, 5000)),
        ("huge", _pow2_mant(rng, rng.integers(52, 1024, 2000)) * _signs(rng, 2000)),        # m 2^e, e in [52, 1023]
        ("tiny", tiny),
        ("multiples", neighbours([k * math.pi / 2 for k in range(-40, 41)] + [k * math.pi / 4 for k in range(-40, 41)])),
        ("special", [0.0, -0.0, INF, -INF, NAN]),
    ])


def _quadrants(rng, big, small, n):
    """(big, small) magnitudes with all four sign combinations in turn"""
    i = np.arange(n)
    return big * np.where(i & 1, -1.0, 1.0), small * np.where(i & 2, -1.0, 1.0)


@functools.lru_cache(None)
def atan2():
    """-> (y, x), blocks"""
    rng = np.random.default_rng(102)
    n = 2000
    # a quotient beyond 2^+-64: the larger operand m 2^e with e over the whole range, the smaller at least 65 binades below
    # (down to the subnormals); gaps of 1024 and more overflow the quotient to inf / underflow it to 0, 1022 .. 1074 to subnormals
    e_big = rng.integers(-1000, 1024, n)
    gap = np.minimum(rng.integers(65, 1200, n), e_big + 1074)
    gap[:40] = np.minimum(np.repeat([1022, 1030, 1050, 1074, 1075, 1100, 1500, 2000], 5), e_big[:40] + 1074)
    big, small = _pow2_mant(rng, e_big), _pow2_mant(rng, e_big - gap)
    big[:8] = [1e300, 1.7976931348623157e308, 1.0, 2.0 ** 64, 2.0 ** 1023, 1e308, 3.0, 1e-250]
    small[:8] = [1e-300, 5e-324, 2.0 ** -64, 1.0, 2.0 ** -1074, 1e-308, 5e-324, 5e-324]
    over = _quadrants(rng, big, small, n)                         # y = big, x = small: |y/x| >= 2^64
    e_big = rng.integers(-1000, 1024, n)
    gap = np.minimum(rng.integers(65, 1200, n), e_big + 1074)
    gap[:40] = np.minimum(np.repeat([1022, 1030, 1050, 1074, 1075, 1100, 1500, 2000], 5), e_big[:40] + 1074)
    big, small = _pow2_mant(rng, e_big), _pow2_mant(rng, e_big - gap)
    big[:8] = [1e300, 1.7976931348623157e308, 1.0, 2.0 ** 65, 2.0 ** 1023, 1e308, 3.0, 1e-250]
    small[:8] = [1e-300, 5e-324, 2.0 ** -65, 0.75, 2.0 ** -1074, 1e-308, 5e-324, 5e-324]
    xs, ys = _quadrants(rng, big, small, n)                       # x = big, y = small: |y/x| < 2^-64
    under = (ys, xs)
    e_big = rng.integers(-300, 300, n)
    xs, ys = _quadrants(rng, _pow2_mant(rng, e_big), _pow2_mant(rng, e_big - rng.integers(29, 64, n)), n)
    small_q = (ys, xs)                                            # 2^-64 < |y/x| < 2^-27: atan returns the quotient itself
    # subnormal operands: y, x or both (the partner m 2^e over the whole exponent range)
    k = np.arange(n) % 3
    partner_y, partner_x = _pow2_mant(rng, rng.integers(-1074, 1024, n)), _pow2_mant(rng, rng.integers(-1074, 1024, n))
    sub = (np.where(k != 1, _subnormals(rng, n), partner_y) * _signs(rng, n), np.where(k != 0, _subnormals(rng, n), partner_x) * _signs(rng, n))
    # quotients at atan's breakpoints: y = (b + u 2^-40) x, |u| < 0.99 (the rounding of y and of y / x moves the quotient by
    # ~2^-52 b), and exactly on them: x with a 20-bit significand, so that b x and (b x) / x are exact
    m = 5000
    b = np.array(ATAN_BREAKS)[np.arange(m) % 4]
    xb = rng.uniform(0.01, 300, m) * _signs(rng, m)
    yb = (b + rng.uniform(-0.99, 0.99, m) * 2.0 ** -40) * xb * _signs(rng, m)
    ex = np.arange(0, m, 25)                                      # 200 exact ones
    xb[ex] = np.ldexp(rng.integers(1, 2 ** 20, len(ex)).astype(np.float64), rng.integers(-30, 10, len(ex))) * _signs(rng, len(ex))
    yb[ex] = b[ex] * xb[ex] * _signs(rng, len(ex))
    sp = np.array(list(itertools.product(ATAN2_SPECIAL, ATAN2_SPECIAL)))
    return _join([("special", (sp[:, 0], sp[:, 1])), ("over", over), ("under", under), ("small_q", small_q), ("subnormal", sub),
                  ("generic", (rng.uniform(-300, 300, 20000), rng.uniform(-300, 300, 20000))), ("breaks", (yb, xb))])


@functools.lru_cache(None)
def atan():
    """-> x, blocks"""
    rng = np.random.default_rng(103)
    edge = neighbours(list(ATAN_BREAKS) + [2.0 ** -27, 2.0 ** 66], 2)
    return _join([("edges", np.concatenate([edge, -edge])), ("special", [INF, -INF, NAN, 0.0, -0.0]),
                  ("log", 2.0 ** rng.uniform(-40, 80, 5000) * _signs(rng, 5000))])


def pow_e_working(rng):
    """the working range: the particle weights' exponents (tests/test_portable_math.py)"""
    return np.concatenate([-rng.uniform(0, 20, 3000) ** 2 / 0.5, -rng.uniform(0, 800, 3000) ** 2 / 20000,
                           -rng.uniform(0, 1e-3, 200), rng.uniform(-740, 700, 500), [0.0, -0.0, -1.0, 1.0, -745.0, -800.0]])


@functools.lru_cache(None)
def pow_e():
    """-> z, blocks"""
    rng = np.random.default_rng(104)
    return _join([("low", rng.uniform(-745.3, -707.5, 20000)),     # results from 0 through the subnormals to just normal
                  ("top", rng.uniform(700, 709.9, 5000)),           # ... up to the largest doubles and inf
                  ("thresholds", neighbours([POW_E_LOW, POW_E_HIGH], 2)),
                  ("special", [0.0, -0.0, 5e-324, -5e-324, INF, -INF, NAN, 1e300, -1e300]),
                  ("working", pow_e_working(np.random.default_rng(2)))])


@functools.lru_cache(None)
def div_plain():
    """-> (a, b), blocks: |a|, |b| and |a / b| within 2^+-500 (a may be +0)"""
    rng = np.random.default_rng(105)
    n = 100000
    # a = ma 2^ea, b = mb 2^eb with ma, mb on [1, 2): |a / b| lies in (2^(ea - eb - 1), 2^(ea - eb + 1))
    ea = rng.integers(-500, 500, n)
    eb = rng.integers(np.maximum(-500, ea - 499), np.minimum(499, ea + 499) + 1)
    a, b = _pow2_mant(rng, ea) * _signs(rng, n), _pow2_mant(rng, eb) * _signs(rng, n)
    zb = _pow2_mant(rng, rng.integers(-500, 500, 1000)) * _signs(rng, 1000)
    # exact powers of two with |a|, |b| or |a / b| at a limit
    pa, pb = [], []
    for x, y in ((500, 0), (-500, 0), (0, 500), (0, -500), (500, 500), (-500, -500), (250, -250), (-250, 250), (500, 1), (-500, -1),
                 (499, -1), (-499, 1), (0, 0), (500, 250), (-500, -250), (1, -499), (-1, 499)):
        for sa, sb in itertools.product((1.0, -1.0), repeat=2):
            pa.append(sa * 2.0 ** x)
            pb.append(sb * 2.0 ** y)
    return _join([("uniform", (a, b)), ("zero", (np.zeros(1000), zb)), ("pow2", (pa, pb))])


@functools.lru_cache(None)
def sqrt_plain():
    """-> x, blocks: 0 or within 2^+-500"""
    rng = np.random.default_rng(106)
    return _join([("uniform", _pow2_mant(rng, rng.integers(-500, 500, 100000))), ("pow2", 2.0 ** np.arange(-500, 501)), ("zero", np.zeros(4))])


HYPOT_LO, HYPOT_HI = 1e-140, 1e140  # the documented domain (auvp_math.h)


@functools.lru_cache(None)
def hypot():
    """-> (x, y), blocks"""
    rng = np.random.default_rng(107)
    n = 50000
    big = 10.0 ** rng.uniform(-140, 140, n)
    big[:4] = [HYPOT_LO, HYPOT_HI, HYPOT_LO, HYPOT_HI]
    small = big * 2.0 ** -rng.uniform(0, 60, n)
    small[:2] = big[:2]
    swap = rng.integers(0, 2, n).astype(bool)
    x, y = np.where(swap, small, big) * _signs(rng, n), np.where(swap, big, small) * _signs(rng, n)
    m = 2000
    z = 10.0 ** rng.uniform(-140, 140, m) * _signs(rng, m)
    z[:4] = [HYPOT_LO, -HYPOT_LO, HYPOT_HI, -HYPOT_HI]
    zeros = np.where(np.arange(m) & 2, -0.0, 0.0)
    zx, zy = np.where(np.arange(m) & 1, z, zeros), np.where(np.arange(m) & 1, zeros, z)
    uf = [1e-200, -3e-180, 5e-324]
    return _join([("domain", (x, y)), ("zero_partner", (zx, zy)), ("both_zero", ([0.0, 0.0, -0.0, -0.0], [0.0, -0.0, 0.0, -0.0])),
                  ("underflow", (uf + [0.0] * 3 + uf + [-0.0] * 3, [0.0] * 3 + uf + [-0.0] * 3 + uf))])


@functools.lru_cache(None)
def bearing():
    """-> (y, x), blocks"""
    rng = np.random.default_rng(108)
    u = lambda n: rng.uniform(-200.0, 200.0, n)
    v = lambda n: rng.uniform(-1.0, 1.0, n)
    xd = u(500)
    xn = -rng.uniform(0.01, 200.0, 200)
    yn = xn * _pow2_mant(rng, -rng.integers(66, 300, 200)) * _signs(rng, 200)
    sp = np.array(list(itertools.product(BEARING_SPECIAL, BEARING_SPECIAL)))
    return _join([("generic", (u(1500), u(1500))), ("y_tiny", (v(500) * 1e-9, u(500))), ("x_tiny", (u(500), v(500) * 1e-9)),
                  ("diagonal", (xd * (1.0 + v(500) * 1e-12), xd)), ("minus_pi", (yn, xn)), ("special", (sp[:, 0], sp[:, 1]))])


def bearing_is_nearest(y, x, r):
    """r is the double nearest to atan2(y, x) (mpmath, 200 bits); for y == +-0, where the angle is 0, -0, pi or -pi by the signs
    alone (mpmath knows no -0): math.atan2's value and sign -- the rule of tests/test_replan_bearing_host.py"""
    import mpmath as mp
    if y == 0.0:
        want = math.atan2(y, x)
        return r == want and math.copysign(1.0, r) == math.copysign(1.0, want)
    with mp.workprec(200):
        true = mp.atan2(mp.mpf(y), mp.mpf(x))
        err = abs(true - mp.mpf(r))
        # no neighbour is closer (a tie does not occur: the true angle is irrational)
        return bool(err <= abs(true - mp.mpf(math.nextafter(r, math.inf))) and err <= abs(true - mp.mpf(math.nextafter(r, -math.inf))))


def same_bits(got, want):
    """indices at which got and want differ: bit for bit (the sign of zero counts), except that a NaN only has to be a NaN"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape
    both_nan = np.isnan(got) & np.isnan(want)
    return np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)) & ~both_nan)


def show(idx, *cols, limit=6):
    """the operands / values at idx in %a form, for an assertion's message"""
    return [tuple(float(c[i]).hex() for c in cols) for i in idx[:limit]]

// replan_measure.h -- a fleet's range / bearing measurements from the states it has committed (auvp_replan_measure,
// include/auvplan.h; replan_measure_kernel, replan_kernels.hip).
//
// Shark f of F is tracked by exactly A AUVs: the AUVs with shark_of == f, in ascending AUV index.  Row (f, a) of the table
// meas [F][A][5], the layout auvp_pf_run reads for one step, is
//   x, y, theta                      of the AUV's state last [7] where it lies in HBM (an AUV that stopped planning keeps its
//                                    last committed state)
//   range   = sqrt(dx*dx + dy*dy)    dx = shark_x - x, dy = shark_y - y, no contraction
//   bearing = atan2(dy, dx) - theta
// The definition on the host is tracking.fleet_measurements, written with math.sqrt and math.atan2, and the kernel is held to it
// bit for bit.  The square root is auvp_math.h's (correctly rounded, as libm's).  The atan2 starts from the particle-filter
// kernel's routine (auvp_atan_body.h: within 1.2 ulp; its last bit differs from libm's for about one argument pair in six) and
// replan_atan2_round below turns that value into the nearest double to the true angle: with a0 ~ atan2(y, x),
// atan2(y, x) = a0 + atan2(y cos a0 - x sin a0, x cos a0 + y sin a0), the second term is below 2 ulp of a0, and sin a0 / cos a0
// in double-double (a Taylor sum after the pi/2 reduction) give it to about 2^-50 of itself -- so a0 + delta, one rounding, is
// correctly rounded unless the angle lies within ~2^-50 ulp of a midpoint.  libm's atan2 is that double too except for about 7
// pairs in 10 000, where ITS last bit is off (3 732 of 5 000 121 pairs on the host, against arbitrary precision): that is how
// often kernel and definition can still differ.  tests/test_replan_bearing_host.py holds the step to arbitrary precision.
// replan_measure_members is the host's part: pure, every index the kernel uses is checked here.
#ifndef AUVP_REPLAN_MEASURE_H
#define AUVP_REPLAN_MEASURE_H
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define AUVP_MEAS_HD __host__ __device__ inline
#else
#define AUVP_MEAS_HD inline
#endif

namespace auvp {

constexpr int REPLAN_MEAS_ROW = 5;  // doubles per measurement row

// ---- double-double helpers (hi + lo, |lo| <= ulp(hi) / 2); every product through an explicit fma, no contraction needed
struct MeasDD { double hi, lo; };
AUVP_MEAS_HD MeasDD meas_two_sum(double a, double b) {
  const double s = a + b, bb = s - a;
  return MeasDD{s, (a - (s - bb)) + (b - bb)};
}
AUVP_MEAS_HD MeasDD meas_two_prod(double a, double b) {
  const double p = a * b;
  return MeasDD{p, __builtin_fma(a, b, -p)};
}
AUVP_MEAS_HD MeasDD meas_dd_add(MeasDD a, MeasDD b) {
  MeasDD s = meas_two_sum(a.hi, b.hi);
  s.lo += a.lo + b.lo;
  return meas_two_sum(s.hi, s.lo);
}
AUVP_MEAS_HD MeasDD meas_dd_mul(MeasDD a, MeasDD b) {
  MeasDD p = meas_two_prod(a.hi, b.hi);
  p.lo += a.hi * b.lo + a.lo * b.hi;
  return meas_two_sum(p.hi, p.lo);
}
AUVP_MEAS_HD MeasDD meas_dd_div_d(MeasDD a, double d) {  // d: a small integer
  const double q1 = a.hi / d;
  const double r = __builtin_fma(-q1, d, a.hi) + a.lo;
  return meas_two_sum(q1, r / d);
}

// sin and cos of the double a, |a| <= 4, in double-double
AUVP_MEAS_HD void meas_sincos_dd(double a, MeasDD* sin_out, MeasDD* cos_out) {
  // pi/2 in three parts (auvp_math.h: AUVP_PIO2_HI / _LO / _LO2)
  const double hi = 0x1.921fb54442d18p+0, lo = 0x1.1a62633145c07p-54, lo2 = -0x1.f1976b7ed8fbcp-110;
  const double k = __builtin_rint(a * 0x1.45f306dc9c883p-1);  // -3 .. 3
  // r = a - k * pi/2: k * hi is exact (k has two bits), the difference of two nearby doubles too
  MeasDD r = meas_two_sum(a, -k * hi);
  const MeasDD t = meas_two_prod(-k, lo);
  r = meas_dd_add(r, t);
  r = meas_dd_add(r, MeasDD{-k * lo2, 0.0});
  const MeasDD r2 = meas_dd_mul(r, r);
  MeasDD s = r, c = MeasDD{1.0, 0.0}, ts = r, tc = MeasDD{1.0, 0.0};
  for (int i = 1; i <= 14; i++) {  // |r| <= pi/4 (+ a little): the terms fall below 2^-100 of the sums
    tc = meas_dd_div_d(meas_dd_mul(tc, r2), (double)((2 * i - 1) * (2 * i)));
    ts = meas_dd_div_d(meas_dd_mul(ts, r2), (double)((2 * i) * (2 * i + 1)));
    tc.hi = -tc.hi; tc.lo = -tc.lo; ts.hi = -ts.hi; ts.lo = -ts.lo;
    c = meas_dd_add(c, tc);
    s = meas_dd_add(s, ts);
  }
  const int q = ((int)k) & 3;  // a = r + q * pi/2 (mod 2 pi)
  const MeasDD ns{-s.hi, -s.lo}, nc{-c.hi, -c.lo};
  *sin_out = q == 0 ? s : (q == 1 ? c : (q == 2 ? ns : nc));
  *cos_out = q == 0 ? c : (q == 1 ? ns : (q == 2 ? nc : s));
}

// the double nearest to atan2(y, x), from a0 within a few ulp of it (finite y, x of unexceptional magnitude; a0 is returned as
// it is where there is nothing to correct: y == x == 0, a non-finite value)
AUVP_MEAS_HD double replan_atan2_round(double y, double x, double a0) {
  if (!(a0 == a0) || !(a0 - a0 == 0.0) || (x == 0.0 && y == 0.0) || !(x - x == 0.0) || !(y - y == 0.0)) return a0;
  MeasDD s, c;
  meas_sincos_dd(a0, &s, &c);
  const double den = x * c.hi + y * s.hi;
  if (!(den > 0.0)) return a0;  // (a0 is not near the angle at all, or the operands underflowed)
  // num = y cos a0 - x sin a0: the leading products cancel to a few ulp
  const MeasDD p1 = meas_two_prod(y, c.hi), p2 = meas_two_prod(x, s.hi);
  const double num = (p1.hi - p2.hi) + ((p1.lo - p2.lo) + (y * c.lo - x * s.lo));
  return num == 0.0 ? a0 : a0 + num / den;  // (a0 exact, a signed zero among them: as it is)
}

struct ReplanMeasureDev {
  int32_t n, A;                 // n = F * A rows
  const int32_t* members;       // [n] AUV of row i; shark i / A
  const double* last;           // [n_auvs][7] the fleet's states
  const double* shark_xy;       // [F][2]
  double* meas;                 // [n][5]
};

enum ReplanMeasureStatus {
  REPLAN_MEAS_OK = 0,
  REPLAN_MEAS_BAD_SHAPE,  // A < 1, no AUV, or n_auvs no multiple of A
  REPLAN_MEAS_BAD_SHARK,  // AUV `bad`: shark_of outside [0, n_auvs / A)
  REPLAN_MEAS_UNEQUAL     // shark `bad` is not tracked by exactly A AUVs
};

struct ReplanMeasurePlan {
  ReplanMeasureStatus status = REPLAN_MEAS_OK;
  int bad = -1;
  int F = 0;
  std::vector<int32_t> members;  // [F * A]
};

inline ReplanMeasurePlan replan_measure_members(const int32_t* shark_of, int n_auvs, int A) {
  ReplanMeasurePlan p;
  if (!shark_of || A < 1 || n_auvs < 1 || n_auvs % A != 0) { p.status = REPLAN_MEAS_BAD_SHAPE; return p; }
  p.F = n_auvs / A;
  std::vector<int32_t> count((size_t)p.F, 0);
  p.members.assign((size_t)n_auvs, -1);
  for (int i = 0; i < n_auvs; i++) {  // (ascending AUV index within every shark)
    const int f = shark_of[i];
    if (f < 0 || f >= p.F) { p.status = REPLAN_MEAS_BAD_SHARK; p.bad = i; return p; }
    if (count[(size_t)f] >= A) { p.status = REPLAN_MEAS_UNEQUAL; p.bad = f; return p; }
    p.members[(size_t)f * (size_t)A + (size_t)count[(size_t)f]++] = i;
  }
  // (n_auvs == F * A and no shark above A: every shark has exactly A)
  return p;
}

}  // namespace auvp
#endif  // AUVP_REPLAN_MEASURE_H

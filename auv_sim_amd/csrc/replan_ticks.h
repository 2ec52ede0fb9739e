// replan_ticks.h -- k measurements per round, taken along the bucket every AUV committed last (auvp_replan_measure with option
// MEAS_TICKS, include/auvplan.h; replan_measure_ticks_kernel, replan_kernels.hip).  No HIP in here: g++ alone compiles it
// (tests/host/replan_ticks_check.cpp), and the kernel is built from the same pieces.
//
// One AUV: its state last [7] and the segment it committed in the MOST RECENT auvp_replan_commit -- n >= 0 rows of 7 doubles in
// the trajectory log; row 0 is the state it had before that commit (replan_commit.h), so its time is the bucket's lo.
//   tick times   lo = seg[0][4]; tau_j = lo + (j + 1) * (round_span / k) for j < k - 1, tau_{k-1} = lo + 1.0 * round_span --
//                replan_bucket's hi, so the last tick is the committed state itself however k * (span / k) rounds.  Every
//                operation rounded on its own (-ffp-contract=off), the same ones as tracking.fleet_measurements_ticks.
//   position     the segment row with the GREATEST index i such that t_i <= tau_j (a NaN time, or a NaN tau: never); row 0 if
//                there is none.  Nothing is interpolated: the AUV stays at the last point it reached, as course_ticks has it
//                (replan_apart.h).  A linear scan by definition: the times need not ascend.
//   n == 0       every tick from `last`: an AUV that stopped planning, a group without a winner, a fleet before its first commit.
// The measurement row itself -- x, y, theta of the chosen row, range, bearing -- is replan_measure.h's, unchanged.
// replan_ticks_plan is the host's part: pure, and every index the kernel uses is checked here.
#ifndef AUVP_REPLAN_TICKS_H
#define AUVP_REPLAN_TICKS_H
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "replan_commit.h"

#if defined(__HIPCC__)
#define AUVP_TICKS_HD __host__ __device__ inline
#else
#define AUVP_TICKS_HD inline
#endif

namespace auvp {

constexpr int REPLAN_MEAS_MAX_TICKS = 64;   // k: one lane of a wavefront per tick
constexpr int REPLAN_MEAS_TICKS_WAVES = 4;  // wavefronts (AUVs) per workgroup of replan_measure_ticks_kernel

AUVP_TICKS_HD bool replan_meas_ticks_ok(long long k) { return k >= 1 && k <= REPLAN_MEAS_MAX_TICKS; }

// the time of tick j of k in the bucket that starts at lo
AUVP_TICKS_HD double replan_meas_tick_time(double lo, double round_span, int k, int j) {
  if (j == k - 1) return lo + 1.0 * round_span;
  const double step = round_span / (double)k;
  return lo + (double)(j + 1) * step;
}

// does row time t qualify for the tick at tau
AUVP_TICKS_HD bool replan_meas_tick_reached(double t, double tau) { return t <= tau; }

// the row of the segment seg [n,7], n >= 1, the AUV is at when the clock shows tau
AUVP_TICKS_HD int replan_meas_tick_row(const double* seg, int n, double tau) {
  int best = 0;
  for (int i = 0; i < n; i++)
    if (replan_meas_tick_reached(seg[(long long)REPLAN_ROW * i + 4], tau)) best = i;
  return best;
}

// The whole rule for one AUV, serially: tau [k] and row [k] (-1: from `last`, the segment is empty).
AUVP_TICKS_HD void replan_meas_ticks_serial(const double* seg, int n, int k, double round_span, double* tau, int32_t* row) {
  for (int j = 0; j < k; j++) {
    tau[j] = n > 0 ? replan_meas_tick_time(seg[4], round_span, k, j) : 0.0;
    row[j] = n > 0 ? replan_meas_tick_row(seg, n, tau[j]) : -1;
  }
}

// ---- what the kernel and its host side share ---------------------------------------------------------------------------------

// one piece of an AUV's trajectory in the log, as the host remembers it: n rows from log row src, committed in round `round`
struct ReplanPiece {
  int32_t auv, n;
  int64_t src;
  int32_t round, _pad;
};

// the segment of one measurement row group (f, a): n rows from log row off; n == 0: none, the AUV's state stands for every tick
struct ReplanMeasSeg {
  int64_t off;
  int32_t n, _pad;
};

struct ReplanMeasTicksDev {
  int32_t n, A, k, _pad;        // n = F * A AUVs, k ticks
  const int32_t* members;       // [n] AUV of row group i; shark i / A
  const ReplanMeasSeg* seg;     // [n]
  const double* last;           // [n_auvs][7] the fleet's states
  const double* log;            // the trajectory log, [*,7]
  const double* shark_xy;       // [k][F][2]
  double* meas;                 // [k][n][5]
  double round_span;            // of the commit the segments come from
};

enum ReplanTicksStatus {
  REPLAN_TICKS_OK = 0,
  REPLAN_TICKS_BAD_K,       // k outside 1 .. REPLAN_MEAS_MAX_TICKS
  REPLAN_TICKS_BAD_MEMBER,  // row group `bad`: its AUV outside [0, n_auvs)
  REPLAN_TICKS_BAD_PIECE    // piece `bad`: AUV outside the fleet, n < 1, rows outside [0, log_rows), or its AUV's second piece of the round
};

struct ReplanTicksPlan {
  ReplanTicksStatus status = REPLAN_TICKS_OK;
  long long bad = -1;
  std::vector<ReplanMeasSeg> seg;  // [n_rows]
};

// The segments of the last commit by measurement row group.  pieces [n_pieces] in round order (every round's pieces together,
// the rounds ascending); last_round: the round index of the most recent commit (-1: none yet) -- an AUV without a piece of that
// round gets n == 0.  members [n_rows]: the AUV of every row group.  log_rows: the rows of the log that commits have written
// into; a piece's offset counts the rows RESERVED before it (every winner's whole course), so this is the log's reserved
// size, which the committed count only bounds from below.
inline ReplanTicksPlan replan_ticks_plan(const ReplanPiece* pieces, size_t n_pieces, int last_round, int n_auvs, const int32_t* members,
                                         int n_rows, long long log_rows, long long k) {
  ReplanTicksPlan p;
  if (!replan_meas_ticks_ok(k)) { p.status = REPLAN_TICKS_BAD_K; return p; }
  std::vector<ReplanMeasSeg> of_auv((size_t)(n_auvs > 0 ? n_auvs : 0), ReplanMeasSeg{0, 0, 0});
  for (size_t i = n_pieces; last_round >= 0 && i-- > 0;) {
    const ReplanPiece& c = pieces[i];
    if (c.round != last_round) break;  // (round order: everything before is older)
    if (c.auv < 0 || c.auv >= n_auvs || c.n < 1 || c.src < 0 || c.src > log_rows || (long long)c.n > log_rows - c.src ||
        of_auv[(size_t)c.auv].n != 0) {
      p.status = REPLAN_TICKS_BAD_PIECE; p.bad = (long long)i; return p;
    }
    of_auv[(size_t)c.auv] = ReplanMeasSeg{c.src, c.n, 0};
  }
  p.seg.assign((size_t)(n_rows > 0 ? n_rows : 0), ReplanMeasSeg{0, 0, 0});
  for (int i = 0; i < n_rows; i++) {
    const int m = members ? members[i] : -1;
    if (m < 0 || m >= n_auvs) { p.status = REPLAN_TICKS_BAD_MEMBER; p.bad = i; p.seg.clear(); return p; }
    p.seg[(size_t)i] = of_auv[(size_t)m];
  }
  return p;
}

}  // namespace auvp
#endif  // AUVP_REPLAN_TICKS_H

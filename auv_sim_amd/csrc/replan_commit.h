// replan_commit.h -- replanning's step between two rounds as pure functions: no HIP in here, g++ alone compiles it
// (tests/host/replan_commit_check.cpp), and rrt_commit_kernel (replan_kernels.hip) is built from the same pieces.
//
// The rule is the reference's host step (path_planning/rrt_dubins.py:82-87: splitPath's first bucket + removeHabitat), restated
// in Python as rrt_dubins.first_bucket_commit -- the definition this header matches bit for bit (the library and the test
// program are built with -ffp-contract=off: every product and sum below is rounded on its own, as numpy rounds them).
//
// One AUV: last[7] (x, y, theta, v, traj_time_stamp, plan_time_stamp, length), keep (bit h: habitat h of the world's table is
// still on its list).  The winner's course: rows c[0..L-1] of 7 doubles as rrt_final_course writes them.
//   row 0      is replaced by `last`, all seven fields (the course starts at the committed state itself)
//   bucket     lo = last[4] + 0 * round_span, hi = last[4] + 1 * round_span
//   selection  row i iff lo <= t_i && t_i <= hi (a NaN time: never); the committed rows are the selected ones in course order
//   habitats   the selected rows in order: m = inside(x, y) & keep; if m != 0 its lowest bit leaves keep
//   inside     habitat h contains (x, y) iff RN(sqrt(dx*dx + dy*dy)) <= size_h, as the test d2 <= hab_t[h] on the squared
//              distance (world_tables.h: sq_threshold)
//   new state  last = the last selected row, keep as folded
#ifndef AUVP_REPLAN_COMMIT_H
#define AUVP_REPLAN_COMMIT_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AUVP_RC_FN __host__ __device__ inline
#else
#define AUVP_RC_FN inline
#endif

namespace auvp {

struct RrtGroupBest;  // (rrt_group_kernel.h)

constexpr int REPLAN_ROW = 7;       // doubles per course row
constexpr int REPLAN_MAX_HAB = 64;  // habitats a keep mask can name

struct ReplanBucket { double lo, hi; };

// splitPath's first edge, the same float operations as the Python: t0 + 0 * span, t0 + (0 + 1) * span
AUVP_RC_FN ReplanBucket replan_bucket(double t0, double round_span) {
  ReplanBucket b;
  b.lo = t0 + 0.0 * round_span;
  b.hi = t0 + 1.0 * round_span;
  return b;
}

AUVP_RC_FN bool replan_selected(const ReplanBucket& b, double t) { return b.lo <= t && t <= b.hi; }

// habitat h of the table hab [H,3] / hab_t [H] contains (x, y)
AUVP_RC_FN bool replan_inside(const double* hab, const double* hab_t, int h, double x, double y) {
  const double dx = x - hab[3 * h], dy = y - hab[3 * h + 1];
  const double d2 = dx * dx + dy * dy;
  return d2 <= hab_t[h];
}

// bit h: habitat h contains (x, y); H <= 64
AUVP_RC_FN uint64_t replan_inside_mask(const double* hab, const double* hab_t, int H, double x, double y) {
  uint64_t m = 0;
  for (int h = 0; h < H && h < REPLAN_MAX_HAB; h++)
    if (replan_inside(hab, hab_t, h, x, y)) m |= 1ull << h;
  return m;
}

// removeHabitat for one point: the first habitat still on the list that contains it leaves the list
AUVP_RC_FN uint64_t replan_keep_fold(uint64_t keep, uint64_t inside) {
  const uint64_t m = inside & keep;
  return m ? keep & ~(m & (0 - m)) : keep;
}

// field k of row i of the course as the rule reads it: row 0 is the committed state
AUVP_RC_FN double replan_row_field(const double* course, const double* last, int i, int k) {
  return i == 0 ? last[k] : course[(long long)REPLAN_ROW * i + k];
}

// The whole rule for one AUV, serially.  course [L,7] (L == 0: no winner, nothing is committed and nothing changes); last [7]
// and *keep are updated in place; sel [L] (may be null) gets 1 / 0 per row; rows_out [up to L,7] gets the committed rows,
// compacted and in order.  Returns the number of committed rows.
AUVP_RC_FN int replan_commit_course(const double* course, int L, double* last, uint64_t* keep, double round_span, const double* hab,
                                    const double* hab_t, int H, uint8_t* sel, double* rows_out) {
  const ReplanBucket b = replan_bucket(last[4], round_span);
  double start[REPLAN_ROW], end[REPLAN_ROW];
  for (int k = 0; k < REPLAN_ROW; k++) start[k] = end[k] = last[k];
  uint64_t kp = *keep;
  int n = 0;
  for (int i = 0; i < L; i++) {
    const bool s = replan_selected(b, replan_row_field(course, start, i, 4));
    if (sel) sel[i] = s ? 1 : 0;
    if (!s) continue;
    for (int k = 0; k < REPLAN_ROW; k++) {
      end[k] = replan_row_field(course, start, i, k);
      rows_out[(long long)REPLAN_ROW * n + k] = end[k];
    }
    if (kp != 0 && H > 0) kp = replan_keep_fold(kp, replan_inside_mask(hab, hab_t, H, end[0], end[1]));
    n++;
  }
  for (int k = 0; k < REPLAN_ROW; k++) last[k] = end[k];
  *keep = kp;
  return n;
}

// ---- what the kernel and its host side share ---------------------------------------------------------------------------

struct ReplanRecord {  // must match auvp_replan_record in include/auvplan.h
  int32_t status, winner, n_committed, path_len;
  double cost[4];
  double last[7];
  uint64_t keep;
  double _reserved[2];
};
static_assert(sizeof(ReplanRecord) == 128, "round record layout");

// one group of the round, as the HOST knows it before the launch: every index the kernel uses comes from here
struct ReplanSlot {
  int32_t auv;         // row of the state arrays, checked against [0, n_auvs)
  int32_t winner;      // episode of the batch, checked against [0, E); -1: nothing to commit
  int32_t path_len;    // rows of the winner's course (0: nothing to commit) -- the space reserved at course_off and log_off
  int32_t status;      // the group record's status
  int64_t course_off;  // first row of the course in the scratch buffer
  int64_t log_off;     // first row of the group's slot in the trajectory log
};

struct ReplanCommitDev {
  int32_t n_slots, H;
  const ReplanSlot* slots;   // [n_slots]
  const RrtGroupBest* best;  // [n_slots] the group records in HBM (cost); null: the probe
  double* course;            // scratch: the courses, [*,7]
  double* log;               // the committed rows, [*,7]
  double* last;              // [n_auvs,7] state, updated in place
  uint64_t* keep;            // [n_auvs]
  ReplanRecord* rec;         // [n_slots]
  const double* hab;         // [H,3]
  const double* hab_t;       // [H]
  double round_span;
};

// one piece of an AUV's trajectory in the log (auvp_replan_traj gathers them into AUV order)
struct ReplanSegment {
  int64_t src, dst;  // first row in the log / in the gathered trajectory
  int32_t n, _pad;
};

}  // namespace auvp
#endif  // AUVP_REPLAN_COMMIT_H

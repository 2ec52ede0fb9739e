// replan_apart.h -- RRT.replanning_batch(teams=..., team_separation=d): the winner selection that keeps the courses teammates
// commit in one round apart, as pure functions: no HIP in here, g++ alone compiles it (tests/host/replan_apart_check.cpp), and
// rrt_course_ticks_kernel and replan_team_pick_apart_kernel (replan_kernels.hip) are built from the same pieces.  The Python
// statement of the rule is rrt_dubins.course_ticks / tick_conflicts / team_pick_separated -- the definition this header matches
// bit for bit (built with -ffp-contract=off, as the library).
//
// A course, rows 0 .. L-1 root -> leaf (row 0: the AUV's committed state), is looked at on the ticks s * tick: between two points
// the AUV stays at the last one it reached, nothing is interpolated.
//   q_i     = ceil(t_i / tick), one division and a ceil in double
//   slot_i  = q_i - q_0 (exact in double), a negative one counts as 0; a NaN q_i has none; one above W - 1 (an infinite time
//             included) owns nothing but extends the table to W - 1
//   table   s_lo = q_0, n = max slot + 1 ticks; owner(j) = the LARGEST row with slot <= j (row 0 has slot 0: every tick has one);
//           xy[j] = the owner's position.  A q_0 that is no number inside int32: the empty table (n = 0)
//   n of a candidate against the trail (the tables of the winners the earlier members of its team chose in this round): its
//           ticks j at which some table of the trail covers s_lo + j and dx * dx + dy * dy < d * d there (a NaN never is)
//   winner  among the candidates with score < inf the smallest (n, score), the lowest tree among equals; its table joins the
//           trail.  The score is the tree's own cost[0], or replan_pick.h's under keep & ~claimed
#ifndef AUVP_REPLAN_APART_H
#define AUVP_REPLAN_APART_H
#include <stdint.h>

#include "replan_pick.h"

namespace auvp {

constexpr int REPLAN_APART_MAX_TICKS = 1024;  // W: the LDS tables of rrt_course_ticks_kernel (20 bytes per tick)
constexpr int REPLAN_APART_MAX_TEAM = 1024;   // members of a team: the winner list of replan_team_pick_apart_kernel in LDS

AUVP_RC_FN bool replan_apart_args_ok(double d, double tick, int W) {
  const double big = 1.7976931348623157e308;
  return d > 0.0 && d <= big && tick > 0.0 && tick <= big && W >= 1 && W <= REPLAN_APART_MAX_TICKS;
}

// the tick index of a time, as a double (NaN for a NaN time)
AUVP_RC_FN double replan_tick_q(double t, double tick) { return __builtin_ceil(t / tick); }

// q_0 can be a table's s_lo
AUVP_RC_FN bool replan_tick_base_ok(double q0) { return q0 > -2147483648.0 && q0 < 2147483648.0; }

// the slot of a row: -1: none (a NaN), W: beyond the window (owns nothing, extends the table to W - 1), else 0 .. W-1
AUVP_RC_FN int replan_tick_slot(double q, double q0, int W) {
  if (q != q) return -1;
  const double r = q - q0;
  if (r <= 0.0) return 0;
  if (r > (double)(W - 1)) return W;
  return (int)r;
}

// a table as the kernels keep it: head[0] = s_lo, head[1] = n, xy [n,2]
struct ReplanTicks {
  int32_t s_lo, n;
  const double* xy;
};

// the serial build (the host; the kernel: proposals by LDS atomic max, a prefix max, a second walk -- the same table).
// t / x / y: the rows' fields, `stride` doubles apart.  xy_out [W,2]; owner_tmp [W].  Returns n.
inline int replan_ticks_build(const double* t, const double* x, const double* y, int L, int stride, double tick, int W, int32_t* s_lo,
                              double* xy_out, int32_t* owner_tmp) {
  *s_lo = 0;
  if (L < 1) return 0;
  const double q0 = replan_tick_q(t[0], tick);
  if (!replan_tick_base_ok(q0)) return 0;
  for (int j = 0; j < W; j++) owner_tmp[j] = -1;
  int top = 0;
  for (int i = 0; i < L; i++) {
    const int s = replan_tick_slot(replan_tick_q(t[(size_t)i * stride], tick), q0, W);
    if (s < 0) continue;
    if (s >= W) { top = W - 1; continue; }
    if (s > top) top = s;
    if (i > owner_tmp[s]) owner_tmp[s] = i;
  }
  int cur = -1;
  for (int j = 0; j <= top; j++) {
    if (owner_tmp[j] > cur) cur = owner_tmp[j];
    xy_out[2 * j] = x[(size_t)cur * stride];
    xy_out[2 * j + 1] = y[(size_t)cur * stride];
  }
  *s_lo = (int32_t)q0;
  return top + 1;
}

// the distance test: plain differences, no contraction; false for a NaN
AUVP_RC_FN bool replan_apart_close(double ax, double ay, double bx, double by, double d2) {
  const double dx = ax - bx, dy = ay - by;
  return dx * dx + dy * dy < d2;
}

// the ticks first, first + stride, ... (< c.n) of candidate c that are in conflict with the trail of n_trail tables, table j being
// table_of(j).  The host takes (first = 0, stride = 1), lane l of the kernel's wavefront (l, 64); the lanes' counts add up.
template <class F>
AUVP_RC_FN int replan_apart_count(const ReplanTicks& c, int first, int stride, int n_trail, F&& table_of, double d2) {
  int hits = 0;
  for (int j = first; j < c.n; j += stride) {
    const double x = c.xy[2 * (size_t)j], y = c.xy[2 * (size_t)j + 1];
    bool hit = false;
    for (int w = 0; w < n_trail; w++) {
      const ReplanTicks tw = table_of(w);
      const int64_t at = (int64_t)c.s_lo + j - (int64_t)tw.s_lo;
      if (at < 0 || at >= (int64_t)tw.n) continue;
      hit = hit || replan_apart_close(x, y, tw.xy[2 * (size_t)at], tw.xy[2 * (size_t)at + 1], d2);
    }
    hits += hit ? 1 : 0;
  }
  return hits;
}

// the winner's fold over the trees in order: the smallest (n, score) among the scores < inf
struct ReplanApartBest {
  double best;  // the winner's score so far
  int32_t n;    // its conflicts
  int32_t k;    // -1: none
};
AUVP_RC_FN bool replan_apart_eligible(double score) { return score < __builtin_inf(); }
AUVP_RC_FN bool replan_apart_fold(ReplanApartBest& b, int n, double score, int k) {
  if (!(b.k < 0 || n < b.n || (n == b.n && score < b.best))) return false;
  b.best = score; b.n = n; b.k = k;
  return true;
}

// ---- the serial rule for one team (the host; the kernel runs the same steps with 64 lanes per candidate) ----------------------

struct ReplanApartCand {
  ReplanPickCand pick;  // path_len 0: the tree has no leaf; words only with claims
  double cost[4];       // the tree's own cost (the score without claims)
  ReplanTicks ticks;
};

struct ReplanApartOut {
  ReplanPickOut pick;
  int32_t conflicts, _pad;
};

// as replan_pick_team; trail_tmp: room for hi - lo candidate indices
inline void replan_apart_team(const int32_t* members, int lo, int hi, const int32_t* slot_of, const uint64_t* keep, int K,
                              const ReplanApartCand* cands, double w1, double w2, bool claims, double d, ReplanApartOut* out, int32_t* trail_tmp) {
  uint64_t claimed = 0;
  int n_trail = 0;
  const double d2 = d * d;
  for (int i = lo; i < hi; i++) {
    const int m = members[i], g = slot_of[m];
    if (g < 0) continue;
    const uint64_t mask = keep[m] & ~claimed;
    ReplanApartBest b{__builtin_inf(), 0, -1};
    ReplanApartOut r;
    r.pick.winner = -1; r.pick._pad = 0; r.pick.claimed = claimed; r.conflicts = 0; r._pad = 0;
    r.pick.cost[0] = r.pick.cost[1] = r.pick.cost[2] = r.pick.cost[3] = __builtin_inf();
    uint64_t vis_w = 0;
    for (int k = 0; k < K; k++) {
      const ReplanApartCand& c = cands[(size_t)g * (size_t)K + (size_t)k];
      if (c.pick.path_len <= 0) continue;
      double s[4] = {c.cost[0], c.cost[1], c.cost[2], c.cost[3]};
      uint64_t vis = 0;
      if (claims) {
        const ReplanPickHits hv = replan_pick_hits(c.pick.words, 0, c.pick.path_len, 1, mask);
        replan_pick_score(hv.hits, hv.vis, mask, w1, w2, c.pick.c2, c.pick.leaf_t, s);
        vis = hv.vis;
      }
      if (!replan_apart_eligible(s[0])) continue;
      const int n = replan_apart_count(c.ticks, 0, 1, n_trail, [&](int w) { return cands[(size_t)trail_tmp[w]].ticks; }, d2);
      if (replan_apart_fold(b, n, s[0], k)) {
        r.pick.cost[0] = s[0]; r.pick.cost[1] = s[1]; r.pick.cost[2] = s[2]; r.pick.cost[3] = s[3];
        vis_w = vis;
      }
    }
    r.pick.winner = b.k;
    r.conflicts = b.k >= 0 ? b.n : 0;
    if (b.k >= 0) trail_tmp[n_trail++] = (int32_t)((size_t)g * (size_t)K + (size_t)b.k);
    claimed |= vis_w;
    out[g] = r;
  }
}

// ---- what the kernels and their host side share -----------------------------------------------------------------------------

// rrt_course_ticks_kernel: one wavefront per episode; episode e's table is head[2e] = s_lo, head[2e + 1] = n, xy + e * W * 2
struct ReplanTicksDev {
  int32_t n_episodes, K, W;
  int32_t from_courses;   // 1: the probe, the courses are the caller's (xyt at off, len); 0: the batch's trees are walked
  double tick;
  const int32_t* auv_of;  // [n_episodes / K] the group's AUV (row of `last`); unused by the probe
  const double* last;     // [n_auvs,7]: row 0 of a course is the AUV's committed state; unused by the probe
  const int64_t* off;     // the probe: [n_episodes] first row of the course in xyt
  const double* xyt;      // the probe: the caller's courses [*,3]
  const int32_t* len;     // the probe: [n_episodes] course lengths (0: no leaf)
  int32_t* head;          // [n_episodes,2]
  double* xy;             // [n_episodes,W,2]
};

// replan_team_pick_apart_kernel: ReplanPickDev (words / off / stride / leaf_t read only with claims) and
struct ReplanApartDev {
  int32_t W, use_claims;
  double d2;
  const int32_t* head;  // as ReplanTicksDev, written by the launch before
  const double* xy;
  int32_t* conflicts;   // [n_slots] zeroed by the host; the members' get their winner's n
};

}  // namespace auvp
#endif  // AUVP_REPLAN_APART_H

// replan_pick.h -- the team-aware winner selection of RRT.replanning_batch(teams=..., team_pick="claims") as pure functions: no
// HIP in here, g++ alone compiles it (tests/host/replan_pick_check.cpp), and rrt_course_words_kernel and replan_team_pick_kernel
// (replan_kernels.hip) are built from the same pieces.  The Python statement of the rule is rrt_dubins.course_habitat_words /
// rescore / team_pick_claims -- the definition this header matches bit for bit (built with -ffp-contract=off, as the library).
//
// One team, per round: claimed = 0; the members that plan in this round in ascending AUV index.  Member m's K trees each offer
// their own best course (as the leaf pass ranked it under keep_m); each is scored under mask = keep_m & ~claimed:
//   word    of a course point: bit h iff habitat h contains it (replan_inside), 0 for a point whose time lies in none of the
//           candidate's selected shark bins (habitat_shark_cost_func skips such a point entirely)
//   hits    points with word & mask != 0; vis: the OR of the lowest bit of word & mask over them; H' = popcount(mask)
//   score   c0 = w1 * popcount(vis) / H' (0.0 if H' == 0), c1 from hits as total_of (rrt_leaf_body.h) computes it, c2 the
//           summary's shark term unchanged, total ((0.0 + c0) + c1) + c2
//   winner  the fold of rrt_group_best_kernel: score < best so far, from inf (the lowest tree among equals, never a NaN, never a
//           tree without a leaf); claimed |= the winner's vis, over its whole course
#ifndef AUVP_REPLAN_PICK_H
#define AUVP_REPLAN_PICK_H
#include <stdint.h>

#include "replan_commit.h"
#include "replan_teams.h"

namespace auvp {

struct RrtSummary;    // (auvp_types.h)
struct RrtGroupBest;  // (rrt_group_kernel.h)

// t lies in one of the bins lo .. hi-1 of bins [T,2] (closed intervals, as cost.py:174)
AUVP_RC_FN bool replan_pick_counted(const double* bins, int lo, int hi, double t) {
  bool in = false;
  for (int b = lo; b < hi; b++) in = in || (t >= bins[2 * b] && t <= bins[2 * b + 1]);
  return in;
}

// the per-point word: the containment mask of a counted point, 0 for a point in no selected bin
AUVP_RC_FN uint64_t replan_pick_word(const double* hab, const double* hab_t, int H, const double* bins, int lo, int hi, double x, double y,
                                     double t) {
  return replan_pick_counted(bins, lo, hi, t) ? replan_inside_mask(hab, hab_t, H, x, y) : 0ull;
}

struct ReplanPickHits {
  int32_t hits;
  uint64_t vis;
};

// hits / vis of words[first], words[first + stride], ... (< L) under mask: a counted point hits the lowest-numbered habitat of
// mask that contains it.  The host takes (first = 0, stride = 1), lane l of the kernel's wavefront (first = l, stride = 64); the
// lanes' results combine by an integer sum and an OR.
AUVP_RC_FN ReplanPickHits replan_pick_hits(const uint64_t* words, int first, int L, int stride, uint64_t mask) {
  ReplanPickHits r{0, 0ull};
  for (int i = first; i < L; i += stride) {
    const uint64_t m = words[i] & mask;
    if (m) { r.hits++; r.vis |= m & (0 - m); }
  }
  return r;
}

// cost [4] of a candidate from hits, vis, the mask it is judged by, its shark term c2 (already divided) and its leaf time: the
// float operations of total_of (rrt_leaf_body.h)
AUVP_RC_FN void replan_pick_score(int hits, uint64_t vis, uint64_t mask, double w1, double w2, double c2, double leaf_t, double* cost4) {
  const int H = __builtin_popcountll(mask);
  const bool w2_int = (w2 == __builtin_rint(w2) && __builtin_fabs(w2) < 1048576.0);
  double c0 = 0.0, c1 = 0.0;
  if (w2_int) c1 = 0.0 + w2 * (double)hits;
  else for (int h = 0; h < hits; h++) c1 = c1 + w2;
  if (leaf_t > 0) c1 = c1 / leaf_t;
  if (H != 0) c0 = w1 * (double)__builtin_popcountll(vis) / (double)H;
  cost4[0] = ((0.0 + c0) + c1) + c2;
  cost4[1] = c0; cost4[2] = c1; cost4[3] = c2;
}

// the winner's fold over the trees in order
struct ReplanPickBest {
  double best;  // from inf
  int32_t k;    // -1: none
};
AUVP_RC_FN bool replan_pick_fold(ReplanPickBest& b, double score, int k) {
  if (!(score < b.best)) return false;
  b.best = score; b.k = k;
  return true;
}

// ---- the serial rule for one team (the host; the kernel runs the same steps with 64 lanes per candidate) ----------------------

struct ReplanPickCand {
  int32_t path_len;       // words of the course; 0: the tree has no leaf
  int32_t _pad;
  const uint64_t* words;  // [path_len]
  double c2, leaf_t;
};

struct ReplanPickOut {
  int32_t winner;    // tree index, -1: none
  int32_t _pad;
  double cost[4];    // the winner's score (inf without one)
  uint64_t claimed;  // the mask the member saw
};

// members[lo .. hi-1] in order; slot_of[m] < 0: m does not plan in this round; member m's candidates are cands[slot_of[m] * K + k]
// and its result goes to out[slot_of[m]]
inline void replan_pick_team(const int32_t* members, int lo, int hi, const int32_t* slot_of, const uint64_t* keep, int K,
                             const ReplanPickCand* cands, double w1, double w2, ReplanPickOut* out) {
  uint64_t claimed = 0;
  for (int i = lo; i < hi; i++) {
    const int m = members[i], g = slot_of[m];
    if (g < 0) continue;
    const uint64_t mask = keep[m] & ~claimed;
    ReplanPickBest b{__builtin_inf(), -1};
    ReplanPickOut r;
    r.winner = -1; r._pad = 0; r.claimed = claimed;
    r.cost[0] = r.cost[1] = r.cost[2] = r.cost[3] = __builtin_inf();
    uint64_t vis_w = 0;
    for (int k = 0; k < K; k++) {
      const ReplanPickCand& c = cands[(size_t)g * (size_t)K + (size_t)k];
      if (c.path_len <= 0) continue;
      const ReplanPickHits hv = replan_pick_hits(c.words, 0, c.path_len, 1, mask);
      double s[4];
      replan_pick_score(hv.hits, hv.vis, mask, w1, w2, c.c2, c.leaf_t, s);
      if (replan_pick_fold(b, s[0], k)) {
        r.cost[0] = s[0]; r.cost[1] = s[1]; r.cost[2] = s[2]; r.cost[3] = s[3];
        vis_w = hv.vis;
      }
    }
    r.winner = b.k;
    claimed |= vis_w;
    out[g] = r;
  }
}

// ---- what the kernels and their host side share -----------------------------------------------------------------------------

constexpr int REPLAN_PICK_WAVES = 4;  // teams per workgroup of replan_team_pick_kernel (one wavefront each)

// rrt_course_words_kernel: one wavefront per episode.  Every offset comes from the host: episode e's words start at off[e], or
// at e * stride where off is null (stride: the host's bound on a course's length, from the batch's capacities).
struct ReplanWordsDev {
  int32_t n_episodes, K, H, n_bins;
  int32_t from_courses;    // 1: the probe, the courses are the caller's (xyt, len, off); 0: the batch's trees are walked
  int32_t _pad;
  int64_t stride;
  const int64_t* off;      // [n_episodes] or null
  const int32_t* auv_of;   // [n_episodes / K] the group's AUV (row of `last`), checked by the host; unused by the probe
  const double* last;      // [n_auvs,7]: row 0 of a course is the AUV's committed state; unused by the probe
  const double* xyt;       // the probe: the caller's courses [*,3] at the words' offsets (never read where every course is empty)
  const int32_t* len;      // the probe: [n_episodes] course lengths (0: no leaf)
  const int32_t* bin_lo;   // [n_episodes] the candidate's selected bins lo .. hi-1; null: every bin of the table
  const int32_t* bin_hi;
  const double* hab;       // [H,3]
  const double* hab_t;     // [H]
  const double* bins;      // [n_bins,2]
  uint64_t* words;
  double* leaf_t;          // [n_episodes] written when the trees are walked (the probe uploads it)
};

// replan_team_pick_kernel: one wavefront per team; member m's group is slot_of[m] (-1: not planning), its candidates the
// episodes slot_of[m] * K .. + K - 1
struct ReplanPickDev {
  int32_t n_teams, K, n_slots, _pad;
  const int32_t* team_off;     // [n_teams + 1]
  const int32_t* members;      // every entry inside keep's and slot_of's range (the host built them)
  const int32_t* slot_of;      // [n_auvs] entries -1 or inside [0, n_slots) (the host built them)
  const uint64_t* keep;        // [n_auvs]
  const RrtSummary* summary;   // [n_slots * K]
  const uint64_t* words;
  const int64_t* off;          // as ReplanWordsDev
  int64_t stride;
  const double* leaf_t;        // [n_slots * K]
  RrtGroupBest* best;          // [n_slots] rrt_group_best_kernel's records; the members' are rewritten
  uint64_t* claimed;           // [n_slots] zeroed by the host; the members' get the mask they saw
  double w1, w2;
};

}  // namespace auvp
#endif  // AUVP_REPLAN_PICK_H

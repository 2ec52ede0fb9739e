// rrt_group_kernel.h -- best-of-K planning: the episodes of a batch form groups (one AUV's K trees), and the winner of every
// group is chosen on the device, so that only the winners' courses leave HBM.
//
// The rule is exploring's own (path_planning/rrt_dubins.py:101,169): a leaf is kept only if new_cost[0] < opt_cost[0], starting
// from inf.  A group's winner is that fold over its members' best costs in member order: the lowest cost, the lowest episode
// index among equal (==) costs; a member without a leaf, or whose cost is a NaN, never wins.
#ifndef AUVP_RRT_GROUP_KERNEL_H
#define AUVP_RRT_GROUP_KERNEL_H
#include "auvp_types.h"
#include "auvp_wave.h"
#include "rrt_explore_kernel.h"

namespace auvp {

struct RrtGroupBest {  // must match auvp_rrt_group_best in include/auvplan.h
  int32_t status, winner, n_with_leaf, path_len;
  double cost[4];
  double length;
};

constexpr int RRT_GROUP_WAVES = 4;  // groups per workgroup of rrt_group_best_kernel

// wave-wide integer minimum / sum (identical on every lane on return; all 64 lanes active): four rotate steps inside the
// 16-lane rows on the DPP path, then the four row results -- as wave_min_f64
__device__ __forceinline__ int wave_min_i32(int v) {
  int t;
  t = __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false); v = t < v ? t : v;
  t = __builtin_amdgcn_update_dpp(0, v, 0x124, 0xf, 0xf, false); v = t < v ? t : v;
  t = __builtin_amdgcn_update_dpp(0, v, 0x122, 0xf, 0xf, false); v = t < v ? t : v;
  t = __builtin_amdgcn_update_dpp(0, v, 0x121, 0xf, 0xf, false); v = t < v ? t : v;
  const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16), c = __builtin_amdgcn_readlane(v, 32),
            d = __builtin_amdgcn_readlane(v, 48);
  const int ab = b < a ? b : a, cd = d < c ? d : c;
  return cd < ab ? cd : ab;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x124, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x122, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x121, 0xf, 0xf, false);
  return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
         __builtin_amdgcn_readlane(v, 48);
}

// One group per wavefront.  Lane l folds members group_off[g] + l, + 64, ... in ascending order (so a lane's best is its
// lowest-indexed minimum); the wave takes the minimum cost and, among the lanes whose best equals it, the lowest episode index
// (an integer minimum: lane order is not index order).  The record's path_len / cost / length are the winner's own summary.
static __global__ __launch_bounds__(RRT_GROUP_WAVES * 64) void rrt_group_best_kernel(const RrtSummary* __restrict__ summary,
                                                                                 const int32_t* __restrict__ group_off,
                                                                                 RrtGroupBest* __restrict__ out, int n_groups) {
  const int g = (int)blockIdx.x * RRT_GROUP_WAVES + (int)(threadIdx.x >> 6);
  if (g >= n_groups) return;  // (the whole wavefront)
  const int lane = lane_id();
  const int lo = group_off[g], hi = group_off[g + 1];
  constexpr int NONE = 0x7fffffff;
  double best = __builtin_inf();
  int best_ep = NONE, with_leaf = 0, failed_ep = NONE;
  for (int e = lo + lane; e < hi; e += 64) {
    const RrtSummary* s = summary + e;
    const int st = s->status, leaf = s->best_leaf;
    const double c = s->best_cost[0];
    if (leaf >= 0) {
      with_leaf++;
      if (c < best) { best = c; best_ep = e; }
    }
    if (st < 0 && failed_ep == NONE) failed_ep = e;
  }
  const double m = wave_min_f64(best);
  const int winner = wave_min_i32((best_ep != NONE && best == m) ? best_ep : NONE);
  const int n = wave_sum_i32(with_leaf);
  const int failed = wave_min_i32(failed_ep);
  if (lane == 0) {
    RrtGroupBest r;
    r.status = failed != NONE ? summary[failed].status : (winner != NONE ? 0 : 1 /* AUVP_NO_QUALIFYING_LEAF */);
    r.winner = winner != NONE ? winner : -1;
    r.n_with_leaf = n;
    r.path_len = 0;
    r.cost[0] = r.cost[1] = r.cost[2] = r.cost[3] = __builtin_inf();
    r.length = 0.0;
    if (winner != NONE) {
      const RrtSummary* s = summary + winner;
      r.path_len = s->best_path_len;
      r.cost[0] = s->best_cost[0]; r.cost[1] = s->best_cost[1]; r.cost[2] = s->best_cost[2]; r.cost[3] = s->best_cost[3];
      r.length = s->best_length;
    }
    out[g] = r;
  }
}

// the root -> leaf course of every group's winner at offsets[g] (one wavefront per group; nothing for a group without one)
static __global__ __launch_bounds__(64) void rrt_group_course_kernel(RrtBuffers B, const RrtGroupBest* __restrict__ best,
                                                              const int64_t* __restrict__ offsets, double* __restrict__ out,
                                                              int n_groups, int n_episodes) {
  const int g = blockIdx.x;
  if (g >= n_groups) return;
  const int ep = best[g].winner;
  if (ep < 0 || ep >= n_episodes) return;
  rrt_final_course(B, ep, out + 7 * (size_t)offsets[g]);
}

}  // namespace auvp
#endif

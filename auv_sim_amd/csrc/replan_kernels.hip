// replan_kernels.hip -- the kernels of the device commit step of RRT.replanning_batch (auvp_replan_*, include/auvplan.h) as a
// translation unit of their own, so that auvplan.hip's device code stays the text it was (leaf_grid_kernels.hip: why).
//
//   rrt_commit_kernel   one wavefront per group of the last auvp_rrt_group_best: the winner's course (rrt_final_course) into a
//                       scratch buffer, the commit rule of replan_commit.h on it, the committed rows into the trajectory log,
//                       the AUV's state (last, keep) in place, one round record
//   replan_gather_kernel  the log's pieces into AUV order, for the one download at the end
//   replan_team_kernel  one wavefront per team (replan_teams.h): every member's keep becomes the AND of the members' masks,
//                       in the state array and in the round's records
//   rrt_course_words_kernel, replan_team_pick_kernel  the team-aware winner selection (replan_pick.h), see below
//   rrt_course_ticks_kernel, replan_team_pick_apart_kernel  the selection that keeps teammates' courses apart (replan_apart.h)
//   replan_measure_kernel  the fleet's range / bearing measurements of its sharks from the committed states (replan_measure.h)
//   replan_measure_ticks_kernel  k such measurements per AUV along the bucket it committed last (replan_ticks.h)
//
// Entry points for the host side (replan_host.h): internal, hidden visibility, not part of the C-ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define AUVP_LEAF_KERNELS_ELSEWHERE 1  // (rrt_leaf_kernel / rrt_leaf_lim_kernel are auvplan.hip's)
#include "rrt_explore_kernel.h"
#include "rrt_group_kernel.h"
#include "replan_commit.h"
#include "replan_teams.h"
#include "replan_pick.h"
#include "replan_apart.h"
#include "rrt_course_walk.h"
#include "replan_measure.h"
#include "replan_ticks.h"
#include "auvp_math_late.h"

namespace auvp {

// The rule of replan_commit.h on the course of `L` rows at `course`, by one wavefront (all 64 lanes active, every argument the
// same on every lane).  The lanes take the rows 64 at a time: selection by ballot, the selected rows to `rows_out` at their
// rank.  The keep fold is serial over the selected rows: for each, lane h tests habitat h and the ballot is the row's
// inside-mask.  last [7] and *keep are read at the start and written by lane 0 at the end.  Returns the committed rows.
__device__ inline int replan_commit_wave(const double* __restrict__ course, int L, double* __restrict__ last_io, uint64_t* __restrict__ keep_io,
                                         double round_span, const double* __restrict__ hab, const double* __restrict__ hab_t, int H,
                                         double* __restrict__ rows_out, double* last_out7, uint64_t* keep_out) {
  const int lane = lane_id();
  double start[REPLAN_ROW], end[REPLAN_ROW];
#pragma unroll
  for (int k = 0; k < REPLAN_ROW; k++) start[k] = end[k] = last_io[k];
  const ReplanBucket b = replan_bucket(start[4], round_span);
  uint64_t kp = *keep_io;
  const bool in_table = lane < H;  // (H <= 64: one lane per habitat)
  int n = 0;
  for (int c = 0; c < L; c += 64) {
    const int i = c + lane;
    const bool valid = i < L;
    double row[REPLAN_ROW];
#pragma unroll
    for (int k = 0; k < REPLAN_ROW; k++) row[k] = valid ? replan_row_field(course, start, i, k) : 0.0;
    const bool s = valid && replan_selected(b, row[4]);
    const unsigned long long mask = __ballot(s ? 1 : 0);
    if (mask == 0) continue;  // (the same on every lane)
    if (s) {
      const int rank = __popcll(mask & ((1ull << lane) - 1ull));
      double* o = rows_out + (size_t)REPLAN_ROW * (size_t)(n + rank);
#pragma unroll
      for (int k = 0; k < REPLAN_ROW; k++) o[k] = row[k];
    }
    if (kp != 0 && H > 0) {
      for (unsigned long long m = mask; m != 0 && kp != 0; m &= m - 1) {
        const int j = __ffsll((long long)m) - 1;
        const double x = __shfl(row[0], j), y = __shfl(row[1], j);
        const unsigned long long inside = __ballot((in_table && replan_inside(hab, hab_t, lane, x, y)) ? 1 : 0);
        kp = replan_keep_fold(kp, inside);
      }
    }
    const int top = 63 - __clzll((long long)mask);
#pragma unroll
    for (int k = 0; k < REPLAN_ROW; k++) end[k] = __shfl(row[k], top);
    n += __popcll(mask);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < REPLAN_ROW; k++) last_io[k] = end[k];
    *keep_io = kp;
  }
#pragma unroll
  for (int k = 0; k < REPLAN_ROW; k++) last_out7[k] = end[k];
  *keep_out = kp;
  return n;
}

// One wavefront (= one workgroup) per slot.  PRODUCE: the course is the winner's, written here by rrt_final_course (the host
// reserved slot.path_len rows from its own copy of the group records; a summary that does not agree with that copy commits
// nothing and reports AUVP_ERR_STATE); otherwise the host put the course there (the probe entry).
template <bool PRODUCE>
static __global__ __launch_bounds__(64) void rrt_commit_kernel(RrtBuffers B, ReplanCommitDev A, int n_episodes) {
  const int g = blockIdx.x;
  if (g >= A.n_slots) return;
  const int lane = lane_id();
  const ReplanSlot slot = A.slots[g];
  int L = slot.path_len > 0 && slot.winner >= 0 ? slot.path_len : 0;
  int status = slot.status;
  double* course = A.course + (size_t)REPLAN_ROW * (size_t)slot.course_off;
  if (PRODUCE && L > 0) {
    const int ep = slot.winner;
    bool ok = ep < n_episodes;
    if (ok) {
      const RrtSummary* s = B.summary + ep;
      ok = s->best_leaf >= 0 && s->best_path_len == L;
    }
    if (ok) rrt_final_course(B, ep, course);
    else { L = 0; status = -4 /* AUVP_ERR_STATE */; }
  }
  __syncthreads();  // (the course's rows were written by other lanes of this wavefront)
  double fin[REPLAN_ROW];
  uint64_t fin_keep = 0;
  const int n = replan_commit_wave(course, L, A.last + (size_t)REPLAN_ROW * (size_t)slot.auv, A.keep + slot.auv, A.round_span, A.hab,
                                   A.hab_t, A.H, A.log + (size_t)REPLAN_ROW * (size_t)slot.log_off, fin, &fin_keep);
  if (lane == 0) {
    ReplanRecord r;
    r.status = status; r.winner = slot.winner; r.n_committed = n; r.path_len = slot.path_len;
    const double inf = __builtin_inf();
    r.cost[0] = r.cost[1] = r.cost[2] = r.cost[3] = inf;
    if (PRODUCE && A.best && slot.winner >= 0) {
      const RrtGroupBest* gb = A.best + g;
      r.cost[0] = gb->cost[0]; r.cost[1] = gb->cost[1]; r.cost[2] = gb->cost[2]; r.cost[3] = gb->cost[3];
    }
#pragma unroll
    for (int k = 0; k < REPLAN_ROW; k++) r.last[k] = fin[k];
    r.keep = fin_keep;
    r._reserved[0] = r._reserved[1] = 0.0;
    A.rec[g] = r;
  }
}

// segment s: n rows from log row src to trajectory row dst (one wavefront per segment, the doubles spread over the lanes)
static __global__ __launch_bounds__(64) void replan_gather_kernel(const ReplanSegment* __restrict__ seg, int n_seg, const double* __restrict__ log,
                                                                  double* __restrict__ out) {
  const int s = blockIdx.x;
  if (s >= n_seg) return;
  const ReplanSegment sg = seg[s];
  const double* from = log + (size_t)REPLAN_ROW * (size_t)sg.src;
  double* to = out + (size_t)REPLAN_ROW * (size_t)sg.dst;
  const int n = sg.n * REPLAN_ROW;
  for (int i = threadIdx.x; i < n; i += 64) to[i] = from[i];
}

// wave-wide AND of a 64-bit word (identical on every lane on return; all 64 lanes active): four rotate steps inside the 16-lane
// rows on the DPP path, each half of the word on its own, then the four row results -- as wave_min_i32
__device__ __forceinline__ uint64_t wave_and_u64(uint64_t v) {
  int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
  lo &= __builtin_amdgcn_update_dpp(0, lo, 0x128, 0xf, 0xf, false); hi &= __builtin_amdgcn_update_dpp(0, hi, 0x128, 0xf, 0xf, false);
  lo &= __builtin_amdgcn_update_dpp(0, lo, 0x124, 0xf, 0xf, false); hi &= __builtin_amdgcn_update_dpp(0, hi, 0x124, 0xf, 0xf, false);
  lo &= __builtin_amdgcn_update_dpp(0, lo, 0x122, 0xf, 0xf, false); hi &= __builtin_amdgcn_update_dpp(0, hi, 0x122, 0xf, 0xf, false);
  lo &= __builtin_amdgcn_update_dpp(0, lo, 0x121, 0xf, 0xf, false); hi &= __builtin_amdgcn_update_dpp(0, hi, 0x121, 0xf, 0xf, false);
  const int l = __builtin_amdgcn_readlane(lo, 0) & __builtin_amdgcn_readlane(lo, 16) & __builtin_amdgcn_readlane(lo, 32) &
                __builtin_amdgcn_readlane(lo, 48);
  const int h = __builtin_amdgcn_readlane(hi, 0) & __builtin_amdgcn_readlane(hi, 16) & __builtin_amdgcn_readlane(hi, 32) &
                __builtin_amdgcn_readlane(hi, 48);
  return ((uint64_t)(uint32_t)h << 32) | (uint32_t)l;
}

// The team fold of replan_teams.h: one wavefront per team of the CSR.  Lane l ANDs the masks of members l, l + 64, ... (a lane
// without a member holds all ones), the wavefront ANDs the lanes, and a second strided pass stores the team's list into every
// member's keep and, where the member has a record in this round, into that record.  Teams are disjoint: plain stores, no
// atomics.  Runs behind rrt_commit_kernel on the same stream, so every commit of the round is in keep when it reads.
static __global__ __launch_bounds__(REPLAN_TEAM_WAVES * 64) void replan_team_kernel(ReplanTeamDev T) {
  const int t = (int)blockIdx.x * REPLAN_TEAM_WAVES + (int)(threadIdx.x >> 6);
  if (t >= T.n_teams) return;  // (the whole wavefront)
  const int lane = lane_id();
  const int lo = T.team_off[t], hi = T.team_off[t + 1];
  const uint64_t k = wave_and_u64(replan_team_and(T.keep, T.members, lo + lane, hi, 64));
  for (int i = lo + lane; i < hi; i += 64) {
    const int m = T.members[i];
    T.keep[m] = k;
    if (T.slot_of) {
      const int s = T.slot_of[m];
      if (s >= 0) T.rec[s].keep = k;
    }
  }
}

// ---- team_pick="claims" (replan_pick.h) ----------------------------------------------------------------------------------------
//
// rrt_course_words_kernel: one wavefront (= one workgroup) per episode that has a leaf; one 64-bit word per point of its best
// course into a scratch buffer in HBM: the containment mask of a counted point, 0 for a point in no selected bin.  Row 0 is the
// AUV's committed state, as in the commit rule.  This is the parallel part of the selection: E * L * H distance tests with
// nothing dependent between them.  LANES OVER POINTS, the habitat table in LDS: the walk of the course already has a point per
// lane (a node's path points are spread over the lanes, as in rrt_final_course), so each lane tests its own point against the
// H table rows, which all lanes read at one LDS address (a broadcast, no bank conflict).  64 points cost H steps and no
// cross-lane operation; one lane per habitat against a broadcast point would cost 64 ballots for the same 64 points (more
// steps whenever H < 64 -- fleets here have about ten habitats) and a shuffle per point on top.
static __global__ __launch_bounds__(64) void rrt_course_words_kernel(RrtBuffers B, ReplanWordsDev A) {
  __shared__ double s_hab[REPLAN_MAX_HAB * 3], s_habt[REPLAN_MAX_HAB];
  const int ep = blockIdx.x;
  if (ep >= A.n_episodes) return;  // (the whole workgroup)
  const int lane = lane_id();
  const int H = A.H < REPLAN_MAX_HAB ? (A.H > 0 ? A.H : 0) : REPLAN_MAX_HAB;
  for (int i = lane; i < 3 * H; i += 64) s_hab[i] = A.hab[i];
  for (int i = lane; i < H; i += 64) s_habt[i] = A.hab_t[i];
  __syncthreads();
  int lo = A.bin_lo ? A.bin_lo[ep] : 0, hi = A.bin_hi ? A.bin_hi[ep] : A.n_bins;
  lo = lo < 0 ? 0 : lo;
  hi = hi > A.n_bins ? A.n_bins : hi;
  uint64_t* w = A.words + (A.off ? A.off[ep] : (int64_t)ep * A.stride);
  const double* bins = A.bins;
  if (A.from_courses) {  // the probe: the caller's course
    const int L = A.len[ep];
    const double* c = A.xyt + 3 * (size_t)A.off[ep];
    for (int i = lane; i < L; i += 64) w[i] = replan_pick_word(s_hab, s_habt, H, bins, lo, hi, c[3 * (size_t)i], c[3 * (size_t)i + 1], c[3 * (size_t)i + 2]);
    return;
  }
  const RrtSummary* s = B.summary + ep;
  const int L = s->best_path_len;
  if (s->best_leaf < 0 || L < 1 || (int64_t)L > A.stride) return;  // (a course longer than the host's bound: no words, and no candidate)
  const double* last = A.last + (size_t)REPLAN_ROW * (size_t)A.auv_of[ep / A.K];
  double* leaf_t = A.leaf_t + ep;
  rrt_course_walk_xyt(B, ep, [&](int at, double x, double y, double t) {
    if (at < 0 || at >= L) return;
    if (at == 0) { x = last[0]; y = last[1]; t = last[4]; }
    w[at] = replan_pick_word(s_hab, s_habt, H, bins, lo, hi, x, y, t);
    if (at == L - 1) *leaf_t = t;
  });
}

// wave-wide OR of a 64-bit word, as wave_and_u64
__device__ __forceinline__ uint64_t wave_or_u64(uint64_t v) {
  int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
  lo |= __builtin_amdgcn_update_dpp(0, lo, 0x128, 0xf, 0xf, false); hi |= __builtin_amdgcn_update_dpp(0, hi, 0x128, 0xf, 0xf, false);
  lo |= __builtin_amdgcn_update_dpp(0, lo, 0x124, 0xf, 0xf, false); hi |= __builtin_amdgcn_update_dpp(0, hi, 0x124, 0xf, 0xf, false);
  lo |= __builtin_amdgcn_update_dpp(0, lo, 0x122, 0xf, 0xf, false); hi |= __builtin_amdgcn_update_dpp(0, hi, 0x122, 0xf, 0xf, false);
  lo |= __builtin_amdgcn_update_dpp(0, lo, 0x121, 0xf, 0xf, false); hi |= __builtin_amdgcn_update_dpp(0, hi, 0x121, 0xf, 0xf, false);
  const int l = __builtin_amdgcn_readlane(lo, 0) | __builtin_amdgcn_readlane(lo, 16) | __builtin_amdgcn_readlane(lo, 32) |
                __builtin_amdgcn_readlane(lo, 48);
  const int h = __builtin_amdgcn_readlane(hi, 0) | __builtin_amdgcn_readlane(hi, 16) | __builtin_amdgcn_readlane(hi, 32) |
                __builtin_amdgcn_readlane(hi, 48);
  return ((uint64_t)(uint32_t)h << 32) | (uint32_t)l;
}

// replan_team_pick_kernel: one wavefront per team of the CSR.  The members run serially -- the rule's own dependence: a member
// is judged by what the members before it claimed.  Per candidate the lanes stride over its words (replan_pick_hits), one wave
// reduction follows (an integer sum and a 64-bit OR), and every lane computes the score and the fold on the same numbers.  Runs
// behind rrt_group_best_kernel and rrt_course_words_kernel on the same stream: it rewrites winner, path_len, cost and length of
// the members' group records (status: a failed member's stays; n_with_leaf stays) and leaves every other group's record alone.
// Teams are disjoint: plain stores.
static __global__ __launch_bounds__(REPLAN_PICK_WAVES * 64) void replan_team_pick_kernel(ReplanPickDev T) {
  const int t = (int)blockIdx.x * REPLAN_PICK_WAVES + (int)(threadIdx.x >> 6);
  if (t >= T.n_teams) return;  // (the whole wavefront)
  const int lane = lane_id();
  const int lo = T.team_off[t], hi = T.team_off[t + 1];
  const double inf = __builtin_inf();
  uint64_t claimed = 0;
  for (int i = lo; i < hi; i++) {
    const int m = T.members[i];
    const int g = T.slot_of[m];
    if (g < 0 || g >= T.n_slots) continue;  // (not planning in this round; the same on every lane)
    const uint64_t mask = T.keep[m] & ~claimed;
    ReplanPickBest b{inf, -1};
    double cost[4] = {inf, inf, inf, inf};
    uint64_t vis_w = 0;
    for (int k = 0; k < T.K; k++) {
      const int ep = g * T.K + k;
      const RrtSummary* s = T.summary + ep;
      const int L = s->best_path_len;
      if (s->best_leaf < 0 || L < 1 || (!T.off && (int64_t)L > T.stride)) continue;  // (the same on every lane)
      const uint64_t* w = T.words + (T.off ? T.off[ep] : (int64_t)ep * T.stride);
      const ReplanPickHits hv = replan_pick_hits(w, lane, L, 64, mask);
      const int hits = wave_sum_i32(hv.hits);
      const uint64_t vis = wave_or_u64(hv.vis);
      double sc[4];
      replan_pick_score(hits, vis, mask, T.w1, T.w2, s->best_cost[3], T.leaf_t[ep], sc);
      if (replan_pick_fold(b, sc[0], k)) {
        cost[0] = sc[0]; cost[1] = sc[1]; cost[2] = sc[2]; cost[3] = sc[3];
        vis_w = vis;
      }
    }
    if (lane == 0) {
      RrtGroupBest r = T.best[g];
      if (r.status >= 0) r.status = b.k >= 0 ? 0 : 1 /* AUVP_NO_QUALIFYING_LEAF */;
      r.winner = b.k >= 0 ? g * T.K + b.k : -1;
      r.path_len = 0;
      r.length = 0.0;
      if (b.k >= 0) {
        const RrtSummary* s = T.summary + (g * T.K + b.k);
        r.path_len = s->best_path_len;
        r.length = s->best_length;
      }
      r.cost[0] = cost[0]; r.cost[1] = cost[1]; r.cost[2] = cost[2]; r.cost[3] = cost[3];
      T.best[g] = r;
      T.claimed[g] = claimed;
    }
    claimed |= vis_w;
  }
}

// ---- team_separation (replan_apart.h) ------------------------------------------------------------------------------------------
//
// rrt_course_ticks_kernel: one wavefront (= one workgroup) per candidate episode; its tick table (s_lo, n, xy [n,2]) into a
// scratch buffer in HBM.  This is the parallel part: E courses with nothing dependent between them.  The walk of the course has
// every row on exactly one lane and a row needs no neighbour: it proposes its index for its own tick with an LDS atomic max
// (the largest row of a tick owns it); a second walk lets the row that won its tick deposit its position there; a prefix max
// over the ticks, 64 at a time, then gives every tick its owner -- the key is (row << 32 | tick the row proposed), so the
// position is read from the owner's own tick.  LDS: W * (4 + 16) bytes, at most 20 KB.  An episode without a leaf, or one whose
// row 0 has no tick inside int32, gets the empty table.
static __global__ __launch_bounds__(64) void rrt_course_ticks_kernel(RrtBuffers B, ReplanTicksDev A) {
  __shared__ int s_prop[REPLAN_APART_MAX_TICKS];
  __shared__ double s_xy[2 * REPLAN_APART_MAX_TICKS];
  __shared__ int s_top;
  const int ep = blockIdx.x;
  if (ep >= A.n_episodes) return;  // (the whole workgroup)
  const int lane = lane_id();
  const int W = A.W < REPLAN_APART_MAX_TICKS ? (A.W > 1 ? A.W : 1) : REPLAN_APART_MAX_TICKS;
  const double tick = A.tick;
  int32_t* head = A.head + 2 * (size_t)ep;
  double* out = A.xy + 2 * (size_t)ep * (size_t)A.W;
  int L = 0;
  const double* c = nullptr;     // the probe: the caller's course
  const double* last = nullptr;  // the batch: the AUV's committed state
  if (A.from_courses) {
    L = A.len[ep];
    c = A.xyt + 3 * (size_t)A.off[ep];
  } else {
    const RrtSummary* s = B.summary + ep;
    L = s->best_leaf >= 0 ? s->best_path_len : 0;
    last = A.last + (size_t)REPLAN_ROW * (size_t)A.auv_of[ep / A.K];
  }
  const double q0 = L >= 1 ? replan_tick_q(A.from_courses ? c[2] : last[4], tick) : __builtin_nan("");
  if (!replan_tick_base_ok(q0)) {  // (the same on every lane)
    if (lane == 0) { head[0] = 0; head[1] = 0; }
    return;
  }
  for (int j = lane; j < W; j += 64) s_prop[j] = -1;
  if (lane == 0) s_top = 0;
  __syncthreads();
  int top = 0;
  auto slot_of = [&](double t) { return replan_tick_slot(replan_tick_q(t, tick), q0, W); };
  auto propose = [&](int at, double t) {
    const int s = slot_of(t);
    if (s < 0) return;
    if (s >= W) { top = W - 1; return; }
    top = s > top ? s : top;
    atomicMax(&s_prop[s], at);
  };
  auto deposit = [&](int at, double x, double y, double t) {
    const int s = slot_of(t);
    if (s < 0 || s >= W || s_prop[s] != at) return;
    s_xy[2 * s] = x; s_xy[2 * s + 1] = y;
  };
  if (A.from_courses) {
    for (int i = lane; i < L; i += 64) propose(i, c[3 * (size_t)i + 2]);
  } else {
    rrt_course_walk_xyt(B, ep, [&](int at, double x, double y, double t) {
      if (at < 0 || at >= L) return;
      propose(at, at == 0 ? last[4] : t);
    });
  }
  atomicMax(&s_top, top);
  __syncthreads();
  if (A.from_courses) {
    for (int i = lane; i < L; i += 64) deposit(i, c[3 * (size_t)i], c[3 * (size_t)i + 1], c[3 * (size_t)i + 2]);
  } else {
    rrt_course_walk_xyt(B, ep, [&](int at, double x, double y, double t) {
      if (at < 0 || at >= L) return;
      if (at == 0) { x = last[0]; y = last[1]; t = last[4]; }
      deposit(at, x, y, t);
    });
  }
  __syncthreads();
  top = s_top;
  long long carry = -1;
  for (int base = 0; base <= top; base += 64) {  // (every lane takes every trip: top is the same on all)
    const int j = base + lane;
    const int p = j <= top ? s_prop[j] : -1;
    long long key = p >= 0 ? ((long long)p << 32) | (long long)j : -1;
    for (int o = 1; o < 64; o <<= 1) {
      const long long u = __shfl_up(key, o);
      if (lane >= o && u > key) key = u;
    }
    if (carry > key) key = carry;
    carry = __shfl(key, 63);
    if (j <= top && key >= 0) {  // (row 0 proposes tick 0: every tick has an owner)
      const int src = (int)(key & 0xffffffffll);
      out[2 * (size_t)j] = s_xy[2 * src]; out[2 * (size_t)j + 1] = s_xy[2 * src + 1];
    }
  }
  if (lane == 0) { head[0] = (int32_t)q0; head[1] = top + 1; }
}

// replan_team_pick_apart_kernel: replan_team_pick_kernel's sibling for team_separation -- one wavefront per team, the members
// serial; that kernel stays what it is.  A candidate's score is the tree's own cost or, with use_claims, the one under the
// claims exactly as there.  Per eligible candidate the lanes stride over its ticks (replan_apart_count) and read, for every
// earlier winner of the team, that winner's table at the same tick -- contiguous across the lanes, no dependent chain --, one
// wave sum gives n, and every lane folds the same numbers.  The earlier winners' episodes are a wave-private list in LDS
// (lane 0 appends, wave_sync orders it for the other lanes).  Through global memory the kernel reads only what an EARLIER launch
// wrote -- the tables (rrt_course_ticks_kernel), the words, the summaries, the group records (which lane 0 reads and rewrites
// itself) --, never what another lane of this launch stored: so the L1-cached loads need no acquire / release handling here.
static __global__ __launch_bounds__(REPLAN_PICK_WAVES * 64) void replan_team_pick_apart_kernel(ReplanPickDev T, ReplanApartDev A) {
  __shared__ int32_t s_trail[REPLAN_PICK_WAVES][REPLAN_APART_MAX_TEAM];
  const int t = (int)blockIdx.x * REPLAN_PICK_WAVES + (int)(threadIdx.x >> 6);
  if (t >= T.n_teams) return;  // (the whole wavefront)
  const int lane = lane_id();
  int32_t* trail = s_trail[threadIdx.x >> 6];
  const int lo = T.team_off[t], hi = T.team_off[t + 1];
  const double inf = __builtin_inf();
  const size_t table = 2 * (size_t)A.W;
  auto table_of = [&](int ep) { return ReplanTicks{A.head[2 * (size_t)ep], A.head[2 * (size_t)ep + 1], A.xy + table * (size_t)ep}; };
  uint64_t claimed = 0;
  int n_trail = 0;
  for (int i = lo; i < hi; i++) {
    const int m = T.members[i];
    const int g = T.slot_of[m];
    if (g < 0 || g >= T.n_slots) continue;  // (not planning in this round; the same on every lane)
    const uint64_t mask = T.keep[m] & ~claimed;
    ReplanApartBest b{inf, 0, -1};
    double cost[4] = {inf, inf, inf, inf};
    uint64_t vis_w = 0;
    for (int k = 0; k < T.K; k++) {
      const int ep = g * T.K + k;
      const RrtSummary* s = T.summary + ep;
      const int L = s->best_path_len;
      if (s->best_leaf < 0 || L < 1) continue;  // (the same on every lane)
      double sc[4] = {s->best_cost[0], s->best_cost[1], s->best_cost[2], s->best_cost[3]};
      uint64_t vis = 0;
      if (A.use_claims) {
        if (!T.off && (int64_t)L > T.stride) continue;
        const uint64_t* w = T.words + (T.off ? T.off[ep] : (int64_t)ep * T.stride);
        const ReplanPickHits hv = replan_pick_hits(w, lane, L, 64, mask);
        const int hits = wave_sum_i32(hv.hits);
        vis = wave_or_u64(hv.vis);
        replan_pick_score(hits, vis, mask, T.w1, T.w2, s->best_cost[3], T.leaf_t[ep], sc);
      }
      if (!replan_apart_eligible(sc[0])) continue;
      const int n = wave_sum_i32(replan_apart_count(table_of(ep), lane, 64, n_trail, [&](int w) { return table_of(trail[w]); }, A.d2));
      if (replan_apart_fold(b, n, sc[0], k)) {
        cost[0] = sc[0]; cost[1] = sc[1]; cost[2] = sc[2]; cost[3] = sc[3];
        vis_w = vis;
      }
    }
    if (lane == 0) {
      RrtGroupBest r = T.best[g];
      if (r.status >= 0) r.status = b.k >= 0 ? 0 : 1 /* AUVP_NO_QUALIFYING_LEAF */;
      r.winner = b.k >= 0 ? g * T.K + b.k : -1;
      r.path_len = 0;
      r.length = 0.0;
      if (b.k >= 0) {
        const RrtSummary* s = T.summary + (g * T.K + b.k);
        r.path_len = s->best_path_len;
        r.length = s->best_length;
      }
      r.cost[0] = cost[0]; r.cost[1] = cost[1]; r.cost[2] = cost[2]; r.cost[3] = cost[3];
      T.best[g] = r;
      T.claimed[g] = claimed;
      A.conflicts[g] = b.k >= 0 ? b.n : 0;
    }
    if (b.k >= 0 && n_trail < REPLAN_APART_MAX_TEAM) {  // (the host refuses a larger team)
      if (lane == 0) trail[n_trail] = g * T.K + b.k;
      n_trail++;
      wave_sync();
    }
    claimed |= vis_w;
  }
}

// ---- measurements from the committed states (replan_measure.h) -----------------------------------------------------------------
//
// One lane per row (f, a) of meas [F][A][5]: the AUV's x, y, theta from the fleet's state array, the shark's position, and the
// row's five doubles with plain stores.  members and n come from the host (replan_measure_members: every AUV index inside the
// fleet).  The square root is pf_step_kernel's (auvp_sqrt_plain); so is the atan2 (auvp_atan2_late), whose value
// replan_atan2_round then rounds correctly -- the host definition is math.atan2 (replan_measure.h).
constexpr int REPLAN_MEAS_THREADS = 64;
static __global__ __launch_bounds__(REPLAN_MEAS_THREADS) void replan_measure_kernel(ReplanMeasureDev M) {
  const int i = (int)blockIdx.x * REPLAN_MEAS_THREADS + (int)threadIdx.x;
  if (i >= M.n) return;
  const int f = i / M.A;
  const double* last = M.last + (size_t)REPLAN_ROW * (size_t)M.members[i];
  const double x = last[0], y = last[1], theta = last[2];
  const double dx = M.shark_xy[2 * (size_t)f] - x, dy = M.shark_xy[2 * (size_t)f + 1] - y;
  double* o = M.meas + (size_t)REPLAN_MEAS_ROW * (size_t)i;
  o[0] = x; o[1] = y; o[2] = theta;
  o[3] = auvp_sqrt_plain(dx * dx + dy * dy);
  o[4] = replan_atan2_round(dy, dx, auvp_atan2_late(dy, dx)) - theta;
}

// ---- k measurements along the last committed bucket (replan_ticks.h) --------------------------------------------------------------
//
// One wavefront per row group (f, a) of meas [k][F][A][5], that is per AUV; REPLAN_MEAS_TICKS_WAVES of them per workgroup, which
// share nothing (no LDS, no barrier).  seg, members and k come from the host (replan_ticks_plan: every row inside the log, every
// AUV inside the fleet, 1 <= k <= 64).
//   row search   lane j holds tau_j.  The lanes take the segment's row times 64 at a time, one row each; for every tick a vote
//                over the chunk (t_i <= tau_j) is the wave-wide reduction: the greatest qualifying index of the chunk is the
//                vote's top bit, and lane j keeps it.  The chunks ascend, so a later one overrides: the greatest index of the
//                whole segment, with no assumption on the order of the times.  n / 64 loads per lane and k votes per chunk --
//                a per-tick max over strided lane-local candidates would read every time k times for the same answer.
//   row compute  lanes 0 .. k-1, one tick each: replan_measure_kernel's five doubles from the chosen row (the AUV's state where
//                the segment is empty) -- the bearing's double-double correction on up to 64 lanes at once.
//   stores       plain vector stores, step-major: row (j, f, a) at ((j * F + f) * A + a) * 5.
static __global__ __launch_bounds__(REPLAN_MEAS_TICKS_WAVES * 64) void replan_measure_ticks_kernel(ReplanMeasTicksDev M) {
  const int i = (int)blockIdx.x * REPLAN_MEAS_TICKS_WAVES + (int)(threadIdx.x >> 6);
  if (i >= M.n) return;  // (the whole wavefront)
  const int lane = lane_id();
  const int k = M.k;
  const ReplanMeasSeg sg = M.seg[i];
  const double* seg = M.log + (size_t)REPLAN_ROW * (size_t)sg.off;
  int best = 0;
  if (sg.n > 0) {  // (the same on every lane)
    const double tau = replan_meas_tick_time(seg[4], M.round_span, k, lane < k ? lane : k - 1);
    for (int c = 0; c < sg.n; c += 64) {
      const int r = c + lane;
      const bool valid = r < sg.n;
      const double t = valid ? seg[(size_t)REPLAN_ROW * (size_t)r + 4] : 0.0;
      for (int j = 0; j < k; j++) {
        const double tau_j = __shfl(tau, j);  // (by every lane: outside the vote's condition)
        const unsigned long long mask = wave_ballot(valid && replan_meas_tick_reached(t, tau_j));
        if (mask != 0 && lane == j) best = c + 63 - __clzll((long long)mask);
      }
    }
  }
  if (lane >= k) return;
  const double* src = sg.n > 0 ? seg + (size_t)REPLAN_ROW * (size_t)best : M.last + (size_t)REPLAN_ROW * (size_t)M.members[i];
  const int f = i / M.A, F = M.n / M.A;
  const double* shark = M.shark_xy + 2 * ((size_t)lane * (size_t)F + (size_t)f);
  const double x = src[0], y = src[1], theta = src[2];
  const double dx = shark[0] - x, dy = shark[1] - y;
  double* o = M.meas + (size_t)REPLAN_MEAS_ROW * ((size_t)lane * (size_t)M.n + (size_t)i);
  o[0] = x; o[1] = y; o[2] = theta;
  o[3] = auvp_sqrt_plain(dx * dx + dy * dy);
  o[4] = replan_atan2_round(dy, dx, auvp_atan2_late(dy, dx)) - theta;
}

}  // namespace auvp

extern "C" __attribute__((visibility("hidden"))) hipError_t auvpi_replan_measure_ticks_launch(const auvp::ReplanMeasTicksDev* M, hipStream_t stream) {
  if (M->n <= 0 || M->A <= 0 || !auvp::replan_meas_ticks_ok(M->k)) return hipSuccess;
  const int blocks = (M->n + auvp::REPLAN_MEAS_TICKS_WAVES - 1) / auvp::REPLAN_MEAS_TICKS_WAVES;
  hipLaunchKernelGGL(auvp::replan_measure_ticks_kernel, dim3(blocks), dim3(auvp::REPLAN_MEAS_TICKS_WAVES * 64), 0, stream, *M);
  return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t auvpi_replan_measure_launch(const auvp::ReplanMeasureDev* M, hipStream_t stream) {
  if (M->n <= 0) return hipSuccess;
  const int blocks = (M->n + auvp::REPLAN_MEAS_THREADS - 1) / auvp::REPLAN_MEAS_THREADS;
  hipLaunchKernelGGL(auvp::replan_measure_kernel, dim3(blocks), dim3(auvp::REPLAN_MEAS_THREADS), 0, stream, *M);
  return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t auvpi_replan_ticks_launch(const auvp::RrtBuffers* B, const auvp::ReplanTicksDev* A,
                                                                                      hipStream_t stream) {
  if (A->n_episodes <= 0) return hipSuccess;
  hipLaunchKernelGGL(auvp::rrt_course_ticks_kernel, dim3(A->n_episodes), dim3(64), 0, stream, B ? *B : auvp::RrtBuffers{}, *A);
  return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t auvpi_replan_pick_apart_launch(const auvp::ReplanPickDev* T, const auvp::ReplanApartDev* A,
                                                                                           hipStream_t stream) {
  if (T->n_teams <= 0) return hipSuccess;
  const int blocks = (T->n_teams + auvp::REPLAN_PICK_WAVES - 1) / auvp::REPLAN_PICK_WAVES;
  hipLaunchKernelGGL(auvp::replan_team_pick_apart_kernel, dim3(blocks), dim3(auvp::REPLAN_PICK_WAVES * 64), 0, stream, *T, *A);
  return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t auvpi_replan_words_launch(const auvp::RrtBuffers* B, const auvp::ReplanWordsDev* A,
                                                                                      hipStream_t stream) {
  if (A->n_episodes <= 0) return hipSuccess;
  hipLaunchKernelGGL(auvp::rrt_course_words_kernel, dim3(A->n_episodes), dim3(64), 0, stream, B ? *B : auvp::RrtBuffers{}, *A);
  return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t auvpi_replan_pick_launch(const auvp::ReplanPickDev* T, hipStream_t stream) {
  if (T->n_teams <= 0) return hipSuccess;
  const int blocks = (T->n_teams + auvp::REPLAN_PICK_WAVES - 1) / auvp::REPLAN_PICK_WAVES;
  hipLaunchKernelGGL(auvp::replan_team_pick_kernel, dim3(blocks), dim3(auvp::REPLAN_PICK_WAVES * 64), 0, stream, *T);
  return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t auvpi_replan_team_launch(const auvp::ReplanTeamDev* T, hipStream_t stream) {
  if (T->n_teams <= 0) return hipSuccess;
  const int blocks = (T->n_teams + auvp::REPLAN_TEAM_WAVES - 1) / auvp::REPLAN_TEAM_WAVES;
  hipLaunchKernelGGL(auvp::replan_team_kernel, dim3(blocks), dim3(auvp::REPLAN_TEAM_WAVES * 64), 0, stream, *T);
  return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t auvpi_replan_commit_launch(const auvp::RrtBuffers* B, const auvp::ReplanCommitDev* A,
                                                                                       int n_episodes, hipStream_t stream) {
  if (A->n_slots <= 0) return hipSuccess;
  if (B) hipLaunchKernelGGL(auvp::rrt_commit_kernel<true>, dim3(A->n_slots), dim3(64), 0, stream, *B, *A, n_episodes);
  else hipLaunchKernelGGL(auvp::rrt_commit_kernel<false>, dim3(A->n_slots), dim3(64), 0, stream, auvp::RrtBuffers{}, *A, 0);
  return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t auvpi_replan_gather_launch(const auvp::ReplanSegment* seg, int n_seg, const double* log,
                                                                                       double* out, hipStream_t stream) {
  if (n_seg <= 0) return hipSuccess;
  hipLaunchKernelGGL(auvp::replan_gather_kernel, dim3(n_seg), dim3(64), 0, stream, seg, n_seg, log, out);
  return hipGetLastError();
}

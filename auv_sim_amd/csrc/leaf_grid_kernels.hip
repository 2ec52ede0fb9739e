// leaf_grid_kernels.hip -- the kernels of the probability sets (auvp_world_set_prob_sets, auvp_rrt_set_episode_grids) as a
// translation unit of their own: rrt_leaf_grid_kernel, the leaf pass of a batch whose episodes each rank their leaves against
// their own shark-occupancy table, prob_set_stats_kernel, the two constants of the leaf pass's error bound per table, and
// sf_place_kernel, which fills the sets from a forecast whose rounds start at a later bin than the planner's first.
//
// Why its own unit: rrt_leaf_kernel and rrt_leaf_lim_kernel (auvplan.hip) are sensitive to their build context (rows_kernels.hip
// records 11 % from a scheduling flag alone); a third instance of rrt_leaf_body.h beside them could move their register
// allocation.  Here it cannot: auvplan.hip's device code is the same text as before, and the body's added lines are behind
// AUVP_LEAF_GRID, which only this file defines.
//
// Entry points for the host side (auvplan.hip): internal, hidden visibility, not part of the C-ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define AUVP_LEAF_KERNELS_ELSEWHERE 1  // (rrt_leaf_kernel / rrt_leaf_lim_kernel are auvplan.hip's)
#include "rrt_explore_kernel.h"
#include "forecast_place.h"

namespace auvp {

// The leaf pass with LIM semantics (the episode's own threshold and habitat list, rrt_leaf_lim_kernel) and, per episode, the
// table sets[set_of[ep]] in place of the world's: its base pointer and its own prob_absmax / prob_one_sign -- the approximate-cost
// bound is only rigorous with the constants of the table the terms come from.
static __global__ __launch_bounds__(RRT_LEAF_WAVES * 64) __attribute__((amdgpu_waves_per_eu(AUVP_LEAF_WPE, AUVP_LEAF_WPE))) void rrt_leaf_grid_kernel(
    WorldDev W, RrtParamsDev P, RrtBuffers B, int n_episodes, int mark_words, const RrtEpisodeLimDev* __restrict__ lim,
    const int32_t* __restrict__ set_of, const RrtProbSetDev* __restrict__ sets) {
  constexpr bool LIM = true;
#define AUVP_LEAF_GRID 1
#include "rrt_leaf_body.h"
#undef AUVP_LEAF_GRID
}

// What auvp_world_set computes on the host for its one table, per set, one workgroup each: absmax = nan if any entry is a nan,
// else max |p| (a maximum: the same double in any order); one_sign = 1 unless there is a nan or both signs occur.  Also fills
// in the set's base pointer.  prob [G][n] with n = T * C.
constexpr int PROB_STATS_THREADS = 256;
static __global__ __launch_bounds__(PROB_STATS_THREADS) void prob_set_stats_kernel(const double* __restrict__ prob, long long n,
                                                                                  RrtProbSetDev* __restrict__ sets) {
  __shared__ double s_max[PROB_STATS_THREADS];
  __shared__ int s_flags[PROB_STATS_THREADS];  // 1: a positive entry, 2: a negative one, 4: a nan
  const double* p = prob + (size_t)blockIdx.x * (size_t)n;
  double mx = 0.0;
  int fl = 0;
  for (long long i = threadIdx.x; i < n; i += PROB_STATS_THREADS) {
    const double v = p[i], a = auvp_fabs(v);
    mx = a > mx ? a : mx;
    fl |= (v > 0 ? 1 : 0) | (v < 0 ? 2 : 0) | (v != v ? 4 : 0);
  }
  s_max[threadIdx.x] = mx;
  s_flags[threadIdx.x] = fl;
  __syncthreads();
  for (int o = PROB_STATS_THREADS / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double t = s_max[threadIdx.x + o];
      if (t > s_max[threadIdx.x]) s_max[threadIdx.x] = t;
      s_flags[threadIdx.x] |= s_flags[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int f = s_flags[0];
    RrtProbSetDev r;
    r.prob = p;
    r.absmax = (f & 4) ? __builtin_nan("") : s_max[0];
    r.one_sign = (!(f & 4) && (f & 3) != 3) ? 1 : 0;
    r._pad = 0;
    sets[blockIdx.x] = r;
  }
}

// The sets [F][T][C] from a forecast's prob [F][R1][C] (forecast_place.h): one workgroup per row (f, t), which copies the C doubles
// of forecast round placed_round(t, first_bin, R1 - 1).  Sixteen bytes per lane and trip where the two rows have the same phase
// against a 16-byte boundary (always with an even C; with an odd C every other row of either side starts on an odd element, so
// one element is peeled in front and / or left behind); element by element where the phases differ.  Plain vector loads and
// stores; rows are disjoint.
constexpr int SF_PLACE_THREADS = 256;
static __global__ __launch_bounds__(SF_PLACE_THREADS) void sf_place_kernel(const double* __restrict__ src, double* __restrict__ dst, int n_rows,
                                                                           int T, int R1, int C, int first_bin) {
  const int row = blockIdx.x;
  if (row >= n_rows) return;  // (the whole workgroup)
  const int f = row / T, t = row - f * T;
  const int r = placed_round(t, first_bin, R1 - 1);
  const double* s = src + ((size_t)f * (size_t)R1 + (size_t)r) * (size_t)C;
  double* d = dst + (size_t)row * (size_t)C;
  const int tid = threadIdx.x;
  const int ps = (int)(((uintptr_t)s >> 3) & 1), pd = (int)(((uintptr_t)d >> 3) & 1);
  if (ps != pd) {
    for (int i = tid; i < C; i += SF_PLACE_THREADS) d[i] = s[i];
    return;
  }
  const int head = pd < C ? pd : C;  // (an odd first element: on its own, the pairs behind it are aligned)
  const int n2 = (C - head) / 2;
  const double2* s2 = reinterpret_cast<const double2*>(s + head);
  double2* d2 = reinterpret_cast<double2*>(d + head);
  for (int i = tid; i < n2; i += SF_PLACE_THREADS) d2[i] = s2[i];
  if (tid == 0) {
    if (head) d[0] = s[0];
    if (head + 2 * n2 < C) d[C - 1] = s[C - 1];
  }
}

}  // namespace auvp

extern "C" __attribute__((visibility("hidden"))) hipError_t auvpi_sf_place_launch(const double* src, double* dst, int n_sets, int T, int R1, int C,
                                                                                  int first_bin, hipStream_t stream) {
  if (n_sets <= 0 || T <= 0 || C <= 0) return hipSuccess;
  hipLaunchKernelGGL(auvp::sf_place_kernel, dim3((unsigned)(n_sets * T)), dim3(auvp::SF_PLACE_THREADS), 0, stream, src, dst, n_sets * T, T, R1, C,
                     first_bin);
  return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t auvpi_rrt_leaf_grid_launch(
    const auvp::WorldDev* W, const auvp::RrtParamsDev* P, const auvp::RrtBuffers* B, int n_episodes, int mark_words,
    const auvp::RrtEpisodeLimDev* lim, const int32_t* set_of, const auvp::RrtProbSetDev* sets, int grid, int block, int lds,
    hipStream_t stream) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(auvp::rrt_leaf_grid_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(auvp::rrt_leaf_grid_kernel, dim3(grid), dim3(block), lds, stream, *W, *P, *B, n_episodes, mark_words, lim, set_of, sets);
  return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t auvpi_prob_set_stats_launch(const double* prob, long long n_per_set, int n_sets,
                                                                                        auvp::RrtProbSetDev* sets, hipStream_t stream) {
  hipLaunchKernelGGL(auvp::prob_set_stats_kernel, dim3(n_sets), dim3(auvp::PROB_STATS_THREADS), 0, stream, prob, n_per_set, sets);
  return hipGetLastError();
}

// astar_sets_kernels.hip -- astar_fixLenSOG against a shark-occupancy table per search instance (auvp_astar_batch_sets), as a
// translation unit of its own: astar_topn_sets_kernel, the top-n tables of the handle's probability sets built where the sets
// lie, and astar_sets_kernel<3> / astar_sets_kernel<3, true>, the one-wavefront and the PAIR form of astar_kernel.h with the two
// table reads of instance e going to set set_of[e].
//
// Why its own unit: astar_kernel<3> and astar_kernel<3, true> (auvplan.hip) keep the code they had -- the added lines of
// astar_kernel.h are behind AUVP_ASTAR_SETS, which only this file defines, and the sets forms are kernels of another name with an
// argument of their own (tests/test_astar_sets_resources.py holds the plain forms to their registers, scratch and occupancy).
//
// Entry points for the host side (auvplan.hip / astar_host.h): internal, hidden visibility, not part of the C-ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define AUVP_ASTAR_SETS 1
#include "astar_kernel.h"

namespace auvp {

// One workgroup per row (set g, bin t) of prob [rows][C]: topn[row][0] = 0.0, topn[row][i + 1] = topn[row][i] + the i-th largest
// entry of the row -- astar_tables.h's astar_topn_rows, bit for bit.  The row lies in dynamic LDS, padded to n = the next power of
// two with -inf (they sort behind every entry; a -inf of the row itself is interchangeable with them), and is sorted descending by
// a bitonic network: a fixed sequence of compare-exchanges, so any input is safe -- a row with a nan merely gets no defined
// order, and the host refuses such a set.  The running sum is a serial chain by definition: one lane adds the sorted entries one
// after the other, in place (no scan tree -- another association is another double); then every lane stores.
constexpr int TOPN_THREADS = 1024;
static __global__ __launch_bounds__(TOPN_THREADS) void astar_topn_sets_kernel(const double* __restrict__ prob, double* __restrict__ topn,
                                                                              int C, int n) {
  extern __shared__ double topn_row[];  // [n], n >= C a power of two (n >= 1)
  const double* src = prob + (size_t)blockIdx.x * (size_t)C;
  double* dst = topn + (size_t)blockIdx.x * ((size_t)C + 1);
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  for (int i = tid; i < n; i += nt) topn_row[i] = i < C ? src[i] : -__builtin_inf();
  __syncthreads();
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j >= 1; j >>= 1) {
      // pair p of n / 2: i = its lower index (bit j clear), i + j its partner; blocks of k alternate direction
      for (int p = tid; p < (n >> 1); p += nt) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const double a = topn_row[i], b = topn_row[i + j];
        const bool desc = (i & k) == 0;
        if (desc ? a < b : b < a) { topn_row[i] = b; topn_row[i + j] = a; }
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    double tot = 0.0;
    for (int i = 0; i < C; i++) { tot += topn_row[i]; topn_row[i] = tot; }
  }
  __syncthreads();
  if (tid == 0) dst[0] = 0.0;
  for (int i = tid; i < C; i += nt) dst[i + 1] = topn_row[i];
}

}  // namespace auvp

// rows = G * T rows of C entries each, 1 <= C <= ASTAR_TOPN_DEV_MAX_C (the caller's check: 8 bytes times the next power of two
// must fit the LDS a workgroup may have)
extern "C" __attribute__((visibility("hidden"))) hipError_t auvpi_astar_topn_sets_launch(const double* prob, double* topn, int rows, int C,
                                                                                         hipStream_t stream) {
  if (rows < 1 || C < 1 || C > 16384) return hipErrorInvalidValue;
  int n = 1;
  while (n < C) n <<= 1;
  const int lds = n * (int)sizeof(double);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(auvp::astar_topn_sets_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return e;
  int block = n / 2 < 64 ? 64 : (n / 2 > auvp::TOPN_THREADS ? auvp::TOPN_THREADS : n / 2);
  hipLaunchKernelGGL(auvp::astar_topn_sets_kernel, dim3(rows), dim3(block), lds, stream, prob, topn, C, n);
  return hipGetLastError();
}

// the variant-3 search of auvp_astar_batch with a table per instance; pair: the two-wavefront form (the host's choice, by
// auvp_astar_batch's rule)
extern "C" __attribute__((visibility("hidden"))) hipError_t auvpi_astar_sets_launch(const auvp::AstarWorldDev* W, const auvp::AstarParamsDev* P,
                                                                                    const auvp::AstarBuffers* B, int n_inst, const double* sets_prob,
                                                                                    const double* sets_topn, const int32_t* set_of, int pair,
                                                                                    int grid, hipStream_t stream) {
  auvp::AstarSetsDev SD;
  SD.prob = sets_prob; SD.topn = sets_topn; SD.set_of = set_of;
  if (pair) hipLaunchKernelGGL((auvp::astar_sets_kernel<3, true>), dim3(grid), dim3(auvp::ASTAR_WAVES * 128), 0, stream, *W, *P, *B, n_inst, SD);
  else hipLaunchKernelGGL((auvp::astar_sets_kernel<3>), dim3(grid), dim3(auvp::ASTAR_WAVES * 64), 0, stream, *W, *P, *B, n_inst, SD);
  return hipGetLastError();
}

#ifdef AUVP_PIPE_DIAG
// diagnostic build only: this unit's copy of the spin limit / delay table (auvp_wave.h; a device variable per translation unit)
extern "C" __attribute__((visibility("hidden"))) hipError_t auvpi_astar_sets_diag(const int* cfg8) {
  return hipMemcpyToSymbol(HIP_SYMBOL(auvp::auvp_diag_cfg), cfg8, 8 * sizeof(int));
}
#endif

// forecast_wide_kernel.h -- sf_wide_kernel: the shark-occupancy forecast of forecast_kernel.h for grids that do not fit one
// wavefront's LDS, one WORKGROUP of B threads per filter (B a multiple of 64 in 64 .. 1 024; forecast_launch.h chooses it).
//
// The chain is the one-wavefront kernel's, bit for bit (counts -> correction -> R rounds of prediction1 level by level, or of
// prediction2), but the grids live in HBM, in the output itself:
//   grids[f][j]    is the input of round j + 1 and grids[f][j + 1] the grid being filled: there is no second copy
//   counts[f]      is counted in place: zeroed, barrier, integer atomicAdd to global memory (order-free, so exact)
//   prob[f][0]     first holds the corrected values in list order, for the correction's sum; its real content overwrites it
// LDS holds two staging chunks for that sum and the broadcast of `total` (SFW_LDS_BYTES, static).  The total stays ONE chain of
// additions in list order, by thread 0: the workgroup loads chunk n + 1 of the list-order copy into LDS while thread 0 adds up
// chunk n, so the summing thread reads LDS, not 40 000 global loads one behind the other.
//
// Every exchange is inside one workgroup: a phase's stores and the next phase's loads are separated by __syncthreads(), which is
// what the HIP memory model asks for between threads of a workgroup.  grids / prob / counts are plain pointers (SfDev): nothing
// tells the compiler that memory the kernel writes is invariant, and the reads stay ordinary vector loads.  Control flow around
// every barrier is uniform: every loop bound is a launch parameter or a word of the host-built schedule (forecast_plan.h), and
// the `total == 0` exit is taken by the whole workgroup after `total` has been broadcast.
//
// Cost: method 1 pays one barrier per level and round.  A raster list of an r x c grid has r + c - 1 levels; a snake
// (boustrophedon) list has one cell per level, hence one barrier per cell and round -- correct, and as slow as it is on the
// one-wavefront kernel.  Compiled with -ffp-contract=off (auvplan.hip's unit): an a * b + c here is two roundings.
#ifndef AUVP_FORECAST_WIDE_KERNEL_H
#define AUVP_FORECAST_WIDE_KERNEL_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "forecast_kernel.h"  // SfDev, SF_OK / SF_ZERO_TOTAL

namespace auvp {

constexpr int SFW_CHUNK = 1024;  // doubles per staging chunk of the correction's sum
constexpr int SFW_LDS_BYTES = (2 * SFW_CHUNK + 1) * (int)sizeof(double);  // two chunks + the broadcast total

__global__ __launch_bounds__(1024) void sf_wide_kernel(SfDev D) {
  __shared__ double stage[2][SFW_CHUNK];
  __shared__ double total_lds;
  const int G = D.rows * D.cols, C = D.C;
  const int t = (int)threadIdx.x, B = (int)blockDim.x;
  const int f = (int)blockIdx.x;  // (the grid is exactly F workgroups)
  const size_t T = (size_t)D.R + 1;
  double* out_g = D.grids + (size_t)f * T * G;
  double* out_p = D.prob + (size_t)f * T * C;
  int32_t* cnt = D.counts + (size_t)f * G;

  // ---- counts: cellToIndex's expression per particle, compared in double before the conversion -------------------------
  for (int i = t; i < G; i += B) { cnt[i] = 0; out_g[i] = 0.0; }
  __syncthreads();
  const double* px = D.pxy + (size_t)f * (size_t)D.f_stride;
  const double n_col = (double)D.cols, n_row = (double)D.rows;
  for (int n = t; n < D.N; n += B) {
    const double x = px[(size_t)n * D.e_stride], y = px[(size_t)n * D.e_stride + D.y_off];
    const double qx = (x - D.minx) / D.cell_size, qy = (y - D.miny) / D.cell_size;
    if (qx >= 0.0 && qx < n_col && qy >= 0.0 && qy < n_row) atomicAdd(&cnt[(int)qy * D.cols + (int)qx], 1);  // (nan: no count)
  }
  __syncthreads();

  // ---- correction --------------------------------------------------------------------------------------------------------
  const double* prior = D.prior + (D.prior_shared ? 0 : (size_t)f * G);
  for (int c = t; c < C; c += B) {
    const int g = D.cell_g[c];
    const double v = ((double)cnt[g] / D.norm) * prior[g];
    out_g[g] = v;
    out_p[c] = v;  // (in list order, for the sum: prob[f][0] as scratch)
  }
  __syncthreads();
  {
    const int n_chunks = (C + SFW_CHUNK - 1) / SFW_CHUNK;
    for (int i = t; i < SFW_CHUNK && i < C; i += B) stage[0][i] = out_p[i];
    __syncthreads();
    double total = 0.0;
    for (int q = 0; q < n_chunks; q++) {
      // chunk q + 1 into the buffer that thread 0 finished with before the last barrier ...
      const int nb = (q + 1) * SFW_CHUNK;
      for (int i = t; i < SFW_CHUNK && nb + i < C; i += B) stage[(q + 1) & 1][i] = out_p[nb + i];
      // ... and chunk q added up, in list order
      if (t == 0) {
        const int n = C - q * SFW_CHUNK < SFW_CHUNK ? C - q * SFW_CHUNK : SFW_CHUNK;
        const double* s = stage[q & 1];
        for (int i = 0; i < n; i++) total = total + s[i];
      }
      __syncthreads();
    }
    if (t == 0) total_lds = total;
    __syncthreads();
  }
  const double total = total_lds;
  if (total == 0.0) {  // (the same for all threads: read from LDS behind a barrier)
    for (size_t i = t; i < T * G; i += B) out_g[i] = 0.0;
    for (size_t i = t; i < T * C; i += B) out_p[i] = 0.0;
    if (t == 0) D.status[f] = SF_ZERO_TOTAL;
    return;
  }
  for (int i = t; i < G; i += B) out_g[i] = out_g[i] / total;
  __syncthreads();
  for (int c = t; c < C; c += B) out_p[c] = out_g[D.cell_g[c]];

  // ---- rounds ------------------------------------------------------------------------------------------------------------
  const int rows = D.rows, cols = D.cols;
  for (int j = 0; j < D.R; j++) {
    const double* ga = out_g + (size_t)j * G;  // the round's input grid
    double* gb = out_g + (size_t)(j + 1) * G;  // the grid being filled (not const, not restrict: its own stores are read back)
    if (D.method == 1) {
      for (int i = t; i < G; i += B) gb[i] = 0.0;
      __syncthreads();
      const double move = 1.0 - D.stay;
      for (int l = 0; l < D.n_levels; l++) {
        const int lo = D.level_off[l], hi = D.level_off[l + 1];
        for (int s = lo + t; s < hi; s += B) {
          const int g = D.sched_g[s];
          const int r = g / cols, c = g - r * cols;
          double v = D.stay * ga[g];
          // up, left, down, right: inside the grid and already non-zero in the grid being filled (-0.0 is not, nan is)
          const bool u0 = r - 1 >= 0 && gb[g - cols] != 0.0;
          const bool u1 = c - 1 >= 0 && gb[g - 1] != 0.0;
          const bool u2 = r + 1 < rows && gb[g + cols] != 0.0;
          const bool u3 = c + 1 < cols && gb[g + 1] != 0.0;
          const int n_usable = (int)u0 + (int)u1 + (int)u2 + (int)u3;
          if (n_usable) {
            const double w = move / (double)n_usable;
            if (u0) v = v + w * ga[g - cols];
            if (u1) v = v + w * ga[g - 1];
            if (u2) v = v + w * ga[g + cols];
            if (u3) v = v + w * ga[g + 1];
          }
          gb[g] = v;
        }
        __syncthreads();  // the level is complete before the next one reads it
      }
    } else {
      for (int i = t; i < G; i += B) {
        const double p = ga[i];
        gb[i] = p + D.k * (D.p_inf[i] - p);
      }
      __syncthreads();
    }
    double* op = out_p + (size_t)(j + 1) * C;
    for (int c = t; c < C; c += B) op[c] = gb[D.cell_g[c]];
    // (no barrier here: the next round reads gb, complete behind the barrier above, and writes another grid)
  }
  if (t == 0) D.status[f] = SF_OK;
}

}  // namespace auvp
#endif  // AUVP_FORECAST_WIDE_KERNEL_H

// forecast_kernel.h -- sf_forecast_kernel: the shark-occupancy forecast of F particle filters in one launch, one wavefront
// per filter (host side: forecast_host.h; the level schedule: forecast_plan.h).
//
// What one wavefront computes is the chain of SharkUpdate's host methods (sharkEstimate.py) on its filter, bit for bit:
//   counts      particles per grid entry: integer LDS atomics (order-free, so exact)
//   correction  g = (counts / norm) * prior in the listed cells, total summed by ONE lane in list order, every entry / total
//   R rounds    prediction1 (the listed cells level by level: a level's cells are independent, forecast_plan.h) or
//               prediction2 (every entry)
// Both grids of a round and the counts live in LDS (20 bytes per grid entry: 80 KiB at the 4 096-entry cap, two workgroups
// per CU); every round is written to `grids` and, gathered in list order, to `prob`.  Hand-offs between lanes go through LDS
// inside the one wavefront (wave_sync: no workgroup barrier anywhere); every loop bound is a launch parameter or a word
// of the host-built schedule, the same for all lanes.  Compiled with -ffp-contract=off: an a * b + c here is two roundings,
// as in the reference.
#ifndef AUVP_FORECAST_KERNEL_H
#define AUVP_FORECAST_KERNEL_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "auvp_wave.h"

namespace auvp {

enum { SF_OK = 0, SF_ZERO_TOTAL = 1 };  // per-filter status: 1 = the correction's total is 0 (ZeroDivisionError)

struct SfDev {
  int32_t F, N, rows, cols, C, R, method, n_levels, prior_shared, _pad;
  // particle coordinates: x of list position n of filter f = pxy[f * f_stride + n * e_stride], y = the same + y_off
  // (PfDev::st [F][5][N]: 5 N, 1, N; a host [F][N][2] array: 2 N, 2, 1)
  long long f_stride;
  int32_t e_stride, y_off;
  const double* pxy;
  double minx, miny, cell_size, stay, k, norm;
  const double* prior;         // [F or 1][rows * cols]
  const double* p_inf;         // [rows * cols] (method 2)
  const int32_t* cell_g;       // [C] grid entry (row * cols + col) of list position c
  const int32_t* sched_g;      // [C] grid entries of the listed cells sorted by (level, list position)
  const int32_t* level_off;    // [n_levels + 1]
  double* grids;               // [F][R + 1][rows * cols]
  double* prob;                // [F][R + 1][C]
  int32_t* counts;             // [F][rows * cols]
  int32_t* status;             // [F]
};

inline size_t sf_lds_bytes(int n_grid) { return (size_t)n_grid * (2 * sizeof(double) + sizeof(int32_t)); }

__global__ __launch_bounds__(64) void sf_forecast_kernel(SfDev D) {
  extern __shared__ __align__(16) unsigned char sf_lds[];
  const int G = D.rows * D.cols, C = D.C;
  double* ga = reinterpret_cast<double*>(sf_lds);  // the round's input grid
  double* gb = ga + G;                             // the grid being filled
  int32_t* cnt = reinterpret_cast<int32_t*>(gb + G);
  const int lane = lane_id();
  const int f = (int)blockIdx.x;
  if (f >= D.F) return;
  const size_t T = (size_t)D.R + 1;
  double* out_g = D.grids + (size_t)f * T * G;
  double* out_p = D.prob + (size_t)f * T * C;

  // ---- counts: cellToIndex's expression per particle, compared in double before the conversion -------------------------
  for (int i = lane; i < G; i += 64) { cnt[i] = 0; ga[i] = 0.0; }
  wave_sync();
  const double* px = D.pxy + (size_t)f * (size_t)D.f_stride;
  const double n_col = (double)D.cols, n_row = (double)D.rows;
  for (int n = lane; n < D.N; n += 64) {
    const double x = px[(size_t)n * D.e_stride], y = px[(size_t)n * D.e_stride + D.y_off];
    const double qx = (x - D.minx) / D.cell_size, qy = (y - D.miny) / D.cell_size;
    if (qx >= 0.0 && qx < n_col && qy >= 0.0 && qy < n_row) atomicAdd(&cnt[(int)qy * D.cols + (int)qx], 1);  // (nan: no count)
  }
  wave_sync();
  for (int i = lane; i < G; i += 64) D.counts[(size_t)f * G + i] = cnt[i];

  // ---- correction --------------------------------------------------------------------------------------------------------
  const double* prior = D.prior + (D.prior_shared ? 0 : (size_t)f * G);
  for (int c = lane; c < C; c += 64) {
    const int g = D.cell_g[c];
    const double v = ((double)cnt[g] / D.norm) * prior[g];
    ga[g] = v;
    gb[c] = v;  // (in list order, for the sum)
  }
  wave_sync();
  double total = 0.0;
  if (lane == 0)
    for (int c = 0; c < C; c++) total = total + gb[c];
  total = __shfl(total, 0);
  if (total == 0.0) {  // (the same for all lanes)
    for (size_t i = lane; i < T * G; i += 64) out_g[i] = 0.0;
    for (size_t i = lane; i < T * C; i += 64) out_p[i] = 0.0;
    if (lane == 0) D.status[f] = SF_ZERO_TOTAL;
    return;
  }
  wave_sync();
  for (int i = lane; i < G; i += 64) {
    const double v = ga[i] / total;
    ga[i] = v;
    out_g[i] = v;
  }
  wave_sync();
  for (int c = lane; c < C; c += 64) out_p[c] = ga[D.cell_g[c]];

  // ---- rounds ------------------------------------------------------------------------------------------------------------
  const int rows = D.rows, cols = D.cols;
  for (int j = 0; j < D.R; j++) {
    if (D.method == 1) {
      for (int i = lane; i < G; i += 64) gb[i] = 0.0;
      wave_sync();
      const double move = 1.0 - D.stay;
      for (int l = 0; l < D.n_levels; l++) {
        const int lo = D.level_off[l], hi = D.level_off[l + 1];
        for (int s = lo + lane; s < hi; s += 64) {
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
        wave_sync();  // the level is complete before the next one reads it
      }
    } else {
      for (int i = lane; i < G; i += 64) {
        const double p = ga[i];
        gb[i] = p + D.k * (D.p_inf[i] - p);
      }
      wave_sync();
    }
    double* t = ga; ga = gb; gb = t;
    double* og = out_g + (size_t)(j + 1) * G;
    for (int i = lane; i < G; i += 64) og[i] = ga[i];
    double* op = out_p + (size_t)(j + 1) * C;
    for (int c = lane; c < C; c += 64) op[c] = ga[D.cell_g[c]];
    wave_sync();
  }
  if (lane == 0) D.status[f] = SF_OK;
}

}  // namespace auvp
#endif  // AUVP_FORECAST_KERNEL_H

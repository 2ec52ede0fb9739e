// forecast_launch.h -- which kernel a shark-occupancy forecast gets, and at what shape: the host's choice as data.
//
// Host only and pure: no HIP runtime call, no handle, no environment.  sf_choose_launch reads the grid's shape, whether the
// caller allows large grids (auvp_sf_forecast_large) and the handle's options (OptionView, launch_plan.h) and returns the
// launch; forecast_host.h launches what it says.  auvp_sf_choose_launch (include/auvplan.h) answers the same question without a
// device: tests/test_forecast_launch.py pins the rules.
//
//   allow_large not set                       today's rule: rows x cols <= SF_MAX_GRID takes sf_forecast_kernel (one wavefront per
//                                             filter, both grids and the counts in LDS), above that SF_LAUNCH_CAPACITY
//   allow_large, rows x cols <  SF_WIDE_MIN   sf_forecast_kernel          (option SF_WIDE_MIN, default SF_MAX_GRID + 1; tests)
//   allow_large, .. <= SF_MAX_GRID_WIDE       sf_wide_kernel (forecast_wide_kernel.h): one workgroup of B threads per filter
//   allow_large, above SF_MAX_GRID_WIDE       SF_LAUNCH_CAPACITY
// SF_MAX_GRID_WIDE = 2^22 is a stated condition, not a hardware limit: one grid is 32 MiB, and every entry index, level
// offset and rows x cols product stays far inside int32.  (SF_WIDE_MIN above SF_MAX_GRID + 1 cannot send a grid to the
// one-wavefront kernel that does not fit its LDS: such a grid takes the wide kernel.)
// Included by auvplan.hip behind launch_plan.h (OptionView) and forecast_plan.h.
#ifndef AUVP_FORECAST_LAUNCH_H
#define AUVP_FORECAST_LAUNCH_H
#include <cstddef>
#include <cstdint>

#include "forecast_plan.h"

namespace auvp {

constexpr int SF_MAX_GRID_WIDE = 1 << 22;  // rows x cols of a forecast grid at most with large grids allowed
constexpr int SF_WIDE_LDS_BYTES = (2 * 1024 + 1) * 8;  // sf_wide_kernel's static LDS (== SFW_LDS_BYTES; forecast_host.h asserts it)
// Threads per workgroup of sf_wide_kernel where option SF_WIDE_BLOCK does not force them: what profiles/shark_forecast_wide.md
// favours at 201 x 201 (raster, 10 rounds: 5.09 ms for one filter, 5.93 for 256, 23.7 for 1 024; 256 threads: 5.56 / 7.02 / 24.2,
// 64 threads: 11.5 / 14.3 / 31.7)
constexpr int SF_WIDE_BLOCK_DEFAULT = 1024;

enum SfKernelKind { SF_KERNEL_ONE_WAVE = 0, SF_KERNEL_WIDE = 1 };
enum SfLaunchStatus {
  SF_LAUNCH_OK = 0,
  SF_LAUNCH_CAPACITY,  // the grid has more entries than the caller's entry point takes
  SF_LAUNCH_ARG        // a shape < 1, or option SF_WIDE_BLOCK is no multiple of 64 in 64 .. 1 024
};

struct SfLaunch {
  SfLaunchStatus status = SF_LAUNCH_OK;
  SfKernelKind kind = SF_KERNEL_ONE_WAVE;
  int block = 0, lds = 0;      // threads per workgroup (one workgroup per filter); LDS bytes of a workgroup, static + dynamic
  long long limit = 0;         // SF_LAUNCH_CAPACITY: the entry count the grid is over
  const char* name = "";       // what auvp_sf_last_kernel reports
};

// n_cells, widest_level: the list's length and the most cells of one level of its schedule (sf_plan); 0: not known.  The
// choice does not read them today -- the measured default block is one figure (profiles/shark_forecast_wide.md) -- but they
// are what a finer rule would go by, so the query carries them.
inline SfLaunch sf_choose_launch(int rows, int cols, int n_cells, int widest_level, bool allow_large, const OptionView& opt) {
  SfLaunch p;
  (void)n_cells; (void)widest_level;
  if (rows < 1 || cols < 1) { p.status = SF_LAUNCH_ARG; return p; }
  const long long G = (long long)rows * cols;
  const long long cap = allow_large ? SF_MAX_GRID_WIDE : SF_MAX_GRID;
  if (G > cap) { p.status = SF_LAUNCH_CAPACITY; p.limit = cap; return p; }
  long long wide_min = opt.opt_num(OPT_SF_WIDE_MIN, (long long)SF_MAX_GRID + 1);
  if (wide_min > (long long)SF_MAX_GRID + 1) wide_min = (long long)SF_MAX_GRID + 1;
  if (!allow_large || G < wide_min) {
    p.kind = SF_KERNEL_ONE_WAVE; p.block = 64; p.lds = (int)(G * (2 * sizeof(double) + sizeof(int32_t)));
    p.name = "sf_forecast_kernel";
    return p;
  }
  const long long B = opt.opt_num(OPT_SF_WIDE_BLOCK, SF_WIDE_BLOCK_DEFAULT);
  if (B < 64 || B > 1024 || B % 64 != 0) { p.status = SF_LAUNCH_ARG; return p; }
  p.kind = SF_KERNEL_WIDE; p.block = (int)B; p.lds = SF_WIDE_LDS_BYTES;
  p.name = "sf_wide_kernel";
  return p;
}

}  // namespace auvp
#endif  // AUVP_FORECAST_LAUNCH_H

// forecast_plan.h -- the level schedule of the shark-occupancy forecast (forecast_kernel.h): which cells of cell_list may be
// filled side by side, as data.
//
// Host only and pure: no HIP runtime call, no handle, no environment.  SharkUpdate.prediction1 (sharkEstimate.py) walks
// cell_list in order, and a cell only counts the 4-neighbours that were filled in before it and came out non-zero: cell i
// depends on exactly those of its neighbours that stand EARLIER in the list.  That is a DAG along list order;
//   level[i] = 0                                  no 4-neighbour of cell i is earlier in the list
//            = 1 + max(level of those neighbours)  otherwise
// Two cells of one level are never neighbours (the later one would be a level above the earlier), so the cells of a level can
// be filled by lanes side by side once every lower level is complete, with the result of the sequential walk.  sf_plan returns
// the list positions sorted by (level, position) and the offsets of the levels; sf_forecast_kernel takes every loop bound from
// it.  A raster list of an r x c grid has r + c - 1 levels, a snake (boustrophedon) list one cell per level.
//
// The list is validated here: a cell outside the grid (the reference raises IndexError, or wraps a negative index silently)
// and a cell listed twice (its second visit would see neighbours that are later in the list: not a DAG) are refused.
// auvp_sf_plan (include/auvplan.h) answers the same question without a device: tests/test_forecast_plan.py pins the rules.
#ifndef AUVP_FORECAST_PLAN_H
#define AUVP_FORECAST_PLAN_H
#include <cstddef>
#include <cstdint>
#include <vector>

namespace auvp {

constexpr int SF_MAX_GRID = 4096;  // rows x cols of a forecast grid at most (two fp64 grids + the counts in one workgroup's LDS)

enum SfPlanStatus {
  SF_PLAN_OK = 0,
  SF_PLAN_BAD_SHAPE,  // rows or cols < 1, or no cell
  SF_PLAN_OUTSIDE,    // cell `bad`: row or column negative or past the grid
  SF_PLAN_DUPLICATE   // cell `bad` names the grid entry an earlier cell of the list names
};

struct SfPlan {
  SfPlanStatus status = SF_PLAN_OK;
  int bad = -1;                    // the list position the status is about
  int n_levels = 0;
  std::vector<int32_t> level;      // [C]            level of list position i
  std::vector<int32_t> order;      // [C]            list positions sorted by (level, position)
  std::vector<int32_t> level_off;  // [n_levels + 1] level l = order[level_off[l] .. level_off[l + 1])
};

// cell_rc [C][2]: (row, column) of every cell of the list, in list order
inline SfPlan sf_plan(int rows, int cols, const int32_t* cell_rc, int n_cells) {
  SfPlan p;
  if (rows < 1 || cols < 1 || n_cells < 1 || !cell_rc) { p.status = SF_PLAN_BAD_SHAPE; return p; }
  const size_t G = (size_t)rows * (size_t)cols;
  std::vector<int32_t> at(G, -1);  // grid entry -> the list position that names it
  for (int i = 0; i < n_cells; i++) {
    const int r = cell_rc[2 * i], c = cell_rc[2 * i + 1];
    if (r < 0 || r >= rows || c < 0 || c >= cols) { p.status = SF_PLAN_OUTSIDE; p.bad = i; return p; }
    int32_t& slot = at[(size_t)r * cols + c];
    if (slot >= 0) { p.status = SF_PLAN_DUPLICATE; p.bad = i; return p; }
    slot = i;
  }
  p.level.assign(n_cells, 0);
  int top = 0;
  for (int i = 0; i < n_cells; i++) {  // (list order: every earlier neighbour already has its level)
    const int r = cell_rc[2 * i], c = cell_rc[2 * i + 1];
    int lv = 0;
    auto see = [&](int rr, int cc) {
      if (rr < 0 || rr >= rows || cc < 0 || cc >= cols) return;
      const int j = at[(size_t)rr * cols + cc];
      if (j >= 0 && j < i && p.level[j] + 1 > lv) lv = p.level[j] + 1;
    };
    see(r - 1, c); see(r, c - 1); see(r + 1, c); see(r, c + 1);
    p.level[i] = lv;
    if (lv > top) top = lv;
  }
  p.n_levels = top + 1;
  p.level_off.assign((size_t)p.n_levels + 1, 0);
  for (int i = 0; i < n_cells; i++) p.level_off[(size_t)p.level[i] + 1]++;
  for (int l = 0; l < p.n_levels; l++) p.level_off[(size_t)l + 1] += p.level_off[l];
  p.order.assign(n_cells, 0);
  std::vector<int32_t> fill(p.level_off.begin(), p.level_off.end() - 1);
  for (int i = 0; i < n_cells; i++) p.order[(size_t)fill[p.level[i]]++] = i;  // (a counting sort: stable, so by (level, position))
  return p;
}

}  // namespace auvp
#endif  // AUVP_FORECAST_PLAN_H

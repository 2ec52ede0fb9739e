// astar_tables.h -- the A* family's device tables as pure host functions: no HIP, no handle, only the standard library and
// world_tables.h.  build_astar_world_tables makes everything astar_build_world uploads (astar_host.h); the top-n table of
// astar_fixLenSOG's heuristic (get_top_n_prob, astar_fixLenSOG.py:516-531) is one text for three users: that build, the host route
// of the probability sets' tables (rows too long for astar_topn_sets_kernel's LDS: astar_host.h) and the host test
// (tests/host/astar_tables_dump.cpp, built with the sanitizers by tests/test_astar_tables_host.py).
//
// Per time bin t:  topn[t][0] = 0.0,  topn[t][i + 1] = topn[t][i] + sorted_desc(prob[t])[i]  -- the additions one after the
// other, in that order, in fp64 (`total = 0; total += probabilities[index]`, :526-530).  Equal values are interchangeable in the
// sort, and as the running sum starts at +0.0 the order of +0.0 and -0.0 cannot show.  A row that holds a nan has no defined
// order (neither in the reference's sorted() nor in std::sort): the caller keeps such rows away.
#ifndef AUVP_ASTAR_TABLES_H
#define AUVP_ASTAR_TABLES_H
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "world_tables.h"  // (sq_threshold)

namespace auvp {

// longest row astar_topn_sets_kernel sorts (its row, padded to a power of two, lies in 128 KB of the CU's 160 KB of LDS)
constexpr int ASTAR_TOPN_DEV_MAX_C = 16384;

// prob [T][C] -> topn [T][C + 1]
inline void astar_topn_rows(const double* prob, size_t T, size_t C, double* topn) {
  std::vector<double> tmp(C);
  for (size_t t = 0; t < T; t++) {
    if (C) std::copy(prob + t * C, prob + (t + 1) * C, tmp.begin());
    std::sort(tmp.begin(), tmp.end(), [](double a, double b) { return a > b; });
    double tot = 0.0;  // total = 0; total += probabilities[index]  (astar_fixLenSOG.py:526-530)
    double* row = topn + t * (C + 1);
    row[0] = 0.0;
    for (size_t i = 0; i < C; i++) { tot += tmp[i]; row[i + 1] = tot; }
  }
}

// Python round(v, 2): decimal rounding of the exact binary value (float.__round__ -> dtoa mode 3)
inline double round2_py(double v) {
  char buf[512];
  snprintf(buf, sizeof buf, "%.2f", v);
  return strtod(buf, nullptr);
}

// Everything astar_build_world uploads and writes into AstarWorldDev, from the host copy of the world:
//   ox, oy, ot [O]   centres and the squared threshold of plain `d <= obstacle.size` per obstacle (no shared dList here)
//   hab [H][4]       x, y, size and the squared threshold of `dist <= size`
//   rc [C][4]        the cells' edges through round(v, 2)
//   topn [T][C + 1]  get_top_n_prob's table (above)
//   cx, cy           Polygon(...).centroid: the area-weighted (shoelace) centroid -- shapely is absent; DESIGN.md.  A polygon of
//                    no area gets what the expression gives in IEEE arithmetic (0 / 0); no polygon: 0, 0
//   gtab, g_*        the product grid, where the cells are one: a row-major list of ncol x nrow cells whose x interval depends on
//                    the column only and whose y interval on the row only, edges ascending, neighbouring intervals touching at
//                    most, no degenerate widths (astar_kernel.h).  gtab = X0 [ncol], X1 [ncol], Y0 [nrow], Y1 [nrow]; g_x1_0 /
//                    g_y1_0 and g_inv_dx / g_inv_dy: origin and 1 / mean spacing of X1 / Y1 (the first guess of a lookup).
//                    No grid (or `no_grid`: option ASTAR_NO_GRID): gtab empty and every g_* zero
struct AstarWorldTables {
  std::vector<double> ox, oy, ot, hab, rc, topn, gtab;
  int g_ncol = 0, g_nrow = 0;
  double g_x1_0 = 0.0, g_y1_0 = 0.0, g_inv_dx = 0.0, g_inv_dy = 0.0, cx = 0.0, cy = 0.0;
};

inline AstarWorldTables build_astar_world_tables(const double* obstacles, int O, const double* habitats, int H, const double* polygon, int V,
                                                 int T, const double* cells, int C, const double* prob, bool no_grid) {
  AstarWorldTables t;
  t.ox.resize((size_t)O); t.oy.resize((size_t)O); t.ot.resize((size_t)O);
  t.hab.resize((size_t)H * 4); t.rc.resize((size_t)C * 4); t.topn.resize((size_t)T * ((size_t)C + 1));
  for (int i = 0; i < O; i++) {
    t.ox[i] = obstacles[3 * i]; t.oy[i] = obstacles[3 * i + 1];
    t.ot[i] = sq_threshold(obstacles[3 * i + 2]);
  }
  for (int i = 0; i < H; i++) {
    t.hab[4 * i] = habitats[3 * i]; t.hab[4 * i + 1] = habitats[3 * i + 1]; t.hab[4 * i + 2] = habitats[3 * i + 2];
    t.hab[4 * i + 3] = sq_threshold(habitats[3 * i + 2]);
  }
  const std::vector<double>& rc = t.rc;
  for (size_t i = 0; i < rc.size(); i++) t.rc[i] = round2_py(cells[i]);
  astar_topn_rows(prob, (size_t)T, (size_t)C, t.topn.data());
  double a2 = 0.0, sx = 0.0, sy = 0.0;
  for (int i = 0; i < V; i++) {
    double x0 = polygon[2 * i], y0 = polygon[2 * i + 1];
    double x1 = polygon[2 * ((i + 1) % V)], y1 = polygon[2 * ((i + 1) % V) + 1];
    double cr = x0 * y1 - x1 * y0;
    a2 += cr;
    sx += (x0 + x1) * cr;
    sy += (y0 + y1) * cr;
  }
  t.cx = V > 0 ? sx / (3.0 * a2) : 0.0;
  t.cy = V > 0 ? sy / (3.0 * a2) : 0.0;
  if (C > 0 && !no_grid) {
    int nc = 1;
    while (nc < C && rc[4 * (size_t)nc + 1] == rc[1] && rc[4 * (size_t)nc + 3] == rc[3]) nc++;
    if (C % nc == 0) {
      const int nr = C / nc;
      std::vector<double> gtab(2 * (size_t)nc + 2 * (size_t)nr);
      double* X0 = gtab.data(); double* X1 = X0 + nc; double* Y0 = X1 + nc; double* Y1 = Y0 + nr;
      for (int c = 0; c < nc; c++) { X0[c] = rc[4 * (size_t)c]; X1[c] = rc[4 * (size_t)c + 2]; }
      for (int r = 0; r < nr; r++) { Y0[r] = rc[4 * (size_t)r * nc + 1]; Y1[r] = rc[4 * (size_t)r * nc + 3]; }
      bool ok = true;
      for (int r = 0; r < nr && ok; r++)
        for (int c = 0; c < nc && ok; c++) {
          const double* q = &rc[4 * ((size_t)r * nc + c)];
          ok = q[0] == X0[c] && q[2] == X1[c] && q[1] == Y0[r] && q[3] == Y1[r];
        }
      auto axis_ok = [](const double* lo, const double* hi, int n) {
        double scale = 1.0;
        for (int i = 0; i < n; i++) {
          if (!std::isfinite(lo[i]) || !std::isfinite(hi[i])) return false;
          scale = std::fmax(scale, std::fmax(std::fabs(lo[i]), std::fabs(hi[i])));
        }
        for (int i = 0; i < n; i++) {
          if (!(hi[i] - lo[i] >= 1e-6 * scale)) return false;
          if (i + 1 < n && !(lo[i + 1] >= hi[i])) return false;
        }
        return true;
      };
      if (ok && axis_ok(X0, X1, nc) && axis_ok(Y0, Y1, nr)) {
        t.g_ncol = nc; t.g_nrow = nr;
        t.g_x1_0 = X1[0]; t.g_y1_0 = Y1[0];
        t.g_inv_dx = nc > 1 ? (nc - 1) / (X1[nc - 1] - X1[0]) : 0.0;
        t.g_inv_dy = nr > 1 ? (nr - 1) / (Y1[nr - 1] - Y1[0]) : 0.0;
        t.gtab.swap(gtab);
      }
    }
  }
  return t;
}

}  // namespace auvp
#endif

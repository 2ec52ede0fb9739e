// world_tables.h -- every table and constant the device's world model (WorldDev, auvp_types.h) is made of, computed on the host.
//
// Host only and pure (as launch_plan.h): no HIP call, no handle, no environment -- only the standard library, so that a plain
// C++17 compiler builds it.  build_world_tables reads a plain description of the world and of the three options that steer the
// tables (WorldIn) and returns everything auvp_world_set uploads or writes into WorldDev (WorldTables); build_habitat_tables is
// the habitats' part alone (auvp_world_set_habitats).  The kernels compare against these doubles bit for bit, so the arithmetic
// below is order-sensitive (the library is built with -ffp-contract=off).  tests/test_world_tables.py builds
// tests/host/world_tables_dump.cpp around this header and checks every table against the reading rule auvp_types.h gives it.
#ifndef AUVP_WORLD_TABLES_H
#define AUVP_WORLD_TABLES_H
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace auvp {

// largest double s with RN(sqrt(s)) <= R  (R < 0 -> -1: `d <= size` can never hold)
inline double sq_threshold(double R) {
  if (!(R >= 0.0)) return -1.0;
  double s = R * R;
  if (std::isinf(s)) return s;
  while (std::sqrt(s) > R) s = std::nextafter(s, -INFINITY);
  for (;;) {
    double n = std::nextafter(s, INFINITY);
    if (std::isinf(n) || std::sqrt(n) > R) break;
    s = n;
  }
  return s;
}

// the arguments of auvp_world_set and the options that steer the tables
struct WorldIn {
  const double* obstacles = nullptr;  // [O,3] x, y, size
  int32_t O = 0;
  const double* habitats = nullptr;   // [H,3] x, y, size
  int32_t H = 0;
  const double* polygon = nullptr;    // [V,2]
  int32_t V = 0;
  const double* bins = nullptr;       // [T,2]
  int32_t T = 0;
  const double* cells = nullptr;      // [C,4] minx, miny, maxx, maxy
  int32_t C = 0;
  const double* prob = nullptr;       // [T,C]
  long long rg_max_entries = 32ll << 20;  // entry budget of the region index (option RG_MAX_ENTRIES)
  bool grid_index = true;                 // separable-grid index allowed (option NO_GRID_INDEX unset)
  bool habitat_grid = true;               // habitat mask grid allowed (option NO_HABITAT_GRID unset)
};

// hab_t and the habitat mask grid (hg_n == 0: no grid, the kernels scan the list)
struct HabitatTables {
  std::vector<double> hab_t;                // [H]
  std::vector<unsigned long long> hg_mask;  // [hg_n * hg_n]
  int32_t hg_n = 0;
  double hg_x0 = 0.0, hg_y0 = 0.0, hg_inv_w = 0.0, hg_inv_h = 0.0;
};

// every table of WorldDev under the name of its pointer, every scalar under its own name
struct WorldTables {
  std::vector<double> ox, oy, ot;
  int32_t n_xbuckets = 0;
  std::vector<int32_t> xb_off, xb_items;
  std::vector<double> xb_data;
  double xb_x0 = 0.0, xb_inv_w = 0.0;
  int32_t rg_enabled = 0, n_rg_bp = 0;
  std::vector<int32_t> rg_first, rg_off, rg_id;
  std::vector<double> rg_bp, rg_pm;
  int32_t sg_enabled = 0, sg_ncol = 0, sg_nrow = 0;
  std::vector<double> sg_x0, sg_x1, sg_y0, sg_y1, sg_col, sg_row;  // empty when the index is off
  double sg_x1_0 = 0.0, sg_y1_0 = 0.0, sg_inv_dx = 0.0, sg_inv_dy = 0.0;
  std::vector<double> os_x, os_y, os_t, os_box;
  std::vector<float> os_r;
  double obst_area = 0.0;  // area of the bounding box of the obstacle centres (0: fewer than two obstacles / degenerate)
  HabitatTables hab;
  double prob_absmax = 0.0;
  int32_t prob_one_sign = 1;
  int32_t bins_sorted = 0;
  double bins_t1_0 = 0.0, bins_inv_len = 0.0;
  double bb[4] = {INFINITY, INFINITY, -INFINITY, -INFINITY};
  double safe_box[4] = {0.0, 0.0, 0.0, 0.0};
  int32_t has_safe_box = 0;
};

// obstacles SoA; ot: T of the suffix max of the radii, list order (auvp_types.h)
inline void build_obstacle_thresholds(const double* obstacles, int O, WorldTables& t) {
  t.ox.resize(O); t.oy.resize(O); t.ot.resize(O);
  double run = -INFINITY;
  for (int i = O - 1; i >= 0; i--) {
    double r = obstacles[3 * i + 2];
    if (r > run) run = r;
    t.ox[i] = obstacles[3 * i];
    t.oy[i] = obstacles[3 * i + 1];
    t.ot[i] = sq_threshold(run);
  }
}

// x-bucket index over the cells
inline void build_xbuckets(const double* cells, int C, WorldTables& t) {
  double X0 = 0.0, inv_w = 0.0;
  int NB = 0;
  std::vector<int32_t>& xoff = t.xb_off;
  std::vector<int32_t>& xitems = t.xb_items;
  std::vector<double>& xdata = t.xb_data;
  xoff.clear(); xitems.clear(); xdata.clear();
  if (C > 0) {
    double lo = INFINITY, hi = -INFINITY, wmin = INFINITY;
    for (int c = 0; c < C; c++) {
      double a = cells[4 * c], b = std::min(cells[4 * c + 2], cells[4 * c + 3]);
      double wdt = cells[4 * c + 2] - cells[4 * c];
      if (wdt > 0 && wdt < wmin) wmin = wdt;
      if (b < a) continue;
      lo = std::min(lo, a);
      hi = std::max(hi, b);
    }
    if (!(hi >= lo)) { lo = 0.0; hi = 1.0; }
    double span = hi - lo;
    NB = 1;
    if (span > 0 && std::isfinite(wmin)) NB = (int)std::min(8192.0, std::max(1.0, std::ceil(span / wmin)));
    X0 = lo;
    inv_w = span > 0 ? (double)NB / span : 0.0;
    std::vector<std::vector<int32_t>> lists(NB);
    for (int c = 0; c < C; c++) {
      double a = cells[4 * c], b = std::min(cells[4 * c + 2], cells[4 * c + 3]);
      if (b < a) continue;
      int b0 = (int)std::floor((a - X0) * inv_w) - 1, b1 = (int)std::floor((b - X0) * inv_w) + 1;
      b0 = std::max(0, std::min(NB - 1, b0));
      b1 = std::max(0, std::min(NB - 1, b1));
      for (int k = b0; k <= b1; k++) lists[k].push_back(c);
    }
    xoff.resize(NB + 1);
    xoff[0] = 0;
    for (int k = 0; k < NB; k++) {
      xoff[k + 1] = xoff[k] + (int32_t)lists[k].size();
      xitems.insert(xitems.end(), lists[k].begin(), lists[k].end());
    }
    xdata.resize(xitems.size() * 4);
    for (int k = 0; k < NB; k++) {
      double suf = INFINITY;
      for (int i = xoff[k + 1] - 1; i >= xoff[k]; i--) {
        const double* cb = cells + 4 * (size_t)xitems[i];
        suf = std::min(suf, cb[1]);
        xdata[4 * (size_t)i] = cb[0];
        xdata[4 * (size_t)i + 1] = std::min(cb[2], cb[3]);
        xdata[4 * (size_t)i + 2] = cb[1];
        xdata[4 * (size_t)i + 3] = suf;
      }
    }
  } else {
    xoff.assign(2, 0);
  }
  t.n_xbuckets = NB; t.xb_x0 = X0; t.xb_inv_w = inv_w;
}

// region index (auvp_types.h): breakpoints, per-region candidate lists with running min of miny.  Reads the bucket map
// build_xbuckets left in `t`; more than `rg_max_entries` list entries: rg_enabled = 0
inline void build_region_index(const double* cells, int C, long long rg_max_entries, WorldTables& t) {
  const double X0 = t.xb_x0, inv_w = t.xb_inv_w;
  const int NB = t.n_xbuckets;
  std::vector<double>& bp = t.rg_bp;
  std::vector<double>& rpm = t.rg_pm;
  std::vector<int32_t>& rfirst = t.rg_first;
  std::vector<int32_t>& roff = t.rg_off;
  std::vector<int32_t>& rid = t.rg_id;
  bp.clear(); rpm.clear(); rid.clear();
  rfirst.assign(NB + 1, 0); roff.assign(2, 0);
  int rg_enabled = 0;
  if (C > 0) {
    bp.reserve((size_t)2 * C);
    for (int c = 0; c < C; c++) {
      const double a = cells[4 * c], b = std::min(cells[4 * c + 2], cells[4 * c + 3]);
      if (b < a || a != a || b != b) continue;
      bp.push_back(a); bp.push_back(b);
    }
    std::sort(bp.begin(), bp.end());
    bp.erase(std::unique(bp.begin(), bp.end()), bp.end());
    const size_t m = bp.size();
    auto bucket_of = [&](double x) {
      const double fb = std::floor((x - X0) * inv_w);
      return fb < 0.0 ? 0 : (fb >= (double)NB ? NB - 1 : (int)fb);
    };
    for (size_t i = 0; i < m; i++) rfirst[bucket_of(bp[i]) + 1]++;
    for (int k = 0; k < NB; k++) rfirst[k + 1] += rfirst[k];
    const size_t R = 2 * m + 1;
    std::vector<int64_t> cnt(R + 1, 0);
    std::vector<int32_t> r0(C, 0), r1(C, -1);
    for (int c = 0; c < C; c++) {
      const double a = cells[4 * c], b = std::min(cells[4 * c + 2], cells[4 * c + 3]);
      if (b < a || a != a || b != b) continue;
      r0[c] = 2 * (int32_t)(std::lower_bound(bp.begin(), bp.end(), a) - bp.begin()) + 1;
      r1[c] = 2 * (int32_t)(std::lower_bound(bp.begin(), bp.end(), b) - bp.begin()) + 1;
      cnt[r0[c]]++; cnt[r1[c] + 1]--;
    }
    int64_t total = 0, run = 0;
    for (size_t r = 0; r < R; r++) { run += cnt[r]; total += run; }
    const int64_t budget = rg_max_entries;
    if (total <= budget && R + 1 < (size_t)INT32_MAX) {
      rg_enabled = 1;
      roff.assign(R + 1, 0);
      run = 0;
      for (size_t r = 0; r < R; r++) { run += cnt[r]; roff[r + 1] = roff[r] + (int32_t)run; }
      rpm.resize((size_t)total); rid.resize((size_t)total);
      std::vector<int32_t> fill(roff.begin(), roff.end() - 1);
      for (int c = 0; c < C; c++)
        for (int32_t r = r0[c]; r <= r1[c]; r++) {
          const int32_t k = fill[r]++;
          rid[k] = c;
          rpm[k] = (k > roff[r]) ? std::min(rpm[k - 1], cells[4 * c + 1]) : cells[4 * c + 1];
        }
    } else {
      bp.clear();
      std::fill(rfirst.begin(), rfirst.end(), 0);
    }
  }
  t.rg_enabled = rg_enabled; t.n_rg_bp = (int32_t)bp.size();
}

// separable-grid index (auvp_types.h): cell_list row-major over non-decreasing X0/X1 (columns) and Y0/Y1 (rows), its
// interleaved copies and the constants of the lookups' first guesses; off (every table empty) for another list or !grid_index
inline void build_separable_grid(const double* cells, int C, bool grid_index, WorldTables& t) {
  std::vector<double>& sgx0 = t.sg_x0;
  std::vector<double>& sgx1 = t.sg_x1;
  std::vector<double>& sgy0 = t.sg_y0;
  std::vector<double>& sgy1 = t.sg_y1;
  sgx0.clear(); sgx1.clear(); sgy0.clear(); sgy1.clear();
  int sg_ncol = 0, sg_nrow = 0;
  if (C > 0) {
    int nc = 1;
    while (nc < C && cells[4 * (size_t)nc + 1] == cells[1] && cells[4 * (size_t)nc + 3] == cells[3]) nc++;
    if (C % nc == 0) {
      const int nr = C / nc;
      bool ok = true;
      sgx0.resize(nc); sgx1.resize(nc); sgy0.resize(nr); sgy1.resize(nr);
      for (int c = 0; c < nc; c++) { sgx0[c] = cells[4 * (size_t)c]; sgx1[c] = cells[4 * (size_t)c + 2]; }
      for (int r = 0; r < nr; r++) { sgy0[r] = cells[4 * (size_t)r * nc + 1]; sgy1[r] = cells[4 * (size_t)r * nc + 3]; }
      for (int r = 0; r < nr && ok; r++)
        for (int c = 0; c < nc; c++) {
          const double* cb = cells + 4 * ((size_t)r * nc + c);
          if (!(cb[0] == sgx0[c] && cb[1] == sgy0[r] && cb[2] == sgx1[c] && cb[3] == sgy1[r])) { ok = false; break; }
        }
      for (int c = 1; c < nc && ok; c++) ok = sgx0[c] >= sgx0[c - 1] && sgx1[c] >= sgx1[c - 1];
      for (int r = 1; r < nr && ok; r++) ok = sgy0[r] >= sgy0[r - 1] && sgy1[r] >= sgy1[r - 1];
      for (int c = 0; c < nc && ok; c++) ok = std::isfinite(sgx0[c]) && std::isfinite(sgx1[c]);
      for (int r = 0; r < nr && ok; r++) ok = std::isfinite(sgy0[r]) && std::isfinite(sgy1[r]);
      if (ok && grid_index) { sg_ncol = nc; sg_nrow = nr; }
    }
  }
  // what was gathered for a list that is no grid, or for an index that is switched off, goes: the sizes below are the index's
  sgx0.resize(sg_ncol); sgx1.resize(sg_ncol); sgy0.resize(sg_nrow); sgy1.resize(sg_nrow);
  std::vector<double>& col = t.sg_col;
  std::vector<double>& row = t.sg_row;
  col.assign((size_t)sg_ncol * 4, 0.0); row.assign((size_t)sg_nrow * 4, 0.0);
  for (int c = 0; c < sg_ncol; c++) { col[4 * (size_t)c] = c ? sgx1[c - 1] : -INFINITY; col[4 * (size_t)c + 1] = sgx1[c]; col[4 * (size_t)c + 2] = sgx0[c]; }
  for (int r = 0; r < sg_nrow; r++) { row[4 * (size_t)r] = r ? sgy1[r - 1] : -INFINITY; row[4 * (size_t)r + 1] = sgy1[r]; row[4 * (size_t)r + 2] = sgy0[r]; }
  t.sg_enabled = sg_ncol > 0 ? 1 : 0; t.sg_ncol = sg_ncol; t.sg_nrow = sg_nrow;
  t.sg_x1_0 = sg_ncol > 0 ? sgx1[0] : 0.0; t.sg_y1_0 = sg_nrow > 0 ? sgy1[0] : 0.0;
  t.sg_inv_dx = (sg_ncol > 1 && sgx1[sg_ncol - 1] > sgx1[0]) ? (double)(sg_ncol - 1) / (sgx1[sg_ncol - 1] - sgx1[0]) : 0.0;
  t.sg_inv_dy = (sg_nrow > 1 && sgy1[sg_nrow - 1] > sgy1[0]) ? (double)(sg_nrow - 1) / (sgy1[sg_nrow - 1] - sgy1[0]) : 0.0;
}

// obstacle tile in 16 slots of at most 16 + slot boxes for rrt_rows_kernel (auvp_types.h), and obst_area.  Reads ox, oy, ot of `t`.
// A steer looks into every slot whose box meets its reach square, so the grouping is the one whose boxes are met least often:
// a four-level median split (every group cut in two at the median of its centres along its longer axis: 16 groups, boxes that
// barely overlap), unless the runs of 16 along the Z curve -- the grouping before it -- come out strictly cheaper.  Which
// obstacles reach the exact test does not depend on the grouping: a slot's box contains the cull square of each of its obstacles.
inline void build_obstacle_slots(WorldTables& t) {
  const int O = (int)t.ox.size();
  const std::vector<double>&ox = t.ox, &oy = t.oy, &ot = t.ot;
  const int NS = 256;
  std::vector<double>& sx = t.os_x;
  std::vector<double>& sy = t.os_y;
  std::vector<double>& st = t.os_t;
  std::vector<double>& box = t.os_box;
  std::vector<float>& sr = t.os_r;
  sx.assign(NS, 0.0); sy.assign(NS, 0.0); st.assign(NS, -1.0); box.assign(16 * 4, 0.0);
  sr.assign(NS, -INFINITY);
  double x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;  // bounding box of the obstacle centres
  for (int i = 0; i < O; i++) { x0 = std::min(x0, ox[i]); x1 = std::max(x1, ox[i]); y0 = std::min(y0, oy[i]); y1 = std::max(y1, oy[i]); }
  t.obst_area = (O > 1 && std::isfinite((x1 - x0) * (y1 - y0))) ? (x1 - x0) * (y1 - y0) : 0.0;
  // the tile's entries from an order: entry k holds obstacle order[k] of the list, padding where that is -1
  auto place = [&](const std::vector<int>& order) {
    for (int k = 0; k < NS; k++) {
      const int i = order[k];
      if (i < 0) { sx[k] = 0.0; sy[k] = 0.0; st[k] = -1.0; sr[k] = -INFINITY; continue; }
      sx[k] = ox[i]; sy[k] = oy[i]; st[k] = ot[i];
      const double rd = ot[i] >= 0.0 ? std::sqrt(ot[i]) * (1.0 + 0x1p-30) + 0x1p-40 : -INFINITY;
      float rf = (float)rd;
      if ((double)rf < rd) rf = std::nextafter(rf, INFINITY);
      sr[k] = rf;
    }
  };
  auto slot_boxes = [&]() {
    for (int s_ = 0; s_ < 16; s_++) {
      double b0 = INFINITY, b1 = INFINITY, b2 = -INFINITY, b3 = -INFINITY;
      for (int k = 16 * s_; k < 16 * s_ + 16; k++) {
        if (!(sr[k] >= 0.0f) && !std::isnan(sx[k])) continue;  // padding / an obstacle that can never collide
        const double r = (double)sr[k];
        if (std::isnan(sx[k]) || std::isnan(sy[k]) || std::isnan(r)) { b0 = b1 = -INFINITY; b2 = b3 = INFINITY; break; }  // never culled
        b0 = std::min(b0, sx[k] - r); b1 = std::min(b1, sy[k] - r); b2 = std::max(b2, sx[k] + r); b3 = std::max(b3, sy[k] + r);
      }
      box[4 * s_] = b0; box[4 * s_ + 1] = b1; box[4 * s_ + 2] = b2; box[4 * s_ + 3] = b3;
    }
  };
  // What a grouping costs: a square of side m set down at random meets a w x h box with a probability that grows as
  // (w + m)(h + m), summed over the slots.  m = 30 m, the side of a steer's reach square at the planner's default step (its
  // half-width is a quarter of freq x dist_to_end = 15 m); one fixed figure for both groupings, read from no parameter.  An
  // empty slot costs nothing; a slot that is never culled (or whose box is not finite) is met by every steer, so those are
  // counted first and the sum over the others decides between groupings with as many of them
  auto boxes_cost = [&]() {
    const double m = 30.0;
    int unbounded = 0;
    double sum = 0.0;
    for (int s_ = 0; s_ < 16; s_++) {
      const double w = box[4 * s_ + 2] - box[4 * s_], h = box[4 * s_ + 3] - box[4 * s_ + 1];
      if (w < 0.0 && h < 0.0) continue;
      if (std::isfinite(w) && std::isfinite(h)) sum += (w + m) * (h + m);
      else unbounded++;
    }
    return std::make_pair(unbounded, sum);
  };
  if (O <= NS) {
    auto spread = [](uint32_t v) { uint64_t x = v & 0xffff; x = (x | (x << 8)) & 0x00ff00ff; x = (x | (x << 4)) & 0x0f0f0f0f;
                                   x = (x | (x << 2)) & 0x33333333; x = (x | (x << 1)) & 0x55555555; return x; };
    std::vector<std::pair<uint64_t, int>> key(O);
    for (int i = 0; i < O; i++) {
      const double fx = x1 > x0 ? (ox[i] - x0) / (x1 - x0) : 0.0, fy = y1 > y0 ? (oy[i] - y0) / (y1 - y0) : 0.0;
      const uint32_t qx = (uint32_t)std::min(65535.0, std::max(0.0, fx * 65535.0)), qy = (uint32_t)std::min(65535.0, std::max(0.0, fy * 65535.0));
      key[i] = {(std::isfinite(fx) && std::isfinite(fy)) ? (spread(qx) | (spread(qy) << 1)) : 0, i};
    }
    std::sort(key.begin(), key.end());
    std::vector<int> morton(NS, -1), median(NS, -1);  // entry k of the tile: the obstacle's index in the list, -1 padding
    for (int k = 0; k < O; k++) morton[k] = key[k].second;
    // the median split: idx[cut[g] .. cut[g + 1]) is group g; a cut leaves ceil(n / 2) and floor(n / 2), so 256 obstacles and
    // fewer end in 16 groups of at most 16.  Sorted by (coordinate, index in the list): the tables are deterministic.  A centre
    // that is not finite counts for no extent, a NaN sorts last
    std::vector<int> idx(O), cut = {0, O};
    for (int i = 0; i < O; i++) idx[i] = i;
    std::vector<std::pair<double, int>> ck;
    for (int level = 0; level < 4; level++) {
      std::vector<int> next;
      for (size_t g = 0; g + 1 < cut.size(); g++) {
        const int a = cut[g], n = cut[g + 1] - a;
        double gx0 = INFINITY, gy0 = INFINITY, gx1 = -INFINITY, gy1 = -INFINITY;
        for (int k = a; k < a + n; k++) {
          const double cx = ox[idx[k]], cy = oy[idx[k]];
          if (std::isfinite(cx)) { gx0 = std::min(gx0, cx); gx1 = std::max(gx1, cx); }
          if (std::isfinite(cy)) { gy0 = std::min(gy0, cy); gy1 = std::max(gy1, cy); }
        }
        const bool along_y = gy1 - gy0 > gx1 - gx0;  // (no finite centre: -inf on that side, never the longer axis)
        ck.resize(n);
        for (int k = 0; k < n; k++) {
          const double c = along_y ? oy[idx[a + k]] : ox[idx[a + k]];
          ck[k] = {std::isnan(c) ? INFINITY : c, idx[a + k]};
        }
        std::sort(ck.begin(), ck.end());
        for (int k = 0; k < n; k++) idx[a + k] = ck[k].second;
        next.push_back(a); next.push_back(a + (n + 1) / 2);
      }
      next.push_back(O);
      cut.swap(next);
    }
    for (int s_ = 0; s_ < 16; s_++)
      for (int k = cut[s_]; k < cut[s_ + 1]; k++) median[16 * s_ + (k - cut[s_])] = idx[k];
    // never worse than before: the Z-curve runs stay where their boxes are strictly cheaper
    place(morton);
    slot_boxes();
    const auto cost_morton = boxes_cost();
    place(median);
    slot_boxes();
    if (cost_morton < boxes_cost()) { place(morton); slot_boxes(); }
  } else {
    slot_boxes();
  }
}

// hab_t, and the habitat mask grid (auvp_types.h): 32 x 32 cells over the box of the habitats' cull squares; a habitat is
// entered into every cell its square touches, one cell of margin on each side against rounding in the cell arithmetic
inline HabitatTables build_habitat_tables(const double* habitats, int H, bool habitat_grid) {
  HabitatTables t;
  t.hab_t.resize(H > 0 ? H : 0);
  for (int i = 0; i < H; i++) t.hab_t[i] = sq_threshold(habitats[3 * i + 2]);
  if (H <= 0 || H > 64 || !habitat_grid) return t;
  const int G = 32;
  double x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
  std::vector<double> rr(H);
  for (int i = 0; i < H; i++) {
    const double th = t.hab_t[i];
    rr[i] = th >= 0.0 ? std::sqrt(th) * (1.0 + 0x1p-30) + 0x1p-40 : -1.0;
    const double hx = habitats[3 * i], hy = habitats[3 * i + 1];
    if (!std::isfinite(hx) || !std::isfinite(hy) || !std::isfinite(rr[i])) return t;  // odd input: keep the plain scan
    if (rr[i] < 0.0) continue;  // can never contain a point
    x0 = std::min(x0, hx - rr[i]); x1 = std::max(x1, hx + rr[i]);
    y0 = std::min(y0, hy - rr[i]); y1 = std::max(y1, hy + rr[i]);
  }
  std::vector<unsigned long long> mask((size_t)G * G, 0ull);
  if (x1 >= x0 && y1 >= y0) {
    // grow the box a little so that every square lies strictly inside it
    const double mx = 1e-6 * (std::fabs(x0) + std::fabs(x1) + 1.0), my = 1e-6 * (std::fabs(y0) + std::fabs(y1) + 1.0);
    x0 -= mx; x1 += mx; y0 -= my; y1 += my;
    const double iw = (double)G / (x1 - x0), ih = (double)G / (y1 - y0);
    for (int i = 0; i < H; i++) {
      if (rr[i] < 0.0) continue;
      const double hx = habitats[3 * i], hy = habitats[3 * i + 1];
      int cx0 = (int)std::floor((hx - rr[i] - x0) * iw) - 1, cx1 = (int)std::floor((hx + rr[i] - x0) * iw) + 1;
      int cy0 = (int)std::floor((hy - rr[i] - y0) * ih) - 1, cy1 = (int)std::floor((hy + rr[i] - y0) * ih) + 1;
      cx0 = std::max(cx0, 0); cy0 = std::max(cy0, 0); cx1 = std::min(cx1, G - 1); cy1 = std::min(cy1, G - 1);
      for (int cy = cy0; cy <= cy1; cy++)
        for (int cx = cx0; cx <= cx1; cx++) mask[(size_t)cy * G + cx] |= 1ull << i;
    }
    t.hg_x0 = x0; t.hg_y0 = y0; t.hg_inv_w = iw; t.hg_inv_h = ih;
  }
  // (else no habitat can contain anything: every cell empty, origin and scale 0)
  t.hg_mask = std::move(mask);
  t.hg_n = G;
  return t;
}

// max |prob| and whether two entries differ in sign
inline void build_prob_stats(const double* prob, size_t n, WorldTables& t) {
  double prob_absmax = 0.0;
  bool any_pos = false, any_neg = false, any_nan = false;
  for (size_t i = 0; i < n; i++) {
    const double a = std::fabs(prob[i]);
    if (a > prob_absmax || a != a) prob_absmax = a;  // a nan poisons the bound: every leaf is then re-summed exactly
    any_pos |= prob[i] > 0; any_neg |= prob[i] < 0; any_nan |= prob[i] != prob[i];
  }
  t.prob_absmax = prob_absmax;
  t.prob_one_sign = (!any_nan && !(any_pos && any_neg)) ? 1 : 0;
}

// constants of the time-bin guess
inline void build_bin_guess(const double* bins, int T, WorldTables& t) {
  bool sorted = T > 0;
  for (int k = 0; k < T && sorted; k++) sorted = std::isfinite(bins[2 * k]) && std::isfinite(bins[2 * k + 1]);
  for (int k = 1; k < T && sorted; k++) sorted = bins[2 * k] >= bins[2 * (k - 1)] && bins[2 * k + 1] >= bins[2 * (k - 1) + 1];
  t.bins_sorted = sorted ? 1 : 0;
  t.bins_t1_0 = T > 0 ? bins[1] : 0.0;
  t.bins_inv_len = (sorted && T > 1 && bins[2 * (T - 1) + 1] > bins[1]) ? (double)(T - 1) / (bins[2 * (T - 1) + 1] - bins[1]) : 0.0;
}

// polygon bounds, and the safe box
inline void build_polygon_boxes(const double* polygon, int V, WorldTables& t) {
  double bb[4] = {INFINITY, INFINITY, -INFINITY, -INFINITY};
  for (int i = 0; i < V; i++) {
    bb[0] = std::min(bb[0], polygon[2 * i]); bb[1] = std::min(bb[1], polygon[2 * i + 1]);
    bb[2] = std::max(bb[2], polygon[2 * i]); bb[3] = std::max(bb[3], polygon[2 * i + 1]);
  }
  memcpy(t.bb, bb, sizeof bb);
  // axis-aligned rectangle given by its 4 corners: strict containment in it implies Point.within
  t.has_safe_box = 0;
  memset(t.safe_box, 0, sizeof t.safe_box);
  if (V == 4) {
    bool rect = true;
    for (int i = 0; i < 4 && rect; i++) {
      const double x0 = polygon[2 * i], y0 = polygon[2 * i + 1], x1 = polygon[2 * ((i + 1) % 4)], y1 = polygon[2 * ((i + 1) % 4) + 1];
      const bool horiz = (y0 == y1) && (x0 != x1), vert = (x0 == x1) && (y0 != y1);
      const double x2 = polygon[2 * ((i + 2) % 4)], y2 = polygon[2 * ((i + 2) % 4) + 1];
      const bool next_vert = (x1 == x2) && (y1 != y2), next_horiz = (y1 == y2) && (x1 != x2);
      rect = (horiz && next_vert) || (vert && next_horiz);
    }
    if (rect) { t.has_safe_box = 1; memcpy(t.safe_box, bb, sizeof bb); }
  }
}

inline WorldTables build_world_tables(const WorldIn& in) {
  WorldTables t;
  build_obstacle_thresholds(in.obstacles, in.O, t);
  build_xbuckets(in.cells, in.C, t);
  build_region_index(in.cells, in.C, in.rg_max_entries, t);
  build_separable_grid(in.cells, in.C, in.grid_index, t);
  build_obstacle_slots(t);
  t.hab = build_habitat_tables(in.habitats, in.H, in.habitat_grid);
  build_prob_stats(in.prob, (size_t)in.T * in.C, t);
  build_bin_guess(in.bins, in.T, t);
  build_polygon_boxes(in.polygon, in.V, t);
  return t;
}

}  // namespace auvp
#endif

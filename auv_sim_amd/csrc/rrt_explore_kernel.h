// rrt_explore_kernel.h -- RRT.exploring (path_planning/rrt_dubins.py:92-176) on gfx950.
//
// One wavefront = one episode, persistent over the whole iteration budget.  A 512-thread workgroup
// carries 8 independent episodes that share the LDS copy of the small world tables (habitats,
// polygon, time bins, obstacle tile); the tree lives in HBM.
//
// Inside one expansion the 64 lanes split the work:
//   steer        lane s = sub-arc s: RNG window tempering, arc geometry and sin/cos in parallel;
//                only the running sums (theta; then x, y, t, length on four lanes) are serial, and
//                they must be, to keep the reference's left-to-right fp64 addition order
//   collision    cull: lane = obstacle (J slots of 64) against the path's bounding box; the few candidates that
//                survive are tested one at a time with lane = path point
//   polygon      lane = path point
//   cost         not here: the qualifying-leaf cost of exploring (:158-171) only decides which leaf is returned, never
//                how the tree grows, so rrt_leaf_kernel evaluates it on the finished tree (lane = node, all lanes busy)
// The steer draw count is data dependent (a sub-arc consumes 2 or 3 random() values): the lanes
// temper a window of the stream, ballot the "taken" predicate for every possible start offset, and
// a lane-parallel fixed-point iteration resolves where each sub-arc starts.
//
// Everything that is the same for all lanes of an episode is forced into SGPRs (readfirstlane), so
// episode-level control flow is scalar branches and the VGPR budget stays with the per-lane work.
#ifndef AUVP_RRT_EXPLORE_KERNEL_H
#define AUVP_RRT_EXPLORE_KERNEL_H
#include "auvp_math.h"
#include "auvp_types.h"
#include "auvp_wave.h"

namespace auvp {

constexpr int RRT_WAVES = 4;       // episodes per workgroup (Planner_RRT)
// RRT.exploring: 8 episodes share one copy of the world tables and the obstacle tile, so three workgroups (24 waves,
// six per SIMD) fit the CU's 160 KB of LDS; the register budget for six waves is 80 VGPRs, and what does not fit
// (loop-invariant lane constants) is spilled once and reloaded about twice per expansion
constexpr int RRT_X_WAVES = 8;
constexpr int RRT_MAX_CHUNK = 63;  // sub-arcs per steer pass (one lane stays idle: chunk-entry angle)
constexpr int RRT_MAX_HAB = 64;    // visited-habitat mask is one 64-bit word
constexpr int RRT_MAX_POLY = 64;
constexpr int RRT_MAX_BINS = 64;
constexpr int RRT_ELIST = 192;     // path elements collected per cost pass group

// The world tables every episode of a workgroup shares, at the start of its LDS and sized by the world at hand
// (a fixed 64-row layout costs 4.4 KB where the Catalina-like world needs 0.9 KB; LDS is what limits the number of
// resident episodes per CU):
//   [WorldDev]  copy of the kernel argument for the code that runs rarely (evaluating a path element for the
//               cost): reading the table pointers from here when they are needed keeps ~40 scalar registers out
//               of the expansion loop, which otherwise spills them to vector-register lanes
//   [RrtParamsDev]  copy of the planning parameters (rrt_explore_kernel)
//   [hab]       n_habitats x {x, y, size, T(size)}      [poly] n_poly x {x, y}      [bins] n_bins x {t0, t1}
struct RrtTables {
  WorldDev* world;
  RrtParamsDev* params;  // RRT.exploring only (staged by the kernel itself)
  double (*hab)[4];
  double (*poly)[2];
  double (*bins)[2];
};
constexpr int RRT_WORLD_ONLY_BYTES = (int)((sizeof(WorldDev) + 15) & ~(size_t)15);
constexpr int RRT_WORLD_BYTES = RRT_WORLD_ONLY_BYTES + (int)((sizeof(RrtParamsDev) + 15) & ~(size_t)15);
__host__ __device__ inline int rrt_tables_bytes(int n_habitats, int n_poly, int n_bins) {
  return RRT_WORLD_BYTES + n_habitats * 32 + n_poly * 16 + n_bins * 16;
}
__device__ __forceinline__ RrtTables rrt_tables_view(unsigned char* base, int n_habitats, int n_poly) {
  RrtTables t;
  t.world = reinterpret_cast<WorldDev*>(base);
  t.params = reinterpret_cast<RrtParamsDev*>(base + RRT_WORLD_ONLY_BYTES);
  t.hab = reinterpret_cast<double(*)[4]>(base + RRT_WORLD_BYTES);
  t.poly = reinterpret_cast<double(*)[2]>(base + RRT_WORLD_BYTES + n_habitats * 32);
  t.bins = reinterpret_cast<double(*)[2]>(base + RRT_WORLD_BYTES + n_habitats * 32 + n_poly * 16);
  return t;
}
// fill the tables (whole workgroup; the caller synchronises)
__device__ __forceinline__ void rrt_tables_stage(const RrtTables& S, const WorldDev& W) {
  for (int i = threadIdx.x; i < W.n_habitats; i += blockDim.x) {
    S.hab[i][0] = W.hab[3 * i]; S.hab[i][1] = W.hab[3 * i + 1]; S.hab[i][2] = W.hab[3 * i + 2];
    S.hab[i][3] = W.hab_t[i];
  }
  if (threadIdx.x == 0) *S.world = W;
  for (int i = threadIdx.x; i < W.n_poly * 2; i += blockDim.x) (&S.poly[0][0])[i] = W.poly[i];
  for (int i = threadIdx.x; i < W.n_bins * 2; i += blockDim.x) (&S.bins[0][0])[i] = W.bins[i];
}

// Per-wave LDS layout (bytes), all sizes multiples of 16:
//   [scratch]  steer: u[3C+3] | {inc[(C+1)*4], sc[(C+1)*2], phi[C+1]}
//   [mt]       624 u32
//   [pts]      max_pts * 2 f64
//   [bins]     (K+2) i32
// before them the world tables (RrtTables); after the RRT_X_WAVES per-wave blocks the obstacle tile shared by the
// workgroup: x, y, T as f64 [J*64] each and the cull radius as f32 [J*64]
struct RrtLdsPlan {
  int chunk;  // C
  int tables, scratch, mt, pts, bins, per_wave, total;
};

__host__ __device__ inline RrtLdsPlan rrt_lds_plan(int K, int max_pts, int nfreq, int obst_slots, int tables_bytes,
                                                   int waves = RRT_X_WAVES) {
  RrtLdsPlan p;
  p.chunk = nfreq < 1 ? 1 : (nfreq > RRT_MAX_CHUNK ? RRT_MAX_CHUNK : nfreq);
  const int C = p.chunk;
  int steer_u = (64 + 3 * C + 3) * 8;  // 64 leading random() values + the steer window
  // inc rows, sc and phi all padded to the even row length CS = C + 1 rounded up
  int steer_s = (7 * ((C + 2) & ~1) + 4) * 8;
  int s = steer_u > steer_s ? steer_u : steer_s;
  p.scratch = (s + 15) & ~15;
  p.mt = 624 * 4;
  p.pts = ((max_pts * 16) + 15) & ~15;
  p.bins = (((K + 2) * 4) + 15) & ~15;
  p.per_wave = p.scratch + p.mt + p.pts + p.bins;
  p.tables = (tables_bytes + 15) & ~15;
  p.total = p.tables + waves * p.per_wave + obst_slots * (3 * 8 + 4);  // + obstacle tile x,y,T (f64), r (f32)
  return p;
}

// Point(x,y).within(polygon): even-odd crossing number with strict comparisons -- the definition
// pinned in tests/golden/_refstubs/install.py (shapely itself is absent).
// Wave-parallel over (point, edge) pairs: lane = p_local * nv + e, so one pass evaluates the edge
// test (with its fp64 division) for floor(64/nv) points at once; a point is inside iff the number
// of crossing edges in its nv-bit group of the ballot is odd.  Returns true when ANY of the
// n_pts points is not strictly inside.
__device__ __forceinline__ bool any_point_outside(const double (*poly)[2], int nv, const double (*pts)[2], int n_pts) {
  const int lane = lane_id();
  // no boundary polygon: no point is within it (the crossing loop of the definition never runs), so a path
  // with any point at all is outside; also keeps 64 / nv below well defined
  if (nv <= 0) return n_pts > 0;
  const int per = 64 / nv;  // points per pass (nv <= 64)
  const int e = lane % nv, pl = lane / nv;
  const int ej = e == 0 ? nv - 1 : e - 1;  // j trails i by one vertex
  const double xi = poly[e][0], yi = poly[e][1], xj = poly[ej][0], yj = poly[ej][1];
  bool outside = false;
  for (int p0 = 0; p0 < n_pts; p0 += per) {
    const int p = p0 + pl;
    const bool live = pl < per && p < n_pts;
    bool cross = false;
    if (live) {
      const double x = pts[p][0], y = pts[p][1];
      if ((yi > y) != (yj > y)) cross = x < (xj - xi) * (y - yi) / (yj - yi) + xi;
    }
    const unsigned long long cm = wave_ballot(cross);
    // lanes 0..per-1 each judge one point of this pass
    const int q = p0 + lane;
    if (lane < per && q < n_pts) {
      const unsigned long long grp = (cm >> (lane * nv)) & (nv == 64 ? ~0ull : ((1ull << nv) - 1ull));
      outside = outside | ((__popcll(grp) & 1) == 0);
    }
  }
  return wave_any(outside);
}

// cost.py:181-184 first-match cell scan through the x-bucket index; returns cell id or -1
// first index i in [0, n) with a[i] >= v (n if none): lower bound on a non-decreasing table, found from a guess by
// comparing against the table's own values, so the result is exact whatever the guess
__device__ __forceinline__ int lower_bound_from(const double* __restrict__ a, int n, double v, int i) {
  i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
  while (i > 0 && a[i - 1] >= v) i--;
  while (i < n && a[i] < v) i++;
  return i;
}

// `grid_lds`: optional copy of the separable-grid tables in LDS, laid out X1[ncol] X0[ncol] Y1[nrow] Y0[nrow]
__device__ __forceinline__ int cell_lookup(const WorldDev& W, double x, double y, const double* grid_lds = nullptr) {
  if (W.n_cells == 0) return -1;
  if (W.sg_enabled && grid_lds) {
    const double *x1 = grid_lds, *x0 = grid_lds + W.sg_ncol, *y1 = x0 + W.sg_ncol, *y0 = y1 + W.sg_nrow;
    int c = (int)auvp_floor((x - W.sg_x1_0) * W.sg_inv_dx) + 1, r = (int)auvp_floor((x - W.sg_y1_0) * W.sg_inv_dy) + 1;
    c = c < 0 ? 0 : (c > W.sg_ncol - 1 ? W.sg_ncol - 1 : c);
    r = r < 0 ? 0 : (r > W.sg_nrow - 1 ? W.sg_nrow - 1 : r);
    // the guess is the lower bound iff a1[g-1] < v <= a1[g]: checked without a loop; the stepping search only runs for
    // the rare lane whose guess is off (rounding next to an edge, a point outside the grid)
    const double xc1 = x1[c], xcm = c > 0 ? x1[c - 1] : -__builtin_inf();
    const double yr1 = y1[r], yrm = r > 0 ? y1[r - 1] : -__builtin_inf();
    if (!(xcm < x && xc1 >= x)) c = lower_bound_from(x1, W.sg_ncol, x, c);
    if (!(yrm < x && yr1 >= x)) r = lower_bound_from(y1, W.sg_nrow, x, r);
    if (c >= W.sg_ncol || r >= W.sg_nrow) return -1;
    return (x0[c] <= x && y0[r] <= y) ? r * W.sg_ncol + c : -1;
  }
  if (W.sg_enabled) {
    // row-major grid: first row with Y0[r] <= y and x <= Y1[r] (sic, cost.py:182), first column with X0[c] <= x <= X1[c].
    // Both guesses are checked with one independent 32-byte read each (the usual case: one round trip); a guess that
    // is off -- rounding next to a cell edge, or a point outside the grid -- falls back to the stepping search.
    int gc = (int)auvp_floor((x - W.sg_x1_0) * W.sg_inv_dx) + 1, gr = (int)auvp_floor((x - W.sg_y1_0) * W.sg_inv_dy) + 1;
    gc = gc < 0 ? 0 : (gc > W.sg_ncol - 1 ? W.sg_ncol - 1 : gc);
    gr = gr < 0 ? 0 : (gr > W.sg_nrow - 1 ? W.sg_nrow - 1 : gr);
    const double4 cc = reinterpret_cast<const double4*>(W.sg_col)[gc];
    const double4 rr = reinterpret_cast<const double4*>(W.sg_row)[gr];
    if (cc.x < x && cc.y >= x && rr.x < x && rr.y >= x) return (cc.z <= x && rr.z <= y) ? gr * W.sg_ncol + gc : -1;
    const int c = lower_bound_from(W.sg_x1, W.sg_ncol, x, gc);
    const int r = lower_bound_from(W.sg_y1, W.sg_nrow, x, gr);
    if (c >= W.sg_ncol || r >= W.sg_nrow) return -1;
    if (!(W.sg_x0[c] <= x) || !(W.sg_y0[r] <= y)) return -1;
    return r * W.sg_ncol + c;
  }
  double fb = auvp_floor((x - W.xb_x0) * W.xb_inv_w);
  int b = fb < 0.0 ? 0 : (fb >= (double)W.n_xbuckets ? W.n_xbuckets - 1 : (int)fb);
  if (W.rg_enabled) {
    // region of x: breakpoints in earlier buckets are < x, in later buckets > x (the bucket map is monotone)
    int lo = W.rg_first[b], hi = W.rg_first[b + 1];
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (W.rg_bp[mid] < x) lo = mid + 1; else hi = mid; }
    const int r = 2 * lo + ((lo < W.n_rg_bp && W.rg_bp[lo] == x) ? 1 : 0);
    const int s = W.rg_off[r], e = W.rg_off[r + 1];
    if (s == e) return -1;
    if (W.rg_pm[s] <= y) return W.rg_id[s];      // the usual case on a grid
    if (!(W.rg_pm[e - 1] <= y)) return -1;       // no candidate reaches down to y
    lo = s; hi = e - 1;                          // pm[lo] > y >= pm[hi]: first index with pm <= y
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (W.rg_pm[mid] <= y) hi = mid; else lo = mid; }
    return W.rg_id[hi];
  }
  int e = W.xb_off[b + 1];
  for (int k = W.xb_off[b]; k < e; k++) {
    const double4 d = reinterpret_cast<const double4*>(W.xb_data)[k];
    if (y < d.w) return -1;  // every remaining candidate has miny > y
    // sic: x is compared with maxy as well as maxx (path_planning/cost.py:182): d.y = min(maxx, maxy)
    if (x >= d.x && x <= d.y && y >= d.z) return W.xb_items[k];
  }
  return -1;
}

// ---- time-bin member lists (RrtBuffers::bin_items): direct-mapped head + on-demand 64-entry chunks --------------------
// (every index below fits 32 bits: the host refuses a bin_stride of 2^31 words or more)
struct BinLists {
  int32_t* direct;  // [K+1][AUVP_BIN_HEAD]
  int32_t* over;    // [n_over][64]
  int32_t* dir;     // [n_slots][K+1]
  int n_over, k1;
};

__device__ __forceinline__ BinLists bin_lists(const RrtBuffers& B, size_t episode, int K) {
  BinLists L;
  L.n_over = B.bin_over; L.k1 = K + 1;
  L.direct = B.bin_items + episode * (size_t)B.bin_stride;
  L.over = L.direct + (size_t)L.k1 * AUVP_BIN_HEAD;
  L.dir = L.over + (size_t)L.n_over * 64;
  return L;
}

// member k of bin b
__device__ __forceinline__ int bin_member(const BinLists& L, int b, int k) {
  if (k < AUVP_BIN_HEAD) return L.direct[b * AUVP_BIN_HEAD + k];
  const int kk = k - AUVP_BIN_HEAD;
  const int chunk = L.dir[(kk >> 6) * L.k1 + b];
  return L.over[chunk * 64 + (kk & 63)];
}

// where member c of bin b goes (nullptr: out of chunks).  The values are uniform over the episode's lanes, every lane
// keeps its copy of next_chunk; only `writer` touches memory.
__device__ __forceinline__ int32_t* bin_slot_for_append(const BinLists& L, int b, int c, int& next_chunk, bool writer) {
  if (c < AUVP_BIN_HEAD) return L.direct + (b * AUVP_BIN_HEAD + c);
  const int kk = c - AUVP_BIN_HEAD;
  int32_t* d = L.dir + ((kk >> 6) * L.k1 + b);
  int chunk;
  if ((kk & 63) == 0) {
    if (next_chunk >= L.n_over) return nullptr;
    chunk = next_chunk++;
    if (writer) *d = chunk;
  } else {
    chunk = *d;
  }
  return L.over + (chunk * 64 + (kk & 63));
}

struct CostAcc {
  double c2;                   // running shark term, summed in path order
  unsigned long long visited;  // habitat bit set
  int hits;                    // number of path points inside some habitat
};

// One path element of habitat_shark_cost_func (path_planning/cost.py:171-193): its shark term w3*prob
// (0.0 when it has none: x + 0.0 == x, an exact no-op in the ordered sum) and the first habitat that
// contains it (-1: none).  An element whose time stamp lies in no bin of [bin_lo, bin_hi) is skipped
// entirely by the reference: (0.0, -1).
// `hab_near` (wave-uniform): false when the caller knows that no habitat can contain the element (its bounding-box
// cull), which skips the habitat scan.
// LIM: only the habitats whose bit is set in `keep` are on the list (the per-episode limits of rrt_leaf_lim_kernel); the
// first match is still taken in table order, which is the order of the shortened list.
template <bool LIM = false>
__device__ __forceinline__ void cost_element(const WorldDev& W, const RrtTables& S, int bin_lo, int bin_hi, double w3,
                                             double x, double y, double t, double& tv, int& hab, bool hab_near = true,
                                             const double* grid_lds = nullptr, unsigned long long keep = ~0ull) {
  int tb = -1;
  if (W.bins_sorted) {
    // bins with non-decreasing ends: the first match is the first bin whose upper end reaches t, if it starts at or
    // before t -- a lower bound, checked against the table's own values (LDS)
    if (bin_hi > bin_lo) {
      int i = (int)auvp_floor((t - W.bins_t1_0) * W.bins_inv_len) + 1;
      i = i < bin_lo ? bin_lo : (i > bin_hi - 1 ? bin_hi - 1 : i);
      const double2 bi = *reinterpret_cast<const double2*>(&S.bins[i][0]);
      const double pm = i > bin_lo ? S.bins[i - 1][1] : -__builtin_inf();
      if (pm < t && bi.y >= t) {  // the guess is the lower bound (the usual case: no loop)
        if (bi.x <= t) tb = i;
      } else {
        while (i > bin_lo && S.bins[i - 1][1] >= t) i--;
        while (i < bin_hi && S.bins[i][1] < t) i++;
        if (i < bin_hi && S.bins[i][0] <= t) tb = i;
      }
    }
  } else {
    // first matching bin in table order, scanned backwards without early exits (the last overwrite is the first
    // match): the table reads (one LDS address for all lanes) are then independent of the compares
    for (int b = bin_hi - 1; b >= bin_lo; b--) {
      const double2 r = *reinterpret_cast<const double2*>(&S.bins[b][0]);
      tb = (t >= r.x && t <= r.y) ? b : tb;
    }
  }
  tv = 0.0;
  hab = -1;
  if (tb >= 0) {
    int c = cell_lookup(W, x, y, grid_lds);
    if (c >= 0) tv = w3 * W.prob[(size_t)tb * W.n_cells + c];
    if (hab_near) {
      if (W.hg_n > 0) {
        // habitat mask grid: the few habitats whose bounding square touches the point's cell, in list order
        const double fx = auvp_floor((x - W.hg_x0) * W.hg_inv_w), fy = auvp_floor((y - W.hg_y0) * W.hg_inv_h);
        unsigned long long m = 0ull;
        if (fx >= 0.0 && fy >= 0.0 && fx < (double)W.hg_n && fy < (double)W.hg_n) m = W.hg_mask[(int)fy * W.hg_n + (int)fx];
        if constexpr (LIM) m &= keep;
        while (m) {
          const int h = __ffsll((long long)m) - 1;
          m &= m - 1ull;
          const double2 hxy = *reinterpret_cast<const double2*>(&S.hab[h][0]);
          const double ddx = hxy.x - x, ddy = hxy.y - y;
          if (ddx * ddx + ddy * ddy <= S.hab[h][3]) { hab = h; break; }
        }
      } else {
        for (int h = W.n_habitats - 1; h >= 0; h--) {
          // dist <= size  <=>  d2 <= T(size): same decision as RN(sqrt(d2)) <= size, no sqrt
          const double2 hxy = *reinterpret_cast<const double2*>(&S.hab[h][0]);
          const double ddx = hxy.x - x, ddy = hxy.y - y;
          if constexpr (LIM) hab = (ddx * ddx + ddy * ddy <= S.hab[h][3] && ((keep >> h) & 1ull)) ? h : hab;
          else hab = (ddx * ddx + ddy * ddy <= S.hab[h][3]) ? h : hab;
        }
      }
    }
  }
}

// One pass of up to 64 evaluated elements (lane order = path order) into the running cost.
// `term` is 64 doubles of wave LDS.
__device__ __forceinline__ void cost_accumulate(int n_valid, double tv, int hab, double* term, CostAcc& acc) {
  const int lane = lane_id();
  term[lane] = tv;
  unsigned long long hm = wave_ballot(hab >= 0);
  acc.hits += __popcll(hm);
  unsigned long long vis = acc.visited;
  while (hm) {  // at most H distinct habitats; usually one or two per pass
    int l = __ffsll((long long)hm) - 1;
    int h = __builtin_amdgcn_readlane(hab, l);
    vis |= (1ull << h);
    hm &= ~wave_ballot(hab == h);
  }
  acc.visited = vis;
  wave_sync();
  // cost[2] += w3*prob in path order: one dependent add per element, LDS reads run ahead
  // Entries past n_valid hold +0.0 (every lane stored its tv) and c2 is never -0.0, so adding them is an exact
  // no-op: the sum runs in batches of 8 -- 8 LDS reads in flight, then 8 dependent adds.
  double c2 = acc.c2;
  for (int i = 0; i < n_valid; i += 8) {
    double2 v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = *reinterpret_cast<const double2*>(term + i + 2 * k);
#pragma unroll
    for (int k = 0; k < 4; k++) { c2 = c2 + v[k].x; c2 = c2 + v[k].y; }
  }
  acc.c2 = c2;
  wave_sync();
}

// cost_element in two halves, for callers that evaluate several elements per lane (the leaf pass): cost_pre does the index
// arithmetic (time bin, cell, habitat-mask cell; LDS tables only when grid_lds is given), the CALLER then issues the two
// global reads of every element back to back -- prob[tb][c] and the habitat mask word -- and cost_post finishes.  Same
// decisions and the same floats as cost_element (which stays the one-element form).
struct CostPre {
  int tb, c, midx;  // time bin (-1: none: the element is skipped), cell (-1: none), habitat-mask cell (-1: outside / no mask grid)
};
__device__ __forceinline__ CostPre cost_pre(const WorldDev& W, const RrtTables& S, int bin_lo, int bin_hi, double x, double y, double t,
                                            const double* grid_lds) {
  CostPre q;
  q.tb = -1; q.c = -1; q.midx = -1;
  if (W.bins_sorted) {
    if (bin_hi > bin_lo) {
      int i = (int)auvp_floor((t - W.bins_t1_0) * W.bins_inv_len) + 1;
      i = i < bin_lo ? bin_lo : (i > bin_hi - 1 ? bin_hi - 1 : i);
      const double2 bi = *reinterpret_cast<const double2*>(&S.bins[i][0]);
      const double pm = i > bin_lo ? S.bins[i - 1][1] : -__builtin_inf();
      if (pm < t && bi.y >= t) {
        if (bi.x <= t) q.tb = i;
      } else {
        while (i > bin_lo && S.bins[i - 1][1] >= t) i--;
        while (i < bin_hi && S.bins[i][1] < t) i++;
        if (i < bin_hi && S.bins[i][0] <= t) q.tb = i;
      }
    }
  } else {
    for (int b = bin_hi - 1; b >= bin_lo; b--) {
      const double2 r = *reinterpret_cast<const double2*>(&S.bins[b][0]);
      q.tb = (t >= r.x && t <= r.y) ? b : q.tb;
    }
  }
  if (q.tb >= 0) {
    q.c = cell_lookup(W, x, y, grid_lds);
    if (W.hg_n > 0) {
      const double fx = auvp_floor((x - W.hg_x0) * W.hg_inv_w), fy = auvp_floor((y - W.hg_y0) * W.hg_inv_h);
      if (fx >= 0.0 && fy >= 0.0 && fx < (double)W.hg_n && fy < (double)W.hg_n) q.midx = (int)fy * W.hg_n + (int)fx;
    }
  }
  return q;
}
template <bool LIM = false>
__device__ __forceinline__ void cost_post(const WorldDev& W, const RrtTables& S, double w3, double x, double y, const CostPre& q,
                                          double prob, unsigned long long m, double& tv, int& hab, unsigned long long keep = ~0ull) {
  tv = 0.0;
  hab = -1;
  if (q.tb >= 0) {
    if (q.c >= 0) tv = w3 * prob;
    if (W.hg_n > 0) {
      if constexpr (LIM) m &= keep;
      while (m) {
        const int h = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        const double2 hxy = *reinterpret_cast<const double2*>(&S.hab[h][0]);
        const double ddx = hxy.x - x, ddy = hxy.y - y;
        if (ddx * ddx + ddy * ddy <= S.hab[h][3]) { hab = h; break; }
      }
    } else {
      for (int h = W.n_habitats - 1; h >= 0; h--) {
        const double2 hxy = *reinterpret_cast<const double2*>(&S.hab[h][0]);
        const double ddx = hxy.x - x, ddy = hxy.y - y;
        if constexpr (LIM) hab = (ddx * ddx + ddy * ddy <= S.hab[h][3] && ((keep >> h) & 1ull)) ? h : hab;
        else hab = (ddx * ddx + ddy * ddy <= S.hab[h][3]) ? h : hab;
      }
    }
  }
}

// evaluate + accumulate up to 64 elements given by value (the standalone cost probe)
__device__ __forceinline__ void cost_pass(const WorldDev& W, const RrtTables& S, int bin_lo, int bin_hi, double w3,
                                          int n_valid, double x, double y, double t, double* term, CostAcc& acc) {
  double tv = 0.0;
  int hab = -1;
  if (lane_id() < n_valid) cost_element(W, S, bin_lo, bin_hi, w3, x, y, t, tv, hab);
  cost_accumulate(n_valid, tv, hab, term, acc);
}

// ---- get_closest_mps (path_planning/rrt_dubins.py:505-513) as a streaming scan ------------------------------------------
// The reference walks mps_list and keeps the FIRST node with the smallest dist = RN(sqrt(dx**2 + dy**2)) (strict <).  The
// scan reads the episode's contiguous x,y mirror (16 B per node: one global_load_dwordx4 per lane, RRT_NN_UNROLL of them in
// flight per lane, 1 KB per wave-instruction) and ranks by the SQUARED distance -- sqrt is monotone, so the minimum of
// RN(sqrt(d2)) is taken where d2 is smallest -- with two running minima per lane:
//   bd / bt  smallest d2 of the lane's nodes and the block it first appeared in (strict <: the first of equal values)
//   sd       second smallest DISTINCT d2 of the lane's nodes (a value equal to the running minimum is skipped: duplicated
//            positions are common -- a steer with zero sub-arcs copies its parent -- and a lane that holds the minimum
//            twice must still see a third, slightly larger value)
// Afterwards gmin = wave minimum of bd.  Two different d2 can still round to the same sqrt; such a value lies within a few
// ulps above gmin.  A lane's values other than its smallest are all >= its sd (sd is the smallest value that differs from
// the final bd: a value skipped as "equal to the running minimum" either equals the final bd or was that minimum when a
// smaller one replaced it, which put it into sd), so if no lane's bd or sd falls in (gmin, gmin (1 + 2^-49)] no node at all
// has its d2 there: every node with RN(sqrt(d2)) == RN(sqrt(gmin)) has d2 == gmin exactly, and the answer is the smallest
// index among them.
// Otherwise (never observed: it needs two nodes equidistant from the sample to 1e-15) the scan is repeated the reference's
// way, sqrt per node.  Entries past the tree's end hold +inf: a block is always read whole.
// (RRT_NN_UNROLL, RRT_NN_BLOCK and rrt_nn_stride: auvp_types.h, where the host's sizing reads them too)

// `force_exact` (wave-uniform): take the sqrt-per-node path regardless (tests); `*slow` reports which path ran.
__device__ __forceinline__ int nn_closest(const double2* __restrict__ xy, int n_nodes, double rx, double ry, bool force_exact = false,
                                          int* slow = nullptr) {
  const int lane = lane_id();
  const double inf = __builtin_inf();
  double bd = inf, sd = inf;
  int bt = 0;
  for (int base = 0; base < n_nodes; base += RRT_NN_BLOCK) {
    double2 q[RRT_NN_UNROLL];
#pragma unroll
    for (int u = 0; u < RRT_NN_UNROLL; u++) q[u] = xy[base + u * 64 + lane];
#pragma unroll
    for (int u = 0; u < RRT_NN_UNROLL; u++) {
      const double ddx = rx - q[u].x, ddy = ry - q[u].y;
      const double d2 = ddx * ddx + ddy * ddy;
      const bool lt = d2 < bd;
      // the larger of {old minimum, newcomer} competes for second place -- unless they are equal (second DISTINCT value)
      sd = (d2 != bd) ? __builtin_fmin(sd, __builtin_fmax(bd, d2)) : sd;
      bd = lt ? d2 : bd;
      bt = lt ? base + u * 64 : bt;
    }
  }
  const double gmin = wave_min_f64(bd);
  const double band = gmin + gmin * 0x1p-49;
  const bool suspect = (bd > gmin && bd <= band) || (sd > gmin && sd <= band);
  int cand = 0x7fffffff;
  const bool exact = wave_any(suspect) || force_exact;
  if (slow) *slow = exact ? 1 : 0;
  if (!exact) {
    const unsigned long long em = wave_ballot(bd == gmin);
    if (__popcll(em) == 1) return uni(__builtin_amdgcn_readlane(bt, __ffsll((long long)em) - 1) + (__ffsll((long long)em) - 1));
    cand = (bd == gmin) ? bt + lane : 0x7fffffff;
  } else {
    // the reference's own ranking
    double bs = inf;
    for (int m = lane; m < n_nodes; m += 64) {
      const double2 q = xy[m];
      const double ddx = rx - q.x, ddy = ry - q.y;
      const double d = auvp_sqrt(ddx * ddx + ddy * ddy);
      if (d < bs) { bs = d; cand = m; }
    }
    const double smin = wave_min_f64(bs);
    cand = (bs == smin) ? cand : 0x7fffffff;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int t = __shfl_xor(cand, o, 64);
    cand = t < cand ? t : cand;
  }
  return uni(cand);
}

template <int J, int MODE, bool DIAG>
__global__ __launch_bounds__(RRT_X_WAVES * 64, (MODE == 2 ? (J <= 4 ? 5 : 2) : (J <= 4 ? 6 : 2))) void rrt_explore_kernel(WorldDev W, RrtParamsDev P, RrtBuffers B,
                                                                     int n_episodes, int max_pts) {
  constexpr bool LIM = false;
  constexpr const RrtEpisodeLimDev* lim = nullptr;
#include "rrt_explore_body.h"
}

// RRT.exploring with per-episode limits (auvp_rrt_prepare_episodes): time-bin mode, no diagnostics; lim [n_episodes].  Every
// episode plans with its own horizon lim[ep].max_traj_time and its own K = lim[ep].K (the random bin draw, the overflow-bin
// rule, the leaf flag); P.K and P.max_traj_time are the batch's caps, which size the LDS plan and the bin lists alike.
template <int J>
__global__ __launch_bounds__(RRT_X_WAVES * 64, (J <= 4 ? 6 : 2)) void rrt_explore_lim_kernel(WorldDev W, RrtParamsDev P, RrtBuffers B,
                                                                                           int n_episodes, int max_pts,
                                                                                           const RrtEpisodeLimDev* __restrict__ lim) {
  constexpr int MODE = 0;
  constexpr bool DIAG = false, LIM = true;
#include "rrt_explore_body.h"
}

// The qualifying-leaf bookkeeping of exploring (:158-171) for a finished tree, one wavefront per episode.
//
// The reference evaluates habitat_shark_cost_func on the path of every accepted node whose traj_time_stamp is within
// 30 s of max_traj_time, in creation order, and keeps the first strict minimum.  None of that feeds back into the
// tree, so it runs here, after the expansion kernel, in ONE sweep over the nodes in creation order, 64 per pass:
//
// 1. terms.  A path element's contribution to a leaf's cost -- w3*prob of its cell in its time bin, and the habitat it
//    lies in -- does not depend on the leaf (its bin is always part of the leaf's sub-dict), so it is evaluated once.
//    The path points of the 64 nodes of a pass are one contiguous run of records: lane = point (two per lane in flight,
//    coalesced reads); each term is added to its owner's slot in LDS (the owner = the last node of the pass whose
//    pt_off is <= the point index: a 6-step search over the pass's offsets; LDS atomics).  Then lane = node: its own
//    state's term.
// 2. running sums down the tree (a node's parent always comes earlier; parents inside the pass are resolved in rounds):
//      node_c = {elements inside some habitat, elements, visited-habitat bit set} of the root..node path (exact)
//      node_f[5] = S = sum of the shark terms of that path, in tree order
// 3. ranking.  cost[0] and cost[1] of a leaf follow from the exact integers as the reference computes them.  S differs
//    from the reference's leaf->root ordered sum only by rounding: both add the same L terms, so each is within
//    gamma_L * sum|term| of the exact sum (gamma_L = L u / (1 - L u), u = 2^-53), and |term| <= |w3| * max|prob|;
//    when the probabilities all have one sign (they do: they are probabilities) sum|term| is also |exact sum|, i.e.
//    about |S| -- a path without any shark term has S = 0 exactly, like the reference's sum, and ties stay ties.
//    That gives every leaf an interval [lo, hi] containing the reference's total.  A leaf whose lo is not below the
//    smallest hi of the leaves before it cannot be a strict minimum; the others (a handful per episode: the record
//    setters and exact ties) are re-summed in the reference's order -- leaf, its points last to first, its parent,
//    ... root, one rounded add per element, the terms evaluated again from the records -- and compared exactly like
//    the reference does.  With the leaf log requested every qualifying leaf is re-summed (the log holds the
//    reference's per-leaf costs).
// The order in which the LDS atomics add a node's terms is not defined; S only steers which leaves are re-summed, every
// reported number comes from the exact integers and the ordered re-summation.
constexpr int RRT_LEAF_WAVES = 4;  // episodes per workgroup of the leaf pass (they share the world tables in LDS)
#ifndef AUVP_LEAF_NPL
#define AUVP_LEAF_NPL 2
#endif
#ifndef AUVP_LEAF_WPE
#define AUVP_LEAF_WPE 4
#endif
__host__ __device__ inline int rrt_leaf_grid_lds_bytes(int sg_enabled, int ncol, int nrow) {
  const long long b = 16LL * ((long long)ncol + nrow);
  return (sg_enabled && b <= 48 * 1024) ? (int)b : 0;  // bigger grids are looked up in the global copy
}
// 32-bit words of the per-episode "ancestor of a qualifying leaf" bit set in LDS (0: the tree is too large, sweep it whole)
__host__ __device__ inline int rrt_leaf_mark_words(int cap_nodes) {
  const int w = (cap_nodes + 31) / 32;
  return w <= 4096 ? w : 0;
}

// (leaf_grid_kernels.hip includes this header for the body's helpers and defines its own instance of the body: it leaves these two
// out, AUVP_LEAF_KERNELS_ELSEWHERE, so that the library holds one copy of each)
#ifndef AUVP_LEAF_KERNELS_ELSEWHERE
static __global__ __launch_bounds__(RRT_LEAF_WAVES * 64) __attribute__((amdgpu_waves_per_eu(AUVP_LEAF_WPE, AUVP_LEAF_WPE))) void rrt_leaf_kernel(WorldDev W, RrtParamsDev P, RrtBuffers B, int n_episodes,
                                                                      int mark_words) {
  constexpr bool LIM = false;
  constexpr const RrtEpisodeLimDev* lim = nullptr;
#include "rrt_leaf_body.h"
}

// the leaf pass of a batch with per-episode limits (rrt_explore_lim_kernel's trees): the episode's own leaf threshold
// (lim[ep].max_traj_time - 30) and habitat list (the habitats of lim[ep].keep, in table order: first match, visited set,
// len(habitats) = popcount(keep))
static __global__ __launch_bounds__(RRT_LEAF_WAVES * 64) __attribute__((amdgpu_waves_per_eu(AUVP_LEAF_WPE, AUVP_LEAF_WPE))) void rrt_leaf_lim_kernel(
    WorldDev W, RrtParamsDev P, RrtBuffers B, int n_episodes, int mark_words, const RrtEpisodeLimDev* __restrict__ lim) {
  constexpr bool LIM = true;
#include "rrt_leaf_body.h"
}
#endif  // AUVP_LEAF_KERNELS_ELSEWHERE

// generate_final_course (:321-331) of episode ep's best leaf, written root -> leaf (exploring reverses it, :174) from o on: one
// wavefront walks leaf -> root and fills the elements from the back (nothing is written for an episode without a leaf)
__device__ inline void rrt_final_course(const RrtBuffers& B, int ep, double* __restrict__ o) {
  const int lane = lane_id();
  const RrtSummary s = B.summary[ep];
  if (s.best_leaf < 0) return;
  const int capn = B.cap_nodes;
  const size_t capp = (size_t)B.cap_points;
  const double* nodeF = B.node_f + (size_t)ep * capn * 8;
  const int4* nodeI = reinterpret_cast<const int4*>(B.node_i) + (size_t)ep * capn;
  const double* ptF = B.points + (size_t)ep * capp * 6;
  const double* init = B.init + (size_t)ep * 6;
  int pos = s.best_path_len - 1;  // element index of the leaf
  auto node_elem = [&](int m, int at) {
    double* e = o + 7 * (size_t)at;
    const int4 r = nodeI[m];
    if (r.y < 0) {
      e[0] = init[0]; e[1] = init[1]; e[2] = init[2]; e[3] = 0.0; e[4] = init[3]; e[5] = init[4]; e[6] = init[5];
    } else {
      const double* nf = nodeF + (size_t)m * 8;
      e[0] = nf[0]; e[1] = nf[1]; e[2] = nf[2]; e[3] = 0.0; e[4] = nf[3]; e[5] = (double)r.x; e[6] = nf[4];
    }
  };
  if (lane == 0) node_elem(s.best_leaf, pos);
  pos--;
  for (int m = s.best_leaf;;) {
    const int4 r = nodeI[m];
    if (r.y < 0) break;
    const int cnt = r.w, off = r.z;
    for (int k = lane; k < cnt; k += 64) {
      // point k of the node sits k places after the node it grew from
      double* e = o + 7 * (size_t)(pos - cnt + 1 + k);
      size_t gi = (size_t)off + k;
      const double* ra = ptF + gi * 3;
      const double* rb = ptF + capp * 3 + gi * 3;
      e[0] = ra[0]; e[1] = ra[1]; e[2] = rb[0]; e[3] = rb[1];
      e[4] = ra[2]; e[5] = (double)r.x; e[6] = rb[2];
    }
    pos -= cnt;
    if (lane == 0) node_elem(r.y, pos);
    pos--;
    m = r.y;
  }
}

// ... of every episode of the batch, at offsets[ep]
static __global__ __launch_bounds__(64) void rrt_final_course_kernel(RrtBuffers B, const int64_t* __restrict__ offsets,
                                                              double* __restrict__ out, int n_episodes) {
  const int ep = blockIdx.x;
  if (ep >= n_episodes) return;
  rrt_final_course(B, ep, out + 7 * (size_t)offsets[ep]);
}

}  // namespace auvp
#endif

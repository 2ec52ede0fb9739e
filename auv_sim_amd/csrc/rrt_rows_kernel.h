// rrt_rows_kernel.h -- RRT.exploring (path_planning/rrt_dubins.py:92-176), time-bin sampling, FOUR episodes per
// wavefront: one 16-lane row (the DPP row) per episode.
//
// rrt_explore_kernel gives a whole wavefront to one episode and is bound by vector-instruction issue with ~20 % of
// the lanes doing useful work (a steer has 14.5 sub-arcs on average, the bookkeeping is one lane's worth).  Here every
// vector instruction serves four episodes: what was wave-uniform (and lived in scalar registers) becomes row-uniform
// (the same value in the 16 lanes of a row), ballots are cut into 16-bit row masks, cross-lane reads stay inside a
// row.  A steer of up to 30 sub-arcs takes two passes of 15 (lane 15 of a row carries the pass-entry angle), the
// running sums keep the reference's left-to-right order (theta by a DPP row shift chain, x/y/t/length by four lanes
// per row through LDS).  The results are bit-identical to rrt_explore_kernel's; rrt_leaf_kernel finishes both.
//
// LDS per episode: the MT19937 state (2 496 B), one scratch block (the tempered random() window of a pass, then the
// four running-sum rows: 576 B) and the time-bin counters as u16.  A workgroup is 12 waves = 48 episodes sharing the
// world tables and the obstacle tile: one workgroup per CU, three waves per SIMD.
//
// Limits (the host falls back to rrt_explore_kernel beyond them): time-bin mode, no diagnostics, freq <= 30,
// <= 256 obstacles, <= 65 534 iterations (u16 bin counters).
#ifndef AUVP_RRT_ROWS_KERNEL_H
#define AUVP_RRT_ROWS_KERNEL_H
#include <type_traits>

#include "rrt_explore_kernel.h"

namespace auvp {

constexpr int RW_WAVES = 12;  // most waves per workgroup (48 episodes: one workgroup fills a CU's LDS); small batches use fewer
constexpr int RW_ROWS = 4;    // episodes per wave
constexpr int RW_C = 15;      // sub-arcs per steer pass (lane 15 of the row: pass-entry angle)
constexpr int RW_MAX_FREQ = 2 * RW_C;
constexpr int RW_MAX_OBST = 256;
constexpr int RW_WIN = 3 * RW_C + 3;  // random() values a pass may look at

struct RowsLdsPlan {
  int tables, mt, scratch, bins, per_ep, obst, total;
};

__host__ __device__ inline RowsLdsPlan rrt_rows_lds_plan(int K, int n_obst_slots, int tables_bytes, int waves = RW_WAVES) {
  RowsLdsPlan p;
  p.tables = (tables_bytes + 15) & ~15;
  p.mt = 624 * 4;
  const int win = RW_WIN * 8, inc = 4 * 18 * 8;
  p.scratch = ((win > inc ? win : inc) + 15) & ~15;
  p.bins = (((K + 2) * 2) + 15) & ~15;
  p.per_ep = p.mt + p.scratch + p.bins;
  p.obst = n_obst_slots * (8 + 8 + 4);  // x, y f64; cull radius f32
  p.total = p.tables + waves * RW_ROWS * p.per_ep + p.obst;
  return p;
}

// ---- row helpers (16 lanes = one episode) ----
__device__ __forceinline__ uint32_t row_ballot(bool pred, int rowbase) {
  return (uint32_t)((wave_ballot(pred) >> rowbase) & 0xffffull);
}
__device__ __forceinline__ int row_read(int v, int src_lane) { return __shfl(v, src_lane, 64); }
__device__ __forceinline__ double row_read_f64(double v, int src_lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __shfl((int)(b & 0xffffffffll), src_lane, 64), hi = __shfl((int)(b >> 32), src_lane, 64);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// minimum / maximum over the 16 lanes of a row, in every lane: four rotate steps on the DPP path (row_ror 8, 4, 2, 1) instead of
// four xor shuffles -- `__shfl_xor` is a ds_bpermute per 32-bit half, an LDS round trip per step for a lone chain
template <int N>
__device__ __forceinline__ double row_ror_f64(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), 0x120 + N, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x120 + N, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double row_min_f64(double v) {
  v = __builtin_fmin(v, row_ror_f64<8>(v)); v = __builtin_fmin(v, row_ror_f64<4>(v));
  v = __builtin_fmin(v, row_ror_f64<2>(v)); v = __builtin_fmin(v, row_ror_f64<1>(v));
  return v;
}
__device__ __forceinline__ double row_max_f64(double v) {
  v = __builtin_fmax(v, row_ror_f64<8>(v)); v = __builtin_fmax(v, row_ror_f64<4>(v));
  v = __builtin_fmax(v, row_ror_f64<2>(v)); v = __builtin_fmax(v, row_ror_f64<1>(v));
  return v;
}
// value of the previous lane of the row (DPP row_shr:1); lane 0 of every row gets `first`
__device__ __forceinline__ double row_prev_f64(double v, double first) {
  const long long b = __double_as_longlong(v), f = __double_as_longlong(first);
  const int lo = __builtin_amdgcn_update_dpp((int)(f & 0xffffffffll), (int)(b & 0xffffffffll), 0x111, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(f >> 32), (int)(b >> 32), 0x111, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// theta += phi, left to right, for the four rows of a wavefront at once: every lane ends with
// (((theta0 + phi_0) + phi_1) + ... + phi_rl), phi_j = the value lane j of its row wrote to `row_phi[j]`.  Lane s adds
// phi_0 .. phi_s itself, the values broadcast out of LDS, under an exec mask that drops lanes rl < j at step j: ONE vector
// instruction per step (the DPP row-shift chain this replaces cost five: two v_mov_dpp + the add + the merge of the first
// lane).  The masks are constants -- lanes with (lane & 15) >= j -- and only shrink, so the LDS reads issued under them still
// reach every lane that will use them; four reads stay in flight.  Expects all 64 lanes enabled at the call (the kernels
// call it from wave-uniform control flow only: the step masks are absolute) and restores the mask it found.
__device__ __forceinline__ double rows_theta_chain(double theta0, const double* row_phi) {
  double th = theta0, t0, t1, t2, t3;
  const uint32_t a = (uint32_t)(size_t)((const __attribute__((address_space(3))) double*)row_phi);
  // (the entry mask is saved and put back: should the compiler ever lower an enclosing condition as divergent, lanes that were
  // masked off stay off -- ADVICE r5; one scalar move)
  unsigned long long exec_in;
  __asm__ volatile(
      "s_mov_b64 %[sv], exec\n\t"
      "s_waitcnt lgkmcnt(0)\n\t"
      "ds_read_b64 %[t0], %[a] offset:0\n\t"
      "ds_read_b64 %[t1], %[a] offset:8\n\t"
      "ds_read_b64 %[t2], %[a] offset:16\n\t"
      "ds_read_b64 %[t3], %[a] offset:24\n\t"
      "s_waitcnt lgkmcnt(3)\n\t"
      "v_add_f64 %[th], %[th], %[t0]\n\t"
      "ds_read_b64 %[t0], %[a] offset:32\n\t"
      "s_waitcnt lgkmcnt(3)\n\t"
      "s_mov_b32 exec_lo, 0xfffefffe\n\ts_mov_b32 exec_hi, 0xfffefffe\n\t"
      "v_add_f64 %[th], %[th], %[t1]\n\t"
      "ds_read_b64 %[t1], %[a] offset:40\n\t"
      "s_waitcnt lgkmcnt(3)\n\t"
      "s_mov_b32 exec_lo, 0xfffcfffc\n\ts_mov_b32 exec_hi, 0xfffcfffc\n\t"
      "v_add_f64 %[th], %[th], %[t2]\n\t"
      "ds_read_b64 %[t2], %[a] offset:48\n\t"
      "s_waitcnt lgkmcnt(3)\n\t"
      "s_mov_b32 exec_lo, 0xfff8fff8\n\ts_mov_b32 exec_hi, 0xfff8fff8\n\t"
      "v_add_f64 %[th], %[th], %[t3]\n\t"
      "ds_read_b64 %[t3], %[a] offset:56\n\t"
      "s_waitcnt lgkmcnt(3)\n\t"
      "s_mov_b32 exec_lo, 0xfff0fff0\n\ts_mov_b32 exec_hi, 0xfff0fff0\n\t"
      "v_add_f64 %[th], %[th], %[t0]\n\t"
      "ds_read_b64 %[t0], %[a] offset:64\n\t"
      "s_waitcnt lgkmcnt(3)\n\t"
      "s_mov_b32 exec_lo, 0xffe0ffe0\n\ts_mov_b32 exec_hi, 0xffe0ffe0\n\t"
      "v_add_f64 %[th], %[th], %[t1]\n\t"
      "ds_read_b64 %[t1], %[a] offset:72\n\t"
      "s_waitcnt lgkmcnt(3)\n\t"
      "s_mov_b32 exec_lo, 0xffc0ffc0\n\ts_mov_b32 exec_hi, 0xffc0ffc0\n\t"
      "v_add_f64 %[th], %[th], %[t2]\n\t"
      "ds_read_b64 %[t2], %[a] offset:80\n\t"
      "s_waitcnt lgkmcnt(3)\n\t"
      "s_mov_b32 exec_lo, 0xff80ff80\n\ts_mov_b32 exec_hi, 0xff80ff80\n\t"
      "v_add_f64 %[th], %[th], %[t3]\n\t"
      "ds_read_b64 %[t3], %[a] offset:88\n\t"
      "s_waitcnt lgkmcnt(3)\n\t"
      "s_mov_b32 exec_lo, 0xff00ff00\n\ts_mov_b32 exec_hi, 0xff00ff00\n\t"
      "v_add_f64 %[th], %[th], %[t0]\n\t"
      "ds_read_b64 %[t0], %[a] offset:96\n\t"
      "s_waitcnt lgkmcnt(3)\n\t"
      "s_mov_b32 exec_lo, 0xfe00fe00\n\ts_mov_b32 exec_hi, 0xfe00fe00\n\t"
      "v_add_f64 %[th], %[th], %[t1]\n\t"
      "ds_read_b64 %[t1], %[a] offset:104\n\t"
      "s_waitcnt lgkmcnt(3)\n\t"
      "s_mov_b32 exec_lo, 0xfc00fc00\n\ts_mov_b32 exec_hi, 0xfc00fc00\n\t"
      "v_add_f64 %[th], %[th], %[t2]\n\t"
      "ds_read_b64 %[t2], %[a] offset:112\n\t"
      "s_waitcnt lgkmcnt(3)\n\t"
      "s_mov_b32 exec_lo, 0xf800f800\n\ts_mov_b32 exec_hi, 0xf800f800\n\t"
      "v_add_f64 %[th], %[th], %[t3]\n\t"
      "s_waitcnt lgkmcnt(2)\n\t"
      "s_mov_b32 exec_lo, 0xf000f000\n\ts_mov_b32 exec_hi, 0xf000f000\n\t"
      "v_add_f64 %[th], %[th], %[t0]\n\t"
      "s_waitcnt lgkmcnt(1)\n\t"
      "s_mov_b32 exec_lo, 0xe000e000\n\ts_mov_b32 exec_hi, 0xe000e000\n\t"
      "v_add_f64 %[th], %[th], %[t1]\n\t"
      "s_waitcnt lgkmcnt(0)\n\t"
      "s_mov_b32 exec_lo, 0xc000c000\n\ts_mov_b32 exec_hi, 0xc000c000\n\t"
      "v_add_f64 %[th], %[th], %[t2]\n\t"
      "s_mov_b64 exec, %[sv]"
      : [th] "+v"(th), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3), [sv] "=&s"(exec_in)
      : [a] "v"(a)
      : "memory");
  return th;
}

// Per-row view of the MT19937 stream (state in the episode's LDS block, refilled in place like WaveRng, 16 words per
// round and row).  pslot / avail / drawn are row-uniform.
struct RowRng {
  uint32_t* s;
  uint32_t pslot, avail;
  unsigned long long drawn;
};

// make sure every row that asks (`want`) has `need` words generated ahead of its consumer.  The generation frontier
// pslot + avail is kept a multiple of 16 (624 = 39 x 16; it starts at 624 = 0): whole 16-word blocks are regenerated, so
// a block never wraps and lane rl's word is block + rl.
__device__ __forceinline__ void rows_ensure(RowRng& r, bool want, uint32_t need, int rl) {
  // (a row that does not ask needs 0 words: the loop's vote is then the ballot of ONE compare, `avail < need` -- a vote on
  // `want && ...` costs two more vector instructions, a 0 / 1 and its compare with zero)
  const uint32_t need_w = want ? need : 0u;
  for (;;) {
    const bool go = r.avail < need_w;
    if (__builtin_amdgcn_uicmp(r.avail, need_w, 36 /* unsigned < */) == 0ull) break;
    // up to 32 words per row and round, two per lane (words 227 apart are independent, so any 32 consecutive are)
    uint32_t n = (624u - r.avail) & ~15u;
    n = n < 32u ? n : 32u;
    n = go ? n : 0u;
    uint32_t f0 = r.pslot + r.avail;
    f0 = f0 >= 624u ? f0 - 624u : f0;
    uint32_t v2[2], kk[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      uint32_t fh = f0 + 16u * (uint32_t)h;
      fh = fh >= 624u ? fh - 624u : fh;
      const uint32_t k = fh + (uint32_t)rl;
      const uint32_t k1 = (k == 623u) ? 0u : k + 1u;
      uint32_t km = k + 397u;
      km = km >= 624u ? km - 624u : km;
      const uint32_t a = r.s[k], b = r.s[k1], c = r.s[km];
      const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
      v2[h] = c ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      kk[h] = k;
    }
    wave_sync();  // every lane's reads are issued before any lane's write
    if (n >= 16u) r.s[kk[0]] = v2[0];
    if (n >= 32u) r.s[kk[1]] = v2[1];
    wave_sync();
    r.avail += n;
  }
}
__device__ __forceinline__ double rows_random_at(const RowRng& r, uint32_t j) {
  uint32_t k = r.pslot + 2u * j;
  k = k >= 624u ? k - 624u : k;
  const uint32_t k1 = (k + 1u == 624u) ? 0u : k + 1u;
  const uint32_t a = mt_temper(r.s[k]) >> 5, b = mt_temper(r.s[k1]) >> 6;
  return py_random_from(a, b);
}
__device__ __forceinline__ void rows_advance(RowRng& r, bool on, uint32_t nwords) {
  if (on) {
    uint32_t p = r.pslot + nwords;  // nwords < 624: one wrap at most
    p = p >= 624u ? p - 624u : p;
    r.pslot = p;
    r.avail -= nwords;
    r.drawn += nwords;
  }
}

// The kernel: rrt_rows_body.h with the generator in LDS; rrt_rows_stream_kernel.h builds its kernel from the same body.
// (internal linkage: the kernel is compiled -- and launched -- by rows_kernels.hip, a translation unit with its own scheduler
// strategy; other units that include this header for the row helpers drop their unused copy)
static __global__ __launch_bounds__(RW_WAVES * 64, 1) void rrt_rows_kernel(WorldDev W, RrtParamsDev P, RrtBuffers B, int n_episodes) {
#define AUVP_ROWS_BODY_STREAM 0  // CPython's generator in LDS
#include "rrt_rows_body.h"
#undef AUVP_ROWS_BODY_STREAM
}

}  // namespace auvp
#endif

// rrt_rows_kernel.h -- RRT.exploring (path_planning/rrt_dubins.py:92-176), time-bin sampling, FOUR episodes per
// wavefront: one 16-lane row (the DPP row) per episode.
//
// rrt_explore_kernel gives a whole wavefront to one episode and is bound by vector-instruction issue with ~20 % of
// the lanes doing useful work (a steer has 14.5 sub-arcs on average, the bookkeeping is one lane's worth).  Here every
// vector instruction serves four episodes: what was wave-uniform (and lived in scalar registers) becomes row-uniform
// (the same value in the 16 lanes of a row), ballots are cut into 16-bit row masks, cross-lane reads stay inside a
// row.  A steer of up to 30 sub-arcs takes two passes of 15 (lane 15 of a row carries the pass-entry angle), the
// running sums keep the reference's left-to-right order (theta by a chain of 64-bit DPP row broadcasts, x/y/t/length by four lanes
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
// (((theta0 + phi_0) + phi_1) + ... + phi_rl), phi_j = the `phi` of lane j of its row.  Lane s adds phi_0 .. phi_s itself, under
// an exec mask that drops lanes rl < j at step j: ONE vector instruction per step, and no LDS -- step j reads lane j of every row
// through the 64-bit DPP row broadcast (row_newbcast:j).  (Before, the phis went through the row's LDS scratch: a ds_write_b64, a
// wave barrier and fifteen ds_read_b64 broadcasts per pass, each with its wait on the chain -- 1 340 cycles per wave and trip,
// profiles/rows_theta_dpp.md; before that, a DPP row-shift chain of five instructions per step.)
// 64-bit DPP exists for VOP1 / VOP2 encodings only and v_add_f64 is VOP3 (the assembler: "dpp variant of this instruction is
// not supported"), so a step is v_fmac_f64_dpp with a register pair that holds 1.0: th = fma(phi_j, 1.0, th).  The product by
// 1.0 is exact for every input, the fma then rounds th + phi_j once -- v_add_f64's result bit for bit, signed zeros and
// infinities included (tests/test_gpu_theta_chain.py holds the device to it).  The masks are constants -- lanes with
// (lane & 15) >= j -- so lane j itself is on when its phi is fetched and a lane's own sum stops at phi_rl.  (Fifteen steps,
// j = 0 .. 14: lane 15, the kernels' pass-entry lane, ends with lane 14's sum and its own phi is never read.)  Expects all 64
// lanes enabled at the call (the kernels call it from wave-uniform control flow only: the step masks are absolute) and restores
// the mask it found (should the compiler ever lower an enclosing condition as divergent, lanes that were masked off stay off).
// Wait states (nothing inside an asm statement is padded; LLVM's gfx940 hazard recognizer): a DPP instruction needs 2 after a
// VALU write of ANY vector register it reads -- `phi` comes out of the division's last v_fmac right before the call, hence the
// opening s_mov_b64 + s_nop 0; between steps `th` is written by one fmac and read by the next, and the two scalar exec moves
// are those two states.  (A VALU write of EXEC would need 5; these writes are scalar and not in that rule.)
__device__ __forceinline__ double rows_theta_chain_dpp(double theta0, double phi) {
  double th = theta0;
  const double one = 1.0;
  unsigned long long exec_in;
#define AUVP_THETA_STEP(J) "v_fmac_f64_dpp %[th], %[phi], %[one] row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"
#define AUVP_THETA_MASK(M) "s_mov_b32 exec_lo, " #M "\n\ts_mov_b32 exec_hi, " #M "\n\t"
  __asm__ volatile(
      "s_mov_b64 %[sv], exec\n\t"
      "s_nop 0\n\t"
      AUVP_THETA_STEP(0)
      AUVP_THETA_MASK(0xfffefffe) AUVP_THETA_STEP(1)
      AUVP_THETA_MASK(0xfffcfffc) AUVP_THETA_STEP(2)
      AUVP_THETA_MASK(0xfff8fff8) AUVP_THETA_STEP(3)
      AUVP_THETA_MASK(0xfff0fff0) AUVP_THETA_STEP(4)
      AUVP_THETA_MASK(0xffe0ffe0) AUVP_THETA_STEP(5)
      AUVP_THETA_MASK(0xffc0ffc0) AUVP_THETA_STEP(6)
      AUVP_THETA_MASK(0xff80ff80) AUVP_THETA_STEP(7)
      AUVP_THETA_MASK(0xff00ff00) AUVP_THETA_STEP(8)
      AUVP_THETA_MASK(0xfe00fe00) AUVP_THETA_STEP(9)
      AUVP_THETA_MASK(0xfc00fc00) AUVP_THETA_STEP(10)
      AUVP_THETA_MASK(0xf800f800) AUVP_THETA_STEP(11)
      AUVP_THETA_MASK(0xf000f000) AUVP_THETA_STEP(12)
      AUVP_THETA_MASK(0xe000e000) AUVP_THETA_STEP(13)
      AUVP_THETA_MASK(0xc000c000) AUVP_THETA_STEP(14)
      "s_mov_b64 exec, %[sv]"
      : [th] "+v"(th), [sv] "=&s"(exec_in)
      : [phi] "v"(phi), [one] "v"(one));
#undef AUVP_THETA_STEP
#undef AUVP_THETA_MASK
  return th;
}

// What a lane of a steer pass of n sub-arcs adds to the pass's five ordered sums when it has no arc of its own: +0.0 below n (an
// untaken sub-arc), -0.0 from n on (an idle lane).  x + (-0.0) == x for EVERY x, x + (+0.0) == x for every x but -0.0: with -0.0
// past n a chain that runs on over the idle lanes ends with the value it had at sub-arc n - 1, bit for bit, the sign of a zero
// sum included -- which is what lets rows_pass_ends_dpp take the row's end state from the chain ends.  The prefix values below n
// are what they were with +0.0 there (nothing past n goes into them).
__device__ __forceinline__ double rows_idle_zero(bool below_n) { return below_n ? 0.0 : -0.0; }

// x += dx; y += dy; t += dt; length += movement of a steer pass: four serial chains per row, on lanes 0 .. 3, over the 18-double
// rows of `inc` (entry j of row q = what lane j of the episode wrote for sum q; rows_idle_zero past n, so all 15 steps can run).
// Eight independent 16-byte reads up front, fifteen chained additions, eight writes -- no loop, no round trip per step.  The
// prefix sums replace the increments in place; entry 15 only fills the last 16-byte pair: it is read and written back as it
// was, never added, and nobody has to set it.  `acc` comes in as the lane's start value (lane 0: x, 1: y, 2: t, 3: length) and
// leaves, on lanes 0 .. 3 of the rows that are `on`, as the row's sum after the pass.
__device__ __forceinline__ double rows_sums_chain(double* inc, int rl, bool on, double acc) {
  if (rl < 4 && on) {
    double2* rowp = reinterpret_cast<double2*>(inc + rl * 18);
    double2 v[8];
#pragma unroll
    for (int s2 = 0; s2 < 8; s2++) v[s2] = rowp[s2];
#pragma unroll
    for (int s2 = 0; s2 < 8; s2++) {
      acc = acc + v[s2].x; v[s2].x = acc;
      if (s2 < 7) { acc = acc + v[s2].y; v[s2].y = acc; }
    }
#pragma unroll
    for (int s2 = 0; s2 < 8; s2++) rowp[s2] = v[s2];
  }
  return acc;
}

// The row's state after a steer pass, in every lane: x, y, t, length = `acc` of lanes 0 .. 3 (rows_sums_chain), theta = `th` of
// lane 14 (rows_theta_chain_dpp: the sum of all fifteen phis).  Five 64-bit DPP moves (v_mov_b64 row_newbcast) instead of two
// 16-byte LDS reads and two ds_bpermute with a wait each: the numbers are in registers already.  A row that is not `on` needs no
// guard of its own: rows_sums_chain did not run for it, so `acc` of its lanes 0 .. 3 still IS its x, y, t, length, and all of its
// lanes are idle, so its `th` is theta0 + fifteen times -0.0 = theta0, bit for bit.  The moves run with all 64 lanes enabled
// (the source lanes with them), whatever mask the call finds, and that mask is restored; the kernels call it from wave-uniform
// control flow.  Wait states: a DPP read needs 2 after a VALU write of the register (`acc`: the chain's last add; `th`: the
// theta chain's last fmac) -- the two scalar moves and the s_nop are three.
__device__ __forceinline__ void rows_pass_ends_dpp(double acc, double th, double& x, double& y, double& t, double& len,
                                                   double& theta) {
  unsigned long long exec_in;
#define AUVP_END_MOV(D, S, J) "v_mov_b64_dpp %[" #D "], %[" #S "] row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"
  __asm__ volatile(
      "s_mov_b64 %[sv], exec\n\t"
      "s_mov_b64 exec, -1\n\t"
      "s_nop 0\n\t"
      AUVP_END_MOV(x, acc, 0) AUVP_END_MOV(y, acc, 1) AUVP_END_MOV(t, acc, 2) AUVP_END_MOV(len, acc, 3) AUVP_END_MOV(theta, th, 14)
      "s_mov_b64 exec, %[sv]"
      : [x] "=&v"(x), [y] "=&v"(y), [t] "=&v"(t), [len] "=&v"(len), [theta] "=&v"(theta), [sv] "=&s"(exec_in)
      : [acc] "v"(acc), [th] "v"(th));
#undef AUVP_END_MOV
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

// rrt_rows_stream_kernel.h -- rrt_rows_kernel (RRT.exploring, time-bin sampling, four episodes per wavefront) reading its
// random() numbers from a PRE-GENERATED stream (rrt_stream_kernel.h) instead of running CPython's generator itself (round 6).
// Same algorithm, same operations on the same values in the same order -- the trees are bit-identical -- but:
//   * no MT19937 state in LDS (2 496 B per episode), no refill, no tempering: random() number j of the episode is
//     stream[j]; a ring of RS_RING doubles per episode in LDS (2 KB) holds the next ones, topped up once per trip -- right after
//     the parent's record has arrived, where the vector-memory counter is drained anyway -- with 32-double chunks that were
//     requested a trip earlier (register-staged: the loads have a whole trip to land; 16 bytes per lane and load);
//   * the window of a steer pass is the ring itself (entry j of a pass = ring[(pos + first + j) & (RS_RING - 1)], or, with the
//     ring's first entries mirrored behind it, one address per lane plus an immediate: below): the copy into a window area is
//     gone, the running-sum scratch has its 576 B to itself;
//   * an episode that runs past its stream (B.stream_cap) ends with AUVP_ST_STREAM; the host redoes the batch on
//     rrt_rows_kernel.
// This header has what is the stream's own: the LDS plan, RowStream and its functions.  The kernel's body is rrt_rows_body.h, the
// one text rrt_rows_kernel is built from as well (AUVP_ROWS_BODY_STREAM picks the variant where the two differ).
#ifndef AUVP_RRT_ROWS_STREAM_KERNEL_H
#define AUVP_RRT_ROWS_STREAM_KERNEL_H
#include "rrt_rows_kernel.h"

namespace auvp {

constexpr int RS_RING = 256;   // doubles of the stream an episode keeps in LDS (a power of two: slot = number & 255)
constexpr int RS_MIRROR = 48;  // ring entries kept a second time behind the ring (the mirrored form): the farthest a read looks past its base
constexpr int RS_WAVES = 16;   // wavefronts of the largest workgroup of the four-per-SIMD instantiation (128 registers; measured slower: profiles/r6_rows_stream.md)
// A row asks for its stream in chunks of RS_CHUNK numbers, lane rl loading RS_PIECE of them in one piece: 16 bytes, so two
// global_load_dwordx4 and two ds_write_b128 per trip where 8-byte pieces took four loads and four writes, each under its own
// branch and wait -- 81.9-82.7 -> 79.5-80.0 ms on the headline batch together with the mirrored ring, most of it from here
// (profiles/stream_ring.md; 32-byte pieces measured another 0.2 ms at five times the slow-path entries and 168 registers in the
// masked form: not taken)
#ifndef AUVP_RS_PIECE
#define AUVP_RS_PIECE 2
#endif
constexpr int RS_PIECE = AUVP_RS_PIECE;         // numbers a lane loads at once: 2 (1: the 8-byte form, for experiments)
constexpr int RS_CHUNK = 16 * RS_PIECE;         // numbers of a row's request
constexpr int RS_PEND = 64 / RS_CHUNK;          // chunks that may be on their way per row (requested in one trip, written in the next)
typedef double rs_f64x2 __attribute__((ext_vector_type(2)));
template <int N> struct RsPiece { typedef double type; };
template <> struct RsPiece<2> { typedef rs_f64x2 type; };
typedef RsPiece<RS_PIECE>::type rs_piece;
constexpr int RS_LDS_LIMIT = 160 * 1024;

// The ring has two forms, a kernel each (below):
//   masked    ring[RS_RING]; number e of the stream at slot e & 255, every read forms (pos + j) & 255 itself;
//   mirrored  ring[RS_RING + RS_MIRROR]; whoever writes slot s < RS_MIRROR writes slot s + RS_RING as well, so number pos + j is at
//             ring[(pos & 255) + j] for every j <= RS_MIRROR without a mask: a lane keeps ONE LDS address per window (stream_base) and
//             its reads are that register plus an immediate offset (ds_read_b64 ... offset:N).  No read of the body looks farther:
//             a steer pass's window starts at the row's position (+ the selection's draws, at most 16, folded into the base) and
//             ends with ROWS_WIN(j + 1) at j = 47.
struct RowsStreamLdsPlan {
  int tables, ring, scratch, bins, per_ep, obst, total;
};
__host__ __device__ inline RowsStreamLdsPlan rrt_rows_stream_lds_plan(int K, int n_obst_slots, int tables_bytes, int waves = RW_WAVES, bool mirror = false) {
  RowsStreamLdsPlan p;
  p.tables = (tables_bytes + 15) & ~15;
  p.ring = (RS_RING + (mirror ? RS_MIRROR : 0)) * 8;
  p.scratch = (4 * 18 * 8 + 15) & ~15;
  p.bins = (((K + 2) * 2) + 15) & ~15;
  p.per_ep = p.ring + p.scratch + p.bins;
  p.obst = n_obst_slots * (8 + 8 + 4);
  p.total = p.tables + waves * RW_ROWS * p.per_ep + p.obst;
  return p;
}

// The host's choice of a launch: the waves per workgroup are what the MASKED plan admits below the LDS limit (a wavefront fewer
// costs 8.7 %: profiles/r6_rows_waves.md); the mirrored form is taken where its plan fits at that very count.  force: < 0 the
// rule, 0 masked, 1 mirrored (option ROWS_STREAM_MIRROR; a forced mirrored form gives up waves until it fits).
struct RowsStreamShape {
  int waves;
  bool mirror;
  RowsStreamLdsPlan plan;
};
__host__ inline RowsStreamShape rrt_rows_stream_shape(int K, int n_obst_slots, int tables_bytes, int waves_wanted, int force = -1) {
  int sw = waves_wanted < 1 ? 1 : (waves_wanted > RW_WAVES ? RW_WAVES : waves_wanted);
  while (sw > 1 && rrt_rows_stream_lds_plan(K, n_obst_slots, tables_bytes, sw, false).total > RS_LDS_LIMIT) sw--;
  bool mirror = force < 0 ? rrt_rows_stream_lds_plan(K, n_obst_slots, tables_bytes, sw, true).total <= RS_LDS_LIMIT : force != 0;
  while (mirror && sw > 1 && rrt_rows_stream_lds_plan(K, n_obst_slots, tables_bytes, sw, true).total > RS_LDS_LIMIT) sw--;
  RowsStreamShape s;
  s.waves = sw; s.mirror = mirror;
  s.plan = rrt_rows_stream_lds_plan(K, n_obst_slots, tables_bytes, sw, mirror);
  return s;
}

// Per-row view of the episode's stream.  pos / front / req are row-uniform: random() numbers consumed, written to the ring,
// requested from memory (front <= req <= cap, both multiples of RS_CHUNK; front - pos <= RS_RING).  The stream's length `cap` is a
// multiple of 64 (the host rounds it: rrt_stream_len; the launcher refuses another), so a chunk is inside the stream or past it as a
// whole and the requests simply stop at the end: no test per chunk.
struct RowStream {
  double* ring;
  const double* src;
  uint32_t pos, front, req, cap;
  rs_piece pend[RS_PEND];  // lane rl: piece rl of the chunks [front + RS_CHUNK c, front + RS_CHUNK (c + 1)), c < (req - front) / RS_CHUNK
#ifdef AUVP_STREAM_COUNT_SLOW
  uint32_t slow;           // EXPERIMENT ONLY (never defined in the product build): slow-path entries of stream_ensure
#endif
};

// the chunks requested earlier land in the ring (mirrored form: a piece is RS_PIECE aligned slots, wholly below RS_MIRROR or not)
template <bool MIRROR>
__device__ __forceinline__ void stream_commit(RowStream& r, int rl) {
#pragma unroll
  for (int c = 0; c < RS_PEND; c++)
    if (r.front + (uint32_t)(RS_CHUNK * c) < r.req) {
      const uint32_t s = (r.front + (uint32_t)(RS_CHUNK * c) + (uint32_t)(RS_PIECE * rl)) & (uint32_t)(RS_RING - 1);
      *reinterpret_cast<rs_piece*>(r.ring + s) = r.pend[c];
      if (MIRROR && s < (uint32_t)RS_MIRROR) *reinterpret_cast<rs_piece*>(r.ring + s + (uint32_t)RS_RING) = r.pend[c];
    }
  r.front = r.req;
}
// ... and as many new ones as the ring has room for -- and the stream has left -- are requested
__device__ __forceinline__ void stream_request(RowStream& r, bool on, int rl) {
  const uint32_t room = (uint32_t)RS_RING - (r.front - r.pos), left = r.cap - r.req;
  uint32_t n = (room < left ? room : left) / (uint32_t)RS_CHUNK;
  n = n > (uint32_t)RS_PEND ? (uint32_t)RS_PEND : n;
  n = on ? n : 0u;
#pragma unroll
  for (int c = 0; c < RS_PEND; c++)
    if ((uint32_t)c < n)
      r.pend[c] = __builtin_nontemporal_load(reinterpret_cast<const rs_piece*>(r.src + r.req + (uint32_t)(RS_CHUNK * c) + (uint32_t)(RS_PIECE * rl)));
  r.req += (uint32_t)RS_CHUNK * n;
}
// the chunks on their way have arrived from here on, as far as the compiler's count of pending loads goes (no instruction)
__device__ __forceinline__ void stream_settle(RowStream& r) {
#pragma unroll
  for (int c = 0; c < RS_PEND; c++) asm volatile("" : "+v"(r.pend[c]));
}
// once per trip: what was requested a trip ago is written, the next chunks are requested
template <bool MIRROR>
__device__ __forceinline__ void stream_top_up(RowStream& r, bool on, int rl) {
  stream_commit<MIRROR>(r, rl);
  stream_request(r, on, rl);
}
// make sure every row that asks has `need` numbers in the ring from its position on; false for a row whose stream ends before
// that.  (The fast path is one compare and a vote: the top-up keeps the ring one to two trips ahead.)
template <bool MIRROR>
__device__ __forceinline__ bool stream_ensure(RowStream& r, bool want, uint32_t need, int rl) {
  const uint32_t need_w = want ? need : 0u;
  // (the end is looked at first: a row whose stream ends before `need` asks for nothing, so nothing past the end is waited for)
  const bool ok = r.pos + need_w <= r.cap;
  for (;;) {
    if (__builtin_amdgcn_uicmp(r.front - r.pos, ok ? need_w : 0u, 36 /* unsigned < */) == 0ull) break;
    const bool go = ok && r.front - r.pos < need_w;
#ifdef AUVP_STREAM_COUNT_SLOW
    if (go) r.slow++;
#endif
    // the slow path (start of an episode, or a trip that used more than the top-up had fetched): write what is on its way, fetch
    // more, wait for it
    stream_commit<MIRROR>(r, rl);
    stream_request(r, go && ok, rl);
    stream_commit<MIRROR>(r, rl);
    stream_settle(r);  // (without it the chunks count as on their way after the loop, and their next use drains the counter)
    wave_sync();
    if (!wave_any(go && ok && r.front - r.pos < need_w)) break;
  }
  wave_sync();
  return ok;
}
// Reads.  stream_base(r, b, rl): what lane rl keeps for a window that starts b numbers past the row's position -- the address of
// its own entry (mirrored: entry rl of the window, every read an immediate or a small signed distance away) or the window's
// first number (masked).  stream_read(base, j, rl): window entry j; j - rl folds to a constant where j is rl + a constant.
template <bool MIRROR> struct StreamBase;
template <> struct StreamBase<true> { const double* p; };
template <> struct StreamBase<false> { const double* ring; uint32_t first; };
template <bool MIRROR>
__device__ __forceinline__ StreamBase<MIRROR> stream_base(const RowStream& r, uint32_t b, int rl) {
  if constexpr (MIRROR) return StreamBase<true>{r.ring + (((r.pos + b) & (uint32_t)(RS_RING - 1)) + (uint32_t)rl)};
  else return StreamBase<false>{r.ring, r.pos + b};
}
__device__ __forceinline__ double stream_read(const StreamBase<true>& w, int j, int rl) { return w.p[j - rl]; }
__device__ __forceinline__ double stream_read(const StreamBase<false>& w, int j, int) { return w.ring[(w.first + (uint32_t)j) & (uint32_t)(RS_RING - 1)]; }
__device__ __forceinline__ void stream_advance(RowStream& r, bool on, uint32_t n) {
  if (on) r.pos += n;
}

// (internal linkage: the kernel is compiled -- and launched -- by rows_kernels.hip, a translation unit with its own scheduler
// strategy; other units that include this header for the LDS plan drop their unused copy)
// MAXW: wavefronts of the largest workgroup the instantiation is launched with -- 12 (three per SIMD, 168 registers: batches of up
// to 48 episodes per CU) or RS_WAVES = 16 (four per SIMD, 128 registers: 64 episodes per CU, what the smaller LDS footprint admits)
// The two forms of the ring (above) are two kernels from the one body: rrt_rows_stream_kernel, the mirrored form -- what every
// launch the host admits today runs -- and rrt_rows_stream_masked_kernel (MIRROR is the body's name for the choice).
template <int MAXW>
static __global__ __launch_bounds__(MAXW * 64, 1) void rrt_rows_stream_kernel(WorldDev W, RrtParamsDev P, RrtBuffers B, int n_episodes) {
  constexpr bool MIRROR = true;
#define AUVP_ROWS_BODY_STREAM 1  // the numbers come from B.stream
#include "rrt_rows_body.h"
#undef AUVP_ROWS_BODY_STREAM
}
template <int MAXW>
static __global__ __launch_bounds__(MAXW * 64, 1) void rrt_rows_stream_masked_kernel(WorldDev W, RrtParamsDev P, RrtBuffers B, int n_episodes) {
  constexpr bool MIRROR = false;
#define AUVP_ROWS_BODY_STREAM 1
#include "rrt_rows_body.h"
#undef AUVP_ROWS_BODY_STREAM
}

}  // namespace auvp
#endif

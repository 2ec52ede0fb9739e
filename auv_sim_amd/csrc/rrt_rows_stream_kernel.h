// rrt_rows_stream_kernel.h -- rrt_rows_kernel (RRT.exploring, time-bin sampling, four episodes per wavefront) reading its
// random() numbers from a PRE-GENERATED stream (rrt_stream_kernel.h) instead of running CPython's generator itself (round 6).
// Same algorithm, same operations on the same values in the same order -- the trees are bit-identical -- but:
//   * no MT19937 state in LDS (2 496 B per episode), no refill, no tempering: random() number j of the episode is
//     stream[j]; a ring of RS_RING doubles per episode in LDS (2 KB) holds the next ones, topped up once per trip -- right after
//     the parent's record has arrived, where the vector-memory counter is drained anyway -- with 16-double chunks that were
//     requested a trip earlier (register-staged: the loads have a whole trip to land);
//   * the window of a steer pass is the ring itself (entry j of a pass = ring[(pos + first + j) & (RS_RING - 1)]): the
//     copy into a window area is gone, the running-sum scratch has its 576 B to itself;
//   * an episode that runs past its stream (B.stream_cap) ends with AUVP_ST_STREAM; the host redoes the batch on
//     rrt_rows_kernel.
// This header has what is the stream's own: the LDS plan, RowStream and its functions.  The kernel's body is rrt_rows_body.h, the
// one text rrt_rows_kernel is built from as well (AUVP_ROWS_BODY_STREAM picks the variant where the two differ).
#ifndef AUVP_RRT_ROWS_STREAM_KERNEL_H
#define AUVP_RRT_ROWS_STREAM_KERNEL_H
#include "rrt_rows_kernel.h"

namespace auvp {

constexpr int RS_RING = 256;   // doubles of the stream an episode keeps in LDS (a power of two: slot = number & 255)
constexpr int RS_WAVES = 16;   // wavefronts of the largest workgroup of the four-per-SIMD instantiation (128 registers; measured slower: profiles/r6_rows_stream.md)
constexpr int RS_PEND = 4;     // 16-double chunks that may be on their way per row (requested in one trip, written in the next)

struct RowsStreamLdsPlan {
  int tables, ring, scratch, bins, per_ep, obst, total;
};
__host__ __device__ inline RowsStreamLdsPlan rrt_rows_stream_lds_plan(int K, int n_obst_slots, int tables_bytes, int waves = RW_WAVES) {
  RowsStreamLdsPlan p;
  p.tables = (tables_bytes + 15) & ~15;
  p.ring = RS_RING * 8;
  p.scratch = (4 * 18 * 8 + 15) & ~15;
  p.bins = (((K + 2) * 2) + 15) & ~15;
  p.per_ep = p.ring + p.scratch + p.bins;
  p.obst = n_obst_slots * (8 + 8 + 4);
  p.total = p.tables + waves * RW_ROWS * p.per_ep + p.obst;
  return p;
}

// Per-row view of the episode's stream.  pos / front / req are row-uniform: random() numbers consumed, written to the ring,
// requested from memory (front <= req, both multiples of 16; front - pos <= RS_RING).
struct RowStream {
  double* ring;
  const double* src;
  uint32_t pos, front, req, cap;
  double pend[RS_PEND];  // lane rl: element rl of the chunks [front + 16 c, front + 16 c + 16), c < (req - front) / 16
};

// the chunks requested earlier land in the ring
__device__ __forceinline__ void stream_commit(RowStream& r, int rl) {
#pragma unroll
  for (int c = 0; c < RS_PEND; c++)
    if (r.front + 16u * (uint32_t)c < r.req) r.ring[(r.front + 16u * (uint32_t)c + (uint32_t)rl) & (uint32_t)(RS_RING - 1)] = r.pend[c];
  r.front = r.req;
}
// ... and as many new ones as the ring has room for are requested (a chunk past the end of the stream is not: its values
// would never be looked at -- stream_ensure reports the end first)
__device__ __forceinline__ void stream_request(RowStream& r, bool on, int rl) {
  const uint32_t room = (uint32_t)RS_RING - (r.front - r.pos);
  uint32_t n = room >> 4;
  n = n > (uint32_t)RS_PEND ? (uint32_t)RS_PEND : n;
  n = on ? n : 0u;
#pragma unroll
  for (int c = 0; c < RS_PEND; c++) {
    const uint32_t e = r.req + 16u * (uint32_t)c + (uint32_t)rl;
    if ((uint32_t)c < n && e < r.cap) r.pend[c] = __builtin_nontemporal_load(r.src + e);
  }
  r.req += 16u * n;
}
// once per trip: what was requested a trip ago is written, the next chunks are requested
__device__ __forceinline__ void stream_top_up(RowStream& r, bool on, int rl) {
  stream_commit(r, rl);
  stream_request(r, on, rl);
}
// make sure every row that asks has `need` numbers in the ring from its position on; false for a row whose stream ends before
// that.  (The fast path is one compare and a vote: the top-up keeps the ring one to two trips ahead.)
__device__ __forceinline__ bool stream_ensure(RowStream& r, bool want, uint32_t need, int rl) {
  const uint32_t need_w = want ? need : 0u;
  // (the requests run ahead of the stream's end without loading -- `front` may be past `cap` -- so the end is looked at first)
  const bool ok = r.pos + need_w <= r.cap;
  for (;;) {
    if (__builtin_amdgcn_uicmp(r.front - r.pos, ok ? need_w : 0u, 36 /* unsigned < */) == 0ull) break;
    const bool go = ok && r.front - r.pos < need_w;
    // the slow path (start of an episode, or a trip that used more than the top-up had fetched): write what is on its way, fetch
    // more, wait for it
    stream_commit(r, rl);
    stream_request(r, go && ok, rl);
    stream_commit(r, rl);
    wave_sync();
    if (!wave_any(go && ok && r.front - r.pos < need_w)) break;
  }
  wave_sync();
  return ok;
}
__device__ __forceinline__ double stream_at(const RowStream& r, uint32_t j) { return r.ring[(r.pos + j) & (uint32_t)(RS_RING - 1)]; }
__device__ __forceinline__ void stream_advance(RowStream& r, bool on, uint32_t n) {
  if (on) r.pos += n;
}

// (internal linkage: the kernel is compiled -- and launched -- by rows_kernels.hip, a translation unit with its own scheduler
// strategy; other units that include this header for the LDS plan drop their unused copy)
// MAXW: wavefronts of the largest workgroup the instantiation is launched with -- 12 (three per SIMD, 168 registers: batches of up
// to 48 episodes per CU) or RS_WAVES = 16 (four per SIMD, 128 registers: 64 episodes per CU, what the smaller LDS footprint admits)
template <int MAXW>
static __global__ __launch_bounds__(MAXW * 64, 1) void rrt_rows_stream_kernel(WorldDev W, RrtParamsDev P, RrtBuffers B, int n_episodes) {
#define AUVP_ROWS_BODY_STREAM 1  // the numbers come from B.stream
#include "rrt_rows_body.h"
#undef AUVP_ROWS_BODY_STREAM
}

}  // namespace auvp
#endif

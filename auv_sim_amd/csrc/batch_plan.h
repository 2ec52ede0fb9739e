// batch_plan.h -- what a batch of RRT.exploring / Planner_RRT needs in HBM, and the small host rules beside it: the sizing as data.
//
// Host only and pure (as launch_plan.h and world_tables.h): no HIP call, no handle, no environment.  rrt_batch_plan /
// prrt_batch_plan read a plain description of the batch and return either a refusal or every capacity the kernels index by and
// the byte count of every buffer; auvplan.hip and planner_rrt_host.h reserve, upload and launch what the plan says and map a
// refusal to its message.  Every conversion from a double to an int is checked here first (a NaN horizon, an infinite freq),
// and no byte count wraps.  tests/host/batch_plan_check.cpp runs all of it with the sanitizers (tests/test_batch_plan_host.py).
#ifndef AUVP_BATCH_PLAN_H
#define AUVP_BATCH_PLAN_H
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../include/auvplan.h"
#include "auvp_types.h"
#include "launch_options.h"

namespace auvp {

// ---- helpers -----------------------------------------------------------------------------------------------------------------

// (int)v where the conversion is defined: v is a number and its integer part fits.  false otherwise (*out is not written)
inline bool double_to_int(double v, int* out) {
  if (!(v > -2147483649.0 && v < 2147483648.0)) return false;
  *out = (int)v;
  return true;
}

// no buffer of a batch may reach this many bytes (far above any device; what matters is that the product below cannot wrap)
constexpr unsigned long long BATCH_BYTES_LIMIT = 1ull << 62;
// the product of the factors; BATCH_BYTES_LIMIT where it would reach that, or where a factor is negative
inline unsigned long long batch_bytes(std::initializer_list<long long> factors) {
  for (long long f : factors)
    if (f < 0) return BATCH_BYTES_LIMIT;
  for (long long f : factors)
    if (f == 0) return 0;
  unsigned long long b = 1;
  for (long long f : factors) {
    if (b > (BATCH_BYTES_LIMIT - 1) / (unsigned long long)f) return BATCH_BYTES_LIMIT;
    b *= (unsigned long long)f;
  }
  return b;
}
// the first of the named byte counts that reaches the limit; nullptr: none does
struct NamedBytes { const char* name; unsigned long long bytes; };
inline const char* first_too_large(std::initializer_list<NamedBytes> all) {
  for (const NamedBytes& b : all)
    if (b.bytes >= BATCH_BYTES_LIMIT) return b.name;
  return nullptr;
}

// ---- RRT.exploring -------------------------------------------------------------------------------------------------------------

struct RrtBatchIn {
  int E = 0;
  auvp_rrt_params p{};
  int flags = 0;
  int n_obstacles = 0;  // of the world
  // (per-episode limits change no size: the rows are the cap's)
};

// one status per refusal, in the order of the checks.  RRT_BATCH_FIELD: a value whose conversion or size is not defined;
// RrtBatchPlan::field names it
enum RrtBatchStatus {
  RRT_BATCH_OK = 0, RRT_BATCH_BAD_ARGS, RRT_BATCH_BAD_PARAMS, RRT_BATCH_BIN_INTERVAL, RRT_BATCH_OBSTACLES, RRT_BATCH_FIELD,
  RRT_BATCH_TOO_MANY_BINS, RRT_BATCH_POINTS, RRT_BATCH_BIN_LISTS
};

struct RrtBatchBytes {  // of every buffer rrt_prepare_impl reserves (a log that is not asked for: 0)
  unsigned long long nodes_f = 0, nodes_i = 0, points = 0, bin_items = 0, bin_count = 0, summary = 0, node_c = 0, node_q = 0, node_xy = 0,
                     itlog_i = 0, itlog_b = 0, leaf_c = 0, leaf_i = 0, leaf_stats = 0, phase = 0, mt = 0;
};

struct RrtBatchPlan {
  RrtBatchStatus status = RRT_BATCH_OK;
  const char* field = "";  // RRT_BATCH_FIELD: what was refused
  RrtParamsDev P{};        // complete: inv_bin_interval, K (as computed: also where it is refused as too large) and flags
  int max_pts = 0;         // path points of a steer at most: floor(freq) + 2
  RrtBuffers B{};          // every capacity and stride; the pointers are null (the caller's reservations fill them in)
  RrtBatchBytes bytes;
  long long itlog_n = 0;   // entries of one iteration-log column: E x max_iter
};

inline RrtBatchPlan rrt_batch_plan(const RrtBatchIn& in) {
  RrtBatchPlan r;
  const auvp_rrt_params& p = in.p;
  const int E = in.E, flags = in.flags;
  auto refuse = [&r](RrtBatchStatus s, const char* field = "") { r.status = s; r.field = field; return r; };
  if (E <= 0) return refuse(RRT_BATCH_BAD_ARGS);
  if (p.max_iter <= 0 || !(p.freq >= 0) || p.mode < 0 || p.mode > 2) return refuse(RRT_BATCH_BAD_PARAMS);
  if (p.mode == AUVP_MODE_TIMEBIN && !(p.bin_interval > 0)) return refuse(RRT_BATCH_BIN_INTERVAL);
  if (in.n_obstacles > 16 * 64) return refuse(RRT_BATCH_OBSTACLES);
  // (floor(freq) + 64 below must fit as well)
  int nfreq = 0;
  if (!double_to_int(std::floor(p.freq), &nfreq) || nfreq > INT_MAX - 64) return refuse(RRT_BATCH_FIELD, "freq");
  if (p.max_iter == INT_MAX) return refuse(RRT_BATCH_FIELD, "max_iter");
  RrtParamsDev& P = r.P;
  P.dist_to_end = p.dist_to_end; P.diff_max = p.diff_max; P.freq = p.freq; P.min_dist = p.min_dist;
  P.bin_interval = p.bin_interval; P.v = p.v; P.max_traj_time = p.max_traj_time; P.max_plan_time = p.max_plan_time;
  P.w[0] = p.w[0]; P.w[1] = p.w[1]; P.w[2] = p.w[2];
  P.mode = p.mode; P.max_iter = p.max_iter; P.flags = flags;
  P.inv_bin_interval = p.bin_interval > 0 ? 1.0 / p.bin_interval : 0.0;
  P.K = 0;
  if (p.mode == AUVP_MODE_TIMEBIN && !double_to_int(std::ceil(p.max_traj_time / p.bin_interval), &P.K))
    return refuse(RRT_BATCH_FIELD, "max_traj_time / bin_interval");
  if (P.K > 1 << 20) return refuse(RRT_BATCH_TOO_MANY_BINS);
  r.max_pts = nfreq + 2;
  RrtBuffers& B = r.B;
  B.cap_nodes = p.max_iter + 1;
  // Path-point budget.  A steer appends at most n = floor(uniform(0, freq)) points (:258-262) and only an accepted one
  // keeps them, so an episode's total is dominated by a sum of max_iter independent draws of n: mean <= freq/2 each,
  // standard deviation <= freq/sqrt(12).  The default budget is that mean plus EIGHT standard deviations of the sum
  // (exceeded with probability < 1e-15 per episode; the bench world uses 68 % of it), never more than the worst case;
  // points_per_iter overrides it (freq + 1 = the worst case).  Running out is AUVP_ERR_CAPACITY, never a truncation.
  if (p.points_per_iter != p.points_per_iter) return refuse(RRT_BATCH_FIELD, "points_per_iter");
  const double n_it = (double)p.max_iter;
  const double worst = n_it * (nfreq > 1 ? nfreq : 1);
  double cp = p.points_per_iter > 0 ? std::ceil(p.points_per_iter * n_it)
                                    : std::ceil(std::fmin(worst, 0.5 * p.freq * n_it + 8.0 * p.freq / std::sqrt(12.0) * std::sqrt(n_it)));
  cp += nfreq + 64;
  if (cp > 2.0e9) return refuse(RRT_BATCH_POINTS);
  B.cap_points = (int32_t)cp;
  B.bin_cap = P.K > 0 ? B.cap_nodes : 1;
  // chunked member lists: AUVP_BIN_HEAD direct-mapped members per bin, the rest in 64-entry chunks (auvp_types.h)
  const bool chunks = B.bin_cap > AUVP_BIN_HEAD;
  B.bin_over = chunks ? (int32_t)(((long long)B.cap_nodes + 63) / 64 + P.K + 1) : 0;
  B.bin_slots = chunks ? (B.bin_cap - AUVP_BIN_HEAD + 63) / 64 : 0;
  B.bin_stride = ((long long)P.K + 1) * AUVP_BIN_HEAD + (long long)B.bin_over * 64 + (long long)B.bin_slots * ((long long)P.K + 1);
  if (B.bin_stride >= (1ll << 31)) return refuse(RRT_BATCH_BIN_LISTS);
  B.cap_leaves = (flags & AUVP_FLAG_LEAF_LOG) ? B.cap_nodes : 1;
  // nearest-neighbour sampling scans a contiguous x,y mirror of the nodes (auvp_types.h); the other modes never touch it
  B.xy_stride = p.mode == AUVP_MODE_NN ? rrt_nn_stride(B.cap_nodes) : 0;
  RrtBatchBytes& b = r.bytes;
  const long long cn = B.cap_nodes, f64 = sizeof(double), i32 = sizeof(int32_t), u64 = sizeof(unsigned long long);
  b.nodes_f = batch_bytes({E, cn, 8, f64});
  b.nodes_i = batch_bytes({E, cn, 4, i32});
  b.points = batch_bytes({E, B.cap_points, 6, f64});
  b.bin_items = batch_bytes({E, B.bin_stride, i32});
  b.bin_count = batch_bytes({E, (long long)P.K + 1, i32});
  b.summary = batch_bytes({E, (long long)sizeof(RrtSummary)});
  b.node_c = batch_bytes({E, cn, 8, i32});
  b.node_q = batch_bytes({E, cn});
  if (p.mode == AUVP_MODE_NN) b.node_xy = batch_bytes({E, B.xy_stride, 2, f64});
  if (flags & AUVP_FLAG_ITER_LOG) {
    r.itlog_n = (long long)E * p.max_iter;
    b.itlog_i = batch_bytes({r.itlog_n, 2, i32});
    b.itlog_b = batch_bytes({r.itlog_n});
  }
  if (flags & AUVP_FLAG_LEAF_LOG) {
    b.leaf_c = batch_bytes({E, B.cap_leaves, 6, f64});
    b.leaf_i = batch_bytes({E, B.cap_leaves, i32});
  }
  b.leaf_stats = 8 * u64;
  if (flags & AUVP_FLAG_PHASE_CLOCKS) b.phase = batch_bytes({E, 5, u64});
  b.mt = batch_bytes({E, 624, (long long)sizeof(uint32_t)});
  if (const char* name = first_too_large({{"nodes", b.nodes_f}, {"points", b.points}, {"time-bin lists", b.bin_items}, {"time-bin counts", b.bin_count},
                                          {"nearest-neighbour mirror", b.node_xy}, {"iteration log", b.itlog_i}, {"leaf log", b.leaf_c}}))
    return refuse(RRT_BATCH_FIELD, name);  // (the buffers not named are no larger than one that is)
  return r;
}

// The rows of auvp_rrt_prepare_episodes: every episode's horizon, habitats and own K = ceil(max_traj_time / bin_interval) (<= the
// cap's K: ceil is monotone).  bad_episode >= 0: the first episode that is refused, and why
enum RrtEpisodeRefusal { RRT_EPISODE_OK = 0, RRT_EPISODE_HORIZON, RRT_EPISODE_KEEP, RRT_EPISODE_BINS };
struct RrtEpisodeLimits {
  int bad_episode = -1;
  RrtEpisodeRefusal why = RRT_EPISODE_OK;
  std::vector<RrtEpisodeLimDev> lim;
  std::vector<int32_t> K;
};
inline RrtEpisodeLimits rrt_episode_limits(const auvp_rrt_params& p, int H, const auvp_rrt_episode* episodes, int E) {
  RrtEpisodeLimits r;
  const uint64_t all = H >= 64 ? ~0ull : ((1ull << H) - 1ull);
  r.lim.resize((size_t)E);
  r.K.resize((size_t)E);
  for (int e = 0; e < E; e++) {
    const double t = episodes[e].max_traj_time;
    int K = 0;
    if (!(t > 0.0 && t <= p.max_traj_time)) r.why = RRT_EPISODE_HORIZON;
    else if (episodes[e].habitat_keep & ~all) r.why = RRT_EPISODE_KEEP;
    else if (!double_to_int(std::ceil(t / p.bin_interval), &K)) r.why = RRT_EPISODE_BINS;
    if (r.why != RRT_EPISODE_OK) { r.bad_episode = e; return r; }
    r.lim[(size_t)e] = RrtEpisodeLimDev{t, episodes[e].habitat_keep, K, 0};
    r.K[(size_t)e] = K;
  }
  return r;
}

// ---- the pre-generated random stream (rrt_stream_kernel.h): who keeps its buffer, how much to take, what was drawn ---------------

// "A batch like this keeps the stream buffer, and wants it once a figure is known": time-bin mode without per-episode limits,
// at least 1 000 iterations, option ROWS_STREAM not 0, and a four-episode kernel -- `rows`: by options and size before the batch
// has run (rrt_rows_wanted), the kernel it got after.  With a figure seen this is when rrt_choose_launch names
// rrt_rows_stream_kernel, except that the choice also knows the four-episode kernel's own limits and serves ROWS_STREAM = 1
// from 16 iterations on (tests/test_batch_plan_host.py lists the inputs)
inline bool rrt_stream_keeps(const OptionView& opt, int mode, int max_iter, bool lim, bool rows) {
  return !lim && mode == AUVP_MODE_TIMEBIN && max_iter >= 1000 && opt.opt_flag(OPT_ROWS_STREAM, true) && rows;
}

// The bytes to allocate for a stream of `bytes` when `free_b` are free on the device and the buffer holds `held` (< bytes): a
// buffer that has to grow is taken 1/16 larger than asked for where that fits beside a 4 GB margin -- the length follows the
// busiest episode seen so far, which creeps up by a few parts in a thousand from batch to batch, and every re-allocation of tens
// of GB is a second or two.  0: not even `bytes` fit beside the margin
inline unsigned long long rrt_stream_want_bytes(unsigned long long free_b, unsigned long long held, unsigned long long bytes) {
  const unsigned long long have = free_b + held, margin = 4ull << 30;
  const unsigned long long padded = bytes + bytes / 16;
  const unsigned long long want = have >= padded + margin ? padded : bytes;
  return have < want + margin ? 0 : want;
}

// What complete passes of RRT.exploring drew, per parameter block (the last four): the most random() numbers of one episode and
// the largest batch seen -- the length of the next batch's stream.  The most seen with these parameters: worlds that alternate
// between a little more and a little less do not make every other batch run past its stream
struct DrawnMemory {
  struct Slot { RrtParamsDev P{}; long long most = 0; int E = 0; unsigned long long used = 0; bool valid = false; };
  Slot slots[4];
  unsigned long long clock = 0;
  const Slot* find(const RrtParamsDev& P) const {
    for (const Slot& d : slots)
      if (d.valid && memcmp(&d.P, &P, sizeof P) == 0) return &d;
    return nullptr;
  }
  // a parameter block not seen before takes the slot used longest ago
  const Slot& record(const RrtParamsDev& P, long long most, int E) {
    Slot* d = const_cast<Slot*>(find(P));
    if (!d) {
      d = &slots[0];
      for (Slot& x : slots)
        if (!x.valid || (d->valid && x.used < d->used)) d = &x;
      *d = Slot{};
      d->P = P;
      d->valid = true;
    }
    d->most = d->most > most ? d->most : most;
    d->E = d->E > E ? d->E : E;
    d->used = ++clock;
    return *d;
  }
};

// ---- Planner_RRT ---------------------------------------------------------------------------------------------------------------

constexpr int PRRT_MAX_CAP_NODES = 1 << 24;    // a bucket's size is kept in 24 bits (PrrtBuffers::buckets)
constexpr double PRRT_MAX_BUCKETS = 5.0e7;
// sizes of the records planner_rrt_kernel.h defines (planner_rrt_host.h asserts them)
constexpr long long PRRT_NODE_BYTES = 64, PRRT_BUCKET_BYTES = 8, PRRT_SUMMARY_BYTES = 112;

struct PrrtBatchIn {
  int E = 0;
  auvp_prrt_params p{};
  int flags = 0;
  int n_obstacles = 0;
};

// in the order of the checks; from PRRT_BATCH_EMPTY_GRID on the previous batch has been given up (prrt_configure)
enum PrrtBatchStatus {
  PRRT_BATCH_OK = 0, PRRT_BATCH_BAD_ARGS, PRRT_BATCH_OBSTACLES, PRRT_BATCH_BAD_PARAMS, PRRT_BATCH_FIELD,
  PRRT_BATCH_EMPTY_GRID, PRRT_BATCH_BUCKETS, PRRT_BATCH_POINTS, PRRT_BATCH_STEPS
};

struct PrrtBatchBytes {
  unsigned long long nodes = 0, node_bucket = 0, points = 0, occupied = 0, buckets = 0, mt = 0, rng_state = 0, summary = 0, step_bucket = 0,
                     start = 0, goal = 0, st_log = 0;
};

struct PrrtBatchPlan {
  PrrtBatchStatus status = PRRT_BATCH_OK;
  const char* field = "";  // PRRT_BATCH_FIELD: what was refused
  int rows = 0, cols = 0, n_buckets = 0;
  double delta_theta = 0.0;
  int cap_nodes = 0, max_pts = 0, cap_points = 0;
  PrrtBatchBytes bytes;
};

inline PrrtBatchPlan prrt_batch_plan(const PrrtBatchIn& in) {
  PrrtBatchPlan r;
  const auvp_prrt_params& p = in.p;
  const int E = in.E;
  auto refuse = [&r](PrrtBatchStatus s, const char* field = "") { r.status = s; r.field = field; return r; };
  if (E <= 0) return refuse(PRRT_BATCH_BAD_ARGS);
  if (in.n_obstacles > 16 * 64) return refuse(PRRT_BATCH_OBSTACLES);
  int ics = 0, height = 0, width = 0, nfreq = 0;
  if (!double_to_int(p.cell_side_length, &ics)) return refuse(PRRT_BATCH_FIELD, "cell_side_length");
  if (ics <= 0 || p.subsections <= 0 || p.max_step <= 0 || !(p.freq >= 0)) return refuse(PRRT_BATCH_BAD_PARAMS);
  if (!double_to_int(std::floor(p.freq), &nfreq) || nfreq > INT_MAX - 64) return refuse(PRRT_BATCH_FIELD, "freq");
  if (p.max_step == INT_MAX) return refuse(PRRT_BATCH_FIELD, "max_step");
  // discretize_env (gym_rrt/envs/rrt_dubins.py:77-93): int(height) // int(cell), int(width) // int(cell)
  if (!double_to_int(p.rect[3] - p.rect[1], &height) || !double_to_int(p.rect[2] - p.rect[0], &width)) return refuse(PRRT_BATCH_FIELD, "rect");
  r.rows = height / ics;
  r.cols = width / ics;
  if (r.rows <= 0 || r.cols <= 0) return refuse(PRRT_BATCH_EMPTY_GRID);
  const double nbd = (double)r.rows * r.cols * p.subsections;
  if (nbd > PRRT_MAX_BUCKETS) return refuse(PRRT_BATCH_BUCKETS);
  r.n_buckets = (int)nbd;
  r.delta_theta = (double)(2.0 * M_PI) / (double)p.subsections;  // grid_cell_rrt.py:49
  r.cap_nodes = p.max_step + 1;
  r.max_pts = nfreq + 3;
  const double cp = (double)p.max_step * (double)(nfreq > 0 ? nfreq : 1) + 64;  // every taken sub-arc is stored
  if (cp > 2.0e9) return refuse(PRRT_BATCH_POINTS);
  r.cap_points = (int32_t)cp;
  if (r.cap_nodes >= PRRT_MAX_CAP_NODES) return refuse(PRRT_BATCH_STEPS);
  PrrtBatchBytes& b = r.bytes;
  const long long cn = r.cap_nodes, f64 = sizeof(double), i32 = sizeof(int32_t);
  b.nodes = batch_bytes({E, cn, PRRT_NODE_BYTES});
  b.node_bucket = batch_bytes({E, cn, i32});
  b.points = batch_bytes({E, r.cap_points, 4, f64});
  b.occupied = batch_bytes({E, cn, i32});
  b.buckets = batch_bytes({E, r.n_buckets, PRRT_BUCKET_BYTES});
  b.mt = batch_bytes({E, 624, (long long)sizeof(uint32_t)});
  b.rng_state = batch_bytes({E, 4, i32});
  b.summary = batch_bytes({E, PRRT_SUMMARY_BYTES});
  b.step_bucket = batch_bytes({E, i32});
  b.start = batch_bytes({E, 4, f64});
  b.goal = batch_bytes({E, 2, f64});
  if (in.flags & AUVP_FLAG_ITER_LOG) b.st_log = batch_bytes({E, p.max_step, 8, i32});
  if (const char* name = first_too_large({{"nodes", b.nodes}, {"points", b.points}, {"buckets", b.buckets}, {"step log", b.st_log}}))
    return refuse(PRRT_BATCH_FIELD, name);
  return r;
}

// random.getstate()'s position inside the 624 words -> the kernels' row {pos, left, 0, 0} (PrrtBuffers::rng_state): 624 = a
// block is due, so nothing is left and the position is the first word's
inline std::vector<int32_t> prrt_rng_state_rows(const int32_t* mt_index, int E) {
  std::vector<int32_t> rs((size_t)E * 4, 0);
  for (int e = 0; e < E; e++) {
    const int idx = mt_index[e] < 0 ? 0 : (mt_index[e] > 624 ? 624 : mt_index[e]);
    rs[4 * (size_t)e] = idx == 624 ? 0 : idx;
    rs[4 * (size_t)e + 1] = 624 - idx;
  }
  return rs;
}

// ---- epoch tags ----------------------------------------------------------------------------------------------------------------

// A table whose entries carry an 8-bit tag (Planner_RRT's buckets, the A* visited words) is emptied by taking the next tag; it is
// cleared where its allocation is new (`must_clear`) or the tag would wrap (tag 0 is never current).
// (255: tests/test_gpu_epoch_wrap.py runs 260 batches on one handle and counts on the wrap falling at batch 256, and
// tests/test_gpu_astar_pair.py::test_the_redo_clears_the_visited_words_at_the_tag_wrap gives up on batch 255)
struct EpochTag { uint32_t tag; bool clear; };
inline EpochTag epoch_tag_next(uint32_t tag, bool must_clear) {
  const bool clear = must_clear || tag >= 255u;
  return EpochTag{(clear ? 0u : tag) + 1u, clear};
}

}  // namespace auvp
#endif  // AUVP_BATCH_PLAN_H

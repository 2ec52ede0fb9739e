// launch_plan.h -- which kernel a batch of RRT.exploring / Planner_RRT gets, and at what shape: the host's choice as data.
//
// Host only and pure: no HIP runtime call, no heap, no handle, no environment.  rrt_choose_launch / prrt_choose_launch read a
// plain description of the batch (RrtLaunchIn / PrrtLaunchIn) and the handle's options (OptionView) and return the launch
// (RrtLaunchPlan / PrrtLaunchPlan); auvplan.hip and planner_rrt_host.h launch what the plan says.  Every threshold below is a
// measured number (the comment beside it names the tool).  auvp_rrt_choose_launch / auvp_prrt_choose_launch (include/auvplan.h)
// answer the same question without a device: tests/test_launch_plan.py pins the rules, tests/test_gpu_launch_plan.py that a
// handle launches what the query says.
// Included by auvplan.hip behind the kernel headers whose LDS plans and limits it reads.
#ifndef AUVP_LAUNCH_PLAN_H
#define AUVP_LAUNCH_PLAN_H
#include <cmath>
#include <type_traits>

#include "launch_options.h"  // (the options, OptionView, rrt_rows_by_size, rrt_stream_len: free of the kernel headers)

namespace auvp {

constexpr int LDS_LIMIT = 160 * 1024;  // of a workgroup, bytes

// Obstacles per lane (J) of the kernels that hold the obstacle list in J x 64 slots: the compile-time specialisation a world of
// n_obstacles gets.  cap: 4 (duo / trio / pipe: at most 256 obstacles) or 16 (rrt_explore_kernel, prrt_kernel: at most 1 024)
inline int obstacle_J(int n_obstacles, int cap) {
  const int j = n_obstacles <= 64 ? 1 : (n_obstacles <= 128 ? 2 : (n_obstacles <= 256 ? 4 : (n_obstacles <= 512 ? 8 : 16)));
  return j < cap ? j : cap;
}
// f(std::integral_constant<int, J>) for that J -- only the J up to CAP are instantiated
template <int CAP, class F>
auto for_obstacle_J(int n_obstacles, F&& f) {
  static_assert(CAP == 4 || CAP == 16, "the kernels are instantiated up to J = 4 or J = 16");
  const int j = obstacle_J(n_obstacles, CAP);
  if (j == 1) return f(std::integral_constant<int, 1>{});
  if (j == 2) return f(std::integral_constant<int, 2>{});
  if constexpr (CAP > 4) {
    if (j == 8) return f(std::integral_constant<int, 8>{});
    if (j == 16) return f(std::integral_constant<int, 16>{});
  }
  return f(std::integral_constant<int, 4>{});
}

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- RRT.exploring ---------------------------------------------------------------------------------------------------------

struct RrtLaunchIn {
  int E = 0;       // episodes of the batch
  int n_cu = 256;  // compute units of the device
  int mode = 0, max_iter = 0, K = 0, flags = 0;  // of the batch's RrtParamsDev
  double freq = 0.0, dist_to_end = 0.0;          // ...
  int max_pts = 0;                               // path points of a steer at most (floor(freq) + 2)
  int O = 0, H = 0, V = 0, T = 0;                // the world: obstacles, habitats, boundary vertices, time bins
  double obst_area = 0.0;      // area of the bounding box of the obstacle centres (0: fewer than two obstacles / degenerate)
  bool lim = false;            // per-episode limits (auvp_rrt_prepare_episodes)
  bool one_wave_only = false;  // never a speculative pipeline (the pipeline fallback's second pass)
  bool no_stream = false;      // the random numbers are generated inside the expansion kernel whatever option ROWS_STREAM says
  long long seen_most = 0;     // what earlier batches with this parameter block drew: the most random() numbers of one episode
  int seen_E = 0;              // ... and the largest such batch (0: nothing seen)
};

enum RrtKernelKind { RRT_EXPLORE, RRT_EXPLORE_LIM, RRT_DUO, RRT_TRIO, RRT_ROWS, RRT_ROWS_STREAM };
enum LaunchPlanStatus {
  PLAN_OK = 0,
  PLAN_LDS_ONE_WAVE,  // the one-episode-per-wavefront plan needs lds_need bytes > LDS_LIMIT (checked for every batch, as ever)
  PLAN_LDS_PIPELINE  // the duo / trio plan does
};

struct RrtLaunchPlan {
  RrtKernelKind kind = RRT_EXPLORE;
  int J = 1;          // obstacles per lane (explore, explore_lim, duo, trio)
  bool quad = false;  // trio: the parent lookup as a fourth wavefront per episode
  int grid = 0, block = 0, lds = 0;
  int lds_max = 0;  // the kernel's dynamic-LDS attribute (the four-episode kernels: see below; lds otherwise)
  int kflags = 0;   // AUVP_KFLAG_TIGHT_CULL | AUVP_KFLAG_NN_EXACT: or-ed into the kernel's copy of the parameters
  long long stream_len = 0;             // rows_stream: random() numbers per episode generated ahead
  int stream_waves = 0, mirror = 0;     // rows_stream: waves per workgroup; the ring's form (1 mirrored, 0 masked)
  const char* name = "";                // what auvp_rrt_last_kernel reports
  LaunchPlanStatus status = PLAN_OK;
  long long lds_need = 0;
  bool rows() const { return kind == RRT_ROWS || kind == RRT_ROWS_STREAM; }
};

inline RrtLaunchPlan rrt_choose_launch(const RrtLaunchIn& in, const OptionView& opt) {
  RrtLaunchPlan p;
  const int E = in.E, n_cu = in.n_cu, O = in.O;
  const int nfreq = (int)std::floor(in.freq);
  const int tables = rrt_tables_bytes(in.H, in.V, in.T);
  // Where the obstacles are dense the cull of a steer uses the tight box of its path points instead of the square of
  // its total movement (fewer exact tests for ~100 extra instructions): decided here from the expected number of
  // obstacles inside a typical reach square, 4 (freq dist_to_end / 4)^2 O / (area of the obstacles' bounding box).
  {
    const double reach = 0.25 * in.freq * in.dist_to_end;
    const double lam = in.obst_area > 0.0 ? 4.0 * reach * reach * (double)O / in.obst_area : (O > 0 ? 1e9 : 0.0);
    if (opt.opt_flag(OPT_TIGHT_CULL, lam > 0.5)) p.kflags |= AUVP_KFLAG_TIGHT_CULL;
    if (opt.opt_on(OPT_NN_EXACT)) p.kflags |= AUVP_KFLAG_NN_EXACT;
  }
  const bool diag = (in.flags & (AUVP_FLAG_ITER_LOG | AUVP_FLAG_LEAF_LOG | AUVP_FLAG_PHASE_CLOCKS)) != 0;
  // One episode per wavefront (rrt_explore_kernel.h).
  // Small batches (at most eight episodes per CU: config 2's 1 024 replicas) get workgroups of fewer waves, so that every CU
  // holds one (1 024 episodes: 256 workgroups of four waves = one wave per SIMD, instead of 128 CUs with two per SIMD:
  // 208 -> 229 M expansions/s).  A latency instantiation on top of that -- 124 VGPRs without the 80-register cap, the steer's
  // running sums as 32 unrolled steps with all reads up front -- was bit-identical and SLOWER (4.2 -> 5.7 us per expansion:
  // the loops only run n / 2 ~ 7 trips) and is not kept.
  const int xw = E <= 8 * n_cu ? clamp_int(ceil_div(E, n_cu), 1, RRT_X_WAVES) : RRT_X_WAVES;
  p.J = obstacle_J(O, 16);
  const long long x_lds = rrt_lds_plan(in.K, in.max_pts, nfreq, p.J * 64, tables, xw).total;
  if (x_lds > LDS_LIMIT) { p.status = PLAN_LDS_ONE_WAVE; p.lds_need = x_lds; return p; }
  // four episodes per wavefront (rrt_rows_kernel.h) where its limits allow; one episode per wavefront otherwise
  const RowsLdsPlan rp = rrt_rows_lds_plan(in.K, RW_MAX_OBST, tables);
  const bool iter_log = (in.flags & (AUVP_FLAG_ITER_LOG | AUVP_FLAG_PHASE_CLOCKS)) != 0;
  // ... and where it pays: a batch the one-episode kernel can keep resident in one go (6 waves per SIMD = 24 episodes per
  // CU) runs faster there -- the rows kernel would leave the SIMDs with one or two waves.  Measured on MI355X, M
  // expansions/s one-episode vs rows: 4 096 episodes 616 vs 507, 6 144 episodes 704 vs 645, 8 192 episodes 699 vs 849,
  // 10 240 episodes 737 vs 877.  End of round 6 (the rows kernel has lost a quarter of its instructions since), same batches:
  // 4 096 episodes 631 vs 606, 5 120: 609 vs 647, 6 144: 727 vs 773, 8 192: 715 vs 1 014 -- the crossover is between 16 and 20
  // episodes per CU now: rows above 18 (tools/batch_size_probe.py).  Option ROWS = 1 / 0 forces it on (limits permitting) / off.
  // (a batch with per-episode limits runs rrt_explore_lim_kernel, whatever the options say)
  const bool rows_ok = !in.lim && in.mode == 0 && !iter_log && nfreq <= RW_MAX_FREQ && O <= RW_MAX_OBST && in.max_iter < 65534 &&
                       rp.total <= LDS_LIMIT;
  const bool use_rows = rows_ok && rrt_rows_wanted(opt, E, n_cu);
  // latency runs (at most four episodes per CU: one episode, config 2's 1 024 replicas): two wavefronts per episode
  // (rrt_duo_kernel.h).  Option DUO = 1 / 0 forces it on (limits permitting) / off.
  const bool duo_ok = !in.lim && in.mode == 0 && !diag && nfreq <= DUO_MAX_FREQ && nfreq >= 1 && O <= 256 && in.max_pts <= 64;
  // Measured (tools/duo_probe.py, M expansions/s one vs two wavefronts per episode): 1 episode 0.25 vs 0.32, 256: 62 vs 80,
  // 1 024: 227 vs 271 (config 2's replicas, 64 obstacles: 241 vs 283), 2 048: 409 vs 435, 4 096: 621 vs 485
  const bool use_duo = duo_ok && !use_rows && !in.one_wave_only && opt.opt_flag(OPT_DUO, E <= 8 * n_cu);
  // ... and three (rrt_trio_kernel.h: stream, geometry, tree -- a pipeline over the iterations) for at most four episodes per
  // CU.  Measured (tools/duo_probe.py, M expansions/s, one / two / three wavefronts per episode): 1 episode 0.25 / 0.32 / 0.40,
  // 256: 61 / 80 / 95, 1 024: 226 / 271 / 303 (config 2's replicas: 239 / 282 / 309), 2 048: 406 / 434 / 304.
  // Option TRIO = 1 / 0 forces it on (limits permitting) / off; an explicit DUO = 1 takes precedence.
  const bool use_trio = duo_ok && !use_rows && !in.one_wave_only && opt.opt_flag(OPT_TRIO, E <= TRIO_EP * n_cu && !opt.opt_on(OPT_DUO));
  if (use_trio || use_duo) {
    const int eps_wg = clamp_int(ceil_div(E, n_cu), 1, use_trio ? TRIO_EP : DUO_EP);
    p.kind = use_trio ? RRT_TRIO : RRT_DUO;
    p.name = use_trio ? "rrt_trio_kernel" : "rrt_duo_kernel";
    p.J = obstacle_J(O, 4);
    p.lds = use_trio ? trio_lds_bytes(in.K, p.J * 64, tables, eps_wg) : duo_lds_bytes(in.K, in.max_pts, p.J * 64, tables, eps_wg);
    if (p.lds > LDS_LIMIT) { p.status = PLAN_LDS_PIPELINE; p.lds_need = p.lds; return p; }
    // the parent lookup as a fourth wavefront per episode (rrt_trio_kernel<J, 4>) where every episode has a CU to itself: one
    // episode 2.52 -> 2.49 us per expansion, 256 episodes 95 -> 100 M/s (1 024: 303 -> 262 M/s, so not there).  Option QUAD
    p.quad = use_trio && opt.opt_flag(OPT_QUAD, E <= n_cu);
    if (p.quad) p.name = "rrt_trio_kernel<4 wavefronts>";
    p.grid = ceil_div(E, eps_wg);
    p.block = eps_wg * (use_trio ? (p.quad ? 256 : 192) : 128);
    p.lds_max = p.lds;
    return p;
  }
  if (!use_rows) {
    p.kind = in.lim ? RRT_EXPLORE_LIM : RRT_EXPLORE;
    p.name = in.lim ? "rrt_explore_lim_kernel" : "rrt_explore_kernel";
    p.grid = ceil_div(E, xw); p.block = xw * 64; p.lds = p.lds_max = (int)x_lds;
    return p;
  }
  // a workgroup of up to 12 waves (48 episodes) fills one CU; a batch that cannot give every CU such a workgroup is
  // spread over all CUs with fewer waves per workgroup instead of leaving CUs idle
  // (option ROWS_WG_WAVES: the waves per workgroup instead, both forms of the kernel -- tests: small batches at the shapes
  // only full-chip batches get otherwise)
  const int wanted = (int)opt.opt_num(OPT_ROWS_WG_WAVES, ceil_div(E, RW_ROWS * n_cu));
  // round 6: the episodes' random() numbers generated AHEAD by a launch of its own (rrt_stream_kernel.h: one wavefront per
  // episode, every lane busy) and read by rrt_rows_stream_kernel -- no generator, no tempering, 2.5 KB less LDS per episode in
  // the expansion kernel.  Measured on the headline batch: the expansion launch 93.7 -> 81.5 ms (953 instead of 1 284 vector
  // instructions per trip), generating 46 GB of numbers ahead 9.4 ms, the pass 99.6 -> 96.9 ms (profiles/r6_rows_stream.md).
  // The stream's length is a bound, and how many numbers an iteration draws depends on the PARAMETERS (44.8 with the bench's,
  // 92 with the leaves looked at every iteration) and hardly on the world (bench world, 64 / 256 obstacles, dense boxes,
  // concave outlines, accept rates 0.54 .. 0.99: the busiest of 1 024 episodes draws 45.56 .. 45.86 per iteration at 10 000
  // iterations, profiles/r6_rows_stream.md): it is set from what earlier batches with the same parameter block drew -- the
  // busiest episode seen + 3 % + 1 024 numbers (rrt_leaf_kernel reports the figure: leaf_stats[4]) -- whatever world they
  // ran on, so a caller that replans on a changing world (replanning: rrt_dubins.py:297-331) is served as well.  The first
  // batch with a parameter block runs rrt_rows_kernel and the following ones this path; an episode that runs past its
  // stream all the same is reported through the mapped flag and auvp_rrt_run redoes the batch with the kernel above (which
  // records the new figure).  Option ROWS_STREAM = 0: never; = 1: also without a previous batch (46.5 numbers
  // per iteration + 4 096), and a stream that does not fit the free memory beside a 4 GB margin is an error instead of a
  // quiet no (rrt_run_pass); ROWS_STREAM_CAP: the length in numbers (tests).
  // (a batch at most four times the size of the one the figure comes from: the busiest of more episodes is busier)
  const bool seen = in.seen_most > 0 && !((long long)in.seen_E * 4 < E);
  bool use_stream = !in.no_stream && in.max_iter >= 16 && opt.opt_flag(OPT_ROWS_STREAM, seen && in.max_iter >= 1000);
  if (use_stream) {
    p.stream_len = rrt_stream_len(opt, seen ? in.seen_most : 0, in.max_iter);
    if (p.stream_len > 0x7fffffffll) { use_stream = false; p.stream_len = 0; }  // (positions are 32-bit in the kernel)
  }
  if (!use_stream) {
    // (the kernel's dynamic-LDS attribute is the twelve-wave plan's total whatever the launch's own count)
    const int wg_waves = clamp_int(wanted, 1, RW_WAVES);
    p.kind = RRT_ROWS;
    p.name = "rrt_rows_kernel";
    p.grid = ceil_div(E, wg_waves * RW_ROWS); p.block = wg_waves * 64;
    p.lds = rrt_rows_lds_plan(in.K, RW_MAX_OBST, tables, wg_waves).total;
    p.lds_max = rp.total;
    return p;
  }
  // without the generator's state an episode needs 2.3 KB of LDS instead of 3.3: a CU holds 64 of them -- sixteen wavefronts,
  // four per SIMD -- but that instantiation spills (rows_kernels.hip): twelve at most, like rrt_rows_kernel (option
  // ROWS_STREAM_WAVES: fewer, for experiments)
  // (the four-per-SIMD form measured 0.93 G expansions/s against 1.16: 100 B of scratch per lane at 128 registers)
  const int sw_max = (int)opt.opt_num(OPT_ROWS_STREAM_WAVES, RW_WAVES);
  const int sw = wanted < 1 ? 1 : (wanted > sw_max ? sw_max : wanted);
  // the ring's form: its first 48 entries mirrored behind it (reads at one address per lane plus an immediate: 3 KB per
  // episode) where that plan fits at the wave count the masked plan (2.8 KB) allows -- never a wavefront fewer for it
  // (rrt_rows_stream_shape; option ROWS_STREAM_MIRROR = 0 / 1: the masked / the mirrored form whatever the rule says)
  const RowsStreamShape shape = rrt_rows_stream_shape(in.K, RW_MAX_OBST, tables, sw,
                                                      opt.opt_has[OPT_ROWS_STREAM_MIRROR] ? (opt.opt_on(OPT_ROWS_STREAM_MIRROR) ? 1 : 0) : -1);
  p.kind = RRT_ROWS_STREAM;
  p.name = "rrt_rows_stream_kernel";
  p.stream_waves = shape.waves; p.mirror = shape.mirror ? 1 : 0;
  p.grid = ceil_div(E, shape.waves * RW_ROWS); p.block = shape.waves * 64;
  p.lds = p.lds_max = shape.plan.total;
  return p;
}

// ---- Planner_RRT -----------------------------------------------------------------------------------------------------------

struct PrrtLaunchIn {
  int E = 0, n_cu = 256;
  int O = 0;          // obstacles of the world
  double freq = 0.0;  // of the batch's parameters
  int max_pts = 0, cap_nodes = 0;              // of its buffers
  int n_buckets = 0, max_step = 0, flags = 0;  // of its parameters
  int step_mode = 0;           // 0 planning(max_step), 1 generate_one_node
  bool waits = true;           // the call waits for the launch (an enqueue-only call of the device-resident loop does not)
  bool one_wave_only = false;  // never the speculative pipeline (the pipeline fallback's second launch)
  int rows = -1;               // the four-episode choice: -1 decide it (prrt_configure: once per batch), 0 / 1 the frozen value
};

enum PrrtKernelKind { PRRT_ONE, PRRT_PIPE, PRRT_ROWS };

struct PrrtLaunchPlan {
  PrrtKernelKind kind = PRRT_ONE;
  bool lat = false;   // latency batch: prrt_kernel's latency instantiation, small workgroups
  bool rows = false;  // four episodes per wavefront (frozen per batch)
  bool pipe = false, draw_wave = false;      // the pipeline; its fifth wavefront per episode
  bool next_lds = false, bk_lds = false;     // pipeline: the member lists' next links / the bucket table + occupied list in LDS
  bool obst_lds = false;                     // rows: the obstacle slot tables as an LDS tile
  int occ_bytes = 0;                         // rows: LDS copy of an episode's occupied list (prrt_rows_occ_bytes)
  int eps_wg = 0;                            // episodes per workgroup
  int grid = 0, block = 0, lds = 0, J = 1;
  const char* name = "";                     // what auvp_prrt_last_kernel reports
  LaunchPlanStatus status = PLAN_OK;         // PLAN_LDS_ONE_WAVE: prrt_kernel's plan needs lds_need bytes (checked for every batch)
  long long lds_need = 0;
};

// Throughput batches (more than twelve episodes per CU) of the environment's planner shape run four episodes per
// wavefront (planner_rows_kernel.h); the others are latency batches (at most three waves per SIMD on this GPU: register budget
// and steer of prrt_kernel differ, planner_rrt_kernel.h).
// (Twelve: re-measured at the end of round 6 on config 4's world, M steps/s one wavefront per episode (latency
// instantiation) / four episodes per wavefront: 2 048 episodes 276 / 178, 3 072: 334 / 262, 4 096: 311 / 342, 8 192: 359 / 588
// -- tools/prrt_batch_probe.py; the threshold had been eight per CU.)
constexpr int PRRT_LAT_EP_PER_CU = 12;

inline PrrtLaunchPlan prrt_choose_launch(const PrrtLaunchIn& in, const OptionView& opt) {
  PrrtLaunchPlan p;
  const int E = in.E, n_cu = in.n_cu, O = in.O;
  const int nfreq = (int)std::floor(in.freq);
  const bool iter_log = (in.flags & AUVP_FLAG_ITER_LOG) != 0;
  p.lat = opt.opt_flag(OPT_PRRT_LAT, E <= PRRT_LAT_EP_PER_CU * n_cu);
  // option PRRT_ROWS = 0 / 1 forces the four-episode choice where the kernel's limits allow it.  Decided once per batch: the two
  // kernels keep the generator's lazy state in different block phases
  const bool rows_ok = nfreq <= PRW_MAX_FREQ && O <= RW_MAX_OBST && !iter_log;
  p.rows = in.rows < 0 ? rows_ok && opt.opt_flag(OPT_PRRT_ROWS, !p.lat) : in.rows != 0;
  // latency runs: workgroups small enough that every CU gets one (512 episodes: 256 workgroups of two waves)
  const int wg_waves = p.lat ? clamp_int(ceil_div(E, n_cu), 1, RRT_WAVES) : RRT_WAVES;
  const size_t one_lds = (size_t)wg_waves * prrt_lds_per_wave(in.max_pts, nfreq, p.lat);
  if (one_lds > (size_t)LDS_LIMIT) { p.status = PLAN_LDS_ONE_WAVE; p.lds_need = (long long)one_lds; return p; }
  // plan-mode latency runs of at most four episodes per CU: a pipeline of four wavefronts per episode (planner_pipe_kernel.h).
  // Option PRRT_PIPE = 0 / 1 forces the choice where the kernel's limits allow it.  Only where the call waits for the launch:
  // the pipeline is speculative and an episode it gives up on is redone on prrt_kernel (pipeline fallback, prrt_launch).
  p.pipe = in.waits && !in.one_wave_only && !p.rows && in.step_mode == 0 && p.lat && !iter_log && nfreq <= DUO_MAX_FREQ && O <= 256 &&
           in.max_pts <= DUO_CS + 2 && opt.opt_flag(OPT_PRRT_PIPE, E <= 4 * n_cu);
  if (p.rows) {
    // persistent rows (four episodes per wavefront) fed from a device counter: as many workgroups as fit the chip at
    // three per CU (one wave per SIMD each), fewer when the batch is smaller
    p.kind = PRRT_ROWS;
    p.name = "prrt_rows_kernel";
    p.eps_wg = PRW_WAVES * RW_ROWS;
    p.grid = ceil_div(E, p.eps_wg) < 3 * n_cu ? ceil_div(E, p.eps_wg) : 3 * n_cu;
    // (option PRRT_ROWS_GRID: at most that many workgroups, at least one -- it only ever lowers the grid, and the kernel has no
    // waits between workgroups, so any grid >= 1 is valid.  tests: with fewer rows than episodes every batch refills its rows,
    // which by default depends on timing below 48 episodes per CU)
    if (opt.opt_has[OPT_PRRT_ROWS_GRID]) {
      const long long cap = opt.opt_val[OPT_PRRT_ROWS_GRID] < 1 ? 1 : opt.opt_val[OPT_PRRT_ROWS_GRID];
      if (cap < p.grid) p.grid = (int)cap;
    }
    p.block = PRW_WAVES * 64;
    p.occ_bytes = prrt_rows_occ_bytes(in.n_buckets, in.max_step);
    p.lds = p.eps_wg * (PRW_LDS_PER_EP + p.occ_bytes);
    // the obstacle slot tables as an LDS tile where three workgroups per CU still fit beside it (option PRRT_OBST_LDS overrides)
    // (LDS is handed out in 1 280-byte granules on this GPU: three workgroups of 53 760 B fit a CU, three of 54 272 B do not)
    const int granules = (p.lds + PRW_OBST_TILE + 1279) / 1280 * 1280;
    p.obst_lds = opt.opt_flag(OPT_PRRT_OBST_LDS, 3 * granules <= LDS_LIMIT);
    if (p.obst_lds) p.lds += PRW_OBST_TILE;
  } else if (p.pipe) {
    // four wavefronts per episode, feed-forward (planner_pipe_kernel.h)
    p.kind = PRRT_PIPE;
    p.name = "prrt_pipe_kernel";
    p.J = obstacle_J(O, 4);
    p.eps_wg = clamp_int(ceil_div(E, n_cu), 1, PPIPE_EP);
    // round 6: a FIFTH wavefront per episode takes the sub-arc draws off H, the slowest stage (planner_pipe_kernel.h: D) -- where
    // a workgroup of five-wavefront episodes fits the 1 024-thread limit (at most three episodes per workgroup: up to 768
    // episodes on this GPU; config 4's 512 run two per CU).  Option PRRT_PIPE_DRAW = 0 / 1 forces the choice within that limit.
    p.draw_wave = p.eps_wg <= PPIPE_EP5 && opt.opt_flag(OPT_PRRT_PIPE_DRAW, true);
    p.grid = ceil_div(E, p.eps_wg);
    p.block = p.eps_wg * (p.draw_wave ? 320 : 256);
    const size_t fits = (size_t)150 * 1024;
    // the member lists' next links in LDS where they fit beside the slots (option PRRT_NEXT_LDS = 0 keeps them in memory)
    p.next_lds = (size_t)p.eps_wg * ppipe_per_episode_bytes(in.max_pts, in.cap_nodes) <= fits && opt.opt_flag(OPT_PRRT_NEXT_LDS, true);
    // round 6: ... and the bucket table + the occupied list, where they fit too (config 4: 1 600 buckets = 19 KB per episode;
    // option PRRT_BUCKET_LDS = 0 keeps them in memory)
    const int next_nodes = p.next_lds ? in.cap_nodes : 0, occ_cap = ppipe_occ_entries(in.n_buckets, in.cap_nodes);
    p.bk_lds = (size_t)p.eps_wg * ppipe_per_episode_bytes(in.max_pts, next_nodes, in.n_buckets, occ_cap) <= fits &&
               opt.opt_flag(OPT_PRRT_BUCKET_LDS, true);
    p.lds = (int)((size_t)p.eps_wg * ppipe_per_episode_bytes(in.max_pts, next_nodes, p.bk_lds ? in.n_buckets : 0, p.bk_lds ? occ_cap : 0));
  } else {
    p.kind = PRRT_ONE;
    p.name = "prrt_kernel";
    p.J = obstacle_J(O, 16);
    p.eps_wg = wg_waves;
    p.grid = ceil_div(E, wg_waves); p.block = wg_waves * 64; p.lds = (int)one_lds;
  }
  return p;
}

}  // namespace auvp
#endif  // AUVP_LAUNCH_PLAN_H

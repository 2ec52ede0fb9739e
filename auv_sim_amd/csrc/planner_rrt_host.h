// planner_rrt_host.h -- C-ABI entry points for Planner_RRT (auvp_prrt_*), host side.
// Included at the end of auvplan.hip (same translation unit: uses auvp_handle, fail, HIPCHK, upload).
#ifndef AUVP_PLANNER_RRT_HOST_H
#define AUVP_PLANNER_RRT_HOST_H

static_assert(sizeof(auvp_prrt_summary) == sizeof(auvp::PrrtSummary), "prrt summary layout");
static_assert(sizeof(auvp::PrrtNode) == auvp::PRRT_NODE_BYTES && sizeof(int2) == auvp::PRRT_BUCKET_BYTES &&
              sizeof(auvp::PrrtSummary) == auvp::PRRT_SUMMARY_BYTES, "the record sizes batch_plan.h counts bytes by");

namespace {

struct PrrtState {
  bool ready = false;
  int E = 0;
  auvp::PrrtParamsDev P{};
  auvp::PrrtBuffers B{};
  DevBuf nodes, node_bucket, points, occupied, buckets, mt, rng_state, start, goal, step_bucket, summary, st_log,
      tmp_off, tmp_out, env_done, thetas, seeds;
  // the bucket table's current epoch (PrrtBuffers::bucket_epoch): a new batch on the same allocation takes the next one; the
  // table is cleared when the allocation changes or the 8-bit tag would wrap
  int bucket_epoch = 0;
  void* bucket_alloc = nullptr;
  size_t bucket_alloc_bytes = 0;
  size_t bucket_bytes = 0;  // of the configured batch's table (the plan's figure)
  // work counter of the four-episodes-per-wavefront kernel (planner_rows_kernel.h).  It is never reset between launches: a
  // launch hands out ids counter - work_base, and every one of its rows ends with exactly one pull that finds no episode, so
  // the next launch's base is known on the host (no fill launch per plan / step)
  DevBuf snap_sum, snap_rng, snap_mt, redo_mask, redo_count;  // the pipeline fallback's snapshot of a launch's episodes
  DevBuf work;
  int work_base = 0;
  bool work_memset = false;  // set by the first launch under stream capture: the counter is zeroed by a memset node per launch
  bool use_rows = false;  // decided once per batch: the two kernels keep the generator's lazy state in different block phases
  const char* last_kernel = "";
  DevBuf env_err;    // device int32[2]: {status, environment} of the first episode that failed inside the device-resident loop
  // captured step graphs of the device-resident loop (auvp_graph_*).  A graph holds raw device pointers (this batch's
  // buffers and the caller's observation / reward arrays): it dies with the batch it was captured for -- prrt_configure
  // destroys them, and the ids stay taken so that a stale id can never reach another batch's graph.
  std::vector<hipGraphExec_t> graphs;
  void drop_graphs() { for (auto& g : graphs) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; } }
  ~PrrtState() { drop_graphs(); }
  bool thetas_ready = false;
};

PrrtState* prrt_of(auvp_handle* h);

}  // namespace
extern "C" hipError_t auvpi_prrt_rows_launch(int obst_lds, const auvp::WorldDev* W, const auvp::PrrtParamsDev* P, const auvp::PrrtBuffers* B,
                                             int n_episodes, int* work_counter, int work_base, int occ_bytes, int grid, int block, int lds,
                                             hipStream_t stream);
namespace {

// what prrt_choose_launch (launch_plan.h) reads of a batch; rows: -1 decide the four-episode choice, else the batch's frozen value
auvp::PrrtLaunchIn prrt_launch_in(const auvp_handle* h, const PrrtState& S, int E, int rows) {
  auvp::PrrtLaunchIn in;
  in.E = E; in.n_cu = h->n_cu; in.O = h->W.n_obstacles; in.freq = S.P.freq;
  in.max_pts = S.B.max_pts; in.cap_nodes = S.B.cap_nodes;
  in.n_buckets = S.P.n_buckets; in.max_step = S.P.max_step; in.flags = S.P.flags;
  in.rows = rows;
  return in;
}

// `sync`: wait for the launch and record its HIP-event time (the device-resident loop passes false: it only enqueues)
int prrt_launch(auvp_handle* h, PrrtState& S, int step_mode, bool sync = true, bool one_wave_only = false) {
  S.P.step_mode = step_mode;
  if (!one_wave_only) { h->pipe_clear(); h->pipe_fallback_last = 0; }
  auvp::PrrtLaunchIn in = prrt_launch_in(h, S, S.E, S.use_rows ? 1 : 0);
  in.step_mode = step_mode; in.waits = sync; in.one_wave_only = one_wave_only;
  const auvp::PrrtLaunchPlan plan = auvp::prrt_choose_launch(in, h->opt);
  if (plan.status != auvp::PLAN_OK) return fail(h, AUVP_ERR_ARG, "LDS need %zu B > 160 KiB", (size_t)plan.lds_need);
  const int O = h->W.n_obstacles;
  auto launch = [&](auto kern, const auto&... more) {
    return launch_kernel(kern, plan.grid, plan.block, plan.lds, h->stream, h->W, S.P, S.B, S.E, more...);
  };
  if (sync) HIPCHK(h, hipEventRecord(h->ev0, h->stream));  // (enqueue-only calls may be under stream capture: no events)
  hipError_t le;
  S.last_kernel = plan.name;
  switch (plan.kind) {
  case auvp::PRRT_ROWS: {
    // The ids a launch hands out are counter - work_base.  Eager launches carry the base as an argument (no memset per
    // launch).  A launch recorded into a hipGraph would freeze that argument while the counter keeps advancing on every
    // replay, so from the first capture on this state zeroes the counter with a memset NODE in front of every launch and
    // passes base 0 -- captured and eager launches alike (a replay may run between any two eager launches).
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(h->stream, &cap);
    if (cap != hipStreamCaptureStatusNone) S.work_memset = true;
    if (!S.work.p) {
      if (cap != hipStreamCaptureStatusNone) return fail(h, AUVP_ERR_STATE, "the rows work counter must exist before a stream capture (run one eager step first)");
      le = S.work.reserve(sizeof(int));
      if (le == hipSuccess) le = hipMemsetAsync(S.work.p, 0, sizeof(int), h->stream);
      S.work_base = 0;
    } else if (S.work_memset || S.work_base > (1 << 30)) {
      le = hipMemsetAsync(S.work.p, 0, sizeof(int), h->stream);
      S.work_base = 0;
    } else le = hipSuccess;
    if (le == hipSuccess) {
      // (the kernel lives in prrt_rows_kernels.hip: a translation unit with its own compiler flags)
      le = auvpi_prrt_rows_launch(plan.obst_lds ? 1 : 0, &h->W, &S.P, &S.B, S.E, S.work.as<int>(), S.work_base, plan.occ_bytes, plan.grid,
                                  plan.block, plan.lds, h->stream);
      // every episode once + one empty pull per row; a failed launch pulled nothing, a memset-fronted one restarts at 0
      if (le == hipSuccess && !S.work_memset) S.work_base += S.E + plan.grid * plan.eps_wg;
    }
    break;
  }
  case auvp::PRRT_PIPE: {
    // what the fallback needs to take an episode back to where this launch found it: its record, generator and position
    le = S.snap_sum.reserve((size_t)S.E * sizeof(auvp::PrrtSummary));
    if (le == hipSuccess) le = S.snap_rng.reserve((size_t)S.E * 4 * sizeof(int32_t));
    if (le == hipSuccess) le = S.snap_mt.reserve((size_t)S.E * 624 * sizeof(uint32_t));
    if (le == hipSuccess) le = S.redo_mask.reserve((size_t)S.E);
    HIPCHK(h, le);
    hipLaunchKernelGGL(auvp::prrt_snapshot_kernel, dim3(S.E), dim3(256), 0, h->stream, S.B, S.snap_sum.as<auvp::PrrtSummary>(),
                       S.snap_rng.as<int32_t>(), S.snap_mt.as<uint32_t>());
    HIPCHK(h, hipGetLastError());
    // (ev0 was recorded before the snapshot: the time a caller is told includes it -- every latency-path plan call pays it)
    const int in_lds = (plan.next_lds ? 1 : 0) | (plan.bk_lds ? 2 : 0);  // (one kernel argument: bit 0 the links, bit 1 the bucket table)
    le = auvp::for_obstacle_J<4>(O, [&](auto j) {
      constexpr int J = decltype(j)::value;
      return plan.draw_wave ? launch(auvp::prrt_pipe_kernel<J, 5>, in_lds) : launch(auvp::prrt_pipe_kernel<J, 4>, in_lds);
    });
    break;
  }
  case auvp::PRRT_ONE:
    le = auvp::for_obstacle_J<16>(O, [&](auto j) {
      constexpr int J = decltype(j)::value;
      return plan.lat ? launch(auvp::prrt_kernel<J, true>) : launch(auvp::prrt_kernel<J, false>);
    });
    break;
  }
  HIPCHK(h, le);
  if (sync) HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  h->last_grid = plan.grid; h->last_block = plan.block; h->last_lds = plan.lds;
  if (!sync) return AUVP_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  h->last_ms = ms;
  if (plan.pipe && h->pipe_failed()) {
    // some episode's pipeline gave up (AUVP_ERR_PIPELINE): those episodes go back to where this launch found them (record,
    // generator, bucket table; the tree is append-only) and are planned by the one-wavefront kernel -- the others, finished, are
    // not touched (redo_mask).  Option PIPE_FALLBACK = 0 leaves the status in the summaries instead.
    h->pipe_clear();
    if (h->opt_flag(OPT_PIPE_FALLBACK, true)) {
      HIPCHK(h, S.redo_count.reserve(sizeof(int32_t)));
      HIPCHK(h, hipMemsetAsync(S.redo_count.p, 0, sizeof(int32_t), h->stream));
      hipLaunchKernelGGL(auvp::prrt_undo_kernel, dim3((S.E + 63) / 64), dim3(64), 0, h->stream, S.P, S.B, S.E, S.snap_sum.as<auvp::PrrtSummary>(),
                         S.snap_rng.as<int32_t>(), S.snap_mt.as<uint32_t>(), S.redo_mask.as<uint8_t>(), S.redo_count.as<int32_t>());
      HIPCHK(h, hipGetLastError());
      int32_t n = 0;
      HIPCHK(h, hipMemcpyAsync(&n, S.redo_count.p, sizeof n, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      if (n > 0) {
        h->pipe_fallback_last += n;
        h->pipe_fallback_total += n;
        S.B.redo_mask = S.redo_mask.as<uint8_t>();
        const int rc = prrt_launch(h, S, step_mode, true, true);
        S.B.redo_mask = nullptr;
        h->last_ms += ms;  // (the time the caller waited)
        if (rc != AUVP_OK) return rc;
      }
    }
  }
  return AUVP_OK;
}

}  // namespace

extern "C" {

// parameters + buffers of a batch of E episodes (everything of auvp_prrt_create_batch that does not depend on where
// the starts, goals and generator states come from)
static int prrt_configure(auvp_handle* h, PrrtState& S, int32_t E, const auvp_prrt_params* p, int32_t flags) {
  if (!h->have_world) return fail(h, AUVP_ERR_STATE, "auvp_world_set not called (obstacle list)");
  if (!p) return fail(h, AUVP_ERR_ARG, "bad batch arguments");
  // the grid, every capacity and byte count of the batch, or why there is none (batch_plan.h)
  auvp::PrrtBatchIn in;
  in.E = E; in.p = *p; in.flags = flags; in.n_obstacles = h->W.n_obstacles;
  const auvp::PrrtBatchPlan plan = auvp::prrt_batch_plan(in);
  // (as ever: a batch that gets as far as its grid gives up the previous one, whatever comes of it)
  if (plan.status == auvp::PRRT_BATCH_OK || plan.status >= auvp::PRRT_BATCH_EMPTY_GRID) {
    S.ready = false;
    S.drop_graphs();  // they replay launches on the previous batch's buffers
  }
  switch (plan.status) {
    case auvp::PRRT_BATCH_OK: break;
    case auvp::PRRT_BATCH_BAD_ARGS: return fail(h, AUVP_ERR_ARG, "bad batch arguments");
    case auvp::PRRT_BATCH_OBSTACLES: return fail(h, AUVP_ERR_ARG, "n_obstacles %d > 1024", h->W.n_obstacles);
    case auvp::PRRT_BATCH_BAD_PARAMS: return fail(h, AUVP_ERR_ARG, "bad params");
    case auvp::PRRT_BATCH_FIELD: return fail(h, AUVP_ERR_ARG, "%s: not a number the batch can be sized from, or too large", plan.field);
    case auvp::PRRT_BATCH_EMPTY_GRID: return fail(h, AUVP_ERR_ARG, "empty grid");
    case auvp::PRRT_BATCH_BUCKETS: return fail(h, AUVP_ERR_ARG, "too many buckets");
    case auvp::PRRT_BATCH_POINTS: return fail(h, AUVP_ERR_ARG, "point capacity too large");
    case auvp::PRRT_BATCH_STEPS: return fail(h, AUVP_ERR_ARG, "max_step %d: a bucket's size is kept in 24 bits", p->max_step);
  }
  auvp::PrrtParamsDev& P = S.P;
  for (int i = 0; i < 4; i++) P.rect[i] = p->rect[i];
  P.exp_rate = p->exp_rate; P.dist_to_end = p->dist_to_end; P.diff_max = p->diff_max; P.freq = p->freq;
  P.cell = p->cell_side_length;
  P.S = p->subsections;
  P.rows = plan.rows; P.cols = plan.cols; P.n_buckets = plan.n_buckets;
  P.max_step = p->max_step; P.flags = flags; P.step_mode = 0;
  P.delta_theta = plan.delta_theta;
  auvp::PrrtBuffers& B = S.B;
  B.cap_nodes = plan.cap_nodes; B.max_pts = plan.max_pts; B.cap_points = plan.cap_points;
  const auvp::PrrtBatchBytes& bytes = plan.bytes;
  HIPCHK(h, S.nodes.reserve(bytes.nodes));
  HIPCHK(h, S.node_bucket.reserve(bytes.node_bucket));
  HIPCHK(h, S.points.reserve(bytes.points));
  HIPCHK(h, S.occupied.reserve(bytes.occupied));
  HIPCHK(h, S.buckets.reserve(S.bucket_bytes = bytes.buckets));
  HIPCHK(h, S.mt.reserve(bytes.mt));
  HIPCHK(h, S.rng_state.reserve(bytes.rng_state));
  HIPCHK(h, S.summary.reserve(bytes.summary));
  HIPCHK(h, S.step_bucket.reserve(bytes.step_bucket));
  HIPCHK(h, S.start.reserve(bytes.start));
  HIPCHK(h, S.goal.reserve(bytes.goal));
  B.nodes = S.nodes.as<auvp::PrrtNode>(); B.node_bucket = S.node_bucket.as<int32_t>();
  B.points = S.points.as<double>(); B.occupied = S.occupied.as<int32_t>(); B.buckets = S.buckets.as<int2>();
  B.mt = S.mt.as<uint32_t>(); B.rng_state = S.rng_state.as<int32_t>(); B.summary = S.summary.as<auvp::PrrtSummary>();
  B.step_bucket = S.step_bucket.as<int32_t>();
  B.start = S.start.as<double>(); B.goal = S.goal.as<double>();
  B.st_log = nullptr;
  B.env_flags = 0; B._pad_env = 0; B.env_done = nullptr; B.env_reward = nullptr; B.env_done_out = nullptr;
  B.env_bucket_out = nullptr; B.env_agent_seed = 0ull; B.env_err = nullptr;
  B.pipe_fail = h->pipe_fail_dev; B.redo_mask = nullptr;
  B.env_obs_grid = nullptr; B.env_obs_has = nullptr; B.env_obs_num = nullptr;
  if (flags & AUVP_FLAG_ITER_LOG) {
    HIPCHK(h, S.st_log.reserve(bytes.st_log));
    HIPCHK(h, hipMemsetAsync(S.st_log.p, 0xff, bytes.st_log, h->stream));
    B.st_log = S.st_log.as<int32_t>();
  }
  // four episodes per wavefront or one: decided here, once per batch (launch_plan.h)
  S.use_rows = auvp::prrt_choose_launch(prrt_launch_in(h, S, E, -1), h->opt).rows;
  return AUVP_OK;
}

// mps_list = [start]; add_node_to_grid(start)  (:53,:108-159): one thread per episode places the start node with the
// kernel's own add_node_to_grid arithmetic (starts / goals / generator states are already on the device)
static int prrt_plant(auvp_handle* h, PrrtState& S, int32_t E) {
  {
    // every bucket of the new batch is empty: a fresh epoch does that without touching the table (E x n_buckets x 8 bytes);
    // the table itself is cleared when its allocation changed or the 8-bit tag wraps (tag 0 is never current)
    const size_t need = S.bucket_bytes;
    const auvp::EpochTag next = auvp::epoch_tag_next((uint32_t)S.bucket_epoch, S.bucket_alloc != S.buckets.p || need > S.bucket_alloc_bytes);
    if (next.clear) {
      HIPCHK(h, hipMemsetAsync(S.buckets.p, 0, need, h->stream));
      S.bucket_alloc = S.buckets.p; S.bucket_alloc_bytes = need;
    }
    S.B.bucket_epoch = S.bucket_epoch = (int)next.tag;
  }
  HIPCHK(h, S.env_done.reserve((size_t)E));
  HIPCHK(h, S.env_err.reserve(2 * sizeof(int32_t)));
  S.thetas_ready = false;
  // (the planting launch also clears the device-resident loop's finished flags and error word: no fill launches)
  hipLaunchKernelGGL(auvp::prrt_init_kernel, dim3((E + 255) / 256), dim3(256), 0, h->stream, S.P, S.B, (int)E, S.env_done.as<uint8_t>(),
                     S.env_err.as<int32_t>());
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  S.E = E;
  S.ready = true;
  return AUVP_OK;
}

int auvp_prrt_create_batch(auvp_handle* h, int32_t E, const double* starts, const double* goals,
                           const auvp_prrt_params* p, const uint64_t* seeds, const uint32_t* mt, const int32_t* mt_index,
                           int32_t flags) {
  if (!h) return AUVP_ERR_ARG;
  if (E <= 0 || !starts || !goals || !p || (!seeds && !(mt && mt_index))) return fail(h, AUVP_ERR_ARG, "bad batch arguments");
  HIPCHK(h, hipSetDevice(h->device));
  PrrtState& S = *prrt_of(h);
  int rc;
  if ((rc = prrt_configure(h, S, E, p, flags))) return rc;
  if ((rc = upload(h, S.start, starts, (size_t)E * 4))) return rc;
  if ((rc = upload(h, S.goal, goals, (size_t)E * 2))) return rc;
  // generator states: random.seed(seeds[e]) on the device (init_by_array, 64 generators per workgroup), or the caller's own
  if (seeds) {
    HIPCHK(h, S.seeds.reserve((size_t)E * sizeof(uint64_t)));
    HIPCHK(h, hipMemcpyAsync(S.seeds.p, seeds, (size_t)E * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(auvp::mt_seed_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  auvp::MT_SEED_LDS));
    hipLaunchKernelGGL(auvp::mt_seed_kernel, dim3((E + 63) / 64), dim3(64), auvp::MT_SEED_LDS, h->stream,
                       S.seeds.as<unsigned long long>(), S.B.mt, S.B.rng_state, (int)E);
    HIPCHK(h, hipGetLastError());
  } else {
    const std::vector<uint32_t> words(mt, mt + (size_t)E * 624);
    const std::vector<int32_t> rs = auvp::prrt_rng_state_rows(mt_index, E);
    if ((rc = upload(h, S.mt, words.data(), words.size()))) return rc;
    if ((rc = upload(h, S.rng_state, rs.data(), rs.size()))) return rc;
  }
  return prrt_plant(h, S, E);
}

int auvp_prrt_plan(auvp_handle* h) {
  if (!h) return AUVP_ERR_ARG;
  PrrtState& S = *prrt_of(h);
  if (!S.ready) return fail(h, AUVP_ERR_STATE, "auvp_prrt_create_batch not called");
  HIPCHK(h, hipSetDevice(h->device));
  return prrt_launch(h, S, 0);
}

int auvp_prrt_step(auvp_handle* h, const int32_t* bucket_ids, const uint32_t* mt, const int32_t* mt_index) {
  if (!h || !bucket_ids) return AUVP_ERR_ARG;
  PrrtState& S = *prrt_of(h);
  if (!S.ready) return fail(h, AUVP_ERR_STATE, "auvp_prrt_create_batch not called");
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  if ((rc = upload(h, S.step_bucket, bucket_ids, (size_t)S.E))) return rc;
  if (mt && mt_index) {  // continue an external generator (the global `random` state) for this step
    const std::vector<int32_t> rs = auvp::prrt_rng_state_rows(mt_index, S.E);
    if ((rc = upload(h, S.mt, mt, (size_t)S.E * 624))) return rc;
    if ((rc = upload(h, S.rng_state, rs.data(), rs.size()))) return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return prrt_launch(h, S, 1);
}

int auvp_prrt_summaries(auvp_handle* h, auvp_prrt_summary* out) {
  if (!h || !out) return AUVP_ERR_ARG;
  PrrtState& S = *prrt_of(h);
  if (!S.ready) return fail(h, AUVP_ERR_STATE, "no planner batch");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpy(out, S.B.summary, (size_t)S.E * sizeof(auvp::PrrtSummary), hipMemcpyDeviceToHost));
  return AUVP_OK;
}

int auvp_prrt_goals(auvp_handle* h, double* goals2) {
  if (!h || !goals2) return AUVP_ERR_ARG;
  PrrtState& S = *prrt_of(h);
  if (!S.ready) return fail(h, AUVP_ERR_STATE, "no planner batch");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpy(goals2, S.B.goal, (size_t)S.E * 2 * sizeof(double), hipMemcpyDeviceToHost));
  return AUVP_OK;
}

int auvp_prrt_paths(auvp_handle* h, const int64_t* offsets, double* out) {
  if (!h || !offsets || !out) return AUVP_ERR_ARG;
  PrrtState& S = *prrt_of(h);
  if (!S.ready) return fail(h, AUVP_ERR_STATE, "no planner batch");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t total = (size_t)offsets[S.E];
  int rc;
  if ((rc = upload(h, S.tmp_off, offsets, (size_t)S.E + 1))) return rc;
  HIPCHK(h, S.tmp_out.reserve(std::max<size_t>(total, 1) * 5 * sizeof(double)));
  hipLaunchKernelGGL(auvp::prrt_final_course_kernel, dim3(S.E), dim3(64), 0, h->stream, S.B, S.tmp_off.as<int64_t>(),
                     S.tmp_out.as<double>(), S.E);
  HIPCHK(h, hipGetLastError());
  if (total) HIPCHK(h, hipMemcpyAsync(out, S.tmp_out.p, total * 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return AUVP_OK;
}

int auvp_prrt_tree(auvp_handle* h, int32_t ep, double* nodes4, int32_t* node_i4, int32_t* node_bucket, double* points4) {
  if (!h) return AUVP_ERR_ARG;
  PrrtState& S = *prrt_of(h);
  if (!S.ready || ep < 0 || ep >= S.E) return fail(h, AUVP_ERR_STATE, "bad episode");
  HIPCHK(h, hipSetDevice(h->device));
  auvp::PrrtSummary s;
  HIPCHK(h, hipMemcpy(&s, S.B.summary + ep, sizeof s, hipMemcpyDeviceToHost));
  const size_t N = (size_t)s.n_nodes, NP = (size_t)s.n_points, capp = (size_t)S.B.cap_points;
  if (nodes4 || node_i4 || node_bucket) {
    std::vector<auvp::PrrtNode> rec(N);
    HIPCHK(h, hipMemcpy(rec.data(), S.B.nodes + (size_t)ep * S.B.cap_nodes, N * sizeof(auvp::PrrtNode), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; i++) {
      const auvp::PrrtNode& r = rec[i];
      if (nodes4) { nodes4[4 * i] = r.x; nodes4[4 * i + 1] = r.y; nodes4[4 * i + 2] = r.theta; nodes4[4 * i + 3] = r.t; }
      if (node_i4) { node_i4[4 * i] = r.step; node_i4[4 * i + 1] = r.parent; node_i4[4 * i + 2] = r.pt_off; node_i4[4 * i + 3] = r.pt_cnt; }
      if (node_bucket) node_bucket[i] = r.bucket;
    }
  }
  if (points4 && NP) HIPCHK(h, hipMemcpy(points4, S.B.points + (size_t)ep * capp * 4, NP * 4 * sizeof(double), hipMemcpyDeviceToHost));
  return AUVP_OK;
}

// one node of one episode: its record and its run of path points (what a step-mode caller needs to materialise the
// node the device just accepted, instead of downloading the whole tree every step)
int auvp_prrt_node(auvp_handle* h, int32_t ep, int32_t node, double* node4, int32_t* node_i4, int32_t* node_bucket,
                   double* points4, int32_t cap_points) {
  if (!h) return AUVP_ERR_ARG;
  PrrtState& S = *prrt_of(h);
  if (!S.ready || ep < 0 || ep >= S.E) return fail(h, AUVP_ERR_STATE, "bad episode");
  if (node < 0 || node >= S.B.cap_nodes) return fail(h, AUVP_ERR_ARG, "node %d outside 0..%d", node, S.B.cap_nodes - 1);
  HIPCHK(h, hipSetDevice(h->device));
  const size_t at = (size_t)ep * S.B.cap_nodes + (size_t)node, capp = (size_t)S.B.cap_points;
  auvp::PrrtNode r;
  HIPCHK(h, hipMemcpy(&r, S.B.nodes + at, sizeof r, hipMemcpyDeviceToHost));
  if (node4) { node4[0] = r.x; node4[1] = r.y; node4[2] = r.theta; node4[3] = r.t; }
  if (node_i4) { node_i4[0] = r.step; node_i4[1] = r.parent; node_i4[2] = r.pt_off; node_i4[3] = r.pt_cnt; }
  if (node_bucket) *node_bucket = r.bucket;
  const int off = r.pt_off, cnt = r.pt_cnt;
  if (points4 && cnt > 0) {
    if (cnt > cap_points) return fail(h, AUVP_ERR_CAPACITY, "node has %d points, buffer holds %d", cnt, cap_points);
    if (off < 0 || (size_t)off + (size_t)cnt > capp) return fail(h, AUVP_ERR_STATE, "node record out of range");
    HIPCHK(h, hipMemcpy(points4, S.B.points + ((size_t)ep * capp + (size_t)off) * 4, (size_t)cnt * 4 * sizeof(double), hipMemcpyDeviceToHost));
  }
  return AUVP_OK;
}

int auvp_prrt_grid(auvp_handle* h, int32_t ep, int32_t* occupied, int32_t* bucket_counts, int32_t* dims4) {
  if (!h) return AUVP_ERR_ARG;
  PrrtState& S = *prrt_of(h);
  if (!S.ready || ep < 0 || ep >= S.E) return fail(h, AUVP_ERR_STATE, "bad episode");
  HIPCHK(h, hipSetDevice(h->device));
  auvp::PrrtSummary s;
  HIPCHK(h, hipMemcpy(&s, S.B.summary + ep, sizeof s, hipMemcpyDeviceToHost));
  if (dims4) { dims4[0] = S.P.rows; dims4[1] = S.P.cols; dims4[2] = S.P.S; dims4[3] = s.n_occ; }
  if (occupied && s.n_occ) HIPCHK(h, hipMemcpy(occupied, S.B.occupied + (size_t)ep * S.B.cap_nodes, (size_t)s.n_occ * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (bucket_counts) {
    std::vector<int2> tab((size_t)S.P.n_buckets);
    HIPCHK(h, hipMemcpy(tab.data(), S.B.buckets + (size_t)ep * S.P.n_buckets, tab.size() * sizeof(int2), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < tab.size(); i++)
      bucket_counts[i] = (int32_t)((uint32_t)tab[i].x >> 24) == S.B.bucket_epoch ? (tab[i].x & 0xffffff) : 0;
  }
  return AUVP_OK;
}

int auvp_prrt_step_log(auvp_handle* h, int32_t ep, int32_t* log8) {
  if (!h || !log8) return AUVP_ERR_ARG;
  PrrtState& S = *prrt_of(h);
  if (!S.ready || ep < 0 || ep >= S.E || !S.B.st_log) return fail(h, AUVP_ERR_STATE, "no step log");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpy(log8, S.B.st_log + (size_t)ep * S.P.max_step * 8, (size_t)S.P.max_step * 8 * sizeof(int32_t), hipMemcpyDeviceToHost));
  return AUVP_OK;
}

const char* auvp_prrt_last_kernel(auvp_handle* h) {
  if (!h) return "";
  return prrt_of(h)->last_kernel;
}

void* auvp_prrt_summaries_dev(auvp_handle* h) {
  if (!h) return nullptr;
  PrrtState& S = *prrt_of(h);
  return S.ready ? (void*)S.B.summary : nullptr;
}

// RRTEnv observation arrays (gym_rrt/envs/rrt_env.py:250-295) for every episode, written to
// caller-owned DEVICE buffers: rrt_grid [E,n_buckets,4] f64 = cell.x, cell.y, subsection.theta,
// len(node_array); has_node [E,n_buckets] i64; num_nodes [E,n_buckets] i64.
static int prrt_observation_enqueue(auvp_handle* h, PrrtState& S, void* rrt_grid_dev, void* has_node_dev, void* num_nodes_dev) {
  if (!S.thetas_ready) {
    // subsection thetas exactly as Grid_cell_RRT builds them (grid_cell_rrt.py:49-55); once per batch
    std::vector<double> th(S.P.S);
    const double pi = M_PI;
    double theta = 0.0;
    for (int i = 0; i < S.P.S; i++) {
      th[i] = theta;
      theta = theta + S.P.delta_theta;
      while (!(-pi <= theta && theta <= pi)) theta += theta > pi ? (-2 * pi) : (2 * pi);
    }
    int rc;
    if ((rc = upload(h, S.thetas, th.data(), th.size()))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));  // `th` goes out of scope
    S.thetas_ready = true;
  }
  const long long total = (long long)S.E * S.P.n_buckets;
  const int grid = (int)std::min<long long>((total + 255) / 256, 65535LL * 16);
  hipLaunchKernelGGL(auvp::prrt_observation_kernel, dim3(grid), dim3(256), 0, h->stream, S.P, S.B, S.thetas.as<double>(), S.E,
                     reinterpret_cast<double*>(rrt_grid_dev), reinterpret_cast<long long*>(has_node_dev),
                     reinterpret_cast<long long*>(num_nodes_dev));
  HIPCHK(h, hipGetLastError());
  return AUVP_OK;
}

int auvp_prrt_observation_dev(auvp_handle* h, void* rrt_grid_dev, void* has_node_dev, void* num_nodes_dev) {
  if (!h || !rrt_grid_dev) return AUVP_ERR_ARG;
  PrrtState& S = *prrt_of(h);
  if (!S.ready) return fail(h, AUVP_ERR_STATE, "no planner batch");
  HIPCHK(h, hipSetDevice(h->device));
  int rc = prrt_observation_enqueue(h, S, rrt_grid_dev, has_node_dev, num_nodes_dev);
  if (rc != AUVP_OK) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return AUVP_OK;
}

// ---- the device-resident RRTEnv loop: every call below only ENQUEUES on the handle's stream (auvp_stream_sync waits) ----
// One environment step = generate_one_node for every live environment, with the step's outcome (reward, done flag) written
// by the same launch and -- AUVP_ENV_AGENT -- the stand-in agent's pick made inside it.  The observation arrays are either
// rewritten whole by a second launch (E x n_buckets entries, what the reference env rebuilds after every node) or --
// AUVP_ENV_OBS_DELTA -- updated in place by the planner launch itself: a step changes ONE bucket per environment.  (Batches
// the four-episodes-per-wavefront kernel serves keep the agent and the outcome as small launches of their own and always
// rewrite the observation.)
static int prrt_env_step_enqueue(auvp_handle* h, PrrtState& S, int32_t flags, uint64_t agent_seed, int32_t* bucket_ids_dev,
                                 void* rrt_grid_dev, void* has_node_dev, void* num_nodes_dev, int64_t* reward_dev, uint8_t* done_dev) {
  const bool agent = (flags & AUVP_ENV_AGENT) != 0;
  const bool delta = (flags & AUVP_ENV_OBS_DELTA) != 0 && rrt_grid_dev != nullptr;
  auvp::PrrtBuffers& B = S.B;
  B.env_done = S.env_done.as<uint8_t>(); B.env_reward = reinterpret_cast<long long*>(reward_dev); B.env_done_out = done_dev;
  B.env_bucket_out = bucket_ids_dev; B.env_agent_seed = agent_seed; B.env_err = S.env_err.as<int32_t>();
  B.env_obs_grid = reinterpret_cast<double*>(rrt_grid_dev); B.env_obs_has = reinterpret_cast<long long*>(has_node_dev);
  B.env_obs_num = reinterpret_cast<long long*>(num_nodes_dev);
  const int32_t* own = B.step_bucket;
  B.step_bucket = bucket_ids_dev;
  int rc;
  bool full_obs = rrt_grid_dev != nullptr && !delta;
  if (!S.use_rows) {
    B.env_flags = PRRT_ENV_OUTCOME | (agent ? PRRT_ENV_AGENT : 0) | (delta ? PRRT_ENV_DELTA : 0);
    rc = prrt_launch(h, S, 1, false);
  } else {
    B.env_flags = 0;
    full_obs = rrt_grid_dev != nullptr;
    if (agent) {
      hipLaunchKernelGGL(auvp::prrt_policy_random_kernel, dim3((S.E + 255) / 256), dim3(256), 0, h->stream, B, S.E,
                         (unsigned long long)agent_seed, bucket_ids_dev);
      HIPCHK(h, hipGetLastError());
    }
    rc = prrt_launch(h, S, 1, false);
    if (rc == AUVP_OK) {
      hipLaunchKernelGGL(auvp::prrt_env_outcome_kernel, dim3((S.E + 255) / 256), dim3(256), 0, h->stream, B, S.E, bucket_ids_dev);
      rc = hipGetLastError() == hipSuccess ? AUVP_OK : fail(h, AUVP_ERR_HIP, "prrt_env_outcome_kernel launch");
    }
  }
  B.step_bucket = own;
  B.env_flags = 0;
  if (rc != AUVP_OK) return rc;
  if (full_obs) return prrt_observation_enqueue(h, S, rrt_grid_dev, has_node_dev, num_nodes_dev);
  return AUVP_OK;
}

int auvp_prrt_env_step_dev(auvp_handle* h, const int32_t* bucket_ids_dev, void* rrt_grid_dev, void* has_node_dev, void* num_nodes_dev,
                           int64_t* reward_dev, uint8_t* done_dev) {
  return auvp_prrt_env_step_ex_dev(h, 0, 0, const_cast<int32_t*>(bucket_ids_dev), rrt_grid_dev, has_node_dev, num_nodes_dev, reward_dev, done_dev);
}

int auvp_prrt_env_step_ex_dev(auvp_handle* h, int32_t flags, uint64_t agent_seed, int32_t* bucket_ids_dev, void* rrt_grid_dev,
                              void* has_node_dev, void* num_nodes_dev, int64_t* reward_dev, uint8_t* done_dev) {
  if (!h || !bucket_ids_dev || !reward_dev || (flags & ~(AUVP_ENV_AGENT | AUVP_ENV_OBS_DELTA))) return AUVP_ERR_ARG;
  PrrtState& S = *prrt_of(h);
  if (!S.ready) return fail(h, AUVP_ERR_STATE, "auvp_prrt_create_batch not called");
  HIPCHK(h, hipSetDevice(h->device));
  return prrt_env_step_enqueue(h, S, flags, agent_seed, bucket_ids_dev, rrt_grid_dev, has_node_dev, num_nodes_dev, reward_dev, done_dev);
}

int auvp_prrt_policy_random_dev(auvp_handle* h, const int64_t* has_node_dev, uint64_t seed, int32_t* bucket_ids_dev) {
  (void)has_node_dev;  // the agent reads the planner's own list of occupied buckets: the set has_node marks, without the scan
  if (!h || !bucket_ids_dev) return AUVP_ERR_ARG;
  PrrtState& S = *prrt_of(h);
  if (!S.ready) return fail(h, AUVP_ERR_STATE, "no planner batch");
  HIPCHK(h, hipSetDevice(h->device));
  auvp::PrrtBuffers B = S.B;
  B.env_done = S.env_done.as<uint8_t>();
  hipLaunchKernelGGL(auvp::prrt_policy_random_kernel, dim3((S.E + 255) / 256), dim3(256), 0, h->stream, B, S.E, (unsigned long long)seed,
                     bucket_ids_dev);
  HIPCHK(h, hipGetLastError());
  return AUVP_OK;
}

// {status, environment} of the first episode that failed on the device inside the device-resident loop (0: none).  Waits
// for the stream.  The host loop (auvp_prrt_step + summaries) surfaces the same failures as summary.status < 0.
int auvp_prrt_env_check(auvp_handle* h, int32_t* status, int32_t* env) {
  if (!h || !status) return AUVP_ERR_ARG;
  PrrtState& S = *prrt_of(h);
  if (!S.ready) return fail(h, AUVP_ERR_STATE, "no planner batch");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int32_t e2[2] = {0, 0};
  HIPCHK(h, hipMemcpy(e2, S.env_err.p, sizeof e2, hipMemcpyDeviceToHost));
  *status = e2[0];
  if (env) *env = e2[1];
  return AUVP_OK;
}

int auvp_stream_sync(auvp_handle* h) {
  if (!h) return AUVP_ERR_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return AUVP_OK;
}

void* auvp_stream(auvp_handle* h) { return h ? (void*)h->stream : nullptr; }

// HIP-event time of a region of the handle's stream the CALLER brackets (enqueue-only loops: auvp_prrt_env_step_dev,
// auvp_graph_launch): auvp_stream_mark(h, 0) before, auvp_stream_mark(h, 1) after, auvp_stream_elapsed_ms waits and reads.
int auvp_stream_mark(auvp_handle* h, int32_t which) {
  if (!h || (which != 0 && which != 1)) return AUVP_ERR_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipEventRecord(which ? h->ev1 : h->ev0, h->stream));
  return AUVP_OK;
}

int auvp_stream_elapsed_ms(auvp_handle* h, double* ms) {
  if (!h || !ms) return AUVP_ERR_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipEventSynchronize(h->ev1));
  float f = 0.f;
  HIPCHK(h, hipEventElapsedTime(&f, h->ev0, h->ev1));
  *ms = f;
  return AUVP_OK;
}

// ---- hipGraph capture of a launch-bound inner loop on the handle's stream ------------------------------------------------
// Between auvp_graph_begin and auvp_graph_end every enqueue-only entry point (auvp_prrt_policy_random_dev,
// auvp_prrt_env_step_dev, a caller's own kernels on auvp_stream) is recorded instead of run; auvp_graph_launch replays the
// recorded step n times back to back.  Call the entry points once un-captured first (they allocate and upload on first use).
int auvp_graph_begin(auvp_handle* h) {
  if (!h) return AUVP_ERR_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
  return AUVP_OK;
}

int auvp_graph_end(auvp_handle* h, int32_t* graph_id) {
  if (!h || !graph_id) return AUVP_ERR_ARG;
  PrrtState& S = *prrt_of(h);
  hipGraph_t g = nullptr;
  HIPCHK(h, hipStreamEndCapture(h->stream, &g));
  hipGraphExec_t ge = nullptr;
  hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) return fail(h, AUVP_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
  S.graphs.push_back(ge);
  *graph_id = (int32_t)S.graphs.size() - 1;
  return AUVP_OK;
}

int auvp_graph_launch(auvp_handle* h, int32_t graph_id, int32_t n_times) {
  if (!h || n_times < 0) return AUVP_ERR_ARG;
  PrrtState& S = *prrt_of(h);
  if (graph_id < 0 || graph_id >= (int32_t)S.graphs.size()) return fail(h, AUVP_ERR_ARG, "no such graph");
  if (!S.graphs[graph_id]) return fail(h, AUVP_ERR_STATE, "graph %d was captured for an earlier batch (a new batch invalidates its graphs)", graph_id);
  HIPCHK(h, hipSetDevice(h->device));
  for (int i = 0; i < n_times; i++) HIPCHK(h, hipGraphLaunch(S.graphs[graph_id], h->stream));
  return AUVP_OK;
}

// the same for one episode, copied to host arrays
int auvp_prrt_observation(auvp_handle* h, int32_t ep, double* rrt_grid, int64_t* has_node, int64_t* num_nodes) {
  if (!h || !rrt_grid) return AUVP_ERR_ARG;
  PrrtState& S = *prrt_of(h);
  if (!S.ready || ep < 0 || ep >= S.E) return fail(h, AUVP_ERR_STATE, "bad episode");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t nb = (size_t)S.P.n_buckets, tot = (size_t)S.E * nb;
  DevBuf g, hn, nn;
  HIPCHK(h, g.reserve(tot * 4 * sizeof(double)));
  HIPCHK(h, hn.reserve(tot * sizeof(int64_t)));
  HIPCHK(h, nn.reserve(tot * sizeof(int64_t)));
  int rc = auvp_prrt_observation_dev(h, g.p, hn.p, nn.p);
  if (rc != AUVP_OK) return rc;
  HIPCHK(h, hipMemcpy(rrt_grid, g.as<double>() + (size_t)ep * nb * 4, nb * 4 * sizeof(double), hipMemcpyDeviceToHost));
  if (has_node) HIPCHK(h, hipMemcpy(has_node, hn.as<int64_t>() + (size_t)ep * nb, nb * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (num_nodes) HIPCHK(h, hipMemcpy(num_nodes, nn.as<int64_t>() + (size_t)ep * nb, nb * sizeof(int64_t), hipMemcpyDeviceToHost));
  return AUVP_OK;
}

}  // extern "C"
#endif

// astar_host.h -- C-ABI entry points for the A* variants (auvp_astar_*), host side.
// Included at the end of auvplan.hip (same translation unit: uses auvp_handle, fail, HIPCHK, upload; sq_threshold is world_tables.h's).
#ifndef AUVP_ASTAR_HOST_H
#define AUVP_ASTAR_HOST_H
#include "astar_tables.h"

// astar_sets_kernels.hip (a translation unit of its own, so that this unit's astar_kernel<3> forms keep their code): the top-n
// tables of the probability sets, and the variant-3 search with a table per instance
extern "C" hipError_t auvpi_astar_topn_sets_launch(const double* prob, double* topn, int rows, int C, hipStream_t stream);
extern "C" hipError_t auvpi_astar_sets_launch(const auvp::AstarWorldDev* W, const auvp::AstarParamsDev* P, const auvp::AstarBuffers* B, int n_inst,
                                              const double* sets_prob, const double* sets_topn, const int32_t* set_of, int pair, int grid,
                                              hipStream_t stream);

static_assert(sizeof(auvp_astar_summary) == sizeof(auvp::AstarSummary), "astar summary layout");

namespace {

struct AstarState {
  bool ready = false;
  unsigned world_version = ~0u;
  int E = 0;
  auvp::AstarWorldDev W{};
  auvp::AstarParamsDev P{};
  auvp::AstarBuffers B{};
  DevBuf ox, oy, ot, hab, poly, bins, rcells, prob, topn, gridtab;
  DevBuf start, goal, limit, nodes, node_i, cellinfo, hab_left, exp_log, summary, off, path, cost, npath, smooth;
  long long visited_set_for = -1;  // entry count of a bitmap uploaded by auvp_astar_set_visited, -1 none
  // epoch of the words in `cellinfo` (astar_kernel.h): bumped per batch instead of clearing 1.4 MB per instance;
  // cellinfo_clean_cap = capacity (bytes) that has been zeroed since the buffer was (re)allocated
  uint32_t epoch = 0;
  size_t cellinfo_clean_cap = 0;
  // auvp_astar_batch_sets: top-n tables [G][T][C+1] of the handle's probability sets, built on the first batch (or read-back) that
  // asks for them and kept while sets_version is the handle's; sets_nan[g]: set g holds a nan and has no table; the batch's set_of
  DevBuf sets_topn, set_of;
  unsigned sets_version = ~0u;
  std::vector<char> sets_nan;
};

AstarState* astar_of(auvp_handle* h) {
  if (!h->astar) {
    h->astar = new AstarState();
    h->astar_free = [](void* p) { delete static_cast<AstarState*>(p); };
  }
  return static_cast<AstarState*>(h->astar);
}

// the visited words' next epoch (epoch_tag_next, batch_plan.h), clearing them where the rule says so
int astar_next_epoch(auvp_handle* h, AstarState& S, bool new_buffer) {
  const auvp::EpochTag next = auvp::epoch_tag_next(S.epoch, new_buffer);
  if (next.clear) {
    HIPCHK(h, hipMemsetAsync(S.cellinfo.p, 0, S.cellinfo.cap, h->stream));
    S.cellinfo_clean_cap = S.cellinfo.cap;
  }
  S.epoch = next.tag;
  return AUVP_OK;
}

int astar_build_world(auvp_handle* h, AstarState& S) {
  const int O = (int)(h->w_obst.size() / 3), H = (int)(h->w_hab.size() / 3), V = (int)(h->w_poly.size() / 2);
  const int T = (int)(h->w_bins.size() / 2), C = (int)(h->w_cells.size() / 4);
  if (H > auvp::ASTAR_MAX_HAB) return fail(h, AUVP_ERR_ARG, "n_habitats %d > %d", H, auvp::ASTAR_MAX_HAB);
  const auvp::AstarWorldTables t = auvp::build_astar_world_tables(h->w_obst.data(), O, h->w_hab.data(), H, h->w_poly.data(), V, T, h->w_cells.data(), C,
                                                                  h->w_prob.data(), h->opt_on(OPT_ASTAR_NO_GRID));
  // (no grid: no table, and the buffer is not touched)
  int rc = upload_tables(h, {{S.gridtab, t.gtab}, {S.ox, t.ox}, {S.oy, t.oy}, {S.ot, t.ot}, {S.hab, t.hab}, {S.poly, h->w_poly}, {S.bins, h->w_bins},
                             {S.rcells, t.rc}, {S.prob, h->w_prob}, {S.topn, t.topn}});
  if (rc != AUVP_OK) return rc;
  auvp::AstarWorldDev& W = S.W;
  W.n_obstacles = O; W.n_habitats = H; W.n_poly = V; W.n_bins = T; W.n_cells = C;
  W.ox = S.ox.as<double>(); W.oy = S.oy.as<double>(); W.ot = S.ot.as<double>(); W.hab = S.hab.as<double>();
  W.poly = S.poly.as<double>(); W.bins = S.bins.as<double>(); W.rcells = S.rcells.as<double>();
  W.prob = S.prob.as<double>(); W.topn = S.topn.as<double>();
  W.g_ncol = t.g_ncol; W.g_nrow = t.g_nrow;
  W.gx0 = W.gx1 = W.gy0 = W.gy1 = nullptr;
  if (t.g_ncol > 0) { W.gx0 = S.gridtab.as<double>(); W.gx1 = W.gx0 + t.g_ncol; W.gy0 = W.gx1 + t.g_ncol; W.gy1 = W.gy0 + t.g_nrow; }
  W.g_x1_0 = t.g_x1_0; W.g_y1_0 = t.g_y1_0; W.g_inv_dx = t.g_inv_dx; W.g_inv_dy = t.g_inv_dy;
  W.cx = t.cx; W.cy = t.cy;
  S.world_version = h->world_version;
  return AUVP_OK;
}

// The top-n tables of the handle's probability sets (h->d_sets_prob [G][T][C], in place): astar_topn_sets_kernel for rows that
// fit its LDS, astar_topn_rows on a read-back for longer ones.  A set that holds a nan (its record's absmax, written by
// prob_set_stats_kernel, is a nan) gets no defined table; astar_batch_run refuses the instances that name it.  h->last_ms: the
// time of the device route's launch (0 on the host route).
int astar_build_set_tables(auvp_handle* h, AstarState& S) {
  const int G = h->n_sets, T = h->W.n_bins, C = h->W.n_cells;
  const size_t rows = (size_t)G * T, n_in = rows * C, n_out = rows * ((size_t)C + 1);
  S.sets_version = ~0u;
  std::vector<auvp::RrtProbSetDev> rec((size_t)G);
  HIPCHK(h, hipMemcpyAsync(rec.data(), h->d_sets_rec.p, rec.size() * sizeof(auvp::RrtProbSetDev), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  S.sets_nan.assign((size_t)G, 0);
  for (int g = 0; g < G; g++) S.sets_nan[(size_t)g] = rec[(size_t)g].absmax != rec[(size_t)g].absmax ? 1 : 0;
  HIPCHK(h, S.sets_topn.reserve(n_out * sizeof(double)));
  h->last_ms = 0.0;
  if (C <= auvp::ASTAR_TOPN_DEV_MAX_C) {
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    HIPCHK(h, auvpi_astar_topn_sets_launch(h->d_sets_prob.as<double>(), S.sets_topn.as<double>(), (int)rows, C, h->stream));
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->last_ms = ms;
  } else {
    std::vector<double> prob(n_in), topn(n_out, 0.0);
    HIPCHK(h, hipMemcpyAsync(prob.data(), h->d_sets_prob.p, n_in * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int g = 0; g < G; g++)  // (std::sort on a row with a nan is not defined: such a set's table stays zero)
      if (!S.sets_nan[(size_t)g])
        auvp::astar_topn_rows(prob.data() + (size_t)g * T * C, (size_t)T, (size_t)C, topn.data() + (size_t)g * T * ((size_t)C + 1));
    HIPCHK(h, hipMemcpyAsync(S.sets_topn.p, topn.data(), n_out * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  S.sets_version = h->sets_version;
  return AUVP_OK;
}

// auvp_astar_batch (set_of null) and auvp_astar_batch_sets: one host function, so that epochs, visited words, the PAIR choice and
// the redo are the same text for both
int astar_batch_run(auvp_handle* h, int32_t E, const double* starts, const double* goals, const double* limits,
                    const auvp_astar_params* p, int32_t flags, const int32_t* set_of) {
  if (!h) return AUVP_ERR_ARG;
  if (!h->have_world) return fail(h, AUVP_ERR_STATE, "auvp_world_set not called");
  if (E <= 0 || !starts || !p || p->variant < 0 || p->variant > 3) return fail(h, AUVP_ERR_ARG, "bad arguments");
  if (p->variant <= 1 && !goals) return fail(h, AUVP_ERR_ARG, "goals required for astar / astar_real");
  if (p->variant >= 2 && !limits) return fail(h, AUVP_ERR_ARG, "pathLenLimit required for the fixLen variants");
  if (p->variant >= 1 && h->w_poly.size() < 6) return fail(h, AUVP_ERR_ARG, "boundary polygon needs >= 3 vertices");
  if (p->cap_nodes < 16) return fail(h, AUVP_ERR_ARG, "cap_nodes too small");
  const bool sets = set_of != nullptr;
  if (sets) {
    if (p->variant != 3) return fail(h, AUVP_ERR_ARG, "a table per instance is astar_fixLenSOG's (variant 3), not variant %d", p->variant);
    if (h->n_sets < 1) return fail(h, AUVP_ERR_STATE, "no probability sets on this handle (auvp_world_set_prob_sets)");
    for (int e = 0; e < E; e++)
      if (set_of[e] < 0 || set_of[e] >= h->n_sets) return fail(h, AUVP_ERR_ARG, "instance %d: set %d outside [0, %d)", e, set_of[e], h->n_sets);
  }
  HIPCHK(h, hipSetDevice(h->device));
  AstarState& S = *astar_of(h);
  S.ready = false;
  int rc;
  if (S.world_version != h->world_version && (rc = astar_build_world(h, S))) return rc;
  if (sets) {
    if (S.sets_version != h->sets_version && (rc = astar_build_set_tables(h, S))) return rc;
    for (int e = 0; e < E; e++)
      if (S.sets_nan[(size_t)set_of[e]])
        return fail(h, AUVP_ERR_ARG, "probability set %d holds a nan: it has no top-n table (instance %d)", set_of[e], e);
    if ((rc = upload(h, S.set_of, set_of, (size_t)E))) return rc;
  }
  auvp::AstarParamsDev& P = S.P;
  P.variant = p->variant; P.cap_nodes = p->cap_nodes; P.flags = flags;
  if (h->opt_on(OPT_ASTAR_NO_LIST)) P.flags |= AUVP_KFLAG_ASTAR_NO_LIST;
  P.cap_exp = (flags & AUVP_FLAG_ITER_LOG) ? p->cap_nodes : 0;
  for (int i = 0; i < 4; i++) { P.box[i] = p->box[i]; P.w[i] = p->w[i]; }
  P.velocity = p->velocity;
  P.vx = p->variant == 2 ? 550 : 600;  // np.zeros([550, 600]) (astar_fixLen.py:51) / [600, 600] (astar_fixLenSOG.py:117)
  P.vy = 600;
  auvp::AstarBuffers& B = S.B;
  if ((rc = upload(h, S.start, starts, (size_t)E * 2))) return rc;
  B.start = S.start.as<double>();
  B.goal = nullptr; B.limit = nullptr;
  if (p->variant <= 1) { if ((rc = upload(h, S.goal, goals, (size_t)E * 2))) return rc; B.goal = S.goal.as<double>(); }
  else { if ((rc = upload(h, S.limit, limits, (size_t)E))) return rc; B.limit = S.limit.as<double>(); }
  const size_t cn = (size_t)E * p->cap_nodes;
  HIPCHK(h, S.nodes.reserve(cn * 9 * sizeof(double)));
  HIPCHK(h, S.node_i.reserve(cn * sizeof(int32_t)));
  HIPCHK(h, S.summary.reserve((size_t)E * sizeof(auvp::AstarSummary)));
  const int H = S.W.n_habitats;
  HIPCHK(h, S.hab_left.reserve((size_t)E * (H > 0 ? H : 1) * sizeof(int32_t)));
  B.nodes = S.nodes.as<double>(); B.node_i = S.node_i.as<int32_t>(); B.summary = S.summary.as<auvp::AstarSummary>();
  B.hab_left = S.hab_left.as<int32_t>();
  B.cellinfo = nullptr;
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));  // the batch time includes whatever reset the batch needs
  if (p->variant >= 2) {
    if (p->variant == 3 && S.W.n_cells >= 65535) return fail(h, AUVP_ERR_ARG, "n_cells %d does not fit the 16-bit cell-key field", S.W.n_cells);
    const size_t entries = (size_t)E * P.vx * P.vy, vb = entries * sizeof(uint32_t);
    HIPCHK(h, S.cellinfo.reserve(vb));
    if (flags & AUVP_FLAG_KEEP_VISITED) {
      // the reference keeps self.visited_nodes across astar() calls on one solver object
      // (astar_fixLen.py:51, astar_fixLenSOG.py:117): the caller uploaded it with auvp_astar_set_visited,
      // tagged with the current epoch
      if (S.visited_set_for != (long long)entries) return fail(h, AUVP_ERR_STATE, "auvp_astar_set_visited not called for this batch shape");
    } else {
      // a fresh visited array = a new epoch; the words are only cleared when the buffer is new or the tag wraps
      if ((rc = astar_next_epoch(h, S, S.cellinfo_clean_cap != S.cellinfo.cap))) return rc;
    }
    S.visited_set_for = -1;
    P.epoch = S.epoch;
    B.cellinfo = S.cellinfo.as<uint32_t>();
  }
  B.exp_log = nullptr;
  if (P.cap_exp) {
    HIPCHK(h, S.exp_log.reserve((size_t)E * P.cap_exp * 8 * sizeof(double)));
    B.exp_log = S.exp_log.as<double>();
  }
  B.pipe_fail = h->pipe_fail_dev;
  h->pipe_clear();
  h->pipe_fallback_last = 0;
  const int grid = (E + auvp::ASTAR_WAVES - 1) / auvp::ASTAR_WAVES;
  bool pair = false;
  // variant 3, plain or with a table per instance (astar_sets_kernels.hip)
  auto launch3 = [&](bool two) -> hipError_t {
    if (sets)
      return auvpi_astar_sets_launch(&S.W, &P, &B, (int)E, h->d_sets_prob.as<double>(), S.sets_topn.as<double>(), S.set_of.as<int32_t>(), two ? 1 : 0,
                                     grid, h->stream);
    if (two) hipLaunchKernelGGL((auvp::astar_kernel<3, true>), dim3(grid), dim3(auvp::ASTAR_WAVES * 128), 0, h->stream, S.W, P, B, (int)E);
    else hipLaunchKernelGGL(auvp::astar_kernel<3>, dim3(grid), dim3(auvp::ASTAR_WAVES * 64), 0, h->stream, S.W, P, B, (int)E);
    return hipSuccess;
  };
  switch (P.variant) {
    case 0: hipLaunchKernelGGL(auvp::astar_kernel<0>, dim3(grid), dim3(auvp::ASTAR_WAVES * 64), 0, h->stream, S.W, P, B, (int)E); break;
    case 1: hipLaunchKernelGGL(auvp::astar_kernel<1>, dim3(grid), dim3(auvp::ASTAR_WAVES * 64), 0, h->stream, S.W, P, B, (int)E); break;
    case 2: hipLaunchKernelGGL(auvp::astar_kernel<2>, dim3(grid), dim3(auvp::ASTAR_WAVES * 64), 0, h->stream, S.W, P, B, (int)E); break;
    default: {
      // latency batches on a product grid: a second wavefront per instance (astar_kernel.h, PAIR); option ASTAR_PAIR = 0 / 1
      // forces the choice.  Not with a visited array the caller carries over (KEEP_VISITED): a batch that had to be repeated on
      // the one-wavefront kernel (pipeline fallback, below) could not get it back.
      pair = S.W.g_ncol > 0 && !(flags & AUVP_FLAG_KEEP_VISITED) && h->opt_flag(OPT_ASTAR_PAIR, E <= (size_t)8 * (size_t)h->n_cu);
      HIPCHK(h, launch3(pair));
      break;
    }
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (pair && h->pipe_failed()) {
    // the searching wavefront of some instance stopped waiting for its partner (AUVP_ERR_PIPELINE): the batch is searched again
    // by the one-wavefront kernel, on a fresh epoch of the visited words (same results, visited arrays included:
    // tests/test_gpu_astar_pair.py makes the waits run out under the diagnostic build and counts the instances redone)
    std::vector<auvp::AstarSummary> sm((size_t)E);
    HIPCHK(h, hipMemcpy(sm.data(), B.summary, sm.size() * sizeof(auvp::AstarSummary), hipMemcpyDeviceToHost));
    int n = 0;
    for (const auvp::AstarSummary& r : sm) n += r.status == AUVP_ERR_PIPELINE ? 1 : 0;
    h->pipe_clear();
    if (n > 0 && h->opt_flag(OPT_PIPE_FALLBACK, true)) {
      h->pipe_fallback_last = n;
      h->pipe_fallback_total += n;
      if ((rc = astar_next_epoch(h, S, false))) return rc;
      P.epoch = S.epoch;
      pair = false;
      HIPCHK(h, launch3(false));  // (with sets: the one-wavefront sets form, every instance on its own table again)
      HIPCHK(h, hipGetLastError());
      HIPCHK(h, hipEventRecord(h->ev1, h->stream));  // (the time the caller waited: both searches)
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
  }
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  h->last_ms = ms;
  h->last_grid = grid; h->last_block = auvp::ASTAR_WAVES * (pair ? 128 : 64); h->last_lds = 0;
  S.E = E;
  S.ready = true;
  return AUVP_OK;
}

}  // namespace

extern "C" {

int auvp_astar_batch(auvp_handle* h, int32_t E, const double* starts, const double* goals, const double* limits,
                     const auvp_astar_params* p, int32_t flags) {
  return astar_batch_run(h, E, starts, goals, limits, p, flags, nullptr);
}

int auvp_astar_batch_sets(auvp_handle* h, int32_t E, const double* starts, const double* limits, const auvp_astar_params* p, int32_t flags,
                          const int32_t* set_of) {
  if (!h) return AUVP_ERR_ARG;
  if (!set_of) return fail(h, AUVP_ERR_ARG, "set_of required");
  return astar_batch_run(h, E, starts, nullptr, limits, p, flags, set_of);
}

int auvp_astar_sets_topn(auvp_handle* h, double* out) {
  if (!h || !out) return AUVP_ERR_ARG;
  if (h->n_sets < 1) return fail(h, AUVP_ERR_STATE, "no probability sets on this handle (auvp_world_set_prob_sets)");
  HIPCHK(h, hipSetDevice(h->device));
  AstarState& S = *astar_of(h);
  int rc;
  if (S.sets_version != h->sets_version && (rc = astar_build_set_tables(h, S))) return rc;
  const size_t n = (size_t)h->n_sets * h->W.n_bins * ((size_t)h->W.n_cells + 1);
  HIPCHK(h, hipMemcpyAsync(out, S.sets_topn.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return AUVP_OK;
}

int auvp_astar_summaries(auvp_handle* h, auvp_astar_summary* out) {
  if (!h || !out) return AUVP_ERR_ARG;
  AstarState& S = *astar_of(h);
  if (!S.ready) return fail(h, AUVP_ERR_STATE, "no A* batch");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpy(out, S.B.summary, (size_t)S.E * sizeof(auvp::AstarSummary), hipMemcpyDeviceToHost));
  return AUVP_OK;
}

int auvp_astar_paths(auvp_handle* h, const int64_t* offsets, double* path3, double* cost_list, double* node_path8,
                     double* smooth3) {
  if (!h || !offsets || !path3) return AUVP_ERR_ARG;
  AstarState& S = *astar_of(h);
  if (!S.ready) return fail(h, AUVP_ERR_STATE, "no A* batch");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t total = (size_t)offsets[S.E], n = std::max<size_t>(total, 1);
  int rc;
  if ((rc = upload(h, S.off, offsets, (size_t)S.E + 1))) return rc;
  HIPCHK(h, S.path.reserve(n * 3 * sizeof(double)));
  HIPCHK(h, S.cost.reserve(n * sizeof(double)));
  HIPCHK(h, S.npath.reserve(n * 8 * sizeof(double)));
  HIPCHK(h, S.smooth.reserve(n * 3 * sizeof(double)));
  hipLaunchKernelGGL(auvp::astar_path_kernel, dim3(S.E), dim3(64), 0, h->stream, S.W, S.P, S.B, S.off.as<int64_t>(),
                     S.path.as<double>(), S.cost.as<double>(), S.npath.as<double>(), S.smooth.as<double>(), S.E);
  HIPCHK(h, hipGetLastError());
  if (total) {
    HIPCHK(h, hipMemcpyAsync(path3, S.path.p, total * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (cost_list) HIPCHK(h, hipMemcpyAsync(cost_list, S.cost.p, total * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (node_path8) HIPCHK(h, hipMemcpyAsync(node_path8, S.npath.p, total * 8 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (smooth3) HIPCHK(h, hipMemcpyAsync(smooth3, S.smooth.p, total * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return AUVP_OK;
}

int auvp_astar_exp_log(auvp_handle* h, int32_t ep, double* out8) {
  if (!h || !out8) return AUVP_ERR_ARG;
  AstarState& S = *astar_of(h);
  if (!S.ready || ep < 0 || ep >= S.E || !S.B.exp_log) return fail(h, AUVP_ERR_STATE, "no expansion log");
  HIPCHK(h, hipSetDevice(h->device));
  auvp::AstarSummary s;
  HIPCHK(h, hipMemcpy(&s, S.B.summary + ep, sizeof s, hipMemcpyDeviceToHost));
  const size_t n = (size_t)std::min(s.n_expansions, S.P.cap_exp);
  if (n) HIPCHK(h, hipMemcpy(out8, S.B.exp_log + (size_t)ep * S.P.cap_exp * 8, n * 8 * sizeof(double), hipMemcpyDeviceToHost));
  return AUVP_OK;
}

// visited bitmap in / out (variants 2,3): [E][vx*vy] bytes, vx = 550 (fixLen) or 600 (SOG), vy = 600;
// set before auvp_astar_batch(..., AUVP_FLAG_KEEP_VISITED), get after any batch.  On the device the array is
// the epoch-tagged word array of astar_kernel.h; the byte view of the reference is converted here.
int auvp_astar_set_visited(auvp_handle* h, int32_t E, int32_t variant, const uint8_t* bitmap) {
  if (!h || !bitmap || E <= 0 || variant < 2 || variant > 3) return AUVP_ERR_ARG;
  AstarState& S = *astar_of(h);
  HIPCHK(h, hipSetDevice(h->device));
  const size_t entries = (size_t)E * (variant == 2 ? 550 : 600) * 600;
  HIPCHK(h, S.cellinfo.reserve(entries * sizeof(uint32_t)));
  // (as auvp_astar_batch: tests/test_gpu_epoch_wrap.py puts bitmaps in on either side of the wrap)
  if (int rc = astar_next_epoch(h, S, S.cellinfo_clean_cap != S.cellinfo.cap)) return rc;
  std::vector<uint32_t> words(entries);
  const uint32_t tag = S.epoch << 24;
  for (size_t i = 0; i < entries; i++) words[i] = bitmap[i] ? (tag | 0x10000u) : 0u;
  HIPCHK(h, hipMemcpyAsync(S.cellinfo.p, words.data(), entries * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  S.visited_set_for = (long long)entries;
  return AUVP_OK;
}

int auvp_astar_get_visited(auvp_handle* h, int32_t ep, uint8_t* bitmap) {
  if (!h || !bitmap) return AUVP_ERR_ARG;
  AstarState& S = *astar_of(h);
  if (!S.ready || ep < 0 || ep >= S.E || !S.B.cellinfo) return fail(h, AUVP_ERR_STATE, "no visited bitmap");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t one = (size_t)S.P.vx * S.P.vy;
  std::vector<uint32_t> words(one);
  HIPCHK(h, hipMemcpy(words.data(), S.B.cellinfo + (size_t)ep * one, one * sizeof(uint32_t), hipMemcpyDeviceToHost));
  const uint32_t tag = S.P.epoch << 24;
  for (size_t i = 0; i < one; i++) bitmap[i] = ((words[i] & 0xff000000u) == tag && (words[i] & 0x10000u)) ? 1 : 0;
  return AUVP_OK;
}

int auvp_astar_hab_left(auvp_handle* h, int32_t ep, int32_t* out) {
  if (!h || !out) return AUVP_ERR_ARG;
  AstarState& S = *astar_of(h);
  if (!S.ready || ep < 0 || ep >= S.E) return fail(h, AUVP_ERR_STATE, "bad instance");
  HIPCHK(h, hipSetDevice(h->device));
  const int H = S.W.n_habitats;
  if (H) HIPCHK(h, hipMemcpy(out, S.B.hab_left + (size_t)ep * H, (size_t)H * sizeof(int32_t), hipMemcpyDeviceToHost));
  return AUVP_OK;
}

}  // extern "C"
#endif

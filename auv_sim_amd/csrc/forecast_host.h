// forecast_host.h -- host side of the shark-occupancy forecast (auvp_sf_*, include/auvplan.h): the level schedule and the
// launch choice as handle-less queries, and the launch of sf_forecast_kernel (forecast_kernel.h) or sf_wide_kernel
// (forecast_wide_kernel.h), whichever sf_choose_launch (forecast_launch.h) names, on a host array of particle coordinates or
// on the handle's particle-filter batch where it lies in HBM.
// Included at the end of auvplan.hip, behind pf_host.h (PfState) and the two kernel headers.
#ifndef AUVP_FORECAST_HOST_H
#define AUVP_FORECAST_HOST_H
#include "forecast_launch.h"
#include "forecast_plan.h"

static_assert(auvp::SF_WIDE_LDS_BYTES == auvp::SFW_LDS_BYTES, "forecast_launch.h reports sf_wide_kernel's static LDS");

namespace {

struct SfState {
  DevBuf xy, prior, p_inf, cell_g, sched_g, level_off, grids, prob, counts, status;
  int F = 0, T = 0, C = 0;  // shape of `prob` after the last forecast that completed (F == 0: none)
  const char* last_kernel = "";  // the kernel that forecast ran (auvp_sf_last_kernel)
};

SfState* sf_of(auvp_handle* h) {
  if (!h->sf) {
    h->sf = new SfState();
    h->sf_free = [](void* p) { delete static_cast<SfState*>(p); };
  }
  return static_cast<SfState*>(h->sf);
}

// auvp_sf_forecast / auvp_sf_forecast_large: one implementation, allow_large is the only difference
int sf_forecast_impl(auvp_handle* h, bool allow_large, const double* box4, int32_t rows, int32_t cols, double cell_size,
                     const double* cells, int32_t n_cells, int32_t n_filters, const double* particles_xy, int32_t n_particles,
                     const double* prior, int32_t prior_is_shared, int32_t method, const double* p_inf, double stay_prob, double k,
                     double norm, int32_t n_rounds, double* grids, double* prob, int32_t* counts, int32_t* status) {
  if (!h) return AUVP_ERR_ARG;
  if (!box4 || !cells || !prior) return fail(h, AUVP_ERR_ARG, "null argument");
  if (rows < 1 || cols < 1 || n_cells < 1 || n_filters < 1 || n_particles < 1 || n_rounds < 0)
    return fail(h, AUVP_ERR_ARG, "need rows, cols, cells, filters, particles >= 1 and rounds >= 0");
  if (method != 1 && method != 2) return fail(h, AUVP_ERR_ARG, "method %d is neither 1 (prediction1) nor 2 (prediction2)", method);
  if (!(cell_size > 0.0) || !std::isfinite(cell_size)) return fail(h, AUVP_ERR_ARG, "cell_size must be finite and > 0");
  if (norm == 0.0 || std::isnan(norm)) return fail(h, AUVP_ERR_ARG, "norm must be a non-zero number");
  // the launch, before anything is allocated (the choice reads neither the list's length nor its levels today: 0 = not known)
  const auvp::SfLaunch launch = auvp::sf_choose_launch(rows, cols, n_cells, 0, allow_large, h->opt);
  if (launch.status == auvp::SF_LAUNCH_CAPACITY)
    return fail(h, AUVP_ERR_CAPACITY, "%d x %d grid entries > %lld (%s)", rows, cols, launch.limit,
                allow_large ? "auvp_sf_forecast_large's stated limit" : "one workgroup's LDS; auvp_sf_forecast_large takes larger grids");
  if (launch.status != auvp::SF_LAUNCH_OK)
    return fail(h, AUVP_ERR_ARG, "option SF_WIDE_BLOCK must be a multiple of 64 in 64 .. 1024");
  const bool wide = launch.kind == auvp::SF_KERNEL_WIDE;
  const int G = rows * cols, C = n_cells, F = n_filters, N = n_particles, R = n_rounds;
  const double minx = box4[0], miny = box4[1];
  // cellToIndex per cell, then the schedule (which also validates the list)
  std::vector<int32_t> rc((size_t)C * 2);
  for (int c = 0; c < C; c++) {
    const double qr = (cells[4 * (size_t)c + 1] - miny) / cell_size, qc = (cells[4 * (size_t)c] - minx) / cell_size;
    if (!(qr > -1.0 && qr < (double)rows && qc > -1.0 && qc < (double)cols))  // (int() truncates: (-1, 0) is index 0)
      return fail(h, AUVP_ERR_ARG, "cell %d lies outside the %d x %d grid (the reference: IndexError, or a wrapped negative index)", c, rows, cols);
    rc[2 * (size_t)c] = (int32_t)qr;
    rc[2 * (size_t)c + 1] = (int32_t)qc;
  }
  const auvp::SfPlan plan = auvp::sf_plan(rows, cols, rc.data(), C);
  if (plan.status == auvp::SF_PLAN_DUPLICATE)
    return fail(h, AUVP_ERR_ARG, "cell %d names a grid entry an earlier cell of the list names (a cell may be listed once)", plan.bad);
  if (plan.status != auvp::SF_PLAN_OK) return fail(h, AUVP_ERR_ARG, "cell %d lies outside the grid", plan.bad);
  std::vector<int32_t> cell_g(C), sched_g(C);
  for (int c = 0; c < C; c++) cell_g[c] = rc[2 * (size_t)c] * cols + rc[2 * (size_t)c + 1];
  for (int s = 0; s < C; s++) sched_g[s] = cell_g[plan.order[s]];
  std::vector<double> ave;
  if (method == 2 && !p_inf) {  // predictOnAve's P_inf: 1 / len(cell_list) in the listed cells
    ave.assign(G, 0.0);
    for (int c = 0; c < C; c++) ave[cell_g[c]] = 1.0 / (double)C;
    p_inf = ave.data();
  }
  HIPCHK(h, hipSetDevice(h->device));
  SfState& S = *sf_of(h);
  S.F = 0; S.last_kernel = "";  // (auvp_sf_prob_dev: nothing to hand out until this forecast has completed)
  auvp::SfDev D{};
  D.F = F; D.N = N; D.rows = rows; D.cols = cols; D.C = C; D.R = R; D.method = method; D.n_levels = plan.n_levels;
  D.prior_shared = prior_is_shared ? 1 : 0;
  D.minx = minx; D.miny = miny; D.cell_size = cell_size; D.stay = stay_prob; D.k = k; D.norm = norm;
  int rc2;
  if (particles_xy) {
    if ((rc2 = upload(h, S.xy, particles_xy, (size_t)F * N * 2))) return rc2;
    D.pxy = S.xy.as<double>(); D.f_stride = 2ll * N; D.e_stride = 2; D.y_off = 1;
  } else {
    PfState* P = static_cast<PfState*>(h->pf);
    if (!P || !P->ready) return fail(h, AUVP_ERR_STATE, "no particle-filter batch on this handle (particles_xy is NULL)");
    if (P->F != F || P->N != N)
      return fail(h, AUVP_ERR_ARG, "the handle's batch has %d filters x %d particles, not %d x %d", P->F, P->N, F, N);
    D.pxy = P->st.as<double>(); D.f_stride = 5ll * N; D.e_stride = 1; D.y_off = N;
  }
  const size_t T = (size_t)R + 1;
  if ((rc2 = upload(h, S.prior, prior, (size_t)(prior_is_shared ? 1 : F) * G))) return rc2;
  if (method == 2 && (rc2 = upload(h, S.p_inf, p_inf, (size_t)G))) return rc2;
  if ((rc2 = upload(h, S.cell_g, cell_g.data(), cell_g.size()))) return rc2;
  if ((rc2 = upload(h, S.sched_g, sched_g.data(), sched_g.size()))) return rc2;
  if ((rc2 = upload(h, S.level_off, plan.level_off.data(), plan.level_off.size()))) return rc2;
  HIPCHK(h, S.grids.reserve((size_t)F * T * G * sizeof(double)));
  HIPCHK(h, S.prob.reserve((size_t)F * T * C * sizeof(double)));
  HIPCHK(h, S.counts.reserve((size_t)F * G * sizeof(int32_t)));
  HIPCHK(h, S.status.reserve((size_t)F * sizeof(int32_t)));
  D.prior = S.prior.as<double>(); D.p_inf = method == 2 ? S.p_inf.as<double>() : nullptr;
  D.cell_g = S.cell_g.as<int32_t>(); D.sched_g = S.sched_g.as<int32_t>(); D.level_off = S.level_off.as<int32_t>();
  D.grids = S.grids.as<double>(); D.prob = S.prob.as<double>(); D.counts = S.counts.as<int32_t>(); D.status = S.status.as<int32_t>();
  const size_t lds = (size_t)launch.lds;
  if (wide) {  // (its LDS is static)
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(auvp::sf_wide_kernel, dim3(F), dim3(launch.block), 0, h->stream, D);
  } else {
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(auvp::sf_forecast_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(auvp::sf_forecast_kernel, dim3(F), dim3(64), lds, h->stream, D);
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  if (grids) HIPCHK(h, hipMemcpyAsync(grids, S.grids.p, (size_t)F * T * G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (prob) HIPCHK(h, hipMemcpyAsync(prob, S.prob.p, (size_t)F * T * C * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (counts) HIPCHK(h, hipMemcpyAsync(counts, S.counts.p, (size_t)F * G * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (status) HIPCHK(h, hipMemcpyAsync(status, S.status.p, (size_t)F * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // (the host vectors go out of scope)
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  h->last_ms = ms; h->last_grid = F; h->last_block = launch.block; h->last_lds = (int)lds;
  S.F = F; S.T = (int)T; S.C = C; S.last_kernel = launch.name;
  return AUVP_OK;
}

}  // namespace

extern "C" {

int auvp_sf_plan(int32_t rows, int32_t cols, const int32_t* cell_rc, int32_t n_cells, int32_t* level, int32_t* order,
                 int32_t* level_off, int32_t* n_levels) {
  const auvp::SfPlan p = auvp::sf_plan(rows, cols, cell_rc, n_cells);
  if (p.status != auvp::SF_PLAN_OK) return AUVP_ERR_ARG;
  if (n_levels) *n_levels = p.n_levels;
  if (level) std::copy(p.level.begin(), p.level.end(), level);
  if (order) std::copy(p.order.begin(), p.order.end(), order);
  if (level_off) std::copy(p.level_off.begin(), p.level_off.end(), level_off);
  return AUVP_OK;
}

int auvp_sf_forecast(auvp_handle* h, const double* box4, int32_t rows, int32_t cols, double cell_size, const double* cells,
                     int32_t n_cells, int32_t n_filters, const double* particles_xy, int32_t n_particles, const double* prior,
                     int32_t prior_is_shared, int32_t method, const double* p_inf, double stay_prob, double k, double norm,
                     int32_t n_rounds, double* grids, double* prob, int32_t* counts, int32_t* status) {
  return sf_forecast_impl(h, false, box4, rows, cols, cell_size, cells, n_cells, n_filters, particles_xy, n_particles, prior,
                          prior_is_shared, method, p_inf, stay_prob, k, norm, n_rounds, grids, prob, counts, status);
}

int auvp_sf_forecast_large(auvp_handle* h, const double* box4, int32_t rows, int32_t cols, double cell_size, const double* cells,
                           int32_t n_cells, int32_t n_filters, const double* particles_xy, int32_t n_particles,
                           const double* prior, int32_t prior_is_shared, int32_t method, const double* p_inf, double stay_prob,
                           double k, double norm, int32_t n_rounds, double* grids, double* prob, int32_t* counts,
                           int32_t* status) {
  return sf_forecast_impl(h, true, box4, rows, cols, cell_size, cells, n_cells, n_filters, particles_xy, n_particles, prior,
                          prior_is_shared, method, p_inf, stay_prob, k, norm, n_rounds, grids, prob, counts, status);
}

const char* auvp_sf_last_kernel(auvp_handle* h) {
  const SfState* S = h ? static_cast<const SfState*>(h->sf) : nullptr;
  return S ? S->last_kernel : "";
}

int auvp_sf_choose_launch(const auvp_sf_launch_query* q, auvp_sf_launch_choice* c) {
  OptionView opt;
  if (!q || !c || !query_options(q->n_options, q->option_names, q->option_values, &opt)) return AUVP_ERR_ARG;
  const auvp::SfLaunch p = auvp::sf_choose_launch(q->rows, q->cols, q->n_cells, q->widest_level, q->allow_large != 0, opt);
  *c = auvp_sf_launch_choice{p.status == auvp::SF_LAUNCH_OK ? AUVP_OK : (p.status == auvp::SF_LAUNCH_CAPACITY ? AUVP_ERR_CAPACITY : AUVP_ERR_ARG),
                             (int32_t)p.kind, p.block, p.lds, p.name};
  return AUVP_OK;
}

int auvp_sf_prob_dev(auvp_handle* h, const void** prob_dev, int32_t* n_filters, int32_t* n_bins, int32_t* n_cells) {
  if (!h) return AUVP_ERR_ARG;
  const SfState* S = static_cast<const SfState*>(h->sf);
  if (!S || S->F < 1) return fail(h, AUVP_ERR_STATE, "no forecast has run on this handle");
  if (prob_dev) *prob_dev = S->prob.p;
  if (n_filters) *n_filters = S->F;
  if (n_bins) *n_bins = S->T;
  if (n_cells) *n_cells = S->C;
  return AUVP_OK;
}

}  // extern "C"
#endif  // AUVP_FORECAST_HOST_H

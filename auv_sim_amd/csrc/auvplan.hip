// auvplan.hip -- C-ABI (include/auvplan.h) + host runtime of libauvplan.so for MI355X / gfx950.
//
// Host side of the hot path: owns the device copy of the world model and the per-episode tree
// storage in HBM, seeds the per-episode MT19937 states the way CPython's random.seed() does,
// launches the persistent expansion kernel (one wavefront per episode) on the handle's own HIP
// stream and times it with HIP events on that stream.  No CPU compute path exists here: if the
// device or the code object is unusable every entry point fails with AUVP_ERR_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/auvplan.h"
#include "auvp_seed.h"
#include "rrt_explore_kernel.h"
#include "rrt_group_kernel.h"
#include "rrt_rows_kernel.h"
#include "rrt_rows_stream_kernel.h"  // (the LDS plan; the kernel itself is launched from rows_kernels.hip)
#include "rrt_duo_kernel.h"
#include "rrt_trio_kernel.h"
#include "planner_rrt_kernel.h"
#include "planner_rows_kernel.h"
#include "planner_goal_arc.h"
#include "planner_pipe_kernel.h"
#include "launch_plan.h"  // (behind every kernel header whose LDS plan and limits the choice reads)
#include "batch_plan.h"   // (what a batch needs in HBM, the stream's rules, the epoch tags: pure as well)
#include "world_tables.h"
#include "forecast_place.h"

using namespace auvp;

// rrt_rows_kernel lives in rows_kernels.hip (a translation unit with its own compiler flags); this is its launcher
extern "C" hipError_t auvpi_rrt_stream_launch(const auvp::RrtBuffers* B, int n_episodes, hipStream_t stream);
extern "C" hipError_t auvpi_rrt_rows_stream_launch(const auvp::WorldDev* W, const auvp::RrtParamsDev* P, const auvp::RrtBuffers* B, int n_episodes,
                                                   int grid, int block, int lds_max, int lds, int mirror, hipStream_t stream);
extern "C" hipError_t auvpi_rrt_rows_launch(const auvp::WorldDev* W, const auvp::RrtParamsDev* P, const auvp::RrtBuffers* B, int n_episodes,
                                            int grid, int block, int lds_max, int lds, hipStream_t stream);
// rrt_leaf_grid_kernel and prob_set_stats_kernel live in leaf_grid_kernels.hip (so that this unit's leaf kernels keep their code)
extern "C" hipError_t auvpi_rrt_leaf_grid_launch(const auvp::WorldDev* W, const auvp::RrtParamsDev* P, const auvp::RrtBuffers* B, int n_episodes,
                                                 int mark_words, const auvp::RrtEpisodeLimDev* lim, const int32_t* set_of,
                                                 const auvp::RrtProbSetDev* sets, int grid, int block, int lds, hipStream_t stream);
extern "C" hipError_t auvpi_prob_set_stats_launch(const double* prob, long long n_per_set, int n_sets, auvp::RrtProbSetDev* sets,
                                                  hipStream_t stream);
// ... and sf_place_kernel: the sets from a forecast placed at a first bin (forecast_place.h)
extern "C" hipError_t auvpi_sf_place_launch(const double* src, double* dst, int n_sets, int T, int R1, int C, int first_bin, hipStream_t stream);

#ifdef AUVP_PIPE_DIAG
extern "C" hipError_t auvpi_astar_sets_diag(const int* cfg8);  // (astar_sets_kernels.hip; the other launchers: astar_host.h)
#endif

static_assert(sizeof(auvp_rrt_summary) == sizeof(RrtSummary), "summary layout");
static_assert(sizeof(struct auvp_rrt_group_best) == sizeof(RrtGroupBest), "group record layout");

namespace {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
    if (e == hipSuccess) cap = bytes ? bytes : 16;
    return e;
  }
  void release() { if (p) { (void)hipFree(p); p = nullptr; cap = 0; } }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

}  // namespace

struct auvp_handle {
  OptionView opt;  // the options (launch_plan.h: the list, the accessors)
  bool opt_flag(int k, bool dflt) const { return opt.opt_flag(k, dflt); }
  bool opt_on(int k) const { return opt.opt_on(k); }
  long long opt_num(int k, long long dflt) const { return opt.opt_num(k, dflt); }
  int device = 0;
  int n_cu = 256;  // compute units of the device (256 where the query fails): read once, by auvp_create
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_mid = nullptr, ev_pre = nullptr;
  double last_expand_ms = 0.0, last_leaf_ms = 0.0, last_stream_ms = 0.0;
  long long last_stream_len = 0;  // numbers per episode the last pass generated ahead (0: none)
  int last_stream_mirror = -1;    // the ring's form in the last pass's rrt_rows_stream_kernel: 1 mirrored, 0 masked (-1: another kernel ran)
  DrawnMemory drawn;  // what complete passes of RRT.exploring drew (batch_plan.h): the length of the next batch's stream
  int last_rows = 0;
  const char* last_rrt_kernel = "";
  std::string err;
  // world
  bool have_world = false;
  double obst_area = 0.0;  // area of the bounding box of the obstacle centres (0: fewer than two obstacles / degenerate)
  WorldDev W{};
  DevBuf d_ox, d_oy, d_ot, d_hab, d_habt, d_poly, d_bins, d_cells, d_prob, d_xoff, d_xitems, d_xdata, d_rgfirst, d_rgbp, d_rgoff,
      d_rgpm, d_rgid, d_sgx0, d_sgx1, d_sgy0, d_sgy1, d_sgcol, d_sgrow, d_osx, d_osy, d_ost, d_osr, d_osbox, d_hgmask;
  // rrt batch
  int E = 0;
  RrtParamsDev P{};
  RrtBuffers B{};
  int max_pts = 0;
  DevBuf d_nodes_f, d_nodes_i, d_points, d_bin_items, d_bin_count, d_mt, d_mtidx, d_seeds, d_init, d_summary, d_itlog_i, d_itlog_b,
      d_leaf_c, d_leaf_i, d_phase, d_leaf_stats, d_node_c, d_node_q, d_node_xy, d_tmp0, d_tmp1, d_tmp2, d_tmp3, d_tmp4, d_tmp5, d_stream;
  bool have_batch = false, prepared = false;
  // best-of-K selection (auvp_rrt_group_best) of the batch that ran last: the records in HBM and their host copy (the offsets
  // of auvp_rrt_group_paths are checked against it before anything is written)
  DevBuf d_group_off, d_group_best, d_group_pos;
  std::vector<RrtGroupBest> group_best;
  bool have_group = false;
  // per-episode limits (auvp_rrt_prepare_episodes): the batch runs rrt_explore_lim_kernel + rrt_leaf_lim_kernel; lim_K: every
  // episode's own K (P.K is the cap's)
  bool lim = false;
  DevBuf d_lim;
  std::vector<int32_t> lim_K;
  // probability sets (auvp_world_set_prob_sets): n_sets tables [T,C] over the world's bins and cells and their records; grids:
  // the prepared batch has a set per episode (auvp_rrt_set_episode_grids) and its leaf pass is rrt_leaf_grid_kernel
  int n_sets = 0;
  unsigned sets_version = 0;  // bumped whenever the sets change or go: what is derived from them (astar_host.h: top-n tables) is stale
  bool grids = false;
  DevBuf d_sets_prob, d_sets_rec, d_set_of;
  double last_ms = 0.0;
  int last_grid = 0, last_block = 0, last_lds = 0;
  // planner families that live in their own headers keep their state behind an opaque pointer
  void* prrt = nullptr;
  void (*prrt_free)(void*) = nullptr;
  std::vector<double> w_obst, w_hab, w_poly, w_bins, w_cells, w_prob;  // host copy of the world
  unsigned world_version = 0;
  void* astar = nullptr;
  void (*astar_free)(void*) = nullptr;
  void* pf = nullptr;
  void (*pf_free)(void*) = nullptr;
  void* sf = nullptr;  // shark-occupancy forecast buffers (forecast_host.h)
  void (*sf_free)(void*) = nullptr;
  void* comm = nullptr;  // RCCL communicator state (gather_host.h)
  void (*comm_free)(void*) = nullptr;
  void* replan = nullptr;  // a fleet's replanning state and trajectory log (replan_host.h)
  void (*replan_free)(void*) = nullptr;
  // Pipeline fallback.  The latency kernels (rrt_trio / rrt_duo, prrt_pipe, the paired astar_kernel) are speculative
  // pipelines of several wavefronts per episode whose waits are bounded; an episode whose wait runs out ends with
  // AUVP_ERR_PIPELINE and sets this host-mapped word.  The host then repeats the work on the one-wavefront kernel (same
  // results by construction: tests/test_gpu_duo_kernel.py etc.) -- a caller never sees the status.  Counters: episodes redone.
  int32_t* pipe_fail_host = nullptr;
  int32_t* pipe_fail_dev = nullptr;
  int pipe_fallback_last = 0;
  long long pipe_fallback_total = 0;
  bool pipe_failed() const { return pipe_fail_host && __atomic_load_n(pipe_fail_host, __ATOMIC_ACQUIRE) != 0; }
  void pipe_clear() { if (pipe_fail_host) __atomic_store_n(pipe_fail_host, 0, __ATOMIC_RELEASE); }
};

namespace {

int fail(auvp_handle* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (h) h->err = buf;
  return code;
}

#define HIPCHK(h, call)                                                                        \
  do {                                                                                         \
    hipError_t e__ = (call);                                                                   \
    if (e__ != hipSuccess) return fail(h, AUVP_ERR_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
  } while (0)

// CPython random.seed(int) -> init_by_array over the 32-bit limbs of the seed
// (Modules/_randommodule.c; restated from the MT19937 reference algorithm)
void seed_mt(uint64_t seed, uint32_t* mt) {
  uint32_t key[2] = {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)};
  const int klen = key[1] ? 2 : 1;
  mt[0] = 19650218u;
  for (int i = 1; i < 624; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
  int i = 1, j = 0;
  for (int k = 624; k; k--) {
    mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
    i++; j++;
    if (i >= 624) { mt[0] = mt[623]; i = 1; }
    if (j >= klen) j = 0;
  }
  for (int k = 623; k; k--) {
    mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
    i++;
    if (i >= 624) { mt[0] = mt[623]; i = 1; }
  }
  mt[0] = 0x80000000u;
}

template <class T>
int upload(auvp_handle* h, DevBuf& b, const T* src, size_t n) {
  HIPCHK(h, b.reserve(n * sizeof(T)));
  if (n) HIPCHK(h, hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, h->stream));
  return AUVP_OK;
}

// one table on its way to HBM: the buffer it gets, the host memory it is copied from
struct TableUpload {
  DevBuf& buf;
  const void* src;
  size_t bytes;
  template <class T>
  TableUpload(DevBuf& b, const std::vector<T>& v) : buf(b), src(v.data()), bytes(v.size() * sizeof(T)) {}
  TableUpload(DevBuf& b, const double* p, size_t n) : buf(b), src(p), bytes(n * sizeof(double)) {}
};

// every table of the list, then ONE wait: the host memory behind `src` must live until this returns
int upload_tables(auvp_handle* h, std::initializer_list<TableUpload> tables) {
  for (const TableUpload& u : tables) {
    HIPCHK(h, u.buf.reserve(u.bytes));
    if (u.bytes) HIPCHK(h, hipMemcpyAsync(u.buf.p, u.src, u.bytes, hipMemcpyHostToDevice, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return AUVP_OK;
}

// the habitats' fields of WorldDev from their tables (world_tables.h) and the buffers these were uploaded to
void fill_habitat_dev(auvp_handle* h, int H, const HabitatTables& t) {
  WorldDev& W = h->W;
  W.n_habitats = H;
  W.hab = h->d_hab.as<double>(); W.hab_t = h->d_habt.as<double>();
  W.hg_n = t.hg_n; W._pad_hg = 0;
  W.hg_x0 = t.hg_x0; W.hg_y0 = t.hg_y0; W.hg_inv_w = t.hg_inv_w; W.hg_inv_h = t.hg_inv_h;
  W.hg_mask = t.hg_n ? h->d_hgmask.as<unsigned long long>() : nullptr;
}

// WorldDev from the world's sizes, its tables (world_tables.h) and the buffers these were uploaded to
void fill_world_dev(auvp_handle* h, const WorldIn& in, const WorldTables& t) {
  WorldDev& W = h->W;
  W.n_obstacles = in.O; W.n_poly = in.V; W.n_bins = in.T; W.n_cells = in.C; W.n_xbuckets = t.n_xbuckets;
  W.ox = h->d_ox.as<double>(); W.oy = h->d_oy.as<double>(); W.ot = h->d_ot.as<double>();
  W.os_x = h->d_osx.as<double>(); W.os_y = h->d_osy.as<double>(); W.os_t = h->d_ost.as<double>(); W.os_r = h->d_osr.as<float>();
  W.os_box = h->d_osbox.as<double>();
  W.poly = h->d_poly.as<double>(); W.bins = h->d_bins.as<double>(); W.cells = h->d_cells.as<double>(); W.prob = h->d_prob.as<double>();
  W.xb_off = h->d_xoff.as<int32_t>(); W.xb_items = h->d_xitems.as<int32_t>(); W.xb_data = h->d_xdata.as<double>();
  W.xb_x0 = t.xb_x0; W.xb_inv_w = t.xb_inv_w;
  W.rg_enabled = t.rg_enabled; W.n_rg_bp = t.n_rg_bp;
  W.rg_first = h->d_rgfirst.as<int32_t>(); W.rg_bp = h->d_rgbp.as<double>(); W.rg_off = h->d_rgoff.as<int32_t>();
  W.rg_pm = h->d_rgpm.as<double>(); W.rg_id = h->d_rgid.as<int32_t>();
  W.sg_enabled = t.sg_enabled; W.sg_ncol = t.sg_ncol; W.sg_nrow = t.sg_nrow;
  W.sg_x0 = h->d_sgx0.as<double>(); W.sg_x1 = h->d_sgx1.as<double>(); W.sg_y0 = h->d_sgy0.as<double>(); W.sg_y1 = h->d_sgy1.as<double>();
  W.sg_col = h->d_sgcol.as<double>(); W.sg_row = h->d_sgrow.as<double>();
  W.sg_x1_0 = t.sg_x1_0; W.sg_y1_0 = t.sg_y1_0; W.sg_inv_dx = t.sg_inv_dx; W.sg_inv_dy = t.sg_inv_dy;
  W.bins_sorted = t.bins_sorted; W.bins_t1_0 = t.bins_t1_0; W.bins_inv_len = t.bins_inv_len;
  W.prob_absmax = t.prob_absmax; W.prob_one_sign = t.prob_one_sign; W._pad_prob = 0;
  memcpy(W.bb, t.bb, sizeof W.bb);
  memcpy(W.safe_box, t.safe_box, sizeof W.safe_box);
  W.has_safe_box = t.has_safe_box; W._pad1 = 0;
  fill_habitat_dev(h, in.H, t.hab);
}

}  // namespace

extern "C" {

const char* auvp_version(void) { return "auvplan 0.1 (gfx950)"; }

int auvp_create(int device, auvp_handle** out) {
  if (!out) return AUVP_ERR_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return AUVP_ERR_HIP;
  auvp_handle* h = new auvp_handle();
  h->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess || hipEventCreate(&h->ev_mid) != hipSuccess ||
      hipEventCreate(&h->ev_pre) != hipSuccess) {
    delete h;
    return AUVP_ERR_HIP;
  }
  // options: initial values from AUVP_<NAME>, read here and nowhere else
  for (int k = 0; k < OPT_COUNT; k++) {
    const std::string name = std::string("AUVP_") + AUVP_OPT_NAMES[k];
    if (const char* e = getenv(name.c_str())) { h->opt.opt_has[k] = true; h->opt.opt_val[k] = atoll(e); }
  }
  if (hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || h->n_cu <= 0) h->n_cu = 256;
  if (hipHostMalloc(reinterpret_cast<void**>(&h->pipe_fail_host), 64, hipHostMallocMapped) == hipSuccess) {
    h->pipe_fail_host[0] = 0;
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&h->pipe_fail_dev), h->pipe_fail_host, 0) != hipSuccess) h->pipe_fail_dev = nullptr;
  } else {
    h->pipe_fail_host = nullptr;
    (void)hipGetLastError();
  }
#ifdef AUVP_PIPE_DIAG
  {
    // diagnostic build only (libauvplan_diag.so): spin limit and delay injection of the speculative pipelines (auvp_wave.h)
    int cfg[8] = {0, 0, 1, 0, 0, 0, 0, 0};
    if (const char* e = getenv("AUVP_DIAG_SPIN")) cfg[0] = atoi(e);
    if (const char* e = getenv("AUVP_DIAG_JITTER")) (void)sscanf(e, "%d,%d,%d,%d,%d", &cfg[1], &cfg[2], &cfg[3], &cfg[4], &cfg[5]);
    if (hipMemcpyToSymbol(HIP_SYMBOL(auvp_diag_cfg), cfg, sizeof cfg) != hipSuccess) { auvp_destroy(h); return AUVP_ERR_HIP; }
    // (a device variable per translation unit: astar_sets_kernels.hip's paired kernel reads its own copy)
    if (auvpi_astar_sets_diag(cfg) != hipSuccess) { auvp_destroy(h); return AUVP_ERR_HIP; }
  }
#endif
  *out = h;
  return AUVP_OK;
}

int auvp_set_option(auvp_handle* h, const char* name, int64_t value) {
  if (!h || !name) return AUVP_ERR_ARG;
  const int k = auvp_option_index(name);
  if (k < 0) return fail(h, AUVP_ERR_ARG, "unknown option %s", name);
  h->opt.opt_has[k] = true; h->opt.opt_val[k] = value;
  return AUVP_OK;
}

int auvp_unset_option(auvp_handle* h, const char* name) {
  if (!h || !name) return AUVP_ERR_ARG;
  const int k = auvp_option_index(name);
  if (k < 0) return fail(h, AUVP_ERR_ARG, "unknown option %s", name);
  h->opt.opt_has[k] = false; h->opt.opt_val[k] = 0;
  return AUVP_OK;
}

int auvp_get_option(auvp_handle* h, const char* name, int32_t* is_set, int64_t* value) {
  if (!h || !name) return AUVP_ERR_ARG;
  const int k = auvp_option_index(name);
  if (k < 0) return fail(h, AUVP_ERR_ARG, "unknown option %s", name);
  if (is_set) *is_set = h->opt.opt_has[k] ? 1 : 0;
  if (value) *value = h->opt.opt_val[k];
  return AUVP_OK;
}

int auvp_pipeline_fallbacks(auvp_handle* h, int32_t* last, int64_t* total) {
  if (!h) return AUVP_ERR_ARG;
  if (last) *last = h->pipe_fallback_last;
  if (total) *total = h->pipe_fallback_total;
  return AUVP_OK;
}

void auvp_destroy(auvp_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->prrt && h->prrt_free) h->prrt_free(h->prrt);
  if (h->astar && h->astar_free) h->astar_free(h->astar);
  if (h->pf && h->pf_free) h->pf_free(h->pf);
  if (h->sf && h->sf_free) h->sf_free(h->sf);
  if (h->comm && h->comm_free) h->comm_free(h->comm);
  if (h->replan && h->replan_free) h->replan_free(h->replan);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->ev_mid) (void)hipEventDestroy(h->ev_mid);
  if (h->ev_pre) (void)hipEventDestroy(h->ev_pre);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  if (h->pipe_fail_host) (void)hipHostFree(h->pipe_fail_host);
  delete h;
}

const char* auvp_last_error(auvp_handle* h) { return h ? h->err.c_str() : "null handle"; }

int auvp_world_set(auvp_handle* h, const double* obstacles, int32_t O, const double* habitats, int32_t H,
                   const double* polygon, int32_t V, const double* bins, int32_t T, const double* cells, int32_t C,
                   const double* prob) {
  if (!h) return AUVP_ERR_ARG;
  if (O < 0 || H < 0 || V < 0 || T < 0 || C < 0) return fail(h, AUVP_ERR_ARG, "negative size");
  if (H > RRT_MAX_HAB) return fail(h, AUVP_ERR_ARG, "n_habitats %d > %d", H, RRT_MAX_HAB);
  if (V > RRT_MAX_POLY) return fail(h, AUVP_ERR_ARG, "n_poly %d > %d", V, RRT_MAX_POLY);
  // a boundary needs at least three vertices (shapely's Polygon constructor raises for fewer); V == 0 means
  // "no boundary" and is accepted for the world-only users (cost probe, A* with its own box)
  if (V == 1 || V == 2) return fail(h, AUVP_ERR_ARG, "boundary polygon with %d vertices (need >= 3, or 0 for none)", V);
  if (T > RRT_MAX_BINS) return fail(h, AUVP_ERR_ARG, "n_bins %d > %d", T, RRT_MAX_BINS);
  HIPCHK(h, hipSetDevice(h->device));
  h->n_sets = 0;  // the probability sets belonged to the world that goes (its bins and cells)
  h->sets_version++;
  h->grids = false;
  WorldIn in;
  in.obstacles = obstacles; in.O = O; in.habitats = habitats; in.H = H; in.polygon = polygon; in.V = V;
  in.bins = bins; in.T = T; in.cells = cells; in.C = C; in.prob = prob;
  in.rg_max_entries = h->opt_num(OPT_RG_MAX_ENTRIES, in.rg_max_entries);
  in.grid_index = !h->opt_on(OPT_NO_GRID_INDEX);
  in.habitat_grid = !h->opt_on(OPT_NO_HABITAT_GRID);
  const WorldTables t = build_world_tables(in);
  // a buffer that grows is released first (DevBuf::reserve): from here to the end WorldDev may point into freed memory
  h->have_world = false;
  int rc = upload_tables(h, {
      {h->d_ox, t.ox}, {h->d_oy, t.oy}, {h->d_ot, t.ot},
      {h->d_osx, t.os_x}, {h->d_osy, t.os_y}, {h->d_ost, t.os_t}, {h->d_osr, t.os_r}, {h->d_osbox, t.os_box},
      {h->d_hab, habitats, (size_t)H * 3}, {h->d_habt, t.hab.hab_t}, {h->d_hgmask, t.hab.hg_mask},
      {h->d_poly, polygon, (size_t)V * 2}, {h->d_bins, bins, (size_t)T * 2}, {h->d_cells, cells, (size_t)C * 4},
      {h->d_prob, prob, (size_t)T * C},
      {h->d_xoff, t.xb_off}, {h->d_xitems, t.xb_items}, {h->d_xdata, t.xb_data},
      {h->d_rgfirst, t.rg_first}, {h->d_rgbp, t.rg_bp}, {h->d_rgoff, t.rg_off}, {h->d_rgpm, t.rg_pm}, {h->d_rgid, t.rg_id},
      {h->d_sgx0, t.sg_x0}, {h->d_sgx1, t.sg_x1}, {h->d_sgy0, t.sg_y0}, {h->d_sgy1, t.sg_y1},
      {h->d_sgcol, t.sg_col}, {h->d_sgrow, t.sg_row},
  });
  if (rc != AUVP_OK) return rc;
  fill_world_dev(h, in, t);
  h->obst_area = t.obst_area;
  // host copies: the A* family derives its own device tables from the same world (astar_host.h)
  h->w_obst.assign(obstacles, obstacles + (size_t)O * 3);
  h->w_hab.assign(habitats, habitats + (size_t)H * 3);
  h->w_poly.assign(polygon, polygon + (size_t)V * 2);
  h->w_bins.assign(bins, bins + (size_t)T * 2);
  h->w_cells.assign(cells, cells + (size_t)C * 4);
  h->w_prob.assign(prob, prob + (size_t)T * C);
  h->world_version++;
  h->have_world = true;
  return AUVP_OK;
}

int auvp_world_set_habitats(auvp_handle* h, const double* habitats, int32_t H) {
  if (!h) return AUVP_ERR_ARG;
  if (!h->have_world) return fail(h, AUVP_ERR_STATE, "auvp_world_set not called");
  if (H < 0 || H > RRT_MAX_HAB) return fail(h, AUVP_ERR_ARG, "n_habitats %d outside 0..%d", H, RRT_MAX_HAB);
  HIPCHK(h, hipSetDevice(h->device));
  const HabitatTables t = build_habitat_tables(habitats, H, !h->opt_on(OPT_NO_HABITAT_GRID));
  // no habitat and no grid until the new tables are in place (a buffer that grows is released first)
  h->W.n_habitats = 0; h->W.hg_n = 0;
  int rc = upload_tables(h, {{h->d_hab, habitats, (size_t)H * 3}, {h->d_habt, t.hab_t}, {h->d_hgmask, t.hg_mask}});
  if (rc != AUVP_OK) return rc;
  fill_habitat_dev(h, H, t);
  h->w_hab.assign(habitats, habitats + (size_t)H * 3);
  h->world_version++;
  return AUVP_OK;
}

int auvp_rrt_explore_batch(auvp_handle* h, int32_t E, const double* init, const uint64_t* seeds,
                           const auvp_rrt_params* p, int32_t flags) {
  int rc = auvp_rrt_prepare(h, E, init, seeds, p, flags);
  if (rc != AUVP_OK) return rc;
  return auvp_rrt_run(h);
}

static int rrt_prepare_impl(auvp_handle* h, int32_t E, const double* init, const uint64_t* seeds, const uint32_t* states,
                            const int32_t* state_index, const auvp_rrt_params* p, int32_t flags, bool lim = false);

int auvp_rrt_prepare(auvp_handle* h, int32_t E, const double* init, const uint64_t* seeds,
                     const auvp_rrt_params* p, int32_t flags) {
  if (!seeds) return h ? fail(h, AUVP_ERR_ARG, "seeds is null") : AUVP_ERR_ARG;
  return rrt_prepare_impl(h, E, init, seeds, nullptr, nullptr, p, flags);
}

int auvp_rrt_prepare_states(auvp_handle* h, int32_t E, const double* init, const uint32_t* mt, const int32_t* mt_index,
                            const auvp_rrt_params* p, int32_t flags) {
  if (!mt || !mt_index) return h ? fail(h, AUVP_ERR_ARG, "mt state is null") : AUVP_ERR_ARG;
  return rrt_prepare_impl(h, E, init, nullptr, mt, mt_index, p, flags);
}

int auvp_rrt_prepare_episodes(auvp_handle* h, int32_t E, const double* init, const uint64_t* seeds, const uint32_t* mt,
                              const int32_t* mt_index, const auvp_rrt_params* p, const auvp_rrt_episode* episodes, int32_t flags) {
  if (!h) return AUVP_ERR_ARG;
  if (E <= 0 || !init || !p || !episodes) return fail(h, AUVP_ERR_ARG, "bad batch arguments");
  if (!seeds && (!mt || !mt_index)) return fail(h, AUVP_ERR_ARG, "neither seeds nor mt states");
  if (p->mode != AUVP_MODE_TIMEBIN) return fail(h, AUVP_ERR_ARG, "per-episode limits need time-bin mode");
  if (flags & (AUVP_FLAG_ITER_LOG | AUVP_FLAG_PHASE_CLOCKS)) return fail(h, AUVP_ERR_ARG, "per-episode limits: no iteration log / phase clocks");
  if (!(p->bin_interval > 0)) return fail(h, AUVP_ERR_ARG, "bin_interval <= 0");
  if (!h->have_world) return fail(h, AUVP_ERR_STATE, "auvp_world_set not called");
  const int H = h->W.n_habitats;
  RrtEpisodeLimits lims = rrt_episode_limits(*p, H, episodes, E);
  if (const int e = lims.bad_episode; e >= 0) {
    if (lims.why == RRT_EPISODE_HORIZON)
      return fail(h, AUVP_ERR_ARG, "episode %d: max_traj_time %g outside (0, %g]", e, episodes[e].max_traj_time, p->max_traj_time);
    if (lims.why == RRT_EPISODE_KEEP) return fail(h, AUVP_ERR_ARG, "episode %d: habitat_keep names habitats >= %d", e, H);
    return fail(h, AUVP_ERR_ARG, "episode %d: max_traj_time / bin_interval = %g does not fit an int", e, episodes[e].max_traj_time / p->bin_interval);
  }
  int rc = rrt_prepare_impl(h, E, init, seeds, seeds ? nullptr : mt, seeds ? nullptr : mt_index, p, flags, true);
  if (rc != AUVP_OK) return rc;
  // the batch is prepared only with its limits on the device: a failed upload leaves nothing a later auvp_rrt_run could launch
  // (it would run every episode at the cap's horizon with the whole habitat list)
  h->prepared = false;
  if ((rc = upload(h, h->d_lim, lims.lim.data(), lims.lim.size()))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->prepared = true;
  h->lim = true;
  h->lim_K.swap(lims.K);
  return AUVP_OK;
}

// the message of a batch the plan refuses (batch_plan.h: one status per refusal)
static int rrt_refuse(auvp_handle* h, const RrtBatchPlan& plan, int n_obstacles) {
  switch (plan.status) {
    case RRT_BATCH_BAD_ARGS: return fail(h, AUVP_ERR_ARG, "bad batch arguments");
    case RRT_BATCH_BAD_PARAMS: return fail(h, AUVP_ERR_ARG, "bad params");
    case RRT_BATCH_BIN_INTERVAL: return fail(h, AUVP_ERR_ARG, "bin_interval <= 0");
    case RRT_BATCH_OBSTACLES: return fail(h, AUVP_ERR_ARG, "n_obstacles %d > 1024", n_obstacles);
    case RRT_BATCH_TOO_MANY_BINS: return fail(h, AUVP_ERR_ARG, "too many time bins (%d)", plan.P.K);
    case RRT_BATCH_POINTS: return fail(h, AUVP_ERR_ARG, "point capacity too large");
    case RRT_BATCH_BIN_LISTS: return fail(h, AUVP_ERR_ARG, "time-bin lists too large (K=%d, max_iter=%d)", plan.P.K, plan.P.max_iter);
    default: return fail(h, AUVP_ERR_ARG, "%s: not a number the batch can be sized from, or too large", plan.field);
  }
}

static int rrt_prepare_impl(auvp_handle* h, int32_t E, const double* init, const uint64_t* seeds, const uint32_t* states,
                            const int32_t* state_index, const auvp_rrt_params* p, int32_t flags, bool lim) {
  if (!h) return AUVP_ERR_ARG;
  h->lim = false;
  h->grids = false;
  if (!h->have_world) return fail(h, AUVP_ERR_STATE, "auvp_world_set not called");
  if (!init || !p) return fail(h, AUVP_ERR_ARG, "bad batch arguments");
  // every capacity and byte count of the batch, or why there is none (batch_plan.h): nothing of the handle changes on a refusal
  RrtBatchIn in;
  in.E = E; in.p = *p; in.flags = flags; in.n_obstacles = h->W.n_obstacles;
  const RrtBatchPlan plan = rrt_batch_plan(in);
  if (plan.status != RRT_BATCH_OK) return rrt_refuse(h, plan, h->W.n_obstacles);
  HIPCHK(h, hipSetDevice(h->device));
  const RrtParamsDev& P = h->P = plan.P;
  h->max_pts = plan.max_pts;
  // the pre-generated random stream of earlier batches (tens of GB, rrt_run_pass) stays with the handle while the batches are of
  // its kind -- a caller alternating between worlds does not pay a hipMalloc per call -- and goes back before a batch of
  // another kind reserves its own buffers
  if (h->d_stream.p && !rrt_stream_keeps(h->opt, P.mode, P.max_iter, lim, rrt_rows_wanted(h->opt, E, h->n_cu))) h->d_stream.release();
  RrtBuffers& B = h->B = plan.B;  // (the capacities; every pointer null until its buffer is reserved below)
  const RrtBatchBytes& bytes = plan.bytes;
  HIPCHK(h, h->d_nodes_f.reserve(bytes.nodes_f));
  HIPCHK(h, h->d_nodes_i.reserve(bytes.nodes_i));
  HIPCHK(h, h->d_points.reserve(bytes.points));
  HIPCHK(h, h->d_bin_items.reserve(bytes.bin_items));
  HIPCHK(h, h->d_bin_count.reserve(bytes.bin_count));
  HIPCHK(h, h->d_summary.reserve(bytes.summary));
  HIPCHK(h, h->d_node_c.reserve(bytes.node_c));
  HIPCHK(h, h->d_node_q.reserve(bytes.node_q));
  B.node_f = h->d_nodes_f.as<double>();
  B.node_i = h->d_nodes_i.as<int32_t>();
  B.points = h->d_points.as<double>();
  B.node_c = h->d_node_c.as<int32_t>();
  B.node_q = h->d_node_q.as<uint8_t>();
  // nearest-neighbour sampling scans a contiguous x,y mirror of the nodes (auvp_types.h); the other modes never touch it
  if (P.mode == AUVP_MODE_NN) {
    HIPCHK(h, h->d_node_xy.reserve(bytes.node_xy));
    B.node_xy = h->d_node_xy.as<double>();
  }
  B.bin_items = h->d_bin_items.as<int32_t>();
  B.bin_count = h->d_bin_count.as<int32_t>();
  B.summary = h->d_summary.as<RrtSummary>();
  if (flags & AUVP_FLAG_ITER_LOG) {
    HIPCHK(h, h->d_itlog_i.reserve(bytes.itlog_i));
    HIPCHK(h, h->d_itlog_b.reserve(bytes.itlog_b));
    B.it_parent = h->d_itlog_i.as<int32_t>();
    B.it_npath = B.it_parent + plan.itlog_n;
    B.it_accepted = h->d_itlog_b.as<int8_t>();
  }
  if (flags & AUVP_FLAG_LEAF_LOG) {
    HIPCHK(h, h->d_leaf_c.reserve(bytes.leaf_c));
    HIPCHK(h, h->d_leaf_i.reserve(bytes.leaf_i));
    B.leaf_cost = h->d_leaf_c.as<double>();
    B.leaf_iter = h->d_leaf_i.as<int32_t>();
  }
  HIPCHK(h, h->d_leaf_stats.reserve(bytes.leaf_stats));
  B.leaf_stats = h->d_leaf_stats.as<unsigned long long>();
  B.pipe_fail = h->pipe_fail_dev;
  if (flags & AUVP_FLAG_PHASE_CLOCKS) {
    HIPCHK(h, h->d_phase.reserve(bytes.phase));
    HIPCHK(h, hipMemsetAsync(h->d_phase.p, 0, bytes.phase, h->stream));
    B.phase_clocks = h->d_phase.as<unsigned long long>();
  }
  // seeds -> MT states, once per batch: random.seed(seeds[e]) on the device (auvp_seed.h)
  int rc;
  if (seeds) {
    HIPCHK(h, h->d_mt.reserve(bytes.mt));
    if ((rc = upload(h, h->d_seeds, seeds, (size_t)E))) return rc;
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(auvp::mt_seed_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  auvp::MT_SEED_LDS));
    hipLaunchKernelGGL(auvp::mt_seed_kernel, dim3((E + 63) / 64), dim3(64), auvp::MT_SEED_LDS, h->stream,
                       h->d_seeds.as<unsigned long long>(), h->d_mt.as<uint32_t>(), (int32_t*)nullptr, (int)E);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
  } else {
    if ((rc = upload(h, h->d_mt, states, (size_t)E * 624))) return rc;
    if ((rc = upload(h, h->d_mtidx, state_index, (size_t)E))) return rc;
    B.mt_index = h->d_mtidx.as<int32_t>();
  }
  if ((rc = upload(h, h->d_init, init, (size_t)E * 6))) return rc;
  B.mt = h->d_mt.as<uint32_t>();
  B.init = h->d_init.as<double>();
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->E = E;
  h->prepared = true;
  h->have_batch = false;
  h->have_group = false;
  return AUVP_OK;
}

}  // extern "C"

// 1: the buffer of the pre-generated random stream (rrt_stream_kernel.h) holds `bytes`; 0: it does not fit the free memory beside
// a 4 GB margin (or the allocation failed).  How much a buffer that has to grow takes: rrt_stream_want_bytes (batch_plan.h).
// *grew: an allocation happened (the caller re-records its start event: nothing has been launched yet)
static int rrt_stream_reserve(auvp_handle* h, size_t bytes, bool* grew = nullptr) {
  if (grew) *grew = false;
  if (h->d_stream.cap >= bytes) return 1;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return 0; }
  const size_t want = rrt_stream_want_bytes(free_b, h->d_stream.cap, bytes);
  if (!want || h->d_stream.reserve(want) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  if (grew) *grew = true;
  return 1;
}

// one kernel launch at the plan's shape
template <class Kern, class... Args>
static hipError_t launch_kernel(Kern kern, int grid, int block, int lds, hipStream_t stream, const Args&... args) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, stream, args...);
  return hipGetLastError();
}

// the expansion launch the plan names.  PR: the parameters with the plan's kernel flags
static hipError_t rrt_launch_expansion(auvp_handle* h, const RrtLaunchPlan& plan, const RrtParamsDev& PR) {
  const RrtBuffers& B = h->B;
  const int E = h->E, O = h->W.n_obstacles, max_pts = h->max_pts;
  auto launch = [&](auto kern, const auto&... more) { return launch_kernel(kern, plan.grid, plan.block, plan.lds, h->stream, h->W, PR, B, E, more...); };
  switch (plan.kind) {
    case RRT_TRIO:
      return for_obstacle_J<4>(O, [&](auto j) {
        constexpr int J = decltype(j)::value;
        return plan.quad ? launch(rrt_trio_kernel<J, 4>) : launch(rrt_trio_kernel<J, 3>);
      });
    case RRT_DUO:
      return for_obstacle_J<4>(O, [&](auto j) { return launch(rrt_duo_kernel<decltype(j)::value>, max_pts); });
    case RRT_ROWS:  // (rows_kernels.hip)
      return auvpi_rrt_rows_launch(&h->W, &PR, &B, E, plan.grid, plan.block, plan.lds_max, plan.lds, h->stream);
    case RRT_ROWS_STREAM: {
      RrtBuffers Bs = B;
      Bs.stream = h->d_stream.as<double>();
      Bs.stream_cap = plan.stream_len;
      hipError_t e = auvpi_rrt_stream_launch(&Bs, E, h->stream);
      if (e == hipSuccess) e = hipEventRecord(h->ev_pre, h->stream);
      if (e == hipSuccess) e = auvpi_rrt_rows_stream_launch(&h->W, &PR, &Bs, E, plan.grid, plan.block, plan.lds_max, plan.lds, plan.mirror, h->stream);
      return e;
    }
    case RRT_EXPLORE_LIM:
      return for_obstacle_J<16>(O, [&](auto j) { return launch(rrt_explore_lim_kernel<decltype(j)::value>, max_pts, h->d_lim.as<RrtEpisodeLimDev>()); });
    case RRT_EXPLORE:
      break;
  }
  // compile-time specialisation: obstacles per lane (J), parent-sampling mode, diagnostics on/off
  const bool diag = (PR.flags & (AUVP_FLAG_ITER_LOG | AUVP_FLAG_LEAF_LOG | AUVP_FLAG_PHASE_CLOCKS)) != 0;
  return for_obstacle_J<16>(O, [&](auto j) {
    constexpr int J = decltype(j)::value;
    if (PR.mode == 0) return diag ? launch(rrt_explore_kernel<J, 0, true>, max_pts) : launch(rrt_explore_kernel<J, 0, false>, max_pts);
    if (PR.mode == 1) return diag ? launch(rrt_explore_kernel<J, 1, true>, max_pts) : launch(rrt_explore_kernel<J, 1, false>, max_pts);
    return diag ? launch(rrt_explore_kernel<J, 2, true>, max_pts) : launch(rrt_explore_kernel<J, 2, false>, max_pts);
  });
}

// the trees are complete: rank the qualifying leaves (same stream, inside the timed region)
static int rrt_launch_leaf(auvp_handle* h) {
  const RrtBuffers& B = h->B;
  const int E = h->E;
  // dynamic LDS of the leaf pass: the separable-grid edge tables + one "ancestor of a qualifying leaf" bit per node
  // and episode (trees too large for that are swept whole)
  const int gl = rrt_leaf_grid_lds_bytes(h->W.sg_enabled, h->W.sg_ncol, h->W.sg_nrow);
  // (option LEAF_SWEEP_ALL: no pruning, every node visited -- what trees of more than 131 072 nodes get; for tests)
  const int bm_words = h->opt_on(OPT_LEAF_SWEEP_ALL) ? 0 : rrt_leaf_mark_words(B.cap_nodes);
  const int dyn = gl + RRT_LEAF_WAVES * bm_words * 4;
  const int grid = (E + RRT_LEAF_WAVES - 1) / RRT_LEAF_WAVES;
  if (h->grids)
    HIPCHK(h, auvpi_rrt_leaf_grid_launch(&h->W, &h->P, &B, E, bm_words, h->d_lim.as<RrtEpisodeLimDev>(), h->d_set_of.as<int32_t>(),
                                         h->d_sets_rec.as<RrtProbSetDev>(), grid, RRT_LEAF_WAVES * 64, dyn, h->stream));
  else if (h->lim) HIPCHK(h, launch_kernel(rrt_leaf_lim_kernel, grid, RRT_LEAF_WAVES * 64, dyn, h->stream, h->W, h->P, B, E, bm_words, h->d_lim.as<RrtEpisodeLimDev>()));
  else HIPCHK(h, launch_kernel(rrt_leaf_kernel, grid, RRT_LEAF_WAVES * 64, dyn, h->stream, h->W, h->P, B, E, bm_words));
  return AUVP_OK;
}

// what the pass that just completed drew (the most 32-bit outputs of one episode, in the mapped page beside the pipeline flag):
// kept per parameter block for the length of the next batch's stream
static void rrt_record_drawn(auvp_handle* h, const RrtLaunchPlan& plan) {
  const RrtParamsDev& P = h->P;
  unsigned long long d32 = 0;
  memcpy(&d32, h->pipe_fail_host + 2, sizeof d32);
  if (d32 == 0) return;
  const DrawnMemory::Slot& d = h->drawn.record(P, (long long)((d32 + 1) / 2), h->E);
  // the next batch with these parameters will want its stream: the buffer is taken NOW, in the call that found
  // out (tens of GB: a second of hipMalloc that a later, timed call would pay otherwise)
  if (rrt_stream_keeps(h->opt, P.mode, P.max_iter, h->lim, plan.kind == RRT_ROWS)) {
    const long long cap_next = rrt_stream_len(h->opt, d.most, P.max_iter);
    if (cap_next <= 0x7fffffffll) (void)rrt_stream_reserve(h, (size_t)h->E * (size_t)cap_next * sizeof(double));
  }
}

// HIP-event times of the pass: whole, [stream generator,] expansion, leaf
static int rrt_record_times(auvp_handle* h, bool stream_launched) {
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  h->last_ms = ms;
  HIPCHK(h, hipEventElapsedTime(&ms, stream_launched ? h->ev_pre : h->ev0, h->ev_mid));
  h->last_expand_ms = ms;
  if (stream_launched) {
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev_pre));
    h->last_stream_ms = ms;
  }
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev_mid, h->ev1));
  h->last_leaf_ms = ms;
  return AUVP_OK;
}

// one pass over the prepared batch: the expansion launch rrt_choose_launch names (launch_plan.h) + the leaf pass.
// one_wave_only: never a speculative pipeline; no_stream: the random numbers are generated inside the expansion kernel whatever
// option ROWS_STREAM says (the stream fallback)
static int rrt_run_pass(auvp_handle* h, bool one_wave_only, bool no_stream = false) {
  const RrtParamsDev& P = h->P;
  const RrtBuffers& B = h->B;
  const int E = h->E;
  RrtLaunchIn in;
  in.E = E; in.n_cu = h->n_cu;
  in.mode = P.mode; in.max_iter = P.max_iter; in.K = P.K; in.flags = P.flags; in.freq = P.freq; in.dist_to_end = P.dist_to_end;
  in.max_pts = h->max_pts;
  in.O = h->W.n_obstacles; in.H = h->W.n_habitats; in.V = h->W.n_poly; in.T = h->W.n_bins; in.obst_area = h->obst_area;
  in.lim = h->lim; in.one_wave_only = one_wave_only; in.no_stream = no_stream;
  if (const DrawnMemory::Slot* seen = h->drawn.find(P)) { in.seen_most = seen->most; in.seen_E = seen->E; }
  RrtLaunchPlan plan = rrt_choose_launch(in, h->opt);
  h->last_stream_mirror = -1;
  h->last_stream_ms = 0.0;
  h->last_stream_len = 0;
  if (plan.status == PLAN_LDS_ONE_WAVE)
    return fail(h, AUVP_ERR_ARG, "LDS need %zu B > 160 KiB (K=%d, freq=%d)", (size_t)plan.lds_need, P.K, (int)std::floor(P.freq));
  if (plan.status != PLAN_OK) return fail(h, AUVP_ERR_ARG, "LDS need %d B > 160 KiB (K=%d)", (int)plan.lds_need, P.K);
  if (B.leaf_stats) HIPCHK(h, hipMemsetAsync(B.leaf_stats, 0, 8 * sizeof(unsigned long long), h->stream));  // (before the timed region)
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  if (plan.kind == RRT_ROWS_STREAM) {
    const size_t bytes = (size_t)E * (size_t)plan.stream_len * sizeof(double);
    bool grew = false;
    if (!rrt_stream_reserve(h, bytes, &grew)) {
      if (h->opt_on(OPT_ROWS_STREAM)) return fail(h, AUVP_ERR_CAPACITY, "ROWS_STREAM = 1: %zu bytes of random stream do not fit the free memory", bytes);
      in.no_stream = true;
      plan = rrt_choose_launch(in, h->opt);
    }
    if (grew) HIPCHK(h, hipEventRecord(h->ev0, h->stream));  // (the allocation is not part of the pass's time: nothing was launched yet)
  }
  const bool stream_launched = plan.kind == RRT_ROWS_STREAM;
  if (stream_launched) { h->last_stream_mirror = plan.mirror; h->last_stream_len = plan.stream_len; }
  h->last_rrt_kernel = plan.name;
  RrtParamsDev PR = P;
  PR.flags |= plan.kflags;
  HIPCHK(h, rrt_launch_expansion(h, plan, PR));
  HIPCHK(h, hipEventRecord(h->ev_mid, h->stream));
  int rc = rrt_launch_leaf(h);
  if (rc != AUVP_OK) return rc;
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  // (the most 32-bit outputs one episode drew: eight bytes into the mapped page beside the pipeline flag)
  // (not from a batch with per-episode limits: the figure sizes streams of plain batches with the same parameter block)
  const bool want_drawn = B.leaf_stats && h->pipe_fail_host && !h->lim;
  if (want_drawn) HIPCHK(h, hipMemcpyAsync(h->pipe_fail_host + 2, B.leaf_stats + 4, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (want_drawn && !h->pipe_failed()) rrt_record_drawn(h, plan);
  if ((rc = rrt_record_times(h, stream_launched))) return rc;
  h->last_rows = plan.rows() ? 1 : 0;
  h->last_grid = plan.grid; h->last_block = plan.block; h->last_lds = plan.lds;
  h->have_batch = true;
  return AUVP_OK;
}

// AUVP_ERR_PIPELINE episodes of the pass that just ran (its mapped flag is set): counted from the summaries
static int rrt_count_pipeline_failures(auvp_handle* h, int* n, int* n_stream) {
  std::vector<RrtSummary> s((size_t)h->E);
  HIPCHK(h, hipMemcpy(s.data(), h->B.summary, s.size() * sizeof(RrtSummary), hipMemcpyDeviceToHost));
  *n = 0;
  *n_stream = 0;
  for (const RrtSummary& r : s) { *n += r.status == AUVP_ERR_PIPELINE ? 1 : 0; *n_stream += r.status == AUVP_ERR_STREAM ? 1 : 0; }
  return AUVP_OK;
}

extern "C" {

int auvp_rrt_run(auvp_handle* h) {
  if (!h) return AUVP_ERR_ARG;
  if (!h->prepared) return fail(h, AUVP_ERR_STATE, "auvp_rrt_prepare not called");
  HIPCHK(h, hipSetDevice(h->device));
  h->have_group = false;
  h->pipe_clear();
  h->pipe_fallback_last = 0;
  int rc = rrt_run_pass(h, false);
  if (rc != AUVP_OK || !h->pipe_failed()) return rc;
  // a speculative pipeline gave up on some episode: the batch starts from its prepared state in every pass, so the whole
  // pass is repeated on the one-wavefront kernel (option PIPE_FALLBACK = 0: leave the status in the summaries instead)
  int n = 0, n_stream = 0;
  if ((rc = rrt_count_pipeline_failures(h, &n, &n_stream))) return rc;
  h->pipe_clear();
  if (n + n_stream == 0 || !h->opt_flag(OPT_PIPE_FALLBACK, true)) return AUVP_OK;
  h->pipe_fallback_last = n + n_stream;
  h->pipe_fallback_total += n + n_stream;
  const double first_ms = h->last_ms;
  // (episodes that ran past their pre-generated random stream: the same kernel shape with the generator inside; a pipeline that
  // gave up: the one-wavefront kernel)
  rc = n_stream > 0 ? rrt_run_pass(h, false, true) : rrt_run_pass(h, true);
  h->last_ms += first_ms;  // (the time the caller waited)
  return rc;
}

int auvp_world_set_prob_sets(auvp_handle* h, int32_t n_sets, const double* prob_host, const void* prob_dev) {
  if (!h) return AUVP_ERR_ARG;
  h->sets_version++;
  if (n_sets == 0 && !prob_host && !prob_dev) {
    h->n_sets = 0;
    h->grids = false;
    return AUVP_OK;
  }
  if (n_sets < 1) return fail(h, AUVP_ERR_ARG, "n_sets %d < 1", n_sets);
  if ((prob_host != nullptr) == (prob_dev != nullptr)) return fail(h, AUVP_ERR_ARG, "exactly one of prob_host and prob_dev must be given");
  if (!h->have_world || h->W.n_bins < 1 || h->W.n_cells < 1)
    return fail(h, AUVP_ERR_STATE, "probability sets need a world with time bins and cells (auvp_world_set)");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t n = (size_t)h->W.n_bins * (size_t)h->W.n_cells, bytes = (size_t)n_sets * n * sizeof(double);
  h->n_sets = 0;
  h->grids = false;  // (an assignment was checked against the sets that go)
  HIPCHK(h, h->d_sets_prob.reserve(bytes));
  HIPCHK(h, h->d_sets_rec.reserve((size_t)n_sets * sizeof(RrtProbSetDev)));
  if (prob_host) HIPCHK(h, hipMemcpyAsync(h->d_sets_prob.p, prob_host, bytes, hipMemcpyHostToDevice, h->stream));
  else HIPCHK(h, hipMemcpyAsync(h->d_sets_prob.p, prob_dev, bytes, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, auvpi_prob_set_stats_launch(h->d_sets_prob.as<double>(), (long long)n, n_sets, h->d_sets_rec.as<RrtProbSetDev>(), h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->n_sets = n_sets;
  return AUVP_OK;
}

int auvp_world_set_prob_sets_placed(auvp_handle* h, const void* prob_dev, int32_t n_sets, int32_t n_rounds1, int32_t n_cells, int32_t first_bin) {
  if (!h) return AUVP_ERR_ARG;
  if (!prob_dev || n_sets < 1 || n_rounds1 < 1) return fail(h, AUVP_ERR_ARG, "need prob_dev, n_sets >= 1 and a forecast of >= 1 rounds");
  if (!h->have_world || h->W.n_bins < 1 || h->W.n_cells < 1)
    return fail(h, AUVP_ERR_STATE, "probability sets need a world with time bins and cells (auvp_world_set)");
  if (n_cells != h->W.n_cells) return fail(h, AUVP_ERR_ARG, "the forecast has %d cells, the world %d", n_cells, h->W.n_cells);
  const int T = h->W.n_bins;
  const SfPlacePlan plan = placed_round_of_bin(T, n_rounds1 - 1, first_bin);
  if (plan.status == SF_PLACE_BAD_BIN) return fail(h, AUVP_ERR_ARG, "first_bin %d outside 0 .. %d", first_bin, T - 1);
  if (plan.status != SF_PLACE_OK) return fail(h, AUVP_ERR_ARG, "bad shape");
  if ((long long)n_sets * T > 0x7fffffffll) return fail(h, AUVP_ERR_CAPACITY, "%d sets x %d bins: more than 2^31 - 1 rows", n_sets, T);
  if (plan.identity) return auvp_world_set_prob_sets(h, n_sets, nullptr, prob_dev);  // (the tables as they lie: one copy, no gather)
  h->sets_version++;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t n = (size_t)T * (size_t)n_cells, bytes = (size_t)n_sets * n * sizeof(double);
  h->n_sets = 0;
  h->grids = false;  // (an assignment was checked against the sets that go)
  HIPCHK(h, h->d_sets_prob.reserve(bytes));
  HIPCHK(h, h->d_sets_rec.reserve((size_t)n_sets * sizeof(RrtProbSetDev)));
  HIPCHK(h, auvpi_sf_place_launch(static_cast<const double*>(prob_dev), h->d_sets_prob.as<double>(), n_sets, T, n_rounds1, n_cells, first_bin,
                                  h->stream));
  HIPCHK(h, auvpi_prob_set_stats_launch(h->d_sets_prob.as<double>(), (long long)n, n_sets, h->d_sets_rec.as<RrtProbSetDev>(), h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->n_sets = n_sets;
  return AUVP_OK;
}

int auvp_world_prob_set_stats(auvp_handle* h, double* absmax, int32_t* one_sign) {
  if (!h) return AUVP_ERR_ARG;
  if (h->n_sets < 1) return fail(h, AUVP_ERR_STATE, "no probability sets on this handle");
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<RrtProbSetDev> rec((size_t)h->n_sets);
  HIPCHK(h, hipMemcpyAsync(rec.data(), h->d_sets_rec.p, rec.size() * sizeof(RrtProbSetDev), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int g = 0; g < h->n_sets; g++) {
    if (absmax) absmax[g] = rec[(size_t)g].absmax;
    if (one_sign) one_sign[g] = rec[(size_t)g].one_sign;
  }
  return AUVP_OK;
}

int auvp_world_prob_sets_read(auvp_handle* h, int32_t* n_sets, double* prob) {
  if (!h) return AUVP_ERR_ARG;
  if (h->n_sets < 1) return fail(h, AUVP_ERR_STATE, "no probability sets on this handle");
  if (n_sets) *n_sets = h->n_sets;
  if (!prob) return AUVP_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t bytes = (size_t)h->n_sets * (size_t)h->W.n_bins * (size_t)h->W.n_cells * sizeof(double);
  HIPCHK(h, hipMemcpyAsync(prob, h->d_sets_prob.p, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return AUVP_OK;
}

int auvp_rrt_set_episode_grids(auvp_handle* h, int32_t n_episodes, const int32_t* set_of) {
  if (!h) return AUVP_ERR_ARG;
  if (!set_of) {
    h->grids = false;
    return AUVP_OK;
  }
  if (!h->prepared || !h->lim) return fail(h, AUVP_ERR_STATE, "the batch was not prepared by auvp_rrt_prepare_episodes");
  if (h->n_sets < 1) return fail(h, AUVP_ERR_STATE, "no probability sets on this handle (auvp_world_set_prob_sets)");
  if (n_episodes != h->E) return fail(h, AUVP_ERR_ARG, "n_episodes %d, the prepared batch has %d", n_episodes, h->E);
  for (int e = 0; e < n_episodes; e++)
    if (set_of[e] < 0 || set_of[e] >= h->n_sets) return fail(h, AUVP_ERR_ARG, "episode %d: set %d outside [0, %d)", e, set_of[e], h->n_sets);
  HIPCHK(h, hipSetDevice(h->device));
  h->grids = false;
  int rc = upload(h, h->d_set_of, set_of, (size_t)n_episodes);
  if (rc != AUVP_OK) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->grids = true;
  return AUVP_OK;
}

int auvp_rrt_rerank(auvp_handle* h) {
  if (!h) return AUVP_ERR_ARG;
  if (!h->prepared || !h->have_batch) return fail(h, AUVP_ERR_STATE, "no run has completed since the batch was prepared");
  HIPCHK(h, hipSetDevice(h->device));
  h->have_group = false;
  // the leaf pass alone: it rewrites node_f[6..7], node_c and the summaries' leaf fields from the tree, which it leaves as it is
  if (h->B.leaf_stats) HIPCHK(h, hipMemsetAsync(h->B.leaf_stats, 0, 8 * sizeof(unsigned long long), h->stream));
  HIPCHK(h, hipEventRecord(h->ev_mid, h->stream));
  int rc = rrt_launch_leaf(h);
  if (rc != AUVP_OK) return rc;
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev_mid, h->ev1));
  h->last_leaf_ms = ms;
  h->last_ms = ms;
  return AUVP_OK;
}

int auvp_rrt_summaries(auvp_handle* h, auvp_rrt_summary* out) {
  if (!h || !out) return AUVP_ERR_ARG;
  if (!h->have_batch) return fail(h, AUVP_ERR_STATE, "no batch has run");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(out, h->B.summary, (size_t)h->E * sizeof(RrtSummary), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return AUVP_OK;
}

void* auvp_rrt_summaries_dev(auvp_handle* h) { return (h && h->have_batch) ? (void*)h->B.summary : nullptr; }

int auvp_rrt_paths_dev(auvp_handle* h, const int64_t* offsets, void* out_dev) {
  if (!h || !offsets || !out_dev) return AUVP_ERR_ARG;
  if (!h->have_batch) return fail(h, AUVP_ERR_STATE, "no batch has run");
  HIPCHK(h, hipSetDevice(h->device));
  const int E = h->E;
  HIPCHK(h, h->d_tmp0.reserve((size_t)(E + 1) * sizeof(int64_t)));
  HIPCHK(h, hipMemcpyAsync(h->d_tmp0.p, offsets, (size_t)(E + 1) * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(rrt_final_course_kernel, dim3(E), dim3(64), 0, h->stream, h->B, h->d_tmp0.as<int64_t>(),
                     reinterpret_cast<double*>(out_dev), E);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return AUVP_OK;
}

int auvp_rrt_paths(auvp_handle* h, const int64_t* offsets, double* out) {
  if (!h || !offsets || !out) return AUVP_ERR_ARG;
  if (!h->have_batch) return fail(h, AUVP_ERR_STATE, "no batch has run");
  const size_t total = (size_t)offsets[h->E];
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->d_tmp1.reserve(std::max<size_t>(total, 1) * 7 * sizeof(double)));
  int rc = auvp_rrt_paths_dev(h, offsets, h->d_tmp1.p);
  if (rc != AUVP_OK) return rc;
  if (total) HIPCHK(h, hipMemcpyAsync(out, h->d_tmp1.p, total * 7 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return AUVP_OK;
}

int auvp_rrt_group_best(auvp_handle* h, int32_t G, const int32_t* group_off, struct auvp_rrt_group_best* out) {
  if (!h) return AUVP_ERR_ARG;
  if (!h->have_batch) return fail(h, AUVP_ERR_STATE, "no batch has run");
  if (G < 1 || !group_off) return fail(h, AUVP_ERR_ARG, "bad group arguments");
  const int E = h->E;
  if (G > E || group_off[0] != 0 || group_off[G] != E) return fail(h, AUVP_ERR_ARG, "the groups do not partition the batch of %d", E);
  for (int g = 0; g < G; g++)
    if (group_off[g + 1] <= group_off[g]) return fail(h, AUVP_ERR_ARG, "group %d is empty or out of order", g);
  HIPCHK(h, hipSetDevice(h->device));
  h->have_group = false;
  int rc = upload(h, h->d_group_off, group_off, (size_t)G + 1);
  if (rc != AUVP_OK) return rc;
  HIPCHK(h, h->d_group_best.reserve((size_t)G * sizeof(RrtGroupBest)));
  hipLaunchKernelGGL(rrt_group_best_kernel, dim3((G + RRT_GROUP_WAVES - 1) / RRT_GROUP_WAVES), dim3(RRT_GROUP_WAVES * 64), 0,
                     h->stream, h->B.summary, h->d_group_off.as<int32_t>(), h->d_group_best.as<RrtGroupBest>(), (int)G);
  HIPCHK(h, hipGetLastError());
  h->group_best.resize((size_t)G);
  HIPCHK(h, hipMemcpyAsync(h->group_best.data(), h->d_group_best.p, (size_t)G * sizeof(RrtGroupBest), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (out) memcpy(out, h->group_best.data(), (size_t)G * sizeof(RrtGroupBest));
  h->have_group = true;
  return AUVP_OK;
}

void* auvp_rrt_group_best_dev(auvp_handle* h) { return (h && h->have_batch && h->have_group) ? h->d_group_best.p : nullptr; }

int auvp_rrt_group_paths_dev(auvp_handle* h, const int64_t* offsets, void* out_dev) {
  if (!h || !offsets || !out_dev) return AUVP_ERR_ARG;
  if (!h->have_batch) return fail(h, AUVP_ERR_STATE, "no batch has run");
  if (!h->have_group) return fail(h, AUVP_ERR_STATE, "auvp_rrt_group_best not called for this batch");
  const int G = (int)h->group_best.size();
  if (offsets[0] < 0) return fail(h, AUVP_ERR_ARG, "offsets[0] < 0");
  for (int g = 0; g < G; g++) {
    const RrtGroupBest& r = h->group_best[(size_t)g];
    const int64_t need = r.winner >= 0 ? (int64_t)r.path_len : 0;
    if (offsets[g + 1] - offsets[g] < need) return fail(h, AUVP_ERR_ARG, "group %d: the offsets leave fewer rows than its course of %lld", g, (long long)need);
  }
  HIPCHK(h, hipSetDevice(h->device));
  int rc = upload(h, h->d_group_pos, offsets, (size_t)G + 1);
  if (rc != AUVP_OK) return rc;
  hipLaunchKernelGGL(rrt_group_course_kernel, dim3(G), dim3(64), 0, h->stream, h->B, h->d_group_best.as<RrtGroupBest>(),
                     h->d_group_pos.as<int64_t>(), reinterpret_cast<double*>(out_dev), G, h->E);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return AUVP_OK;
}

int auvp_rrt_group_paths(auvp_handle* h, const int64_t* offsets, double* out) {
  if (!h || !offsets || !out) return AUVP_ERR_ARG;
  if (!h->have_batch) return fail(h, AUVP_ERR_STATE, "no batch has run");
  if (!h->have_group) return fail(h, AUVP_ERR_STATE, "auvp_rrt_group_best not called for this batch");
  const int64_t last = offsets[h->group_best.size()];
  if (last < 0) return fail(h, AUVP_ERR_ARG, "negative offsets");
  const size_t total = (size_t)last;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->d_tmp1.reserve(std::max<size_t>(total, 1) * 7 * sizeof(double)));
  int rc = auvp_rrt_group_paths_dev(h, offsets, h->d_tmp1.p);
  if (rc != AUVP_OK) return rc;
  if (total) HIPCHK(h, hipMemcpyAsync(out, h->d_tmp1.p, total * 7 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return AUVP_OK;
}

int auvp_rrt_tree(auvp_handle* h, int32_t ep, double* nodes6, int32_t* parent, int32_t* pt_off, int32_t* pt_cnt,
                  double* points7) {
  if (!h) return AUVP_ERR_ARG;
  if (!h->have_batch || ep < 0 || ep >= h->E) return fail(h, AUVP_ERR_STATE, "bad episode");
  HIPCHK(h, hipSetDevice(h->device));
  RrtSummary s;
  HIPCHK(h, hipMemcpy(&s, h->B.summary + ep, sizeof s, hipMemcpyDeviceToHost));
  const RrtBuffers& B = h->B;
  const int N = s.n_nodes, NP = s.n_points;
  const size_t capp = (size_t)B.cap_points;
  std::vector<double> nf((size_t)N * 8);
  std::vector<int32_t> ni((size_t)N * 4);
  HIPCHK(h, hipMemcpy(nf.data(), B.node_f + (size_t)ep * B.cap_nodes * 8, nf.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(ni.data(), B.node_i + (size_t)ep * B.cap_nodes * 4, ni.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int i = 0; i < N; i++) {
    if (nodes6) {
      double* d = nodes6 + 6 * (size_t)i;
      const double* f = nf.data() + 8 * (size_t)i;
      d[0] = f[0]; d[1] = f[1]; d[2] = f[2]; d[3] = f[3]; d[4] = (double)ni[4 * (size_t)i]; d[5] = f[4];
    }
    if (parent) parent[i] = ni[4 * (size_t)i + 1];
    if (pt_off) pt_off[i] = ni[4 * (size_t)i + 2];
    if (pt_cnt) pt_cnt[i] = ni[4 * (size_t)i + 3];
  }
  if (points7 && NP > 0) {
    // the points live in two 24-byte record arrays per episode: {x, y, traj_t} and {theta, v, length}
    std::vector<double> ra((size_t)NP * 3), rb((size_t)NP * 3);
    HIPCHK(h, hipMemcpy(ra.data(), B.points + (size_t)ep * 6 * capp, ra.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(rb.data(), B.points + (size_t)ep * 6 * capp + 3 * capp, rb.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < NP; i++) {
      double* d = points7 + 7 * (size_t)i;
      d[0] = ra[3 * (size_t)i]; d[1] = ra[3 * (size_t)i + 1]; d[2] = rb[3 * (size_t)i]; d[3] = rb[3 * (size_t)i + 1];
      d[4] = ra[3 * (size_t)i + 2]; d[6] = rb[3 * (size_t)i + 2];
    }
    // plan_time_stamp of a path point = iteration of the node that owns it
    for (int m = 0; m < N; m++) {
      const int off = ni[4 * (size_t)m + 2], cnt = ni[4 * (size_t)m + 3], plan = ni[4 * (size_t)m];
      for (int k = 0; k < cnt; k++) points7[7 * (size_t)(off + k) + 5] = (double)plan;
    }
  }
  return AUVP_OK;
}

int auvp_rrt_iter_log(auvp_handle* h, int32_t ep, int32_t* it_parent, int8_t* it_accepted, int32_t* it_npath) {
  if (!h) return AUVP_ERR_ARG;
  if (!h->have_batch || ep < 0 || ep >= h->E || !h->B.it_parent) return fail(h, AUVP_ERR_STATE, "no iteration log");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t n = h->P.max_iter, o = (size_t)ep * n;
  if (it_parent) HIPCHK(h, hipMemcpy(it_parent, h->B.it_parent + o, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (it_accepted) HIPCHK(h, hipMemcpy(it_accepted, h->B.it_accepted + o, n, hipMemcpyDeviceToHost));
  if (it_npath) HIPCHK(h, hipMemcpy(it_npath, h->B.it_npath + o, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return AUVP_OK;
}

int auvp_rrt_leaf_log(auvp_handle* h, int32_t ep, double* leaf_cost6, int32_t* leaf_iter) {
  if (!h) return AUVP_ERR_ARG;
  if (!h->have_batch || ep < 0 || ep >= h->E || !h->B.leaf_cost) return fail(h, AUVP_ERR_STATE, "no leaf log");
  HIPCHK(h, hipSetDevice(h->device));
  RrtSummary s;
  HIPCHK(h, hipMemcpy(&s, h->B.summary + ep, sizeof s, hipMemcpyDeviceToHost));
  const size_t n = std::min(s.n_leaves, h->B.cap_leaves), o = (size_t)ep * h->B.cap_leaves;
  if (leaf_cost6 && n) HIPCHK(h, hipMemcpy(leaf_cost6, h->B.leaf_cost + o * 6, n * 6 * sizeof(double), hipMemcpyDeviceToHost));
  if (leaf_iter && n) HIPCHK(h, hipMemcpy(leaf_iter, h->B.leaf_iter + o, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return AUVP_OK;
}

int auvp_rrt_bin_sizes(auvp_handle* h, int32_t ep, int32_t* sizes, int32_t* n_bins) {
  if (!h) return AUVP_ERR_ARG;
  if (!h->have_batch || ep < 0 || ep >= h->E) return fail(h, AUVP_ERR_STATE, "bad episode");
  HIPCHK(h, hipSetDevice(h->device));
  const int K = h->lim ? h->lim_K[(size_t)ep] : h->P.K;  // (per-episode limits: the episode's own K; the rows are the cap's)
  if (n_bins) *n_bins = K;
  if (sizes && K > 0)
    HIPCHK(h, hipMemcpy(sizes, h->B.bin_count + (size_t)ep * (h->P.K + 1) + 1, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost));
  return AUVP_OK;
}

int auvp_rrt_phase_clocks(auvp_handle* h, uint64_t* out) {
  if (!h || !out) return AUVP_ERR_ARG;
  if (!h->have_batch || !h->B.phase_clocks) return fail(h, AUVP_ERR_STATE, "no phase clocks (AUVP_FLAG_PHASE_CLOCKS)");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpy(out, h->B.phase_clocks, (size_t)h->E * 5 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return AUVP_OK;
}

double auvp_last_kernel_ms(auvp_handle* h) { return h ? h->last_ms : -1.0; }

int auvp_rrt_last_launch_parts(auvp_handle* h, double* expand_ms, double* leaf_ms, int32_t* episodes_per_wave) {
  if (!h) return AUVP_ERR_ARG;
  if (!h->have_batch) return fail(h, AUVP_ERR_STATE, "no batch has run");
  if (expand_ms) *expand_ms = h->last_expand_ms;
  if (leaf_ms) *leaf_ms = h->last_leaf_ms;
  if (episodes_per_wave) *episodes_per_wave = h->last_rows ? 4 : 1;
  return AUVP_OK;
}

const char* auvp_rrt_last_kernel(auvp_handle* h) { return h ? h->last_rrt_kernel : ""; }

double auvp_rrt_last_stream_ms(auvp_handle* h) { return h ? h->last_stream_ms : -1.0; }
int64_t auvp_rrt_last_stream_len(auvp_handle* h) { return h ? (int64_t)h->last_stream_len : -1; }
int auvp_rrt_last_stream_mirror(auvp_handle* h) { return h ? h->last_stream_mirror : -1; }

int auvp_rrt_rows_stream_shape(int32_t K, int32_t n_habitats, int32_t n_poly, int32_t n_bins, int32_t waves_wanted, int32_t force,
                               int32_t* waves, int32_t* mirror, int32_t* lds_bytes) {
  if (K < 0 || n_habitats < 0 || n_poly < 0 || n_bins < 0) return AUVP_ERR_ARG;
  const RowsStreamShape s = rrt_rows_stream_shape(K, RW_MAX_OBST, rrt_tables_bytes(n_habitats, n_poly, n_bins), waves_wanted, force);
  if (waves) *waves = s.waves;
  if (mirror) *mirror = s.mirror ? 1 : 0;
  if (lds_bytes) *lds_bytes = s.plan.total;
  return AUVP_OK;
}

// the options a query names, as the view the choice reads; false: an unknown name
static bool query_options(int32_t n, const char* const* names, const int64_t* values, OptionView* opt) {
  if (n < 0 || (n > 0 && (!names || !values))) return false;
  for (int i = 0; i < n; i++) {
    const int k = names[i] ? auvp_option_index(names[i]) : -1;
    if (k < 0) return false;
    opt->opt_has[k] = true; opt->opt_val[k] = values[i];
  }
  return true;
}

int auvp_rrt_choose_launch(const auvp_rrt_launch_query* q, auvp_rrt_launch_choice* c) {
  OptionView opt;
  if (!q || !c || q->n_episodes <= 0 || q->n_cu <= 0 || q->n_obstacles < 0 || q->n_habitats < 0 || q->n_poly < 0 || q->n_bins < 0 ||
      q->n_time_bins < 0 || !query_options(q->n_options, q->option_names, q->option_values, &opt))
    return AUVP_ERR_ARG;
  RrtLaunchIn in;
  in.E = q->n_episodes; in.n_cu = q->n_cu;
  in.mode = q->mode; in.max_iter = q->max_iter; in.K = q->n_time_bins; in.flags = q->flags; in.freq = q->freq; in.dist_to_end = q->dist_to_end;
  in.max_pts = q->max_pts;
  in.O = q->n_obstacles; in.H = q->n_habitats; in.V = q->n_poly; in.T = q->n_bins; in.obst_area = q->obst_area;
  in.lim = q->per_episode_limits != 0; in.one_wave_only = q->one_wave_only != 0; in.no_stream = q->no_stream != 0;
  in.seen_most = q->seen_most; in.seen_E = q->seen_E;
  const RrtLaunchPlan p = rrt_choose_launch(in, opt);
  *c = auvp_rrt_launch_choice{p.status == PLAN_OK ? AUVP_OK : AUVP_ERR_ARG, (int32_t)p.kind, p.J, p.quad ? 1 : 0, p.grid, p.block, p.lds, p.lds_max,
                              p.kflags, p.stream_waves, p.mirror, 0, p.stream_len, p.lds_need, p.name};
  return AUVP_OK;
}

int auvp_prrt_choose_launch(const auvp_prrt_launch_query* q, auvp_prrt_launch_choice* c) {
  OptionView opt;
  if (!q || !c || q->n_episodes <= 0 || q->n_cu <= 0 || q->n_obstacles < 0 || !query_options(q->n_options, q->option_names, q->option_values, &opt))
    return AUVP_ERR_ARG;
  PrrtLaunchIn in;
  in.E = q->n_episodes; in.n_cu = q->n_cu; in.O = q->n_obstacles; in.freq = q->freq;
  in.max_pts = q->max_pts; in.cap_nodes = q->cap_nodes; in.n_buckets = q->n_buckets; in.max_step = q->max_step; in.flags = q->flags;
  in.step_mode = q->step_mode; in.waits = q->waits != 0; in.one_wave_only = q->one_wave_only != 0; in.rows = q->rows;
  const PrrtLaunchPlan p = prrt_choose_launch(in, opt);
  *c = auvp_prrt_launch_choice{p.status == PLAN_OK ? AUVP_OK : AUVP_ERR_ARG, (int32_t)p.kind, p.lat, p.rows, p.pipe, p.draw_wave, p.next_lds, p.bk_lds,
                               p.obst_lds, p.eps_wg, p.grid, p.block, p.lds, p.J, p.lds_need, p.name};
  return AUVP_OK;
}

int auvp_rrt_last_leaf_stats(auvp_handle* h, int64_t* out4) {
  if (!h || !out4) return AUVP_ERR_ARG;
  if (!h->have_batch || !h->B.leaf_stats) return fail(h, AUVP_ERR_STATE, "no batch has run");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpy(out4, h->B.leaf_stats, 4 * sizeof(int64_t), hipMemcpyDeviceToHost));
  return AUVP_OK;
}

int auvp_last_launch(auvp_handle* h, int32_t* grid, int32_t* block, int32_t* lds_bytes) {
  if (!h) return AUVP_ERR_ARG;
  if (grid) *grid = h->last_grid;
  if (block) *block = h->last_block;
  if (lds_bytes) *lds_bytes = h->last_lds;
  return AUVP_OK;
}

}  // extern "C"

#include "probe_kernels.h"
#include "planner_rrt_host.h"

namespace {
PrrtState* prrt_of(auvp_handle* h) {
  if (!h->prrt) {
    h->prrt = new PrrtState();
    h->prrt_free = [](void* p) { delete static_cast<PrrtState*>(p); };
  }
  return static_cast<PrrtState*>(h->prrt);
}
}  // namespace

#include "astar_kernel.h"
#include "astar_host.h"
#include "sog_kernels.h"
#include "pf_types.h"
#include "pf_host.h"
#include "forecast_kernel.h"
#include "forecast_wide_kernel.h"
#include "forecast_host.h"
#include "compose_host.h"
#include "gather_host.h"
#include "replan_host.h"

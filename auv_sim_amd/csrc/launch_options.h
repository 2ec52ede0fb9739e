// launch_options.h -- the options of a handle and the two size rules of the pre-generated random stream: what launch_plan.h (which
// kernel) and batch_plan.h (which sizes) both read.  Host only and pure, and free of the kernel headers launch_plan.h stands
// behind, so that a stand-alone host program can include it.
#ifndef AUVP_LAUNCH_OPTIONS_H
#define AUVP_LAUNCH_OPTIONS_H
#include <cstring>

// Tuning / diagnostic options of a handle (auvp_set_option, include/auvplan.h).  Every kernel choice the host makes has a
// measured default ("auto": the option is unset); an option forces it.  The environment variable AUVP_<NAME> gives an
// option its initial value ONCE, when the handle is created -- no launch path reads the environment.
#define AUVP_OPTIONS(X)                                                                                                     \
  X(ROWS) X(DUO) X(TRIO) X(QUAD) X(TIGHT_CULL) X(NN_EXACT) X(LEAF_SWEEP_ALL) X(NO_HABITAT_GRID) X(RG_MAX_ENTRIES)           \
  X(NO_GRID_INDEX) X(PRRT_LAT) X(PRRT_PIPE) X(PRRT_OBST_LDS) X(PRRT_NEXT_LDS) X(PRRT_ROWS) X(ASTAR_NO_GRID)                 \
  X(ASTAR_NO_LIST) X(ASTAR_PAIR) X(SOG_TILE) X(PIPE_FALLBACK) X(PRRT_PIPE_DRAW) X(PRRT_BUCKET_LDS) X(ROWS_STREAM)           \
  X(ROWS_STREAM_CAP) X(ROWS_STREAM_WAVES) X(ROWS_WG_WAVES) X(ROWS_STREAM_MIRROR) X(PRRT_ROWS_GRID)          \
  X(SF_WIDE_MIN) X(SF_WIDE_BLOCK) X(MEAS_TICKS)
enum AuvpOpt {
#define AUVP_OPT_ENUM(n) OPT_##n,
  AUVP_OPTIONS(AUVP_OPT_ENUM)
#undef AUVP_OPT_ENUM
  OPT_COUNT
};
static const char* const AUVP_OPT_NAMES[OPT_COUNT] = {
#define AUVP_OPT_NAME(n) #n,
  AUVP_OPTIONS(AUVP_OPT_NAME)
#undef AUVP_OPT_NAME
};
// the option called `name` (without the AUVP_ prefix); -1: there is none
inline int auvp_option_index(const char* name) {
  for (int k = 0; k < OPT_COUNT; k++)
    if (!strcmp(name, AUVP_OPT_NAMES[k])) return k;
  return -1;
}

struct OptionView {
  bool opt_has[OPT_COUNT] = {};
  long long opt_val[OPT_COUNT] = {};
  // option K as a yes / no choice: its value when set, `dflt` (the measured heuristic) otherwise
  bool opt_flag(int k, bool dflt) const { return opt_has[k] ? opt_val[k] != 0 : dflt; }
  bool opt_on(int k) const { return opt_has[k] && opt_val[k] != 0; }
  long long opt_num(int k, long long dflt) const { return opt_has[k] ? opt_val[k] : dflt; }
};

namespace auvp {

// "does this batch get a four-episode kernel by its size": above 18 episodes per CU (see rrt_choose_launch; rrt_stream_keeps
// goes by the same figure)
constexpr int RRT_ROWS_EP_PER_CU = 18;
inline bool rrt_rows_by_size(int E, int n_cu) { return E > RRT_ROWS_EP_PER_CU * n_cu; }
// ... or by option ROWS = 1 / 0, which forces it on (the kernel's limits permitting: rrt_choose_launch) / off
inline bool rrt_rows_wanted(const OptionView& opt, int E, int n_cu) { return opt.opt_flag(OPT_ROWS, rrt_rows_by_size(E, n_cu)); }

// The pre-generated random stream of a batch (rrt_stream_kernel.h): its length in numbers per episode -- from what the previous
// batches with the same parameters drew (seen_most > 0), else 46.5 per iteration + 4 096
inline long long rrt_stream_len(const OptionView& opt, long long seen_most, int max_iter) {
  const long long guess = seen_most > 0 ? seen_most + seen_most * 3 / 100 + 1024 : (long long)(46.5 * (double)max_iter) + 4096;
  long long cap = opt.opt_num(OPT_ROWS_STREAM_CAP, guess);
  cap = cap < 64 ? 64 : cap;
  return (cap + 63) / 64 * 64;
}

}  // namespace auvp
#endif  // AUVP_LAUNCH_OPTIONS_H

/* auvplan.h -- C-ABI of libauvplan.so: the MI355X (gfx950) path-planning hot path.
 *
 * The reference (hmc-lair-shark-tracking/auv-sim) is pure Python and has no FFI; its boundary for
 * this path is the Python planner API.  The Python drop-in classes in auv_sim_amd/
 * keep those signatures and call the entry points below through ctypes.  Each entry point cites the
 * reference interface it replaces (paths relative to the reference tree).
 *
 * Conventions: plain C types; host pointers unless a name ends in _dev; caller-allocated outputs;
 * sizes queried first (two-phase) where variable; integer status (0 ok, >0 reference-defined
 * outcome, <0 error + auvp_last_error()); nothing throws across the ABI; one HIP stream per handle;
 * a handle is thread-compatible (no internal global state), not thread-safe.
 */
#ifndef AUVPLAN_H
#define AUVPLAN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct auvp_handle auvp_handle;

enum {
  AUVP_OK = 0,
  AUVP_NO_QUALIFYING_LEAF = 1, /* exploring(): opt_path stayed None -> TypeError at rrt_dubins.py:174 */
  AUVP_ERR_ARG = -1,
  AUVP_ERR_CAPACITY = -2, /* a device buffer sized from the budget overflowed; nothing is truncated silently */
  AUVP_ERR_HIP = -3,
  AUVP_ERR_STATE = -4,
  AUVP_ERR_KEY = -5, /* time-bin key outside 1..K: KeyError at rrt_dubins.py:124 */
  AUVP_ERR_COMM = -6, /* RCCL missing or a collective failed (auvp_comm_*, auvp_gather*) */
  /* per-episode statuses a kernel can leave in a summary record (never returned by an entry point): */
  AUVP_ERR_GENERATOR = -7, /* an episode's stored MT19937 block phase does not fit the kernel that picked it up (a batch was
                            * moved between the one-episode and the four-episodes-per-wavefront planner kernels) */
  AUVP_ERR_PIPELINE = -9   /* a bounded wait of a multi-wavefront (speculative) latency kernel ran out.  The reference cannot
                            * fail there (rrt_dubins.py:116-151, gym_rrt/envs/rrt_dubins.py:205-248): the host repeats the
                            * affected work on the one-wavefront kernel inside the same call and counts it
                            * (auvp_pipeline_fallbacks); the status stays visible only with option PIPE_FALLBACK = 0 */
  ,
  AUVP_ERR_STREAM = -10    /* RRT.exploring with the random numbers generated ahead (large time-bin batches from the second
                            * batch with a parameter block on; option ROWS_STREAM): an episode drew more numbers than
                            * the stream holds (the busiest episode of the previous batch + 3 % + 1 024).  The host repeats
                            * the batch with the generator inside the kernel in the same call and counts it
                            * (auvp_pipeline_fallbacks); visible only with option PIPE_FALLBACK = 0 */
};

enum { AUVP_MODE_TIMEBIN = 0, AUVP_MODE_PLANTIME = 1, AUVP_MODE_NN = 2 };
enum { AUVP_FLAG_ITER_LOG = 1, AUVP_FLAG_LEAF_LOG = 2, AUVP_FLAG_PHASE_CLOCKS = 4, AUVP_FLAG_KEEP_VISITED = 8 };

const char* auvp_version(void);
/* create a planner context on HIP device `device`; fails (AUVP_ERR_HIP) when no gfx950 GPU is
 * usable -- there is no CPU fallback */
int auvp_create(int device, auvp_handle** out);
void auvp_destroy(auvp_handle* h);
/* Tuning / diagnostic options of a handle.  Every kernel choice the host makes (how many wavefronts per episode, LDS tiles,
 * culls) has a measured default; an option forces it: `name` without the AUVP_ prefix, e.g. "ROWS", "DUO", "TRIO", "QUAD",
 * "PRRT_ROWS", "PRRT_PIPE", "PRRT_LAT", "ASTAR_PAIR", "SOG_TILE", "TIGHT_CULL", "NN_EXACT", "PIPE_FALLBACK" (the full list:
 * INTEGRATION.md).  The environment variable AUVP_<NAME> gives an option its initial value when the handle is created; no
 * other call reads the environment.  auvp_unset_option returns the choice to the default.  Unknown name: AUVP_ERR_ARG. */
int auvp_set_option(auvp_handle* h, const char* name, int64_t value);
int auvp_unset_option(auvp_handle* h, const char* name);
int auvp_get_option(auvp_handle* h, const char* name, int32_t* is_set, int64_t* value);
/* episodes / instances the last planning call (*last) and all calls so far (*total) repeated on the one-wavefront kernel
 * because a speculative latency kernel ended them with AUVP_ERR_PIPELINE (0 in normal operation) */
int auvp_pipeline_fallbacks(auvp_handle* h, int32_t* last, int64_t* total);
const char* auvp_last_error(auvp_handle* h);

/* World model shared by every episode of a batch.
 * Replaces the Python-side arguments of RRT.__init__ (path_planning/rrt_dubins.py:26: boundary
 * polygon, obstacle list, sharkGrid dict, cell_list) and the `habitats` list of exploring() (:92).
 *   obstacles [O,3] x,y,size in LIST ORDER (check_collision is order dependent, :535-541)
 *   habitats  [H,3]
 *   polygon   [V,2] boundary vertices (Point.within, :545-546)
 *   bins      [T,2] shark-grid time bins in dict order; cells [C,4] bounds in cell_list order;
 *   prob      [T,C] (createSharkGrid, :612-630) */
int auvp_world_set(auvp_handle* h, const double* obstacles, int32_t n_obstacles, const double* habitats,
                   int32_t n_habitats, const double* polygon, int32_t n_poly, const double* bins,
                   int32_t n_bins, const double* cells, int32_t n_cells, const double* prob);

/* replace only the habitat list (exploring() takes it per call, rrt_dubins.py:92) */
int auvp_world_set_habitats(auvp_handle* h, const double* habitats, int32_t n_habitats);

typedef struct {
  double dist_to_end, diff_max, freq; /* RRT.__init__ kwargs, rrt_dubins.py:26 */
  double min_dist;                     /* steer(min_dist=0.5), call site :141 */
  double bin_interval, v;              /* exploring() args, :92 */
  double max_traj_time;
  double max_plan_time;                /* only feeds ran_time in plan-time mode (:129) */
  double w[3];                         /* weights */
  int32_t mode;                        /* AUVP_MODE_*: (plan_time, traj_time_stamp) flags of :121-139 */
  int32_t max_iter;                    /* iteration budget = virtual clock of SURVEY 8(c) */
  double points_per_iter;              /* device path-point capacity per iteration; 0 -> freq/2 + 8 sigma of the sum */
} auvp_rrt_params;

typedef struct {
  int32_t status, n_nodes, n_points, n_leaves, best_leaf, best_path_len, iters_run,
          n_candidates; /* obstacles that survived the bounding-box cull, whole episode (diagnostic) */
  double best_cost[4]; /* sum, c0, c1, c2 (habitat_shark_cost_func, path_planning/cost.py:145) */
  double best_length;  /* "path length" of the returned dict, rrt_dubins.py:171,176 */
  double rng_after;    /* next random() of the episode's stream (parity probe: same draw count) */
  int64_t leaf_elems;  /* sum over qualifying leaves of len(path) (cost-walk reads; bench byte count) */
  uint64_t n_draw32;   /* 32-bit MT19937 outputs consumed: lets the host advance Python's global `random` */
  uint64_t nn_scanned; /* nearest-neighbour sampling: sum over iterations of len(mps_list) scanned by get_closest_mps */
} auvp_rrt_summary;

/* RRT.exploring (path_planning/rrt_dubins.py:92-176) for E independent episodes, one wavefront
 * each.  init [E,6] = x,y,theta,traj_time_stamp,plan_time_stamp,length of `initial`;
 * seeds [E]: the episode draws the stream `random.seed(seeds[e])` would give. */
int auvp_rrt_explore_batch(auvp_handle* h, int32_t n_episodes, const double* init, const uint64_t* seeds,
                           const auvp_rrt_params* params, int32_t flags);
/* the same in two steps: prepare() sizes the HBM buffers and uploads init/seeds (MT states are
 * seeded on the host like random.seed), run() launches the kernel on the prepared batch and can be
 * repeated (every run restarts from the prepared inputs) */
int auvp_rrt_prepare(auvp_handle* h, int32_t n_episodes, const double* init, const uint64_t* seeds,
                     const auvp_rrt_params* params, int32_t flags);
/* as prepare(), but every episode continues an existing generator: mt [E,624] words + mt_index [E]
 * exactly as random.getstate() reports them (drop-in use: the global `random` state) */
int auvp_rrt_prepare_states(auvp_handle* h, int32_t n_episodes, const double* init, const uint32_t* mt,
                            const int32_t* mt_index, const auvp_rrt_params* params, int32_t flags);
/* as prepare(), with limits of every episode's own (RRT.replanning_batch: many receding-horizon loops, one
 * round per batch): episode e plans with the horizon episodes[e].max_traj_time (its own number of time bins
 * K = ceil(max_traj_time / bin_interval)) and with the habitats of the world's table whose bit is set in
 * episodes[e].habitat_keep, in table order -- as if that shorter list had been set.  params->max_traj_time is the
 * cap: 0 < max_traj_time <= cap, and bits at or above n_habitats are refused.  The generators come from seeds [E]
 * (mt, mt_index NULL) or, with seeds NULL, from mt [E,624] + mt_index [E] as in prepare_states().  Time-bin mode
 * only; AUVP_FLAG_ITER_LOG and AUVP_FLAG_PHASE_CLOCKS are refused (the leaf log is allowed).  run(), summaries(),
 * paths(), tree() work unchanged; bin_sizes() reports the episode's own K.  AUVP_ERR_ARG on any of these. */
typedef struct {
  double max_traj_time;  /* this episode's horizon (<= params->max_traj_time) */
  uint64_t habitat_keep; /* bit h: habitat h of the world's table is on this episode's list */
} auvp_rrt_episode;
int auvp_rrt_prepare_episodes(auvp_handle* h, int32_t n_episodes, const double* init, const uint64_t* seeds,
                              const uint32_t* mt, const int32_t* mt_index, const auvp_rrt_params* params,
                              const auvp_rrt_episode* episodes, int32_t flags);
int auvp_rrt_run(auvp_handle* h);
int auvp_rrt_summaries(auvp_handle* h, auvp_rrt_summary* out /* [E] */);
/* generate_final_course (:321-331) of every episode's best leaf, reversed to root->leaf (:174).
 * offsets [E+1] = exclusive prefix sum of best_path_len; out [offsets[E],7] =
 * x,y,theta,v,traj_time_stamp,plan_time_stamp,length per element */
int auvp_rrt_paths(auvp_handle* h, const int64_t* offsets, double* out);
/* the same, left in HBM: out_dev is a device pointer to [offsets[E],7] doubles (multi-GPU gather) */
int auvp_rrt_paths_dev(auvp_handle* h, const int64_t* offsets, void* out_dev);
/* whole tree of one episode (tests / RRT.mps_list): nodes [n_nodes,6] x,y,theta,traj_t,plan_t,length */
int auvp_rrt_tree(auvp_handle* h, int32_t episode, double* nodes6, int32_t* parent, int32_t* pt_off,
                  int32_t* pt_cnt, double* points7);
int auvp_rrt_iter_log(auvp_handle* h, int32_t episode, int32_t* it_parent, int8_t* it_accepted,
                      int32_t* it_npath);
int auvp_rrt_leaf_log(auvp_handle* h, int32_t episode, double* leaf_cost6, int32_t* leaf_iter);
int auvp_rrt_bin_sizes(auvp_handle* h, int32_t episode, int32_t* sizes /* [K] */, int32_t* n_bins);

/* device-side result records for the multi-GPU gather: pointer to [E] auvp_rrt_summary in HBM */
void* auvp_rrt_summaries_dev(auvp_handle* h);

/* Best-of-K planning: the episodes of the batch that just ran form n_groups groups (one AUV's K trees), group g = episodes
 * group_off[g] .. group_off[g+1]-1, and the winner of every group is chosen on the device.  The rule is exploring's own
 * (rrt_dubins.py:101,169: a leaf is kept only if new_cost[0] < opt_cost[0], from inf) folded over the members' best costs in
 * member order: the lowest best_cost[0], the lowest episode index among equal costs (-0.0 == 0.0); a member without a leaf, or
 * with a NaN cost, never wins.  The groups partition the batch -- group_off[0] == 0, group_off[n_groups] == E, strictly
 * increasing -- anything else (an empty group, n_groups < 1) is AUVP_ERR_ARG; without a batch that has run: AUVP_ERR_STATE.
 * Works after any RRT batch (every mode, every expansion kernel, with or without per-episode limits).
 * (A struct tag, not a typedef: the record and the entry point share their name.) */
struct auvp_rrt_group_best {
  int32_t status;      /* AUVP_OK; AUVP_NO_QUALIFYING_LEAF: no member can win (winner -1); or the status (< 0) of the
                        * lowest-indexed member that failed on the device */
  int32_t winner;      /* episode index in the batch, -1: none */
  int32_t n_with_leaf; /* members with a qualifying leaf */
  int32_t path_len;    /* the winner's best_path_len, best_cost and best_length (0, inf, 0 without a winner) */
  double cost[4];
  double length;
};
/* one launch (rrt_group_best_kernel); out [n_groups] may be NULL: the records stay in HBM (auvp_rrt_group_best_dev) */
int auvp_rrt_group_best(auvp_handle* h, int32_t n_groups, const int32_t* group_off /* [n_groups+1] */,
                        struct auvp_rrt_group_best* out /* [n_groups], may be NULL */);
/* the records of the last auvp_rrt_group_best call, [n_groups] in HBM (NULL: none since the batch ran) */
void* auvp_rrt_group_best_dev(auvp_handle* h);
/* generate_final_course of the winners only (rrt_group_course_kernel): offsets [n_groups+1] = exclusive prefix sum of the
 * records' path_len (0 for a group without a winner); out [offsets[n_groups],7] as auvp_rrt_paths.  Offsets that leave a
 * winner fewer rows than its path_len: AUVP_ERR_ARG.  Before auvp_rrt_group_best (of this batch): AUVP_ERR_STATE. */
int auvp_rrt_group_paths(auvp_handle* h, const int64_t* offsets, double* out);
/* the same, left in HBM: out_dev is a device pointer to [offsets[n_groups],7] doubles */
int auvp_rrt_group_paths_dev(auvp_handle* h, const int64_t* offsets, void* out_dev);

/* Probability sets: a fleet that tracks several sharks plans every AUV against its own shark's occupancy table.
 * auvp_world_set_prob_sets puts n_sets tables [n_sets, T, C] on the handle; they share the world's bins [T] and cells [C]
 * (AUVP_ERR_STATE without a world that has both).  Exactly one of prob_host and prob_dev is non-NULL (both or neither:
 * AUVP_ERR_ARG); prob_dev is a device pointer on the handle's device and is copied device to device into a buffer the handle
 * owns, so the caller's buffer is free again when the call returns.  n_sets < 1 is AUVP_ERR_ARG, except n_sets == 0 with both
 * pointers NULL, which clears the sets.  Per set, a small kernel computes what auvp_world_set computes for its one table: absmax
 * (nan if any entry is a nan, else max |p|) and one_sign (1 unless there is a nan or both signs occur) -- the constants of the
 * leaf pass's error bound, each episode's own.  A later auvp_world_set drops the sets; auvp_world_set_habitats keeps them.
 * The tree growth never reads a probability table: only the leaf ranking depends on the set. */
int auvp_world_set_prob_sets(auvp_handle* h, int32_t n_sets, const double* prob_host, const void* prob_dev);
/* The sets from a forecast whose rounds are counted from "now", placed at the world's absolute bins (csrc/forecast_place.h):
 * prob_dev is a device pointer to [n_sets, n_rounds1, n_cells] on the handle's device (auvp_sf_prob_dev of the forecast's handle);
 * with T world bins, bin t of every set becomes forecast round min(max(t - first_bin, 0), n_rounds1 - 1).  sf_place_kernel gathers
 * on the device, one workgroup per (set, bin) row with 16-byte loads and stores, into the buffer the handle owns; the per-set
 * constants are computed as in auvp_world_set_prob_sets.  first_bin == 0 with n_rounds1 == T is auvp_world_set_prob_sets(h, n_sets,
 * NULL, prob_dev) itself.  AUVP_ERR_ARG: a null pointer, n_sets or n_rounds1 < 1, n_cells not the world's, first_bin outside
 * 0 .. T - 1; AUVP_ERR_STATE without a world that has bins and cells.  A call that fails launches nothing and keeps the sets. */
int auvp_world_set_prob_sets_placed(auvp_handle* h, const void* prob_dev, int32_t n_sets, int32_t n_rounds1, int32_t n_cells,
                                    int32_t first_bin);
/* The sets as they lie in HBM, copied to the host (for checks): n_sets, prob [n_sets, T, C]; each may be NULL.  AUVP_ERR_STATE
 * without sets. */
int auvp_world_prob_sets_read(auvp_handle* h, int32_t* n_sets, double* prob);
/* the per-set constants, absmax [n_sets] and one_sign [n_sets] (each may be NULL); AUVP_ERR_STATE without sets */
int auvp_world_prob_set_stats(auvp_handle* h, double* absmax, int32_t* one_sign);
/* After auvp_rrt_prepare_episodes and before auvp_rrt_run: episode e ranks its leaves against set set_of[e].  An index outside
 * [0, n_sets) or n_episodes other than the prepared batch's: AUVP_ERR_ARG; no sets on the handle, or a batch not prepared by
 * auvp_rrt_prepare_episodes: AUVP_ERR_STATE.  set_of == NULL clears the assignment (the world's own table again); so does every
 * new prepare and every auvp_world_set_prob_sets.  A call that fails launches nothing. */
int auvp_rrt_set_episode_grids(auvp_handle* h, int32_t n_episodes, const int32_t* set_of /* [n_episodes] or NULL */);
/* The leaf ranking alone on the finished trees of the last auvp_rrt_run, with the current assignment (the world's table if
 * there is none): a tree grown once is ranked against another shark's forecast for the price of the leaf pass.  Rewrites the
 * summaries' leaf fields (n_leaves, best_leaf, best_path_len, best_cost, best_length, leaf_elems); summaries, paths,
 * group_best and group_paths work after it (group_best has to be called again).  AUVP_ERR_STATE if no run has completed since
 * the batch was prepared. */
int auvp_rrt_rerank(auvp_handle* h);

/* Replanning a fleet with the step between two rounds on the device (RRT.replanning_batch, commit="device").  The reference's
 * host step (path_planning/rrt_dubins.py:82-87: the first bucket of splitPath, then removeHabitat) is one pure function,
 * csrc/replan_commit.h, and rrt_commit_kernel applies it to every group's winner behind auvp_rrt_group_best: the winners'
 * courses never leave HBM, the committed rows go into a trajectory log the handle owns, and only one fixed-size record per
 * AUV and round crosses the bus.  An AUV's state: last [7] (x, y, theta, v, traj_time_stamp, plan_time_stamp, length) and keep
 * (bit h: habitat h of the world's table is still on its list).  The rule, for a course c[0..L-1] of 7 doubles as
 * auvp_rrt_paths writes it: row 0 is replaced by last; lo = last[4] + 0 * round_span, hi = last[4] + 1 * round_span; row i is
 * committed iff lo <= t_i <= hi (a NaN: never), in course order; every committed row, in order, removes from keep the lowest
 * kept habitat that contains it (sqrt(dx*dx + dy*dy) <= size, no contraction); last becomes the last committed row. */
typedef struct {
  int32_t status;      /* the group record's status (auvp_rrt_group_best); AUVP_ERR_STATE: the batch's summaries no longer
                        * agree with the group records the space was reserved from -- nothing was committed */
  int32_t winner;      /* episode of the batch whose course was committed, -1: none (nothing committed, state unchanged) */
  int32_t n_committed; /* rows appended to the AUV's trajectory */
  int32_t path_len;    /* rows of the winner's course */
  double cost[4];      /* the winner's best_cost (inf without one) */
  double last[7];      /* the AUV's state after the round */
  uint64_t keep;       /* the AUV's list after the round; with teams (auvp_replan_set_teams): its team's list after the round */
  uint64_t claimed;    /* after auvp_replan_team_pick: the habitats the AUV's teammates had claimed when its winner was chosen
                        * (0 for an AUV without a teammate, and after auvp_rrt_group_best) */
  int32_t conflicts;   /* after auvp_replan_team_pick_apart: the ticks at which the committed winner is closer than d to a course
                        * an earlier teammate chose in this round (0 after the other two selections) */
  int32_t _reserved;
} auvp_replan_record; /* 128 bytes */
/* A fleet's state on the handle: last = start7 [n_auvs,7], keep = keep0 [n_auvs] (keep_is_shared != 0: keep0[0] for everyone),
 * an empty log, zeroed counters.  It survives auvp_rrt_prepare*, auvp_rrt_run, auvp_world_set_habitats and
 * auvp_world_set_prob_sets; a new auvp_replan_begin or auvp_destroy drops it. */
int auvp_replan_begin(auvp_handle* h, int32_t n_auvs, const double* start7, const uint64_t* keep0, int32_t keep_is_shared);
/* Teams: AUVs of the fleet with the same label team_of[a] >= 0 share one habitat list; a label < 0 is an AUV on its own, labels
 * need not be dense, and a team of one member is no team.  The rule ("team fold", csrc/replan_teams.h): after every
 * auvp_replan_commit, once all of the round's commits are done, every member's keep becomes the bitwise AND of the keeps of
 * ALL members of its team -- those that are not part of the round included.  Within a round every member plans against the
 * list it had at the round's start.  replan_team_kernel (one wavefront per team) runs behind rrt_commit_kernel on the same
 * stream and writes the team's list into the state and into the round's records before they are copied back, so nothing more
 * crosses the bus.  team_of == NULL clears the teams.  Valid after auvp_replan_begin; a new auvp_replan_begin drops the teams.
 * AUVP_ERR_STATE without a fleet, AUVP_ERR_ARG if n_auvs is not the fleet's size; a call that fails changes nothing. */
int auvp_replan_set_teams(auvp_handle* h, int32_t n_auvs, const int32_t* team_of /* [n_auvs], NULL: clear */);
/* Probe: the team fold on the caller's arrays -- the teams' tables built from team_of [n], one launch of replan_team_kernel,
 * keep_io [n] folded in place.  Needs no world and no fleet; a fleet's state and counters are not touched.  AUVP_ERR_ARG for
 * n < 1 or a null pointer. */
int auvp_replan_team_fold(auvp_handle* h, int32_t n, const int32_t* team_of, uint64_t* keep_io);
/* One round: group g of the last auvp_rrt_group_best is AUV auv_of[g].  One launch (rrt_commit_kernel, one wavefront per
 * group); the round's log space is reserved from the host's copy of the group records before it.  A group without a winner, or
 * whose status is < 0, commits nothing.  out [n_active] may be NULL.  AUVP_ERR_STATE: no auvp_replan_begin, no batch that has
 * run, or no auvp_rrt_group_best for that batch.  AUVP_ERR_ARG: n_active is not the number of groups, an index outside
 * [0, n_auvs), an AUV named twice, round_span not > 0.  A call that fails launches nothing and changes no state. */
int auvp_replan_commit(auvp_handle* h, int32_t n_active, const int32_t* auv_of /* [n_active] */, double round_span,
                       auvp_replan_record* out /* [n_active], may be NULL */);
/* The fleet's range / bearing measurements of the sharks it tracks, from the states it has committed (csrc/replan_measure.h;
 * replan_measure_kernel, one lane per row).  shark_of [n_auvs]: the shark AUV a tracks; every shark 0 .. n_auvs / n_per_shark - 1
 * must be tracked by exactly n_per_shark AUVs, taken in ascending AUV index (anything else: AUVP_ERR_ARG).  shark_xy [F,2]: the
 * sharks' true positions (the only input that crosses the bus).  Row (f, a) of the table [F, n_per_shark, 5] the handle keeps in
 * HBM: the AUV's x, y, theta, range = sqrt(dx*dx + dy*dy), bearing = atan2(dy, dx) - theta, dx = shark_x - x (the layout of
 * auvp_pf_run's meas for one step; the square root correctly rounded, the atan2 the particle-filter kernel's value rounded
 * to the nearest double -- csrc/replan_measure.h: what math.sqrt and math.atan2 give).  An AUV that no longer plans keeps measuring
 * from its last committed state.  *meas_dev_out (may be NULL) gets the table's device pointer: valid until the next
 * auvp_replan_measure or auvp_replan_begin on this handle; the call synchronises its stream before it returns, so a copy enqueued
 * afterwards on another handle's stream on the same device is ordered behind it.  AUVP_ERR_STATE without auvp_replan_begin.
 * With option MEAS_TICKS = k set (1 <= k <= 64; otherwise AUVP_ERR_ARG, nothing is launched and the last table stays): k
 * measurements per AUV along the segment it committed in the most recent auvp_replan_commit (csrc/replan_ticks.h;
 * replan_measure_ticks_kernel, one wavefront per AUV).  shark_xy is then [k,F,2], the sharks at the k ticks, and the table
 * [k, F, n_per_shark, 5], step-major: auvp_pf_run's meas for k steps.  Tick j < k - 1 is at lo + (j + 1) * (round_span / k), the
 * last at lo + 1.0 * round_span, with lo the time of the segment's first row (the state before that commit) and round_span that
 * commit's; the AUV is at the segment row with the greatest index whose time is <= the tick (row 0 if none; nothing is
 * interpolated), so the last tick is the committed state.  An AUV without a segment in that commit -- it no longer plans, its
 * group had no winner, or nothing has been committed yet -- measures from its state at every tick.  k = 1 gives the table of
 * the call without the option, bit for bit. */
int auvp_replan_measure(auvp_handle* h, const int32_t* shark_of /* [n_auvs] */, int32_t n_per_shark, const double* shark_xy /* [F,2] */,
                        const void** meas_dev_out);
/* The last auvp_replan_measure's table copied to the host (for checks): n_sharks, n_per_shark, meas [F, n_per_shark, 5]; each may
 * be NULL.  After a measurement under option MEAS_TICKS = k the whole table, k * F * n_per_shark * 5 doubles ([k, F, n_per_shark,
 * 5]), with the k in force at that measurement.  AUVP_ERR_STATE without one since auvp_replan_begin. */
int auvp_replan_meas(auvp_handle* h, int32_t* n_sharks, int32_t* n_per_shark, double* meas);
/* The team-aware winner selection ("claims", csrc/replan_pick.h), in place of auvp_rrt_group_best in a round: the batch that
 * just ran holds K trees for each of n_active AUVs, group g = episodes g*K .. g*K+K-1 = AUV auv_of[g].  Every group first gets
 * rrt_group_best_kernel's record.  Then, for every team of two or more (auvp_replan_set_teams), the members that are part of
 * the round are taken in ascending AUV index with claimed = 0: each tree's own best course (as the leaf pass ranked it under the
 * member's keep) is scored again under keep & ~claimed -- the habitat terms of habitat_shark_cost_func against the shorter list,
 * the shark term unchanged --, the winner is rrt_group_best's fold over these scores, and the habitats its whole course visits
 * under that mask join claimed.  The members' records carry that winner and its score (cost[4]); the others are untouched.  With
 * claimed == 0 the score is the summary's best_cost bit for bit.  Three launches on the handle's stream (rrt_group_best_kernel,
 * rrt_course_words_kernel: one 64-bit word per course point into a scratch buffer sized from the batch's capacities,
 * replan_team_pick_kernel: one wavefront per team), one copy of the records; auvp_replan_commit, auvp_rrt_group_paths and
 * auvp_replan_traj work behind it as behind auvp_rrt_group_best, and the commit's records carry `claimed`.  out [n_active] may
 * be NULL.  AUVP_ERR_STATE: no auvp_replan_begin, no teams, or no batch that has run.  AUVP_ERR_ARG: n_active * K is not the
 * batch's size, an AUV outside the fleet or named twice.  A call that fails launches nothing and leaves the fleet and the
 * group records as they were.
 * The scratch buffer: (cap_nodes + cap_points) 8-byte words for each of the batch's episodes, reserved by the first call and
 * kept by the handle (4.3 GiB for 16 384 episodes of 2 000 iterations); only callers of this entry point pay for it.
 * Caveat: the commit recognises "the group records are still this call's" by comparing the handle's records with the copy this
 * call kept.  An auvp_rrt_group_best on the SAME batch between this call and auvp_replan_commit that happens to produce
 * byte-identical records (no claim touched any member's list) is therefore not told apart, and that commit's records carry
 * this call's claimed masks instead of 0.  Call one of the two per round. */
int auvp_replan_team_pick(auvp_handle* h, int32_t n_active, const int32_t* auv_of /* [n_active] */, int32_t K,
                          struct auvp_rrt_group_best* out /* [n_active], may be NULL */);
/* Probe: the same three kernels on the caller's candidates, against the world's habitat table and time bins.  n_auvs AUVs with
 * labels team_of and lists keep; group g of n_active is AUV auv_of[g] and has K candidates, candidate e = g*K + k: its course is
 * rows course_off[e] .. course_off[e+1]-1 of courses_xyt [*,3] (x, y, traj_time; none: a tree without a leaf; row 0 is taken
 * as given), cost4 [E,4] its cost as the leaf pass would report it (cost4[.,3] is the shark term that stays), leaf_t [E] its
 * leaf's time, length [E] (may be NULL: 0) its path length, and bin_lo / bin_hi [E] the shark bins lo .. hi-1 that exploring
 * selects for its leaf.  weights3: w1, w2, w3.  out [n_active] gets the group records, claimed_out [n_active] the mask each
 * group's AUV saw.  The fleet of auvp_replan_begin and the handle's group records are not touched. */
int auvp_replan_team_pick_courses(auvp_handle* h, int32_t n_auvs, const int32_t* team_of, const uint64_t* keep, int32_t n_active,
                                  const int32_t* auv_of, int32_t K, const int64_t* course_off /* [n_active*K+1] */,
                                  const double* courses_xyt, const double* cost4, const double* leaf_t, const double* length,
                                  const int32_t* bin_lo, const int32_t* bin_hi, const double* weights3,
                                  struct auvp_rrt_group_best* out, uint64_t* claimed_out);
/* The winner selection that keeps the courses teammates commit in one round apart ("team separation", csrc/replan_apart.h), in
 * place of auvp_rrt_group_best or auvp_replan_team_pick in a round; groups, K and auv_of as there.  Every tree's own best course
 * is sampled on the ticks s * tick of a window of W ticks from its AUV's committed state -- between two points the AUV stays at
 * the last one it reached, the largest row among those with ceil(t / tick) <= s owns tick s -- into a tick table in a scratch
 * buffer (rrt_course_ticks_kernel, one wavefront per episode; n_active * K * W * 16 bytes, kept by the handle).  Then, for every
 * team of two or more, the members that are part of the round are taken in ascending AUV index: n of a candidate is the number
 * of its ticks at which it is closer than d (dx*dx + dy*dy < d*d, no contraction) to the winner an earlier member chose in this
 * call; among the candidates with score < inf the winner is the smallest (n, score), the lowest tree among equals
 * (replan_team_pick_apart_kernel, one wavefront per team).  The score is the tree's own best_cost[0] (use_claims == 0: no words
 * are computed and no scratch for them is reserved) or auvp_replan_team_pick's score under keep & ~claimed (use_claims != 0; the
 * claims accumulate as there).  Where no candidate has a conflict the records are those of auvp_rrt_group_best /
 * auvp_replan_team_pick.  The commit's records carry `conflicts`, the winner's n (and `claimed`).  State and argument errors as
 * auvp_replan_team_pick, and AUVP_ERR_ARG for a d or tick that is not finite and > 0, W outside 1 .. 1024, or a team of more
 * than 1024 members.  A call that fails launches nothing and changes nothing.  The caveat of auvp_replan_team_pick holds. */
int auvp_replan_team_pick_apart(auvp_handle* h, int32_t n_active, const int32_t* auv_of /* [n_active] */, int32_t K, int32_t use_claims,
                                double d, double tick, int32_t W, struct auvp_rrt_group_best* out /* [n_active], may be NULL */);
/* Probe: auvp_replan_team_pick_courses with the kernels of auvp_replan_team_pick_apart on the caller's candidates (row 0 of a
 * course is taken as given); conflicts_out [n_active] gets each group's winner's n.  Nothing of the fleet is touched. */
int auvp_replan_team_pick_apart_courses(auvp_handle* h, int32_t n_auvs, const int32_t* team_of, const uint64_t* keep, int32_t n_active,
                                        const int32_t* auv_of, int32_t K, const int64_t* course_off /* [n_active*K+1] */,
                                        const double* courses_xyt, const double* cost4, const double* leaf_t, const double* length,
                                        const int32_t* bin_lo, const int32_t* bin_hi, const double* weights3, int32_t use_claims,
                                        double d, double tick, int32_t W, struct auvp_rrt_group_best* out, uint64_t* claimed_out,
                                        int32_t* conflicts_out);
/* Every AUV's whole committed trajectory, in round order: AUV a's rows are row_off[a] .. row_off[a+1]-1 of rows [*,7].  The only
 * bulk copy to the host (one gather launch, one copy of rows * 56 bytes).  rows == NULL: row_off [n_auvs+1] alone, to size the
 * buffer.  AUVP_ERR_STATE without auvp_replan_begin. */
int auvp_replan_traj(auvp_handle* h, int64_t* row_off /* [n_auvs+1] */, double* rows /* may be NULL */);
/* Probe: rrt_commit_kernel's rule on the caller's courses and states, against the handle's habitat table (one launch, one
 * wavefront per state).  State i's course is rows course_off[i] .. course_off[i+1]-1 of courses [*,7] (none: a state without a
 * winner); last7 [n,7] and keep [n] are updated in place; out [n] gets the records (winner 0 or -1, cost inf) and rows_out [*,7]
 * state i's committed rows from row course_off[i] on.  The fleet's state of auvp_replan_begin is not touched. */
int auvp_replan_commit_courses(auvp_handle* h, int32_t n_states, const int64_t* course_off /* [n_states+1] */,
                               const double* courses, double* last7, uint64_t* keep, double round_span, auvp_replan_record* out,
                               double* rows_out);
/* Counters since auvp_replan_begin (each pointer may be NULL): the fleet's size (0: none), rounds committed, rows in the log,
 * the bytes the auvp_replan_* entry points have copied to the host, the part of those that auvp_replan_traj copied, and
 * rrt_commit_kernel's time summed over the rounds (HIP events, milliseconds; with teams set the span covers
 * replan_team_kernel too, and auvp_replan_team_pick adds the time of its two own kernels). */
int auvp_replan_info(auvp_handle* h, int32_t* n_auvs, int32_t* rounds, int64_t* rows, int64_t* bytes_to_host, int64_t* bytes_traj,
                     double* commit_ms);

/* ---------------------------------------------------------------------------------------------
 * Planner_RRT (gym_rrt/envs/rrt_dubins.py:34): goal-directed RRT driven by the RL environment.
 * Obstacles come from auvp_world_set (list order matters, :445-451); everything else is here.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  double rect[4];          /* boundary corners x0,y0,x1,y1 (boundary[0], boundary[1], :45) */
  double exp_rate, dist_to_end, diff_max, freq, cell_side_length; /* constructor kwargs, :34 */
  int32_t subsections;     /* subsections_in_cell */
  int32_t max_step;        /* node / step capacity of the batch (planning(max_step), :162) */
} auvp_prrt_params;

typedef struct {
  int32_t status, n_nodes, n_points, n_occ, steps, done, path_len, last_node;
  int32_t last_accepted, last_new_node, n_arc, _pad; /* outcome of the most recent step */
  double arc[6];           /* successful goal arc: x_C, y_C, radius, ang_vel, theta_0, length */
  double rng_after;        /* next random() of the episode's stream (not consumed) */
  uint64_t n_draw32;
} auvp_prrt_summary;

/* Planner_RRT.__init__ for E episodes: starts [E,4] x,y,theta,traj_time_stamp; goals [E,2]; the start
 * node is put into the (row, col, theta-subsection) bucket grid (:53,:108-159).  RNG: seeds [E]
 * (random.seed(seed) streams) or, if seeds is NULL, mt [E,624] + mt_index [E] (random.getstate()). */
int auvp_prrt_create_batch(auvp_handle* h, int32_t n_episodes, const double* starts, const double* goals,
                           const auvp_prrt_params* params, const uint64_t* seeds, const uint32_t* mt,
                           const int32_t* mt_index, int32_t flags);
/* Planner_RRT.planning(max_step) (:162-202) for every episode: device-side loop until done / budget */
int auvp_prrt_plan(auvp_handle* h);
/* Planner_RRT.generate_one_node(grid_cell) (:205-248), one step per episode: bucket_ids [E] =
 * (row*cols + col)*subsections + k of the chosen cell (<0 skips the episode).  mt/mt_index optional:
 * continue that generator for this step (the caller's global `random` state) */
int auvp_prrt_step(auvp_handle* h, const int32_t* bucket_ids, const uint32_t* mt, const int32_t* mt_index);
int auvp_prrt_summaries(auvp_handle* h, auvp_prrt_summary* out /* [E] */);
/* the goals of the resident batch, [E,2] (self.goal of every Planner_RRT, :40) */
int auvp_prrt_goals(auvp_handle* h, double* goals2);
/* generate_final_course(final_node) (:317-327) in planning()'s return order (goal end first);
 * offsets [E+1] prefix sums of path_len; out [offsets[E],5] = x,y,theta,traj_time_stamp,length */
int auvp_prrt_paths(auvp_handle* h, const int64_t* offsets, double* out);
/* one episode's tree: nodes4 [n,4] x,y,theta,traj_t; node_i4 [n,4] step,parent,pt_off,pt_cnt;
 * node_bucket [n]; points4 [n_points,4] x,y,theta,traj_t */
int auvp_prrt_tree(auvp_handle* h, int32_t episode, double* nodes4, int32_t* node_i4, int32_t* node_bucket,
                   double* points4);
/* one node of one episode (the node generate_one_node just appended to mps_list, gym_rrt/envs/rrt_dubins.py:236-240):
 * node4 x,y,theta,traj_t; node_i4 step,parent,pt_off,pt_cnt; its bucket; points4 [pt_cnt,4] (cap_points rows
 * available, AUVP_ERR_CAPACITY if the node has more).  O(path points of the node), not O(tree). */
int auvp_prrt_node(auvp_handle* h, int32_t episode, int32_t node, double* node4, int32_t* node_i4, int32_t* node_bucket,
                   double* points4, int32_t cap_points);
/* env_grid state: occupied_grid_cells_array as bucket ids, len(node_array) per bucket, dims4 =
 * rows, cols, subsections, n_occupied */
int auvp_prrt_grid(auvp_handle* h, int32_t episode, int32_t* occupied, int32_t* bucket_counts, int32_t* dims4);
/* per-step log (AUVP_FLAG_ITER_LOG): [max_step,8] bucket, picked, accepted, done, npath, arc_n, arc_free, new_node */
int auvp_prrt_step_log(auvp_handle* h, int32_t episode, int32_t* log8);
void* auvp_prrt_summaries_dev(auvp_handle* h);
/* which kernel the last auvp_prrt_plan / auvp_prrt_step launch ran: "prrt_kernel" (one episode per wavefront) or
 * "prrt_rows_kernel" (four per wavefront: throughput batches of the environment's planner shape, freq <= 15, <= 256
 * obstacles, no step log) */
const char* auvp_prrt_last_kernel(auvp_handle* h);
/* RRTEnv observation arrays (gym_rrt/envs/rrt_env.py:250-295: convert_rrt_grid_to_1D,
 * generate_rrt_grid_has_node_array, convert_rrt_grid_to_1D_num_of_nodes_only) for all episodes into
 * caller-owned DEVICE buffers: rrt_grid [E,n_buckets,4] f64 = cell.x, cell.y, subsection.theta,
 * len(node_array); has_node [E,n_buckets] i64; num_nodes [E,n_buckets] i64 (either may be NULL) */
int auvp_prrt_observation_dev(auvp_handle* h, void* rrt_grid_dev, void* has_node_dev, void* num_nodes_dev);
/* the same for one episode, copied to host arrays */
int auvp_prrt_observation(auvp_handle* h, int32_t episode, double* rrt_grid, int64_t* has_node, int64_t* num_nodes);
/* RRTEnv.step (gym_rrt/envs/rrt_env.py:182-247) for every environment with NOTHING crossing PCIe: bucket_ids_dev [E]
 * (chosen_grid_cell_idx per environment, -1 = skip; DEVICE memory, e.g. an agent's output) -> generate_one_node, then
 * the observation arrays (as auvp_prrt_observation_dev; rrt_grid_dev may be NULL to skip them) and the step's outcome:
 * reward_dev [E] i64 = 300 R_FOUND_PATH / 0 R_CREATE_NODE / -1 R_INVALID_NODE; 0 for an environment that had already
 * finished or that the caller skipped with -1 (neither is touched; a skipped one keeps its done flag), done_dev [E] u8
 * (may be NULL).  An episode that fails on the device (tree / point capacity, a bucket id outside the grid) is flagged
 * done, rewarded 0 and reported by auvp_prrt_env_check -- the host loop (auvp_prrt_step) shows the same failure as
 * summary.status < 0.  Two launches per step (the outcome is written by the planner launch itself, the observation arrays
 * by a second one; see AUVP_ENV_OBS_DELTA below for one).  Only ENQUEUES on the
 * handle's stream: follow with auvp_stream_sync (or order other work on auvp_stream) before reading results. */
int auvp_prrt_env_step_dev(auvp_handle* h, const int32_t* bucket_ids_dev, void* rrt_grid_dev, void* has_node_dev,
                           void* num_nodes_dev, int64_t* reward_dev, uint8_t* done_dev);
/* the same step with options (flags):
 *   AUVP_ENV_AGENT      the stand-in agent of auvp_prrt_policy_random_dev picks INSIDE the planner launch; bucket_ids_dev [E]
 *                       is then an OUTPUT (what it picked, -1 for finished environments)
 *   AUVP_ENV_OBS_DELTA  rrt_grid_dev / has_node_dev / num_nodes_dev hold the observation of the previous step (or of
 *                       auvp_prrt_observation_dev after the reset) and are UPDATED IN PLACE by the planner launch: a step adds
 *                       at most one node per environment, so one bucket's len(node_array) / has_node / node count changes
 *                       (rrt_env.py:250-295 rebuilds all three lists after every node) -- ONE launch per environment step
 * flags = 0 is auvp_prrt_env_step_dev. */
#define AUVP_ENV_AGENT 1
#define AUVP_ENV_OBS_DELTA 2
int auvp_prrt_env_step_ex_dev(auvp_handle* h, int32_t flags, uint64_t agent_seed, int32_t* bucket_ids_dev, void* rrt_grid_dev,
                              void* has_node_dev, void* num_nodes_dev, int64_t* reward_dev, uint8_t* done_dev);
/* stand-in agent for device-resident runs as a launch of its own: every live environment picks, uniformly, one of its
 * occupied buckets -- read from the planner's own list of occupied buckets, the set the observation's has_node array marks
 * (rrt_env.py:250-265); has_node_dev is accepted for compatibility, not read, and may be NULL -- finished environments get
 * -1; its randomness is its own, not the planner's stream: a pure function of (`seed`, environment, the environment's step
 * count in HBM), so a captured graph of one step draws anew at every replay, and calls repeated WITHOUT a step in between
 * (or for an environment whose step did not run) return the same pick -- vary `seed` to redraw.  Enqueues only. */
int auvp_prrt_policy_random_dev(auvp_handle* h, const int64_t* has_node_dev, uint64_t seed, int32_t* bucket_ids_dev);
/* waits for the stream, then: *status = status (< 0) of the first episode that failed on the device inside the
 * device-resident loop since the batch was created, *env (may be NULL) = its index; 0 = none */
int auvp_prrt_env_check(auvp_handle* h, int32_t* status, int32_t* env);
/* the handle's HIP stream (hipStream_t) and a wait for everything enqueued on it */
void* auvp_stream(auvp_handle* h);
int auvp_stream_sync(auvp_handle* h);
/* HIP-event time of a region of the handle's stream that the caller brackets around enqueue-only calls
 * (auvp_prrt_env_step_dev, auvp_graph_launch ...): mark(h, 0) before, mark(h, 1) after; elapsed_ms waits for the second
 * mark and returns the device time between the two (measurement infrastructure: no reference counterpart) */
int auvp_stream_mark(auvp_handle* h, int32_t which);
int auvp_stream_elapsed_ms(auvp_handle* h, double* ms);
/* hipGraph capture of a launch-bound step loop: everything the enqueue-only entry points (auvp_prrt_policy_random_dev,
 * auvp_prrt_env_step_dev, the caller's own kernels on auvp_stream) put on the stream between begin and end is recorded
 * instead of run; auvp_graph_launch replays it n_times back to back (enqueue only).  Every environment's step count lives in
 * HBM, so every replay of the stand-in agent draws anew.  Run one un-captured step first.  A graph holds the device
 * pointers of the batch (and of the caller's arrays) it was captured with: creating a new batch (auvp_prrt_create_batch,
 * auvp_prrt_replan_particles) destroys the handle's graphs, and auvp_graph_launch of such an id fails with AUVP_ERR_STATE. */
int auvp_graph_begin(auvp_handle* h);
int auvp_graph_end(auvp_handle* h, int32_t* graph_id);
int auvp_graph_launch(auvp_handle* h, int32_t graph_id, int32_t n_times);

/* ---------------------------------------------------------------------------------------------
 * A* variants (path_planning/astar.py, astar_real.py, astar_fixLen.py, astar_fixLenSOG.py), one
 * wavefront per search instance, E instances over the world of auvp_world_set (obstacles = obs_lst,
 * habitats = habitat_list, polygon = boundary_list corners, bins/cells/prob = sharkGrid).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t variant;   /* 0 astar.astar (astar.py:193), 1 astar_real (:144), 2 astar_fixLen (:286), 3 astar_fixLenSOG (:551) */
  int32_t cap_nodes; /* Node capacity per instance; overflow -> AUVP_ERR_CAPACITY in the instance's status */
  double box[4];     /* variant 0: boundary[0].x, boundary[0].y, boundary[1].x, boundary[1].y (astar.py:26-27) */
  double velocity;   /* variant 3: AUV_velocity (astar_fixLenSOG.py:111) */
  double w[4];       /* weights (w1 unused by the searches, as in the reference) */
} auvp_astar_params;

typedef struct {
  int32_t status;        /* 0 ok; <0: capacity, or a state in which the reference raises (IndexError / TypeError) */
  int32_t found;         /* 0: open list ran empty -> the reference returns None */
  int32_t n_nodes, n_expansions;
  int32_t n_children;    /* neighbour cells that passed the bounds test (the "cells/s" unit) */
  int32_t path_len, smooth_len, n_hab_left, visited_count, leaf;
  uint32_t open_scanned_lo, open_scanned_hi; /* sum over pops of len(open_list) (the min-f scan, astar.py:206-211) */
} auvp_astar_summary;

/* starts [E,2]; goals [E,2] (variants 0,1) or limits [E] = pathLenLimit (variants 2,3) */
int auvp_astar_batch(auvp_handle* h, int32_t n_instances, const double* starts, const double* goals,
                     const double* limits, const auvp_astar_params* params, int32_t flags);
int auvp_astar_summaries(auvp_handle* h, auvp_astar_summary* out /* [E] */);
/* offsets [E+1] prefix sums of path_len.  path3 [n,3] root->leaf x,y,round(time_stamp,2); cost_list [n]
 * leaf->root ("cost list"); node_path8 [n,8] root->leaf x,y,g,h,f,cost,pathLen,time_stamp ("node");
 * smooth3 [n,3] smoothPath output (variant 3; smooth_len rows per instance, re-read the summaries) */
int auvp_astar_paths(auvp_handle* h, const int64_t* offsets, double* path3, double* cost_list, double* node_path8,
                     double* smooth3);
/* AUVP_FLAG_ITER_LOG: the popped node of every expansion, [n_expansions,8] like node_path8 */
int auvp_astar_exp_log(auvp_handle* h, int32_t instance, double* out8);
/* variant 2: indices of the habitats still in the caller's habitat_list after the call (:310,:193-197) */
int auvp_astar_hab_left(auvp_handle* h, int32_t instance, int32_t* out);
/* self.visited_nodes (astar_fixLen.py:51 [550,600]; astar_fixLenSOG.py:117 [600,600]) persists across
 * astar() calls on one solver object in the reference: upload it before a batch launched with
 * AUVP_FLAG_KEEP_VISITED ([E][vx*600] bytes, row-major [x_pos][y_pos]) and read it back afterwards */
int auvp_astar_set_visited(auvp_handle* h, int32_t n_instances, int32_t variant, const uint8_t* bitmap);
int auvp_astar_get_visited(auvp_handle* h, int32_t instance, uint8_t* bitmap);
/* A shark-occupancy table per search instance (astar_fixLenSOG, variant 3 only): auvp_astar_batch with instance e reading the
 * probabilities and the top-n heuristic table of probability set set_of[e] (auvp_world_set_prob_sets) in place of the world's.
 * The top-n tables of the sets are built on the device on the first call that needs them and kept until auvp_world_set or
 * auvp_world_set_prob_sets replaces what they were built from.  Flags, visited arrays, expansion log and every read-back call
 * are auvp_astar_batch's.  AUVP_ERR_STATE: no sets on the handle; AUVP_ERR_ARG: set_of[e] outside [0, n_sets) (the message
 * names e), params->variant != 3, or an instance names a set that holds a nan (the message names the set: a nan has no place
 * in the table's descending order).  A call that fails launches no search. */
int auvp_astar_batch_sets(auvp_handle* h, int32_t n_instances, const double* starts, const double* limits,
                          const auvp_astar_params* params, int32_t flags, const int32_t* set_of /* [E] */);
/* The sets' top-n tables as the searches read them: out [n_sets, T, C+1], out[g][t][0] = 0, out[g][t][i+1] = out[g][t][i] + the
 * i-th largest of prob[g][t] (get_top_n_prob, astar_fixLenSOG.py:516-531).  The rows of a set that holds a nan are unspecified. */
int auvp_astar_sets_topn(auvp_handle* h, double* out);

/* ---- shark occupancy / AUV detection grids ------------------------------------------------------
 * SharkOccupancyGrid.convert (path_planning/sharkOccupancyGrid.py:47-74): the producer of the
 * `sharkGrid` dict the A* SOG variant and createSharkGrid consume.  cells [C,4] = bounds of
 * cell_list (splitCell output, :376-393) in list order; box = boundary.bounds; traj_len [S] points
 * per shark in dict order; pts [sum(traj_len),3] = x, y, traj_time_stamp.  Outputs: n_bins
 * (createBinList :306-319), rows/cols (:134), bins [n_bins,2], grids [n_bins,rows,cols] = resultArr.
 * A cell whose index falls outside the grid is the reference's IndexError -> AUVP_ERR_ARG.
 * Call once with grids == NULL (or cap_bins == 0 -> AUVP_ERR_CAPACITY with the sizes filled in) to size
 * the output. */
int auvp_sog_convert(auvp_handle* h, const double* cells, int32_t n_cells, const double* box4, double cell_size,
                     double bin_interval, double detect_range, int32_t n_sharks, const int32_t* traj_len,
                     const double* pts_xyt, int32_t cap_bins, int32_t* n_bins, int32_t* rows, int32_t* cols,
                     double* bins, double* grids);

/* ---- shark particle filters ------------------------------------------------------------------------
 * particleFilter.py driven like robotSim.py:665-701, F independent filters x N particles (N <= 2048),
 * one workgroup per filter.  The reference draws from numpy's global legacy RandomState (its `random`
 * is numpy.random, particleFilter.py:8): each filter carries an MT19937 key [624] + position, handed
 * in and read back so a caller can continue numpy's own stream (np.random.get_state / set_state).
 * Particles are rows {x_p, y_p, v_p, theta_p, weight_p}; `obj` is the object id of a list position
 * (positions that hold the same Particle object after `correct` share an id and are moved once per
 * position by create_and_update, like the reference). */
enum { AUVP_PF_UPDATE = 1,  /* ParticleFilter.create_and_update (:277-282) */
       AUVP_PF_WEIGHTS = 2, /* ParticleFilter.update_weights (:285-310): weight, normalize, correct */
       AUVP_PF_MEAN = 4 };  /* particleMean + meanError (:153-177) */
/* ParticleFilter(x, y, ...).create() for F filters (:311-317, Particle.__init__ :44-53) */
int auvp_pf_create_batch(auvp_handle* h, int32_t n_filters, int32_t n_particles, const double* shark_xy0,
                         const uint32_t* mt_key, const int32_t* mt_pos);
/* start from caller-supplied lists instead: particles [F,N,5], obj [F,N] or NULL (all distinct),
 * list_len [F] or NULL.  Positions of a filter that share an object id are one Particle object: their
 * rows must be bitwise identical, else AUVP_ERR_ARG (the message names the filter and both positions). */
int auvp_pf_set_particles(auvp_handle* h, int32_t n_filters, int32_t n_particles, const double* particles,
                          const int32_t* obj, const int32_t* list_len, const uint32_t* mt_key, const int32_t* mt_pos);
int auvp_pf_set_rng(auvp_handle* h, const uint32_t* mt_key, const int32_t* mt_pos);
/* n_steps x the phases selected (AUVP_PF_* mask, in the order update, weights, mean) in ONE launch.
 * meas [S,F,n_auv,5] = list_of_range_bearing rows {x, y, theta, [3], [4]} (update_weights passes [3] as
 * the bearing and [4] as the range argument of Particle.weight, :293-295); shark_xy [S,F,2] =
 * self.x_shark / y_shark for meanError.  AUVP_FLAG_ITER_LOG records the per-step log below.
 * Per-filter status: 1 = an angle_wrap recursion deeper than CPython allows / nan, 2 = empty
 * list_of_new_particles (numpy raises ValueError). */
int auvp_pf_run(auvp_handle* h, int32_t n_steps, int32_t n_auv, int32_t phases, const double* meas,
                const double* shark_xy, int32_t flags);
/* auvp_pf_run with meas [S,F,n_auv,5] already in HBM on this handle's device (auvp_replan_measure of a planner's handle): copied
 * device to device into the handle's own buffer on its stream, so the producer's buffer is free again when the call returns.  The
 * producer must have synchronised its stream (auvp_replan_measure does).  Everything else as auvp_pf_run. */
int auvp_pf_run_dev_meas(auvp_handle* h, int32_t n_steps, int32_t n_auv, int32_t phases, const void* meas_dev,
                         const double* shark_xy, int32_t flags);
int auvp_pf_particles(auvp_handle* h, double* particles, int32_t* obj);
/* device-resident state for a caller that keeps working on the GPU: SoA [F][5][N] doubles, ids [F][N] */
int auvp_pf_particles_dev(auvp_handle* h, double** particles_soa, int32_t** obj);
/* of the last auvp_pf_run: mean [S,F,2], range_error [S,F], len(list_of_new_particles) [S,F] */
int auvp_pf_estimates(auvp_handle* h, double* mean, double* range_error, int32_t* list_len);
int auvp_pf_status(auvp_handle* h, int32_t* status, uint64_t* n_draw32);
int auvp_pf_rng_state(auvp_handle* h, uint32_t* mt_key, int32_t* mt_pos);
/* AUVP_FLAG_ITER_LOG: updated [S,F,N,5] (the list after create_and_update), choice [S,F,N] (the indices
 * random.choice drew in correct, :248-250) */
int auvp_pf_step_log(auvp_handle* h, double* updated, int32_t* choice);

/* ---- shark-occupancy forecast from the particle filters ---------------------------------------------
 * The link between the filters and the planners' time-binned occupancy table: for every filter, the
 * chain of SharkUpdate's methods (path_planning/sharkEstimate.py) in ONE launch, one wavefront per
 * filter, bit for bit what the host methods compute:
 *   counts      particles per grid entry: list position n counts in [int(qy)][int(qx)], qx = (x - minx) /
 *               cell_size, qy = (y - miny) / cell_size (cellToIndex's expression), iff 0 <= qx < cols and
 *               0 <= qy < rows compared in double; nan and out-of-grid particles are not counted
 *   correction  (:172-199) g = (counts / norm) * prior in the listed cells, total summed in list order,
 *               every grid entry / total.  total == 0 (ZeroDivisionError): status 1, that filter's
 *               grids and prob are all zeros, the other filters are unaffected
 *   rounds      G_0 = the corrected grid, G_{j+1} = prediction1(G_j, stay_prob) (method 1, :56-83) or
 *               prediction2(G_j, k, P_inf) (method 2, :85-103); P_inf = p_inf [rows,cols], or with NULL
 *               predictOnAve's grid (1 / n_cells in the listed cells).  Each round is exactly the host
 *               method; feeding a round's prediction into the next is what SharkUpdate.update's docstring
 *               intends and its code does not do (its second round raises).
 * box4 = boundary.bounds; rows / cols as the reference sizes its grids (int(ceil(extent) / cell_size) + 1);
 * cells [n_cells,4] = bounds of cell_list in list order.  A cell outside the grid (the reference:
 * IndexError or a wrapped negative index) and a cell listed twice are AUVP_ERR_ARG; rows * cols > 4096 is
 * AUVP_ERR_CAPACITY.  particles_xy [F,N,2] on the host, or NULL: the particles of this handle's filter
 * batch, read where they lie in HBM (n_filters / n_particles must be the batch's; AUVP_ERR_STATE without
 * one).  prior [F,rows,cols], or [rows,cols] with prior_is_shared.  Outputs (each may be NULL): grids
 * [F,n_rounds+1,rows,cols], prob [F,n_rounds+1,n_cells] = the same values in list order (the layout of
 * auvp_world_set's prob), counts [F,rows,cols], status [F]. */
int auvp_sf_forecast(auvp_handle* h, const double* box4, int32_t rows, int32_t cols, double cell_size, const double* cells,
                     int32_t n_cells, int32_t n_filters, const double* particles_xy, int32_t n_particles, const double* prior,
                     int32_t prior_is_shared, int32_t method, const double* p_inf, double stay_prob, double k, double norm,
                     int32_t n_rounds, double* grids, double* prob, int32_t* counts, int32_t* status);
/* The same forecast without the 4 096-entry limit: the same arguments, the same implementation, the same results bit for bit.
 * Up to 4 096 grid entries it launches the same kernel as auvp_sf_forecast; from 4 097 to 2^22 entries (a stated condition: one
 * grid of 32 MiB, every index far inside int32) sf_wide_kernel, one workgroup per filter, whose grids live in HBM -- in `grids`
 * itself: round j's grid is round j + 1's input; method 1 costs one workgroup barrier per level and round (a raster list of an
 * r x c grid: r + c - 1 levels; a snake list: one per cell).  Above 2^22 entries AUVP_ERR_CAPACITY, before anything is
 * allocated.  Device memory: n_filters * (n_rounds + 1) * rows * cols * 8 bytes for the grids whether or not `grids` is NULL
 * (3.6 GB for 1 024 filters x 11 bins of a 201 x 201 grid; a caller that plans from `prob` passes NULL and spares the copy to
 * the host); an allocation the device cannot provide is AUVP_ERR_HIP.  Options (auvp_set_option): SF_WIDE_MIN, the smallest rows
 * x cols that takes sf_wide_kernel here (default 4 097; 1: every grid), and SF_WIDE_BLOCK, its threads per workgroup (a multiple
 * of 64 in 64 .. 1 024, else AUVP_ERR_ARG). */
int auvp_sf_forecast_large(auvp_handle* h, const double* box4, int32_t rows, int32_t cols, double cell_size, const double* cells,
                           int32_t n_cells, int32_t n_filters, const double* particles_xy, int32_t n_particles,
                           const double* prior, int32_t prior_is_shared, int32_t method, const double* p_inf, double stay_prob,
                           double k, double norm, int32_t n_rounds, double* grids, double* prob, int32_t* counts,
                           int32_t* status);
/* name of the kernel the last completed forecast on this handle ran: "sf_forecast_kernel" or "sf_wide_kernel" ("": none) */
const char* auvp_sf_last_kernel(auvp_handle* h);
/* Which kernel a forecast would get, at what shape (no device needed; both entry points go through the same rule,
 * csrc/forecast_launch.h).  n_cells / widest_level: the list's length and the most cells of one level of its schedule
 * (auvp_sf_plan), 0 = not known -- carried for a finer rule, not read today.  allow_large: 0 = auvp_sf_forecast, 1 =
 * auvp_sf_forecast_large.  Options as in auvp_rrt_choose_launch. */
typedef struct {
  int32_t rows, cols, n_cells, widest_level, allow_large;
  int32_t n_options;
  const char* const* option_names;
  const int64_t* option_values;
} auvp_sf_launch_query;
enum { AUVP_SF_ONE_WAVE = 0, AUVP_SF_WIDE };
typedef struct {
  int32_t status; /* AUVP_OK; AUVP_ERR_CAPACITY: more grid entries than the entry point takes; AUVP_ERR_ARG: a shape < 1, a bad SF_WIDE_BLOCK */
  int32_t kind;   /* AUVP_SF_* */
  int32_t block, lds; /* threads per workgroup (one workgroup per filter); its LDS bytes, static + dynamic */
  const char* name;   /* what auvp_sf_last_kernel would report */
} auvp_sf_launch_choice;
int auvp_sf_choose_launch(const auvp_sf_launch_query* query, auvp_sf_launch_choice* choice);
/* The device copy of the last forecast's prob [n_filters, n_rounds+1, n_cells], for auvp_world_set_prob_sets(prob_dev) of a
 * planner's handle: the tables go from the forecast to the planner without leaving HBM.  auvp_sf_forecast (and _large) synchronises its
 * stream before it returns, so a copy enqueued afterwards on another handle's stream on the same device is ordered behind the
 * forecast.  The pointer is valid until the next auvp_sf_forecast / auvp_sf_forecast_large on this handle or its destruction.
 * AUVP_ERR_STATE without a completed forecast.  Each output may be NULL. */
int auvp_sf_prob_dev(auvp_handle* h, const void** prob_dev, int32_t* n_filters, int32_t* n_bins, int32_t* n_cells);
/* The schedule the forecast kernel walks for method 1 (no device needed): cell_rc [n_cells,2] = (row,
 * column) per list position.  level [n_cells]: 0 where no 4-neighbour is earlier in the list, else 1 + the
 * highest level among the earlier neighbours; order [n_cells]: list positions sorted by (level, position);
 * level_off [up to n_cells + 1]: level l = order[level_off[l] .. level_off[l+1]); n_levels.  AUVP_ERR_ARG:
 * a cell outside the rows x cols grid, a cell listed twice, an empty list. */
int auvp_sf_plan(int32_t rows, int32_t cols, const int32_t* cell_rc, int32_t n_cells, int32_t* level, int32_t* order,
                 int32_t* level_off, int32_t* n_levels);

/* standalone evaluations on the device (parity probes for the building blocks) */
/* RRT.check_collision (:530-549) of n_paths paths; pts [sum(npts),2], path i = pts[off[i]:off[i+1]] */
int auvp_check_collision_batch(auvp_handle* h, int32_t n_paths, const int32_t* off, const double* pts_xy,
                               int8_t* out_free);
/* habitat_shark_cost_func (path_planning/cost.py:145-207) over bins [bin_lo,bin_hi) */
int auvp_cost_paths(auvp_handle* h, int32_t n_paths, const int32_t* off, const double* pts_xyt,
                    const int32_t* bin_lo, const int32_t* bin_hi, const double* total_traj_time,
                    const double* weights3, double* out4);
/* RRT.get_closest_mps (path_planning/rrt_dubins.py:505-513) for n_queries sample points against one node list xy
 * [n_nodes,2]: index of the FIRST node with the smallest RN(sqrt(dx**2 + dy**2)), by the planner's streaming scan.
 * force_exact != 0 ranks with a sqrt per node (the scan's fallback path); out_slow (optional) reports per query whether
 * that path ran */
int auvp_nn_closest_batch(auvp_handle* h, int32_t n_nodes, const double* xy, int32_t n_queries, const double* q,
                          int32_t force_exact, int32_t* out_index, int32_t* out_slow);
/* Measured HBM streaming rates of this GPU (the roof bench.py quotes its bandwidth fractions against, beside the 8 TB/s
 * datasheet figure): a read of `bytes` (>= 64 MB; use >= 4 GB to get past the 256 MB Infinity Cache) with eight 16-byte
 * loads in flight per lane -- the access shape of the nearest-neighbour scan of get_closest_mps
 * (path_planning/rrt_dubins.py:505-513) -- and a 16-byte copy of one half of the buffer onto the other; best of `reps`
 * launches each, HIP events on the handle's stream.  GB/s = 1e9 bytes per second; copy counts bytes read + written.
 * (No reference counterpart: measurement infrastructure of the boundary.) */
int auvp_hbm_probe(auvp_handle* h, uint64_t bytes, int32_t reps, double* read_GBps, double* copy_GBps);
/* portable sin/cos evaluated on the device (bit-exactness probe for auvp_math.h) */
int auvp_sincos_dev(auvp_handle* h, int32_t n, const double* x, double* s, double* c);
/* one portable elementary function of auv_sim_amd/csrc/auvp_math.h / auvp_exp.h evaluated on the device over n operand pairs
 * (bit-exactness probe: the tests compare with the host build of the same header and with the IEEE operation).  op: 0 sin -> out0,
 * cos -> out1 of a (math.sin / math.cos, path_planning/rrt_dubins.py:275-276); 1 atan2(a, b) (gym_rrt/envs/rrt_dubins.py:387);
 * 2 math.e ** a (particleFilter.py:103-116); 3 the steer's short division a / b and 4 its square root (rrt_dubins.py:268-281;
 * operands of unexceptional magnitude: auvp_div_plain / auvp_sqrt_plain); 5 hypot(a, b); 6 a / b and 7 sqrt(a) as compiled.
 * The forms only device code has, as the kernels call them: 8 sin / cos with the constants in scalar registers (auvp_sincos_sk);
 * 9 atan2(a, b) with late constants (auvp_atan2_late); 10 math.e ** a reading the table's copy in LDS (auvp_pow_e_t); 11 the
 * bearing of auvp_replan_measure without the heading, replan_atan2_round(a, b, auvp_atan2_late(a, b)); 12 atan(a). */
int auvp_math_dev(auvp_handle* h, int32_t op, int32_t n, const double* a, const double* b, double* out0, double* out1);
/* the four-episode RRT kernels' ordered theta sum (rows_theta_chain_dpp, auv_sim_amd/csrc/rrt_rows_kernel.h) on its own, n_waves
 * wavefronts of four 16-lane rows: theta0 [n_waves * 4] one start angle per row, phi [n_waves * 64] one addend per lane; out
 * [n_waves * 64], lane rl of a row gets (((theta0 + phi_0) + phi_1) + ... + phi_rl) of its row; fifteen steps, so lane 15 gets lane 14's sum (bit-exactness probe: the sums of
 * theta += phi in path_planning/rrt_dubins.py:268-281, left to right) */
int auvp_theta_chain_dev(auvp_handle* h, int32_t n_waves, const double* theta0, const double* phi, double* out);
/* the end of a steer pass of the four-episode RRT kernels on its own (rows_idle_zero, rows_sums_chain, rows_pass_ends_dpp,
 * auv_sim_amd/csrc/rrt_rows_kernel.h), n_waves wavefronts of four 16-lane rows: head [n_waves * 4][7] per row n (1 .. 15 sub-arcs),
 * on (0 / 1), the start x, y, t, length, theta; incs [n_waves][5][64] what each lane adds to x, y, t, length, theta (lanes from n on
 * add the kernels' idle value instead); out [n_waves][5][64] the row's x, y, t, length, theta after the pass as every lane of the
 * row holds them: the left-to-right sums over the first n lanes, or the start values for a row that is not on (bit-exactness probe) */
int auvp_row_ends_dev(auvp_handle* h, int32_t n_waves, const double* head, const double* incs, double* out);
/* CPython random() stream of `seed` generated by the wave-level device MT19937 */
int auvp_random_stream_dev(auvp_handle* h, uint64_t seed, int32_t n, double* out);

/* diagnostic: shader clocks each episode spent in {parent selection, steer, collision, accept, cost
 * walk} (needs AUVP_FLAG_PHASE_CLOCKS); out [E,5] */
int auvp_rrt_phase_clocks(auvp_handle* h, uint64_t* out);
/* HIP-event time (ms) of the last batch kernel on the handle's stream, and its launch geometry */
double auvp_last_kernel_ms(auvp_handle* h);
/* of the last auvp_rrt_run: HIP-event times of its two launches (tree expansion; leaf ranking) and which expansion
 * kernel ran (4 = four episodes per wavefront, rrt_rows_kernel; 1 = rrt_explore_kernel) */
int auvp_rrt_last_launch_parts(auvp_handle* h, double* expand_ms, double* leaf_ms, int32_t* episodes_per_wave);
/* ... and of the launch that generated the episodes' random numbers ahead of it (rrt_stream_kernel; 0 when the last auvp_rrt_run
 * ran the generator inside the expansion kernel).  auvp_last_kernel_ms covers all three launches. */
double auvp_rrt_last_stream_ms(auvp_handle* h);
/* ... and how many random() numbers per episode that launch wrote (8 bytes each; 0: none) */
int64_t auvp_rrt_last_stream_len(auvp_handle* h);
/* ... and the form of the LDS ring rrt_rows_stream_kernel read them through: 1 its first 48 entries mirrored behind it, 0 every
 * read masked (-1: the last auvp_rrt_run launched another expansion kernel) */
int auvp_rrt_last_stream_mirror(auvp_handle* h);
/* The launch the host would choose for rrt_rows_stream_kernel (no device needed): K time bins, a world with these table sizes,
 * waves_wanted wavefronts per workgroup (1 .. 12), force < 0 the host's rule / 0 the masked / 1 the mirrored ring.  Out: the
 * wavefronts per workgroup, the ring's form, the workgroup's LDS bytes.  The rule never gives up a wavefront for the mirror. */
int auvp_rrt_rows_stream_shape(int32_t K, int32_t n_habitats, int32_t n_poly, int32_t n_bins, int32_t waves_wanted, int32_t force,
                               int32_t* waves, int32_t* mirror, int32_t* lds_bytes);
/* The whole choice of a launch as a question (no device needed; the library's own launches go through the same rules,
 * csrc/launch_plan.h): which expansion kernel a batch of RRT.exploring would get, at what shape.  The query describes the batch
 * (as auvp_rrt_prepare + auvp_world_set would), the device (n_cu compute units) and the options that are SET: n_options names
 * (without the AUVP_ prefix) and values; an unknown name is AUVP_ERR_ARG.  seen_most / seen_E: what earlier batches with the same
 * parameter block drew (the most random() numbers of one episode, the largest batch; 0 = nothing seen). */
typedef struct {
  int32_t n_episodes, n_cu;
  int32_t mode, max_iter, n_time_bins /* K = ceil(max_traj_time / bin_interval); 0 outside time-bin mode */, flags /* AUVP_FLAG_* */;
  double freq, dist_to_end;
  int32_t max_pts; /* floor(freq) + 2 */
  int32_t n_obstacles, n_habitats, n_poly, n_bins;
  double obst_area; /* area of the bounding box of the obstacle centres (0: fewer than two obstacles) */
  int32_t per_episode_limits, one_wave_only, no_stream; /* auvp_rrt_prepare_episodes; the two fallback passes of auvp_rrt_run */
  int32_t seen_E;
  int64_t seen_most;
  int32_t n_options;
  const char* const* option_names;
  const int64_t* option_values;
} auvp_rrt_launch_query;
enum { AUVP_RRT_EXPLORE = 0, AUVP_RRT_EXPLORE_LIM, AUVP_RRT_DUO, AUVP_RRT_TRIO, AUVP_RRT_ROWS, AUVP_RRT_ROWS_STREAM };
typedef struct {
  int32_t status;    /* AUVP_OK, or AUVP_ERR_ARG: the LDS plan needs lds_need bytes > 160 KiB (auvp_rrt_run fails with that) */
  int32_t kind;      /* AUVP_RRT_* */
  int32_t J, quad;   /* obstacles per lane; rrt_trio_kernel with four wavefronts per episode */
  int32_t grid, block, lds, lds_max; /* lds_max: the kernel's dynamic-LDS attribute */
  int32_t kflags;    /* 1024: the tight cull, 2048: exact nearest-neighbour ranking */
  int32_t stream_waves, mirror; /* rrt_rows_stream_kernel: wavefronts per workgroup, the ring's form */
  int32_t _pad;
  int64_t stream_len; /* ... random() numbers per episode generated ahead */
  int64_t lds_need;
  const char* name;  /* what auvp_rrt_last_kernel would report */
} auvp_rrt_launch_choice;
int auvp_rrt_choose_launch(const auvp_rrt_launch_query* query, auvp_rrt_launch_choice* choice);
/* the same for a launch of Planner_RRT (auvp_prrt_plan: step_mode 0, waits 1; auvp_prrt_step: step_mode 1, waits 1; a step of
 * the device-resident loop: step_mode 1, waits 0).  rows: -1 decide the four-episode choice as auvp_prrt_create_batch does
 * (once per batch), 0 / 1 the batch's frozen value. */
typedef struct {
  int32_t n_episodes, n_cu, n_obstacles;
  int32_t max_pts /* floor(freq) + 3 */, cap_nodes /* max_step + 1 */, n_buckets, max_step, flags;
  double freq;
  int32_t step_mode, waits, one_wave_only, rows;
  int32_t n_options, _pad;
  const char* const* option_names;
  const int64_t* option_values;
} auvp_prrt_launch_query;
enum { AUVP_PRRT_ONE = 0, AUVP_PRRT_PIPE, AUVP_PRRT_ROWS };
typedef struct {
  int32_t status;  /* AUVP_OK, or AUVP_ERR_ARG: prrt_kernel's LDS plan needs lds_need bytes > 160 KiB */
  int32_t kind;    /* AUVP_PRRT_* */
  int32_t lat, rows, pipe, draw_wave; /* latency batch; four episodes per wavefront; the pipeline; its fifth wavefront */
  int32_t next_lds, bk_lds, obst_lds; /* pipeline: next links / bucket table in LDS; rows: the obstacle tile in LDS */
  int32_t eps_wg, grid, block, lds, J;
  int64_t lds_need;
  const char* name; /* what auvp_prrt_last_kernel would report */
} auvp_prrt_launch_choice;
int auvp_prrt_choose_launch(const auvp_prrt_launch_query* query, auvp_prrt_launch_choice* choice);
/* name of the expansion kernel the last auvp_rrt_run launched: "rrt_rows_kernel" (four episodes per wavefront: batches of
 * more than 18 episodes per CU; "rrt_rows_stream_kernel": the same with the random numbers generated ahead by
 * rrt_stream_kernel), "rrt_explore_kernel" (one), "rrt_duo_kernel" (two wavefronts per episode: batches of at
 * most four episodes per CU in time-bin mode -- the helper wavefront produces the half of an iteration that depends only on
 * the random stream, rrt_dubins.py:121-127,252-281, one iteration ahead) */
const char* auvp_rrt_last_kernel(auvp_handle* h);
/* of the last auvp_rrt_run's leaf pass (the qualifying-leaf bookkeeping of exploring, rrt_dubins.py:158-171 +
 * cost.py:145-207), summed over the batch: out4 = {nodes its sweep visited (qualifying leaves and their ancestors), path
 * points of those nodes (each evaluated once), path elements re-summed in the reference's leaf->root order, leaves
 * re-summed}: the units of that kernel's compulsory-traffic figure */
int auvp_rrt_last_leaf_stats(auvp_handle* h, int64_t* out4);
int auvp_last_launch(auvp_handle* h, int32_t* grid, int32_t* block, int32_t* lds_bytes);

/* Config 5 composition (BASELINE.json configs[4]): the particle filter of particleFilter.py:283-317 feeding one
 * Planner_RRT replan per particle (gym_rrt/envs/rrt_dubins.py:162-248), without leaving the device.
 * Needs a filter batch on this handle (auvp_pf_create_batch / auvp_pf_run).  Episode e = f * N + p plans from the
 * shared start4 (x, y, theta, traj_time_stamp) to goal = clamp(particle(f, p).xy * scale_f + offset_f):
 *   xform [F,4] = sx, ox, sy, oy per filter (gx = x * sx + ox, gy = y * sy + oy);   clamp4 = x0, y0, x1, y1
 * with the generator of random.seed(seed_base + e), seeded on the device.  Replaces Planner_RRT.__init__ per
 * particle; follow with auvp_prrt_plan() and the auvp_prrt_* readers. */
int auvp_prrt_replan_particles(auvp_handle* h, const double* start4, const auvp_prrt_params* params, const double* xform,
                               const double* clamp4, uint64_t seed_base, int32_t flags);

/* ---------------------------------------------------------------------------------------------------
 * Multi-GPU result gather (SURVEY.md 8(b) "auvp_gather(comm...)", 8(e)).  The reference is single-process;
 * what these replace is the implicit "results are in this process" of its batch callers
 * (path_planning/performance.py:65-73 collects one result per exploring() call in a Python list).  One
 * process per GPU plans a block of the episode index; afterwards every rank holds every record.
 * Collectives are RCCL (bound at run time) on the handle's stream; all buffers are DEVICE pointers.
 *   auvp_comm_unique_id  rank 0 creates the 128-byte id and hands it to the other ranks (any channel)
 *   auvp_comm_init       every rank, same id: joins the communicator (collective)
 *   auvp_gather          all-gather of equally sized blocks: recv_dev [world][bytes_per_rank]
 *   auvp_gather_var      variable-size blocks, two-phase: counts_out[world] always receives every rank's byte
 *                        count; with recv_dev == NULL only that (size query), else the blocks are written back
 *                        to back in rank order.  Whether the payload phase runs is decided COLLECTIVELY (every rank
 *                        also publishes its capacity): it runs only if every rank passed a buffer that holds
 *                        sum(counts); otherwise every rank returns after the counts (AUVP_ERR_CAPACITY on the ranks
 *                        that passed a buffer), none is left waiting
 *   auvp_gather_counts / auvp_gather_blocks   the two phases as separate calls, for a caller that sizes its
 *                        buffer between them (one count exchange instead of two); counts must be the array
 *                        auvp_gather_counts returned, unchanged, on every rank
 *   auvp_comm_available  1 if an RCCL can be bound in this process (no communicator, no bootstrap thread is created)
 *   auvp_comm_library    path of the RCCL image that was bound (an already mapped one -- PyTorch's -- is preferred
 *                        over opening a second image), or the reason none could be
 *   auvp_comm_info       communicator facts for self-checking runs: world size given, rank and rank count as RCCL
 *                        reports them (ncclCommUserRank, ncclCommCount)
 *   auvp_last_gather_ms  HIP-event time of the last gather on the handle's stream */
#define AUVP_COMM_ID_BYTES 128
int auvp_comm_unique_id(uint8_t* id_out /* [AUVP_COMM_ID_BYTES] */);
int auvp_comm_init(auvp_handle* h, int32_t world_size, int32_t rank, const uint8_t* id);
int auvp_comm_destroy(auvp_handle* h);
int auvp_gather(auvp_handle* h, const void* send_dev, size_t bytes_per_rank, void* recv_dev);
int auvp_gather_var(auvp_handle* h, const void* send_dev, int64_t send_bytes, void* recv_dev, int64_t recv_cap_bytes,
                    int64_t* counts_out);
int auvp_gather_counts(auvp_handle* h, int64_t send_bytes, int64_t* counts_out /* [world] */);
int auvp_gather_blocks(auvp_handle* h, const void* send_dev, void* recv_dev, int64_t recv_cap_bytes,
                       const int64_t* counts /* [world] */);
/* Gather to ONE rank -- what north_star asks for ("an RCCL gather of final paths"); the all-gathers above hand every rank every
 * record.  rank r's block lands at the prefix offset of r in the ROOT's recv_dev (the other ranks pass NULL / 0): one group of
 * ncclSend / ncclRecv, every peer over its own xGMI link.  `counts` [world] as auvp_gather_counts returned them, or computed
 * by the caller where the block sizes are known (fixed-stride records of a block partition).
 *   auvp_gather_blocks_root        the transfer, waited for
 *   auvp_gather_blocks_root_async  the same ENQUEUED on the handle's gather stream -- a second stream, ordered behind what the
 *                                  planner stream holds at the call -- so that the transfer of step k overlaps the kernels
 *                                  of step k + 1.  May be called several times (records, lengths, paths); send_dev and the
 *                                  root's recv_dev must stay untouched until auvp_gather_wait.  No other collective of this
 *                                  handle may be issued while transfers are pending.
 *   auvp_gather_wait               waits for the pending transfers; ms_out = their HIP-event time on the gather stream (first
 *                                  enqueue to completion, waiting for the planner stream's event included), bytes_out = what
 *                                  this rank sent (on the root: received, its own block included).  No-op without pending ones.
 * An RCCL without ncclSend / ncclRecv: AUVP_ERR_COMM (world size 1 needs neither). */
int auvp_gather_blocks_root(auvp_handle* h, int32_t root, const void* send_dev, void* recv_dev, int64_t recv_cap_bytes,
                            const int64_t* counts /* [world] */);
int auvp_gather_blocks_root_async(auvp_handle* h, int32_t root, const void* send_dev, void* recv_dev, int64_t recv_cap_bytes,
                                  const int64_t* counts /* [world] */);
int auvp_gather_wait(auvp_handle* h, double* ms_out, int64_t* bytes_out);
int auvp_comm_available(void);
const char* auvp_comm_library(void);
int auvp_comm_info(auvp_handle* h, int32_t* world_size, int32_t* rank, int32_t* rccl_ranks_seen);
double auvp_last_gather_ms(auvp_handle* h);

#ifdef __cplusplus
}
#endif
#endif

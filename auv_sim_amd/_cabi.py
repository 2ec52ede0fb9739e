"""The C-ABI of libauvplan.so (include/auvplan.h) as ctypes sees it: the public structs, the constants and ONE table of the
entry points' prototypes.  Nothing else in the package assigns a restype or an argtypes: `_lib.load()` calls `bind` once.
tests/test_cabi_prototypes.py checks the table against the header and the structs against the C compiler's layout.

How a header type appears in the table:
    int, int32_t, int64_t, uint64_t, double, size_t     the ctypes scalar of that type
    const char*                                         c_char_p (parameter and return)
    auvp_handle*, void*, const void*                    c_void_p
    T* filled from / read into a host numpy array       POINTER(ctype of T)
    T* that takes a device address (data_ptr()), or an array of records passed from numpy        c_void_p
    a public struct passed byref                        POINTER(its Structure)
    X**                                                 POINTER(c_void_p)
    returns void / void*                                None / c_void_p
"""
import ctypes as C

import numpy as np

# ---- constants (the header's enums) ----
OK, NO_QUALIFYING_LEAF = 0, 1
MODES = {"timebin": 0, "plantime": 1, "nn": 2}
FLAG_ITER_LOG, FLAG_LEAF_LOG, FLAG_PHASE_CLOCKS = 1, 2, 4
KFLAG_TIGHT_CULL, KFLAG_NN_EXACT = 1024, 2048  # auvp_rrt_launch_choice.kflags
# the options of a handle (auvp_set_option).  AUVP_<NAME> in the environment is read ONCE per handle, by
# auvp_create.
OPTION_NAMES = ("ROWS", "DUO", "TRIO", "QUAD", "TIGHT_CULL", "NN_EXACT", "LEAF_SWEEP_ALL", "NO_HABITAT_GRID", "RG_MAX_ENTRIES",
                "NO_GRID_INDEX", "PRRT_LAT", "PRRT_PIPE", "PRRT_OBST_LDS", "PRRT_NEXT_LDS", "PRRT_ROWS", "ASTAR_NO_GRID",
                "ASTAR_NO_LIST", "ASTAR_PAIR", "SOG_TILE", "PIPE_FALLBACK", "PRRT_PIPE_DRAW", "PRRT_BUCKET_LDS", "ROWS_STREAM", "ROWS_STREAM_CAP", "ROWS_STREAM_WAVES",
                "ROWS_WG_WAVES", "ROWS_STREAM_MIRROR", "PRRT_ROWS_GRID", "SF_WIDE_MIN", "SF_WIDE_BLOCK", "MEAS_TICKS")

# ---- the type vocabulary of the table ----
i, i32, i64, u64, f64, sz, s = C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_double, C.c_size_t, C.c_char_p
h = vp = C.c_void_p  # h: the auvp_handle*
P = C.POINTER
dp, ip, bp, i64p = P(C.c_double), P(C.c_int32), P(C.c_int8), P(C.c_int64)
u8p, u32p, u64p, vpp = P(C.c_uint8), P(C.c_uint32), P(C.c_uint64), P(C.c_void_p)


def _i32s(*names):
    return [(n, i32) for n in names]


# ---- the public structs, field for field as the header declares them ----
class RRTParams(C.Structure):
    _fields_ = [("dist_to_end", f64), ("diff_max", f64), ("freq", f64), ("min_dist", f64), ("bin_interval", f64), ("v", f64),
                ("max_traj_time", f64), ("max_plan_time", f64), ("w", f64 * 3), ("mode", i32), ("max_iter", i32),
                ("points_per_iter", f64)]


class RRTSummary(C.Structure):
    _fields_ = _i32s("status", "n_nodes", "n_points", "n_leaves", "best_leaf", "best_path_len", "iters_run", "n_candidates") + \
               [("best_cost", f64 * 4), ("best_length", f64), ("rng_after", f64), ("leaf_elems", i64), ("n_draw32", u64),
                ("nn_scanned", u64)]


class RRTEpisode(C.Structure):
    """one episode's own horizon and habitat list (bit h = habitat h of the world's table)"""
    _fields_ = [("max_traj_time", f64), ("habitat_keep", u64)]


class RRTGroupBest(C.Structure):
    """the winner of one group of episodes"""
    _fields_ = _i32s("status", "winner", "n_with_leaf", "path_len") + [("cost", f64 * 4), ("length", f64)]


class ReplanRecord(C.Structure):
    """one AUV's round of the device commit step"""
    _fields_ = _i32s("status", "winner", "n_committed", "path_len") + \
               [("cost", f64 * 4), ("last", f64 * 7), ("keep", u64), ("claimed", u64), ("conflicts", i32), ("_reserved", i32)]


class PrrtParams(C.Structure):
    _fields_ = [("rect", f64 * 4), ("exp_rate", f64), ("dist_to_end", f64), ("diff_max", f64), ("freq", f64),
                ("cell_side_length", f64), ("subsections", i32), ("max_step", i32)]


class PrrtSummary(C.Structure):
    _fields_ = _i32s("status", "n_nodes", "n_points", "n_occ", "steps", "done", "path_len", "last_node", "last_accepted",
                     "last_new_node", "n_arc", "_pad") + [("arc", f64 * 6), ("rng_after", f64), ("n_draw32", u64)]


class AstarParams(C.Structure):
    _fields_ = [("variant", i32), ("cap_nodes", i32), ("box", f64 * 4), ("velocity", f64), ("w", f64 * 4)]


class AstarSummary(C.Structure):
    _fields_ = _i32s("status", "found", "n_nodes", "n_expansions", "n_children", "path_len", "smooth_len", "n_hab_left",
                     "visited_count", "leaf") + [("open_scanned_lo", C.c_uint32), ("open_scanned_hi", C.c_uint32)]


_OPTIONS = [("option_names", P(s)), ("option_values", i64p)]


class _RrtLaunchQuery(C.Structure):
    _fields_ = _i32s("n_episodes", "n_cu", "mode", "max_iter", "n_time_bins", "flags") + [("freq", f64), ("dist_to_end", f64)] + \
               _i32s("max_pts", "n_obstacles", "n_habitats", "n_poly", "n_bins") + [("obst_area", f64)] + \
               _i32s("per_episode_limits", "one_wave_only", "no_stream", "seen_E") + [("seen_most", i64), ("n_options", i32)] + _OPTIONS


class _RrtLaunchChoice(C.Structure):
    _fields_ = _i32s("status", "kind", "J", "quad", "grid", "block", "lds", "lds_max", "kflags", "stream_waves", "mirror", "_pad") + \
               [("stream_len", i64), ("lds_need", i64), ("name", s)]


class _PrrtLaunchQuery(C.Structure):
    _fields_ = _i32s("n_episodes", "n_cu", "n_obstacles", "max_pts", "cap_nodes", "n_buckets", "max_step", "flags") + [("freq", f64)] + \
               _i32s("step_mode", "waits", "one_wave_only", "rows", "n_options", "_pad") + _OPTIONS


class _PrrtLaunchChoice(C.Structure):
    _fields_ = _i32s("status", "kind", "lat", "rows", "pipe", "draw_wave", "next_lds", "bk_lds", "obst_lds", "eps_wg", "grid", "block",
                     "lds", "J") + [("lds_need", i64), ("name", s)]


class _SfLaunchQuery(C.Structure):
    _fields_ = _i32s("rows", "cols", "n_cells", "widest_level", "allow_large", "n_options") + _OPTIONS


class _SfLaunchChoice(C.Structure):
    _fields_ = _i32s("status", "kind", "block", "lds") + [("name", s)]


# C struct name -> Structure
STRUCTS = {"auvp_rrt_params": RRTParams, "auvp_rrt_summary": RRTSummary, "auvp_rrt_episode": RRTEpisode,
           "auvp_rrt_group_best": RRTGroupBest, "auvp_replan_record": ReplanRecord, "auvp_prrt_params": PrrtParams,
           "auvp_prrt_summary": PrrtSummary, "auvp_astar_params": AstarParams, "auvp_astar_summary": AstarSummary,
           "auvp_rrt_launch_query": _RrtLaunchQuery, "auvp_rrt_launch_choice": _RrtLaunchChoice,
           "auvp_prrt_launch_query": _PrrtLaunchQuery, "auvp_prrt_launch_choice": _PrrtLaunchChoice,
           "auvp_sf_launch_query": _SfLaunchQuery, "auvp_sf_launch_choice": _SfLaunchChoice}


def _astar_summary_dtype():
    """np.dtype(AstarSummary) with the two 32-bit halves of the open-list counter read as the one uint64 they form"""
    d = np.dtype(AstarSummary)
    names = [n for n in d.names if not n.startswith("open_scanned")]
    return np.dtype(dict(names=names + ["open_scanned"], formats=[d.fields[n][0] for n in names] + ["<u8"],
                         offsets=[d.fields[n][1] for n in names] + [d.fields["open_scanned_lo"][1]], itemsize=d.itemsize))


# the records as numpy reads them: the layout is the Structure's
SUMMARY_DTYPE, EPISODE_DTYPE, GROUP_BEST_DTYPE = np.dtype(RRTSummary), np.dtype(RRTEpisode), np.dtype(RRTGroupBest)
REPLAN_RECORD_DTYPE, PRRT_SUMMARY_DTYPE, ASTAR_SUMMARY_DTYPE = np.dtype(ReplanRecord), np.dtype(PrrtSummary), _astar_summary_dtype()

_rp, _pp, _ap = P(RRTParams), P(PrrtParams), P(AstarParams)
_forecast = (i, (h, dp, i32, i32, f64, dp, i32, i32, dp, i32, dp, i32, i32, dp, f64, f64, f64, i32, dp, dp, ip, ip))
_pick_courses = (h, i32, ip, u64p, i32, ip, i32, i64p, dp, dp, dp, dp, ip, ip, dp)

# every entry point of the header: name -> (return type, parameter types), in the header's order
PROTOTYPES = {
    "auvp_version": (s, ()),
    "auvp_create": (i, (i, vpp)),
    "auvp_destroy": (None, (h,)),
    "auvp_set_option": (i, (h, s, i64)),
    "auvp_unset_option": (i, (h, s)),
    "auvp_get_option": (i, (h, s, ip, i64p)),
    "auvp_pipeline_fallbacks": (i, (h, ip, i64p)),
    "auvp_last_error": (s, (h,)),
    "auvp_world_set": (i, (h, dp, i32, dp, i32, dp, i32, dp, i32, dp, i32, dp)),
    "auvp_world_set_habitats": (i, (h, dp, i32)),
    "auvp_rrt_explore_batch": (i, (h, i32, dp, u64p, _rp, i32)),
    "auvp_rrt_prepare": (i, (h, i32, dp, u64p, _rp, i32)),
    "auvp_rrt_prepare_states": (i, (h, i32, dp, u32p, ip, _rp, i32)),
    "auvp_rrt_prepare_episodes": (i, (h, i32, dp, u64p, u32p, ip, _rp, vp, i32)),
    "auvp_rrt_run": (i, (h,)),
    "auvp_rrt_summaries": (i, (h, vp)),
    "auvp_rrt_paths": (i, (h, i64p, dp)),
    "auvp_rrt_paths_dev": (i, (h, i64p, vp)),
    "auvp_rrt_tree": (i, (h, i32, dp, ip, ip, ip, dp)),
    "auvp_rrt_iter_log": (i, (h, i32, ip, bp, ip)),
    "auvp_rrt_leaf_log": (i, (h, i32, dp, ip)),
    "auvp_rrt_bin_sizes": (i, (h, i32, ip, ip)),
    "auvp_rrt_summaries_dev": (vp, (h,)),
    "auvp_rrt_group_best": (i, (h, i32, ip, vp)),
    "auvp_rrt_group_best_dev": (vp, (h,)),
    "auvp_rrt_group_paths": (i, (h, i64p, dp)),
    "auvp_rrt_group_paths_dev": (i, (h, i64p, vp)),
    "auvp_world_set_prob_sets": (i, (h, i32, dp, vp)),
    "auvp_world_set_prob_sets_placed": (i, (h, vp, i32, i32, i32, i32)),
    "auvp_world_prob_sets_read": (i, (h, ip, dp)),
    "auvp_world_prob_set_stats": (i, (h, dp, ip)),
    "auvp_rrt_set_episode_grids": (i, (h, i32, ip)),
    "auvp_rrt_rerank": (i, (h,)),
    "auvp_replan_begin": (i, (h, i32, dp, u64p, i32)),
    "auvp_replan_set_teams": (i, (h, i32, ip)),
    "auvp_replan_team_fold": (i, (h, i32, ip, u64p)),
    "auvp_replan_commit": (i, (h, i32, ip, f64, vp)),
    "auvp_replan_measure": (i, (h, ip, i32, dp, vpp)),
    "auvp_replan_meas": (i, (h, ip, ip, dp)),
    "auvp_replan_team_pick": (i, (h, i32, ip, i32, vp)),
    "auvp_replan_team_pick_courses": (i, _pick_courses + (vp, u64p)),
    "auvp_replan_team_pick_apart": (i, (h, i32, ip, i32, i32, f64, f64, i32, vp)),
    "auvp_replan_team_pick_apart_courses": (i, _pick_courses + (i32, f64, f64, i32, vp, u64p, ip)),
    "auvp_replan_traj": (i, (h, i64p, dp)),
    "auvp_replan_commit_courses": (i, (h, i32, i64p, dp, dp, u64p, f64, vp, dp)),
    "auvp_replan_info": (i, (h, ip, ip, i64p, i64p, i64p, dp)),
    "auvp_prrt_create_batch": (i, (h, i32, dp, dp, _pp, u64p, u32p, ip, i32)),
    "auvp_prrt_plan": (i, (h,)),
    "auvp_prrt_step": (i, (h, ip, u32p, ip)),
    "auvp_prrt_summaries": (i, (h, vp)),
    "auvp_prrt_goals": (i, (h, dp)),
    "auvp_prrt_paths": (i, (h, i64p, dp)),
    "auvp_prrt_tree": (i, (h, i32, dp, ip, ip, dp)),
    "auvp_prrt_node": (i, (h, i32, i32, dp, ip, ip, dp, i32)),
    "auvp_prrt_grid": (i, (h, i32, ip, ip, ip)),
    "auvp_prrt_step_log": (i, (h, i32, ip)),
    "auvp_prrt_summaries_dev": (vp, (h,)),
    "auvp_prrt_last_kernel": (s, (h,)),
    "auvp_prrt_observation_dev": (i, (h, vp, vp, vp)),
    "auvp_prrt_observation": (i, (h, i32, dp, i64p, i64p)),
    "auvp_prrt_env_step_dev": (i, (h, vp, vp, vp, vp, vp, vp)),
    "auvp_prrt_env_step_ex_dev": (i, (h, i32, u64, vp, vp, vp, vp, vp, vp)),
    "auvp_prrt_policy_random_dev": (i, (h, vp, u64, vp)),
    "auvp_prrt_env_check": (i, (h, ip, ip)),
    "auvp_stream": (vp, (h,)),
    "auvp_stream_sync": (i, (h,)),
    "auvp_stream_mark": (i, (h, i32)),
    "auvp_stream_elapsed_ms": (i, (h, dp)),
    "auvp_graph_begin": (i, (h,)),
    "auvp_graph_end": (i, (h, ip)),
    "auvp_graph_launch": (i, (h, i32, i32)),
    "auvp_astar_batch": (i, (h, i32, dp, dp, dp, _ap, i32)),
    "auvp_astar_summaries": (i, (h, vp)),
    "auvp_astar_paths": (i, (h, i64p, dp, dp, dp, dp)),
    "auvp_astar_exp_log": (i, (h, i32, dp)),
    "auvp_astar_hab_left": (i, (h, i32, ip)),
    "auvp_astar_set_visited": (i, (h, i32, i32, u8p)),
    "auvp_astar_get_visited": (i, (h, i32, u8p)),
    "auvp_astar_batch_sets": (i, (h, i32, dp, dp, _ap, i32, ip)),
    "auvp_astar_sets_topn": (i, (h, dp)),
    "auvp_sog_convert": (i, (h, dp, i32, dp, f64, f64, f64, i32, ip, dp, i32, ip, ip, ip, dp, dp)),
    "auvp_pf_create_batch": (i, (h, i32, i32, dp, u32p, ip)),
    "auvp_pf_set_particles": (i, (h, i32, i32, dp, ip, ip, u32p, ip)),
    "auvp_pf_set_rng": (i, (h, u32p, ip)),
    "auvp_pf_run": (i, (h, i32, i32, i32, dp, dp, i32)),
    "auvp_pf_run_dev_meas": (i, (h, i32, i32, i32, vp, dp, i32)),
    "auvp_pf_particles": (i, (h, dp, ip)),
    "auvp_pf_particles_dev": (i, (h, vpp, vpp)),
    "auvp_pf_estimates": (i, (h, dp, dp, ip)),
    "auvp_pf_status": (i, (h, ip, u64p)),
    "auvp_pf_rng_state": (i, (h, u32p, ip)),
    "auvp_pf_step_log": (i, (h, dp, ip)),
    "auvp_sf_forecast": _forecast,
    "auvp_sf_forecast_large": _forecast,
    "auvp_sf_last_kernel": (s, (h,)),
    "auvp_sf_choose_launch": (i, (P(_SfLaunchQuery), P(_SfLaunchChoice))),
    "auvp_sf_prob_dev": (i, (h, vpp, ip, ip, ip)),
    "auvp_sf_plan": (i, (i32, i32, ip, i32, ip, ip, ip, ip)),
    "auvp_check_collision_batch": (i, (h, i32, ip, dp, bp)),
    "auvp_cost_paths": (i, (h, i32, ip, dp, ip, ip, dp, dp, dp)),
    "auvp_nn_closest_batch": (i, (h, i32, dp, i32, dp, i32, ip, ip)),
    "auvp_hbm_probe": (i, (h, u64, i32, dp, dp)),
    "auvp_sincos_dev": (i, (h, i32, dp, dp, dp)),
    "auvp_math_dev": (i, (h, i32, i32, dp, dp, dp, dp)),
    "auvp_theta_chain_dev": (i, (h, i32, dp, dp, dp)),
    "auvp_row_ends_dev": (i, (h, i32, dp, dp, dp)),
    "auvp_random_stream_dev": (i, (h, u64, i32, dp)),
    "auvp_rrt_phase_clocks": (i, (h, u64p)),
    "auvp_last_kernel_ms": (f64, (h,)),
    "auvp_rrt_last_launch_parts": (i, (h, dp, dp, ip)),
    "auvp_rrt_last_stream_ms": (f64, (h,)),
    "auvp_rrt_last_stream_len": (i64, (h,)),
    "auvp_rrt_last_stream_mirror": (i, (h,)),
    "auvp_rrt_rows_stream_shape": (i, (i32, i32, i32, i32, i32, i32, ip, ip, ip)),
    "auvp_rrt_choose_launch": (i, (P(_RrtLaunchQuery), P(_RrtLaunchChoice))),
    "auvp_prrt_choose_launch": (i, (P(_PrrtLaunchQuery), P(_PrrtLaunchChoice))),
    "auvp_rrt_last_kernel": (s, (h,)),
    "auvp_rrt_last_leaf_stats": (i, (h, i64p)),
    "auvp_last_launch": (i, (h, ip, ip, ip)),
    "auvp_prrt_replan_particles": (i, (h, dp, _pp, dp, dp, u64, i32)),
    "auvp_comm_unique_id": (i, (u8p,)),
    "auvp_comm_init": (i, (h, i32, i32, u8p)),
    "auvp_comm_destroy": (i, (h,)),
    "auvp_gather": (i, (h, vp, sz, vp)),
    "auvp_gather_var": (i, (h, vp, i64, vp, i64, i64p)),
    "auvp_gather_counts": (i, (h, i64, i64p)),
    "auvp_gather_blocks": (i, (h, vp, vp, i64, i64p)),
    "auvp_gather_blocks_root": (i, (h, i32, vp, vp, i64, i64p)),
    "auvp_gather_blocks_root_async": (i, (h, i32, vp, vp, i64, i64p)),
    "auvp_gather_wait": (i, (h, dp, i64p)),
    "auvp_comm_available": (i, ()),
    "auvp_comm_library": (s, ()),
    "auvp_comm_info": (i, (h, ip, ip, ip)),
    "auvp_last_gather_ms": (f64, (h,)),
}


def bind(L, prototypes=PROTOTYPES):
    """Set restype and argtypes of every entry point that L exports.  A name L lacks -- an earlier build loaded through
    AUVPLAN_LIBRARY for a comparison has not the newest ones -- is skipped: calling it raises AttributeError, as it always did."""
    for name, (restype, argtypes) in prototypes.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, list(argtypes)
    return L

/* The layout of every public struct of include/auvplan.h as the C (and the C++) compiler sees it, for
 * tests/test_cabi_prototypes.py: one line "name sizeof <bytes>" per struct, one line "name.field <offset> <bytes>" per field. */
#include "auvplan.h"
#include <stddef.h>
#include <stdio.h>

#define S(T, name) printf("%s sizeof %zu\n", name, sizeof(T))
#define F(T, name, f) printf("%s.%s %zu %zu\n", name, #f, offsetof(T, f), sizeof(((T*)0)->f))

int main(void) {
#define T auvp_rrt_params
#define N "auvp_rrt_params"
  S(T, N); F(T, N, dist_to_end); F(T, N, diff_max); F(T, N, freq); F(T, N, min_dist); F(T, N, bin_interval); F(T, N, v);
  F(T, N, max_traj_time); F(T, N, max_plan_time); F(T, N, w); F(T, N, mode); F(T, N, max_iter); F(T, N, points_per_iter);
#undef T
#undef N
#define T auvp_rrt_summary
#define N "auvp_rrt_summary"
  S(T, N); F(T, N, status); F(T, N, n_nodes); F(T, N, n_points); F(T, N, n_leaves); F(T, N, best_leaf); F(T, N, best_path_len);
  F(T, N, iters_run); F(T, N, n_candidates); F(T, N, best_cost); F(T, N, best_length); F(T, N, rng_after); F(T, N, leaf_elems);
  F(T, N, n_draw32); F(T, N, nn_scanned);
#undef T
#undef N
#define T auvp_rrt_episode
#define N "auvp_rrt_episode"
  S(T, N); F(T, N, max_traj_time); F(T, N, habitat_keep);
#undef T
#undef N
#define T struct auvp_rrt_group_best
#define N "auvp_rrt_group_best"
  S(T, N); F(T, N, status); F(T, N, winner); F(T, N, n_with_leaf); F(T, N, path_len); F(T, N, cost); F(T, N, length);
#undef T
#undef N
#define T auvp_replan_record
#define N "auvp_replan_record"
  S(T, N); F(T, N, status); F(T, N, winner); F(T, N, n_committed); F(T, N, path_len); F(T, N, cost); F(T, N, last); F(T, N, keep);
  F(T, N, claimed); F(T, N, conflicts); F(T, N, _reserved);
#undef T
#undef N
#define T auvp_prrt_params
#define N "auvp_prrt_params"
  S(T, N); F(T, N, rect); F(T, N, exp_rate); F(T, N, dist_to_end); F(T, N, diff_max); F(T, N, freq); F(T, N, cell_side_length);
  F(T, N, subsections); F(T, N, max_step);
#undef T
#undef N
#define T auvp_prrt_summary
#define N "auvp_prrt_summary"
  S(T, N); F(T, N, status); F(T, N, n_nodes); F(T, N, n_points); F(T, N, n_occ); F(T, N, steps); F(T, N, done); F(T, N, path_len);
  F(T, N, last_node); F(T, N, last_accepted); F(T, N, last_new_node); F(T, N, n_arc); F(T, N, _pad); F(T, N, arc);
  F(T, N, rng_after); F(T, N, n_draw32);
#undef T
#undef N
#define T auvp_astar_params
#define N "auvp_astar_params"
  S(T, N); F(T, N, variant); F(T, N, cap_nodes); F(T, N, box); F(T, N, velocity); F(T, N, w);
#undef T
#undef N
#define T auvp_astar_summary
#define N "auvp_astar_summary"
  S(T, N); F(T, N, status); F(T, N, found); F(T, N, n_nodes); F(T, N, n_expansions); F(T, N, n_children); F(T, N, path_len);
  F(T, N, smooth_len); F(T, N, n_hab_left); F(T, N, visited_count); F(T, N, leaf); F(T, N, open_scanned_lo);
  F(T, N, open_scanned_hi);
#undef T
#undef N
#define T auvp_rrt_launch_query
#define N "auvp_rrt_launch_query"
  S(T, N); F(T, N, n_episodes); F(T, N, n_cu); F(T, N, mode); F(T, N, max_iter); F(T, N, n_time_bins); F(T, N, flags); F(T, N, freq);
  F(T, N, dist_to_end); F(T, N, max_pts); F(T, N, n_obstacles); F(T, N, n_habitats); F(T, N, n_poly); F(T, N, n_bins);
  F(T, N, obst_area); F(T, N, per_episode_limits); F(T, N, one_wave_only); F(T, N, no_stream); F(T, N, seen_E); F(T, N, seen_most);
  F(T, N, n_options); F(T, N, option_names); F(T, N, option_values);
#undef T
#undef N
#define T auvp_rrt_launch_choice
#define N "auvp_rrt_launch_choice"
  S(T, N); F(T, N, status); F(T, N, kind); F(T, N, J); F(T, N, quad); F(T, N, grid); F(T, N, block); F(T, N, lds); F(T, N, lds_max);
  F(T, N, kflags); F(T, N, stream_waves); F(T, N, mirror); F(T, N, _pad); F(T, N, stream_len); F(T, N, lds_need); F(T, N, name);
#undef T
#undef N
#define T auvp_prrt_launch_query
#define N "auvp_prrt_launch_query"
  S(T, N); F(T, N, n_episodes); F(T, N, n_cu); F(T, N, n_obstacles); F(T, N, max_pts); F(T, N, cap_nodes); F(T, N, n_buckets);
  F(T, N, max_step); F(T, N, flags); F(T, N, freq); F(T, N, step_mode); F(T, N, waits); F(T, N, one_wave_only); F(T, N, rows);
  F(T, N, n_options); F(T, N, _pad); F(T, N, option_names); F(T, N, option_values);
#undef T
#undef N
#define T auvp_prrt_launch_choice
#define N "auvp_prrt_launch_choice"
  S(T, N); F(T, N, status); F(T, N, kind); F(T, N, lat); F(T, N, rows); F(T, N, pipe); F(T, N, draw_wave); F(T, N, next_lds);
  F(T, N, bk_lds); F(T, N, obst_lds); F(T, N, eps_wg); F(T, N, grid); F(T, N, block); F(T, N, lds); F(T, N, J); F(T, N, lds_need);
  F(T, N, name);
#undef T
#undef N
#define T auvp_sf_launch_query
#define N "auvp_sf_launch_query"
  S(T, N); F(T, N, rows); F(T, N, cols); F(T, N, n_cells); F(T, N, widest_level); F(T, N, allow_large); F(T, N, n_options);
  F(T, N, option_names); F(T, N, option_values);
#undef T
#undef N
#define T auvp_sf_launch_choice
#define N "auvp_sf_launch_choice"
  S(T, N); F(T, N, status); F(T, N, kind); F(T, N, block); F(T, N, lds); F(T, N, name);
#undef T
#undef N
  return 0;
}

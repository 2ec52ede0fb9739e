// rrt_course_walk.h -- a sibling of rrt_final_course (rrt_explore_kernel.h) for kernels that read a best course without storing
// its rows: the same leaf -> root walk by one wavefront, but every element goes to a functor instead of a buffer.
#ifndef AUVP_RRT_COURSE_WALK_H
#define AUVP_RRT_COURSE_WALK_H
#include "rrt_explore_kernel.h"

namespace auvp {

// f(at, x, y, traj_time) for every element of episode ep's best course, `at` its index root -> leaf (0 .. best_path_len - 1), each
// element on exactly one lane: the nodes on lane 0, a node's path points spread over the lanes.  Nothing for an episode without
// a leaf.
template <class F>
__device__ inline void rrt_course_walk_xyt(const RrtBuffers& B, int ep, F&& f) {
  const int lane = lane_id();
  const RrtSummary s = B.summary[ep];
  if (s.best_leaf < 0) return;
  const int capn = B.cap_nodes;
  const size_t capp = (size_t)B.cap_points;
  const double* nodeF = B.node_f + (size_t)ep * capn * 8;
  const int4* nodeI = reinterpret_cast<const int4*>(B.node_i) + (size_t)ep * capn;
  const double* ptF = B.points + (size_t)ep * capp * 6;
  const double* init = B.init + (size_t)ep * 6;
  int pos = s.best_path_len - 1;  // element index of the leaf
  auto node_elem = [&](int m, int at) {
    if (nodeI[m].y < 0) f(at, init[0], init[1], init[3]);
    else { const double* nf = nodeF + (size_t)m * 8; f(at, nf[0], nf[1], nf[3]); }
  };
  if (lane == 0) node_elem(s.best_leaf, pos);
  pos--;
  for (int m = s.best_leaf;;) {
    const int4 r = nodeI[m];
    if (r.y < 0) break;
    const int cnt = r.w, off = r.z;
    for (int k = lane; k < cnt; k += 64) {
      const double* ra = ptF + ((size_t)off + k) * 3;  // point k of the node sits k places after the node it grew from
      f(pos - cnt + 1 + k, ra[0], ra[1], ra[2]);
    }
    pos -= cnt;
    if (lane == 0) node_elem(r.y, pos);
    pos--;
    m = r.y;
  }
}

}  // namespace auvp
#endif  // AUVP_RRT_COURSE_WALK_H

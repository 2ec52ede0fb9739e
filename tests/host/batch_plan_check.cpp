// batch_plan_check.cpp -- csrc/batch_plan.h (what a batch needs in HBM, the random stream's rules, the epoch tags) run on the
// host: tests/test_batch_plan_host.py builds this with g++ and the address / undefined-behaviour / float-cast-overflow
// sanitizers, writes one command per line and compares the answers, one line each, with figures worked out by hand.
// Numbers are read with strtod / strtoll, so nan, inf and hexadecimal floats pass through exactly.
//
//   rrt E max_iter freq max_traj_time bin_interval mode points_per_iter flags n_obstacles
//     -> status field K max_pts cap_nodes cap_points bin_cap bin_over bin_slots bin_stride cap_leaves xy_stride flags inv_bin_interval
//        itlog_n, then the sixteen byte counts in RrtBatchBytes' order
//   lim cap_traj_time bin_interval H n {traj_time keep} x n   -> bad_episode why, then n x {K keep traj_time}
//   prrt E x0 y0 x1 y1 cell subsections max_step freq flags n_obstacles
//     -> status field rows cols n_buckets delta_theta cap_nodes max_pts cap_points, then the twelve byte counts
//   rng n index x n          -> n x {pos left 0 0}
//   epoch n new_at           -> per call: tag clear   (a run of n calls from tag 0; call `new_at` (1-based) and call 1 find a new allocation)
//   want free held bytes     -> bytes to allocate
//   keep E n_cu max_iter mode lim ROWS ROWS_STREAM   (options: -1 unset) -> 0 / 1, rows by rrt_rows_wanted
//   drawn {r key most E | f key} ...   one memory; key: the parameter block's max_iter -> per op: most E, or none
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#include "batch_plan.h"

namespace {

double num(std::istringstream& s) { std::string t; s >> t; return strtod(t.c_str(), nullptr); }
long long integer(std::istringstream& s) { std::string t; s >> t; return strtoll(t.c_str(), nullptr, 0); }
unsigned long long natural(std::istringstream& s) { std::string t; s >> t; return strtoull(t.c_str(), nullptr, 0); }

void option(OptionView& opt, int k, long long v) {
  if (v >= 0) { opt.opt_has[k] = true; opt.opt_val[k] = v; }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s commands.txt\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::vector<char> buf(1 << 20);
  while (fgets(buf.data(), (int)buf.size(), f)) {
    std::istringstream s(buf.data());
    std::string cmd;
    if (!(s >> cmd)) continue;
    if (cmd == "rrt") {
      auvp::RrtBatchIn in;
      in.E = (int)integer(s);
      in.p.dist_to_end = 1.0; in.p.diff_max = 0.5; in.p.min_dist = 0.5; in.p.v = 1.0; in.p.max_plan_time = 5.0;
      in.p.w[0] = 1.0; in.p.w[1] = -3.0; in.p.w[2] = -1.0;
      in.p.max_iter = (int32_t)integer(s);
      in.p.freq = num(s); in.p.max_traj_time = num(s); in.p.bin_interval = num(s);
      in.p.mode = (int32_t)integer(s);
      in.p.points_per_iter = num(s);
      in.flags = (int)integer(s);
      in.n_obstacles = (int)integer(s);
      const auvp::RrtBatchPlan r = auvp::rrt_batch_plan(in);
      const auvp::RrtBuffers& B = r.B;
      const auvp::RrtBatchBytes& b = r.bytes;
      printf("%d %s %d %d %d %d %d %d %d %lld %d %lld %d %a %lld", (int)r.status, r.field[0] ? r.field : "-", r.P.K, r.max_pts, B.cap_nodes, B.cap_points,
             B.bin_cap, B.bin_over, B.bin_slots, B.bin_stride, B.cap_leaves, B.xy_stride, r.P.flags, r.P.inv_bin_interval, r.itlog_n);
      for (unsigned long long v : {b.nodes_f, b.nodes_i, b.points, b.bin_items, b.bin_count, b.summary, b.node_c, b.node_q, b.node_xy, b.itlog_i,
                                   b.itlog_b, b.leaf_c, b.leaf_i, b.leaf_stats, b.phase, b.mt})
        printf(" %llu", v);
      printf("\n");
    } else if (cmd == "lim") {
      auvp_rrt_params p{};
      p.max_traj_time = num(s); p.bin_interval = num(s);
      const int H = (int)integer(s), n = (int)integer(s);
      std::vector<auvp_rrt_episode> ep((size_t)n);
      for (auvp_rrt_episode& e : ep) { e.max_traj_time = num(s); e.habitat_keep = natural(s); }
      const auvp::RrtEpisodeLimits r = auvp::rrt_episode_limits(p, H, ep.data(), n);
      printf("%d %d", r.bad_episode, (int)r.why);
      if (r.bad_episode < 0)
        for (int e = 0; e < n; e++) {
          const auvp::RrtEpisodeLimDev& d = r.lim[(size_t)e];
          if (d.K != r.K[(size_t)e] || d._pad != 0) { fprintf(stderr, "episode %d: the row's K and the list's differ\n", e); return 3; }
          printf(" %d %llu %a", d.K, d.keep, d.max_traj_time);
        }
      printf("\n");
    } else if (cmd == "prrt") {
      auvp::PrrtBatchIn in;
      in.E = (int)integer(s);
      for (double& v : in.p.rect) v = num(s);
      in.p.exp_rate = 1.0; in.p.dist_to_end = 1.0; in.p.diff_max = 0.5;
      in.p.cell_side_length = num(s);
      in.p.subsections = (int32_t)integer(s);
      in.p.max_step = (int32_t)integer(s);
      in.p.freq = num(s);
      in.flags = (int)integer(s);
      in.n_obstacles = (int)integer(s);
      const auvp::PrrtBatchPlan r = auvp::prrt_batch_plan(in);
      const auvp::PrrtBatchBytes& b = r.bytes;
      printf("%d %s %d %d %d %a %d %d %d", (int)r.status, r.field[0] ? r.field : "-", r.rows, r.cols, r.n_buckets, r.delta_theta, r.cap_nodes, r.max_pts,
             r.cap_points);
      for (unsigned long long v : {b.nodes, b.node_bucket, b.points, b.occupied, b.buckets, b.mt, b.rng_state, b.summary, b.step_bucket, b.start, b.goal,
                                   b.st_log})
        printf(" %llu", v);
      printf("\n");
    } else if (cmd == "rng") {
      const int n = (int)integer(s);
      std::vector<int32_t> idx((size_t)n);
      for (int32_t& v : idx) v = (int32_t)integer(s);
      for (int32_t v : auvp::prrt_rng_state_rows(idx.data(), n)) printf("%d ", v);
      printf("\n");
    } else if (cmd == "epoch") {
      const int n = (int)integer(s), new_at = (int)integer(s);
      uint32_t tag = 0;
      for (int call = 1; call <= n; call++) {
        const auvp::EpochTag t = auvp::epoch_tag_next(tag, call == 1 || call == new_at);
        tag = t.tag;
        printf("%u %d ", t.tag, t.clear ? 1 : 0);
      }
      printf("\n");
    } else if (cmd == "want") {
      const unsigned long long free_b = natural(s), held = natural(s), bytes = natural(s);
      printf("%llu\n", auvp::rrt_stream_want_bytes(free_b, held, bytes));
    } else if (cmd == "keep") {
      const int E = (int)integer(s), n_cu = (int)integer(s), max_iter = (int)integer(s), mode = (int)integer(s), lim = (int)integer(s);
      OptionView opt;
      option(opt, OPT_ROWS, integer(s));
      option(opt, OPT_ROWS_STREAM, integer(s));
      printf("%d\n", auvp::rrt_stream_keeps(opt, mode, max_iter, lim != 0, auvp::rrt_rows_wanted(opt, E, n_cu)) ? 1 : 0);
    } else if (cmd == "drawn") {
      auvp::DrawnMemory mem;
      std::string op;
      while (s >> op) {
        auvp::RrtParamsDev P{};
        P.max_iter = (int32_t)integer(s);
        P.freq = 30.0;
        const auvp::DrawnMemory::Slot* d = nullptr;
        if (op == "r") {
          const long long most = integer(s);
          const int E = (int)integer(s);
          d = &mem.record(P, most, E);
        } else {
          d = mem.find(P);
        }
        if (d) printf("%lld %d ", d->most, d->E);
        else printf("none ");
      }
      printf("\n");
    } else {
      fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  fclose(f);
  return 0;
}

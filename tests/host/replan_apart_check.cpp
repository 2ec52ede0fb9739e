// replan_apart_check.cpp -- csrc/replan_apart.h (the winner selection of RRT.replanning_batch(team_separation=d)) run on the host:
// tests/test_team_separation_host.py builds this with g++ -ffp-contract=off, once plain and once with the address /
// undefined-behaviour sanitizers, writes cases (tests/separation_cases.py), and compares what comes back with
// rrt_dubins.course_ticks / team_pick_separated.  Every winner's conflicts are counted twice: serially and as the kernel's
// wavefront does it -- 64 strided partial counts, then their sum -- and the two must agree.
//
//   in : int32 n_cases; per case: int32 H, T, n, G, K, W, claims, pad; double d, tick; habitats [H,3]; bins [T,2]; int32 labels [n];
//        uint64 keep [n]; int32 active [G]; double weights [3]; per candidate (G * K): int32 L, bin_lo, bin_hi, pad; double cost[4],
//        leaf_t; xyt [L,3]
//   out: per case: G records {int32 winner (-2: the AUV has no teammate, the program left it alone), pad; double cost[4];
//        uint64 claimed; int32 conflicts, pad}; then every candidate's tick table: int32 s_lo, n; double xy [n,2]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "replan_apart.h"
#include "world_tables.h"

namespace {

template <class T>
bool get(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
bool put(FILE* f, const T* p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
  int32_t n_cases = 0;
  if (!get(in, &n_cases, 1) || n_cases < 0) { fprintf(stderr, "bad header\n"); return 2; }
  for (int c = 0; c < n_cases; c++) {
    int32_t head[8];
    double dt[2];
    if (!get(in, head, 8) || !get(in, dt, 2)) { fprintf(stderr, "case %d: bad record\n", c); return 2; }
    const int H = head[0], T = head[1], n = head[2], G = head[3], K = head[4], W = head[5];
    const bool claims = head[6] != 0;
    if (H < 0 || H > auvp::REPLAN_MAX_HAB || T < 0 || n < 1 || G < 1 || K < 1 || !auvp::replan_apart_args_ok(dt[0], dt[1], W)) {
      fprintf(stderr, "case %d: bad sizes\n", c);
      return 2;
    }
    std::vector<double> hab((size_t)H * 3), hab_t((size_t)H), bins((size_t)T * 2);
    std::vector<int32_t> labels((size_t)n), active((size_t)G);
    std::vector<uint64_t> keep((size_t)n);
    double w[3];
    if (!get(in, hab.data(), hab.size()) || !get(in, bins.data(), bins.size()) || !get(in, labels.data(), labels.size()) ||
        !get(in, keep.data(), keep.size()) || !get(in, active.data(), active.size()) || !get(in, w, 3)) {
      fprintf(stderr, "case %d: short file\n", c);
      return 2;
    }
    for (int h = 0; h < H; h++) hab_t[(size_t)h] = auvp::sq_threshold(hab[3 * (size_t)h + 2]);
    const size_t E = (size_t)G * (size_t)K;
    std::vector<std::vector<uint64_t>> words(E);
    std::vector<std::vector<double>> table(E);
    std::vector<int32_t> s_lo(E), n_ticks(E), owner((size_t)W);
    std::vector<auvp::ReplanApartCand> cands(E);
    for (size_t e = 0; e < E; e++) {
      int32_t ch[4];
      double cd[5];
      if (!get(in, ch, 4) || !get(in, cd, 5) || ch[0] < 0) { fprintf(stderr, "case %d, candidate %zu: short file\n", c, e); return 2; }
      std::vector<double> xyt((size_t)ch[0] * 3);
      if (!get(in, xyt.data(), xyt.size())) { fprintf(stderr, "case %d, candidate %zu: short file\n", c, e); return 2; }
      words[e].resize((size_t)ch[0]);
      for (int i = 0; i < ch[0]; i++)
        words[e][(size_t)i] = auvp::replan_pick_word(hab.data(), hab_t.data(), H, bins.data(), ch[1] < 0 ? 0 : ch[1], ch[2] > T ? T : ch[2],
                                                     xyt[3 * (size_t)i], xyt[3 * (size_t)i + 1], xyt[3 * (size_t)i + 2]);
      table[e].resize((size_t)W * 2);
      s_lo[e] = n_ticks[e] = 0;  // (a tree without a leaf: the empty table)
      if (ch[0] > 0)
        n_ticks[e] = auvp::replan_ticks_build(xyt.data() + 2, xyt.data(), xyt.data() + 1, ch[0], 3, dt[1], W, &s_lo[e], table[e].data(), owner.data());
      auvp::ReplanApartCand& cd_out = cands[e];
      cd_out.pick = auvp::ReplanPickCand{ch[0], 0, words[e].data(), cd[3], cd[4]};
      for (int k = 0; k < 4; k++) cd_out.cost[k] = cd[k];
      cd_out.ticks = auvp::ReplanTicks{s_lo[e], n_ticks[e], table[e].data()};
    }
    std::vector<int32_t> slot_of((size_t)n, -1);
    for (int g = 0; g < G; g++) {
      if (active[(size_t)g] < 0 || active[(size_t)g] >= n) { fprintf(stderr, "case %d: bad active list\n", c); return 2; }
      slot_of[(size_t)active[(size_t)g]] = g;
    }
    std::vector<auvp::ReplanApartOut> res((size_t)G);
    for (auto& r : res) {
      r.pick.winner = -2; r.pick._pad = 0; r.pick.cost[0] = r.pick.cost[1] = r.pick.cost[2] = r.pick.cost[3] = 0.0; r.pick.claimed = 0;
      r.conflicts = 0; r._pad = 0;
    }
    const auvp::ReplanTeamCsr csr = auvp::replan_team_csr(labels.data(), n);
    std::vector<int32_t> trail((size_t)n);
    for (int t = 0; t < csr.n_teams(); t++) {
      const int lo = csr.team_off[(size_t)t], hi = csr.team_off[(size_t)t + 1];
      auvp::replan_apart_team(csr.members.data(), lo, hi, slot_of.data(), keep.data(), K, cands.data(), w[0], w[1], claims, dt[0], res.data(),
                              trail.data());
      // the wavefront's order of operations: every winner against the winners of the members before it, 64 strided partial counts
      std::vector<int32_t> before;
      for (int i = lo; i < hi; i++) {
        const int g = slot_of[(size_t)csr.members[(size_t)i]];
        if (g < 0 || res[(size_t)g].pick.winner < 0) continue;
        const size_t e = (size_t)g * (size_t)K + (size_t)res[(size_t)g].pick.winner;
        int lanes = 0;
        for (int lane = 0; lane < 64; lane++)
          lanes += auvp::replan_apart_count(cands[e].ticks, lane, 64, (int)before.size(), [&](int j) { return cands[(size_t)before[(size_t)j]].ticks; },
                                            dt[0] * dt[0]);
        if (lanes != res[(size_t)g].conflicts) {
          fprintf(stderr, "case %d, group %d: the strided count disagrees with the serial one\n", c, g);
          return 3;
        }
        before.push_back((int32_t)e);
      }
    }
    if (!put(out, res.data(), res.size())) { fprintf(stderr, "case %d: write failed\n", c); return 2; }
    for (size_t e = 0; e < E; e++) {
      const int32_t hd[2] = {s_lo[e], n_ticks[e]};
      if (!put(out, hd, 2) || !put(out, table[e].data(), (size_t)n_ticks[e] * 2)) { fprintf(stderr, "case %d: write failed\n", c); return 2; }
    }
  }
  fclose(in);
  if (fclose(out) != 0) { fprintf(stderr, "write failed\n"); return 2; }
  return 0;
}

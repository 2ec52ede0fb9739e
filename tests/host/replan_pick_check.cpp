// replan_pick_check.cpp -- csrc/replan_pick.h (the team-aware winner selection of RRT.replanning_batch(team_pick="claims")) run on
// the host: tests/test_team_pick_host.py builds this with g++ -ffp-contract=off, once plain and once with the address /
// undefined-behaviour sanitizers, writes cases (tests/team_pick_cases.py), and compares what comes back with
// rrt_dubins.course_habitat_words / team_pick_claims.  Every candidate is counted twice: serially and as the kernel's wavefront
// does it -- 64 strided partial counts, then their sum and OR -- and the two must agree.
//
//   in : int32 n_cases; per case: int32 H, T, n, G, K; habitats [H,3]; bins [T,2]; int32 labels [n]; uint64 keep [n];
//        int32 active [G]; double weights [3]; per candidate (G * K): int32 L, bin_lo, bin_hi, pad; double c2, leaf_t; xyt [L,3]
//   out: per case: G records {int32 winner (-2: the AUV has no teammate, the program left it alone), pad; double cost[4];
//        uint64 claimed}; then every candidate's words [L]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "replan_pick.h"
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
    int32_t head[5];
    if (!get(in, head, 5)) { fprintf(stderr, "case %d: bad record\n", c); return 2; }
    const int H = head[0], T = head[1], n = head[2], G = head[3], K = head[4];
    if (H < 0 || H > auvp::REPLAN_MAX_HAB || T < 0 || n < 1 || G < 1 || K < 1) { fprintf(stderr, "case %d: bad sizes\n", c); return 2; }
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
    std::vector<auvp::ReplanPickCand> cands(E);
    for (size_t e = 0; e < E; e++) {
      int32_t ch[4];
      double cd[2];
      if (!get(in, ch, 4) || !get(in, cd, 2) || ch[0] < 0) { fprintf(stderr, "case %d, candidate %zu: short file\n", c, e); return 2; }
      std::vector<double> xyt((size_t)ch[0] * 3);
      if (!get(in, xyt.data(), xyt.size())) { fprintf(stderr, "case %d, candidate %zu: short file\n", c, e); return 2; }
      words[e].resize((size_t)ch[0]);
      for (int i = 0; i < ch[0]; i++)
        words[e][(size_t)i] = auvp::replan_pick_word(hab.data(), hab_t.data(), H, bins.data(), ch[1] < 0 ? 0 : ch[1], ch[2] > T ? T : ch[2],
                                                     xyt[3 * (size_t)i], xyt[3 * (size_t)i + 1], xyt[3 * (size_t)i + 2]);
      cands[e] = auvp::ReplanPickCand{ch[0], 0, words[e].data(), cd[0], cd[1]};
    }
    std::vector<int32_t> slot_of((size_t)n, -1);
    for (int g = 0; g < G; g++) {
      if (active[(size_t)g] < 0 || active[(size_t)g] >= n) { fprintf(stderr, "case %d: bad active list\n", c); return 2; }
      slot_of[(size_t)active[(size_t)g]] = g;
    }
    std::vector<auvp::ReplanPickOut> res((size_t)G);
    for (auto& r : res) { r.winner = -2; r._pad = 0; r.cost[0] = r.cost[1] = r.cost[2] = r.cost[3] = 0.0; r.claimed = 0; }
    const auvp::ReplanTeamCsr csr = auvp::replan_team_csr(labels.data(), n);
    for (int t = 0; t < csr.n_teams(); t++)
      auvp::replan_pick_team(csr.members.data(), csr.team_off[(size_t)t], csr.team_off[(size_t)t + 1], slot_of.data(), keep.data(), K,
                             cands.data(), w[0], w[1], res.data());
    // the wavefront's order of operations: under every mask a member was judged by, 64 strided partial counts, then their
    // sum and OR
    for (int g = 0; g < G; g++) {
      if (res[(size_t)g].winner == -2) continue;
      const uint64_t mask = keep[(size_t)active[(size_t)g]] & ~res[(size_t)g].claimed;
      for (int k = 0; k < K; k++) {
        const auvp::ReplanPickCand& cd = cands[(size_t)g * (size_t)K + (size_t)k];
        if (cd.path_len <= 0) continue;
        const auvp::ReplanPickHits serial = auvp::replan_pick_hits(cd.words, 0, cd.path_len, 1, mask);
        auvp::ReplanPickHits lanes{0, 0ull};
        for (int lane = 0; lane < 64; lane++) {
          const auvp::ReplanPickHits p = auvp::replan_pick_hits(cd.words, lane, cd.path_len, 64, mask);
          lanes.hits += p.hits; lanes.vis |= p.vis;
        }
        if (lanes.hits != serial.hits || lanes.vis != serial.vis) {
          fprintf(stderr, "case %d, group %d, tree %d: the strided count disagrees with the serial one\n", c, g, k);
          return 3;
        }
      }
    }
    if (!put(out, res.data(), res.size())) { fprintf(stderr, "case %d: write failed\n", c); return 2; }
    for (size_t e = 0; e < E; e++)
      if (!put(out, words[e].data(), words[e].size())) { fprintf(stderr, "case %d: write failed\n", c); return 2; }
  }
  fclose(in);
  if (fclose(out) != 0) { fprintf(stderr, "write failed\n"); return 2; }
  return 0;
}

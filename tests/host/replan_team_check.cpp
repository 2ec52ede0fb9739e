// replan_team_check.cpp -- csrc/replan_teams.h (the team fold of RRT.replanning_batch(teams=...)) run on the host:
// tests/test_replan_teams_host.py builds this with g++ and the address / undefined-behaviour sanitizers, writes cases, and
// compares what comes back with rrt_dubins.team_csr / team_fold.  Every team is folded twice: serially (replan_team_fold) and
// as replan_team_kernel's wavefront does it -- 64 strided partial ANDs, then their AND -- and the two must agree.
//
//   in : int32 n_cases; per case: int32 n; int32 team_of[n]; uint64 keep[n]
//   out: per case: int32 n_teams, n_members; int32 team_off[n_teams+1]; int32 members[n_members]; uint64 keep[n]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "replan_teams.h"

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
    int32_t n = 0;
    if (!get(in, &n, 1) || n < 0) { fprintf(stderr, "case %d: bad record\n", c); return 2; }
    std::vector<int32_t> team_of((size_t)n);
    std::vector<uint64_t> keep((size_t)n);
    if (!get(in, team_of.data(), team_of.size()) || !get(in, keep.data(), keep.size())) { fprintf(stderr, "case %d: short file\n", c); return 2; }
    const auvp::ReplanTeamCsr csr = auvp::replan_team_csr(team_of.data(), n);
    // the wavefront's order of operations on the masks as they were
    std::vector<uint64_t> by_lanes((size_t)csr.n_teams());
    for (int t = 0; t < csr.n_teams(); t++) {
      uint64_t k = ~0ull;
      for (int lane = 0; lane < 64; lane++)
        k &= auvp::replan_team_and(keep.data(), csr.members.data(), csr.team_off[(size_t)t] + lane, csr.team_off[(size_t)t + 1], 64);
      by_lanes[(size_t)t] = k;
    }
    auvp::replan_team_fold(csr, keep.data());
    for (int t = 0; t < csr.n_teams(); t++)
      if (keep[(size_t)csr.members[(size_t)csr.team_off[(size_t)t]]] != by_lanes[(size_t)t]) {
        fprintf(stderr, "case %d, team %d: the strided fold disagrees with the serial one\n", c, t);
        return 3;
      }
    const int32_t head[2] = {csr.n_teams(), (int32_t)csr.members.size()};
    if (!put(out, head, 2) || !put(out, csr.team_off.data(), csr.team_off.size()) || !put(out, csr.members.data(), csr.members.size()) ||
        !put(out, keep.data(), keep.size())) {
      fprintf(stderr, "case %d: write failed\n", c);
      return 2;
    }
  }
  fclose(in);
  if (fclose(out) != 0) { fprintf(stderr, "write failed\n"); return 2; }
  return 0;
}

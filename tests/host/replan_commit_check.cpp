// replan_commit_check.cpp -- csrc/replan_commit.h (the commit rule of replanning's step between two rounds) run on the host:
// tests/test_replan_commit_host.py builds this with g++ and the address / undefined-behaviour sanitizers, writes cases, and
// compares what comes back with rrt_dubins.first_bucket_commit.  hab_t comes from csrc/world_tables.h, as auvp_world_set
// builds it.
//
//   in : int32 n_cases; per case: int32 L, H; uint64 keep; double round_span; double last[7]; double hab[H,3]; double course[L,7]
//   out: per case: int32 n_committed, 0; uint64 keep; double last[7]; uint8 sel[L]; double rows[n_committed,7]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "replan_commit.h"
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
    int32_t LH[2];
    uint64_t keep;
    double span, last[auvp::REPLAN_ROW];
    if (!get(in, LH, 2) || !get(in, &keep, 1) || !get(in, &span, 1) || !get(in, last, auvp::REPLAN_ROW) || LH[0] < 0 || LH[1] < 0 ||
        LH[1] > auvp::REPLAN_MAX_HAB) {
      fprintf(stderr, "case %d: bad record\n", c);
      return 2;
    }
    const int L = LH[0], H = LH[1];
    std::vector<double> hab((size_t)H * 3), course((size_t)L * auvp::REPLAN_ROW), rows((size_t)L * auvp::REPLAN_ROW);
    std::vector<uint8_t> sel((size_t)L);
    if (!get(in, hab.data(), hab.size()) || !get(in, course.data(), course.size())) { fprintf(stderr, "case %d: short file\n", c); return 2; }
    const auvp::HabitatTables t = auvp::build_habitat_tables(hab.data(), H, false);
    const int n = auvp::replan_commit_course(course.data(), L, last, &keep, span, hab.data(), t.hab_t.data(), H, sel.data(), rows.data());
    const int32_t head[2] = {n, 0};
    if (!put(out, head, 2) || !put(out, &keep, 1) || !put(out, last, auvp::REPLAN_ROW) || !put(out, sel.data(), sel.size()) ||
        !put(out, rows.data(), (size_t)n * auvp::REPLAN_ROW)) {
      fprintf(stderr, "case %d: write failed\n", c);
      return 2;
    }
  }
  fclose(in);
  if (fclose(out) != 0) { fprintf(stderr, "write failed\n"); return 2; }
  return 0;
}

// astar_tables_dump -- csrc/astar_tables.h's astar_topn_rows on rows read from a file, for tests/test_astar_tables_host.py.
//   in:  int64 T, int64 C, then T * C doubles (prob [T][C])
//   out: T * (C + 1) doubles (topn [T][C + 1])
#include <cstdint>
#include <cstdio>
#include <vector>

#include "astar_tables.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int64_t dims[2] = {0, 0};
  if (fread(dims, sizeof(int64_t), 2, f) != 2 || dims[0] < 0 || dims[1] < 0) return 4;
  const size_t T = (size_t)dims[0], C = (size_t)dims[1];
  std::vector<double> prob(T * C), topn(T * (C + 1));
  if (!prob.empty() && fread(prob.data(), sizeof(double), prob.size(), f) != prob.size()) return 5;
  fclose(f);
  auvp::astar_topn_rows(prob.data(), T, C, topn.data());
  f = fopen(argv[2], "wb");
  if (!f) return 6;
  if (!topn.empty() && fwrite(topn.data(), sizeof(double), topn.size(), f) != topn.size()) return 7;
  fclose(f);
  return 0;
}

// astar_tables_dump -- csrc/astar_tables.h on inputs read from a file, for tests/test_astar_tables_host.py.
//   astar_tables_dump in out          astar_topn_rows
//     in:  int64 T, int64 C, then T * C doubles (prob [T][C])
//     out: T * (C + 1) doubles (topn [T][C + 1])
//   astar_tables_dump world in out    build_astar_world_tables
//     in:  int32 O, H, V, T, C, no_grid, then obstacles [O,3], habitats [H,3], polygon [V,2], cells [C,4], prob [T,C] (doubles)
//     out: int32 g_ncol, g_nrow; double g_x1_0, g_y1_0, g_inv_dx, g_inv_dy, cx, cy; int64 sizes of ox, oy, ot, hab, rc, topn, gtab;
//          then those seven vectors
//   astar_tables_dump round2 in out   round2_py on every double of the file
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "astar_tables.h"

namespace {

bool get(FILE* f, std::vector<double>& v) { return v.empty() || fread(v.data(), sizeof(double), v.size(), f) == v.size(); }
bool put(FILE* f, const std::vector<double>& v) { return v.empty() || fwrite(v.data(), sizeof(double), v.size(), f) == v.size(); }

int dump_world(FILE* f, const char* dst) {
  int32_t n[6];
  if (fread(n, sizeof(int32_t), 6, f) != 6) return 4;
  for (int32_t v : n)
    if (v < 0) return 4;
  const int O = n[0], H = n[1], V = n[2], T = n[3], C = n[4];
  std::vector<double> obst((size_t)O * 3), hab((size_t)H * 3), poly((size_t)V * 2), cells((size_t)C * 4), prob((size_t)T * C);
  if (!get(f, obst) || !get(f, hab) || !get(f, poly) || !get(f, cells) || !get(f, prob)) return 5;
  fclose(f);
  const auvp::AstarWorldTables t = auvp::build_astar_world_tables(obst.data(), O, hab.data(), H, poly.data(), V, T, cells.data(), C, prob.data(), n[5] != 0);
  f = fopen(dst, "wb");
  if (!f) return 6;
  const int32_t g[2] = {t.g_ncol, t.g_nrow};
  const double s[6] = {t.g_x1_0, t.g_y1_0, t.g_inv_dx, t.g_inv_dy, t.cx, t.cy};
  const std::vector<double>* all[7] = {&t.ox, &t.oy, &t.ot, &t.hab, &t.rc, &t.topn, &t.gtab};
  int64_t sizes[7];
  for (int i = 0; i < 7; i++) sizes[i] = (int64_t)all[i]->size();
  if (fwrite(g, sizeof(int32_t), 2, f) != 2 || fwrite(s, sizeof(double), 6, f) != 6 || fwrite(sizes, sizeof(int64_t), 7, f) != 7) return 7;
  for (const std::vector<double>* v : all)
    if (!put(f, *v)) return 7;
  return fclose(f) == 0 ? 0 : 7;
}

int dump_round2(FILE* f, const char* dst) {
  std::vector<double> v;
  double x;
  while (fread(&x, sizeof x, 1, f) == 1) v.push_back(auvp::round2_py(x));
  fclose(f);
  f = fopen(dst, "wb");
  if (!f) return 6;
  if (!put(f, v)) return 7;
  return fclose(f) == 0 ? 0 : 7;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) return 2;
  FILE* f = fopen(argv[argc - 2], "rb");
  if (!f) return 3;
  if (argc == 4) {
    if (!strcmp(argv[1], "world")) return dump_world(f, argv[3]);
    if (!strcmp(argv[1], "round2")) return dump_round2(f, argv[3]);
    return 2;
  }
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

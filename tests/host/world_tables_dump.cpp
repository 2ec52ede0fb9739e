// world_tables_dump.cpp -- stand-alone host program around csrc/world_tables.h for tests/test_world_tables.py.
//
//   world_tables_dump IN OUT
//
// IN:  int32 O, H, V, T, C, grid_index, habitat_grid, 0;  int64 rg_max_entries;  then the doubles of obstacles [O,3],
//      habitats [H,3], polygon [V,2], bins [T,2], cells [C,4], prob [T,C].
// OUT: one record per table and per scalar of WorldTables: char name[16]; int32 type (0 f64, 1 i32, 2 f32, 3 u64);
//      int32 count; the values.  The habitats' part built alone (build_habitat_tables) follows under "alone_" names.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "world_tables.h"

namespace {

FILE* out_file = nullptr;

void put(const char* name, int32_t type, const void* p, size_t n, size_t size) {
  char tag[16] = {};
  strncpy(tag, name, sizeof tag - 1);
  const int32_t head[2] = {type, (int32_t)n};
  fwrite(tag, 1, sizeof tag, out_file);
  fwrite(head, sizeof head, 1, out_file);
  if (n) fwrite(p, size, n, out_file);
}
void put(const char* name, const std::vector<double>& v) { put(name, 0, v.data(), v.size(), 8); }
void put(const char* name, const std::vector<int32_t>& v) { put(name, 1, v.data(), v.size(), 4); }
void put(const char* name, const std::vector<float>& v) { put(name, 2, v.data(), v.size(), 4); }
void put(const char* name, const std::vector<unsigned long long>& v) { put(name, 3, v.data(), v.size(), 8); }
void put(const char* name, double v) { put(name, 0, &v, 1, 8); }
void put(const char* name, int32_t v) { put(name, 1, &v, 1, 4); }

void put_habitats(const char* prefix, const auvp::HabitatTables& t) {
  const std::string p(prefix);
  put((p + "hab_t").c_str(), t.hab_t);
  put((p + "hg_mask").c_str(), t.hg_mask);
  put((p + "hg_n").c_str(), t.hg_n);
  put((p + "hg_x0").c_str(), t.hg_x0);
  put((p + "hg_y0").c_str(), t.hg_y0);
  put((p + "hg_inv_w").c_str(), t.hg_inv_w);
  put((p + "hg_inv_h").c_str(), t.hg_inv_h);
}

bool read_doubles(FILE* f, std::vector<double>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), 8, n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t head[8];
  int64_t rg_max_entries;
  if (fread(head, sizeof head, 1, f) != 1 || fread(&rg_max_entries, sizeof rg_max_entries, 1, f) != 1) return 3;
  for (int i = 0; i < 5; i++)
    if (head[i] < 0) return 3;
  std::vector<double> obstacles, habitats, polygon, bins, cells, prob;
  auvp::WorldIn in;
  in.O = head[0]; in.H = head[1]; in.V = head[2]; in.T = head[3]; in.C = head[4];
  if (!read_doubles(f, obstacles, (size_t)in.O * 3) || !read_doubles(f, habitats, (size_t)in.H * 3) ||
      !read_doubles(f, polygon, (size_t)in.V * 2) || !read_doubles(f, bins, (size_t)in.T * 2) ||
      !read_doubles(f, cells, (size_t)in.C * 4) || !read_doubles(f, prob, (size_t)in.T * in.C))
    return 3;
  fclose(f);
  in.obstacles = obstacles.data(); in.habitats = habitats.data(); in.polygon = polygon.data(); in.bins = bins.data();
  in.cells = cells.data(); in.prob = prob.data();
  in.grid_index = head[5] != 0; in.habitat_grid = head[6] != 0; in.rg_max_entries = rg_max_entries;

  const auvp::WorldTables t = auvp::build_world_tables(in);
  const auvp::HabitatTables alone = auvp::build_habitat_tables(in.habitats, in.H, in.habitat_grid);

  out_file = fopen(argv[2], "wb");
  if (!out_file) { perror(argv[2]); return 2; }
  put("ox", t.ox); put("oy", t.oy); put("ot", t.ot);
  put("n_xbuckets", t.n_xbuckets); put("xb_off", t.xb_off); put("xb_items", t.xb_items); put("xb_data", t.xb_data);
  put("xb_x0", t.xb_x0); put("xb_inv_w", t.xb_inv_w);
  put("rg_enabled", t.rg_enabled); put("n_rg_bp", t.n_rg_bp); put("rg_first", t.rg_first); put("rg_bp", t.rg_bp);
  put("rg_off", t.rg_off); put("rg_pm", t.rg_pm); put("rg_id", t.rg_id);
  put("sg_enabled", t.sg_enabled); put("sg_ncol", t.sg_ncol); put("sg_nrow", t.sg_nrow);
  put("sg_x0", t.sg_x0); put("sg_x1", t.sg_x1); put("sg_y0", t.sg_y0); put("sg_y1", t.sg_y1);
  put("sg_col", t.sg_col); put("sg_row", t.sg_row);
  put("sg_x1_0", t.sg_x1_0); put("sg_y1_0", t.sg_y1_0); put("sg_inv_dx", t.sg_inv_dx); put("sg_inv_dy", t.sg_inv_dy);
  put("os_x", t.os_x); put("os_y", t.os_y); put("os_t", t.os_t); put("os_r", t.os_r); put("os_box", t.os_box);
  put("obst_area", t.obst_area);
  put_habitats("", t.hab);
  put("prob_absmax", t.prob_absmax); put("prob_one_sign", t.prob_one_sign);
  put("bins_sorted", t.bins_sorted); put("bins_t1_0", t.bins_t1_0); put("bins_inv_len", t.bins_inv_len);
  put("bb", 0, t.bb, 4, 8); put("safe_box", 0, t.safe_box, 4, 8); put("has_safe_box", t.has_safe_box);
  put_habitats("alone_", alone);
  return fclose(out_file) == 0 ? 0 : 3;
}

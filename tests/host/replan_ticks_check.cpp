// replan_ticks_check.cpp -- csrc/replan_ticks.h (the rule replan_measure_ticks_kernel is built from, and the host's index
// checks) under g++ alone, driven by tests/test_replan_ticks_host.py.
//
//   replan_ticks_check <cases.txt>
// reads cases as text, doubles as C hexadecimal floats (or "nan" / "inf"), and prints one answer per case:
//   ticks <n> <k> <span>   then n rows of 7 doubles     ->  "ticks <k>", then k lines "<tau> <row>" (row -1: from `last`)
//   plan <n_pieces> <last_round> <n_auvs> <n_rows> <log_rows> <k>, then n_pieces lines "<auv> <n> <src> <round>", then n_rows
//   member indices                                      ->  "plan <status> <bad> <n_seg>", then n_seg lines "<off> <n>"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "replan_ticks.h"

static double read_double(FILE* f) {
  char word[64];
  if (fscanf(f, "%63s", word) != 1) { fprintf(stderr, "short input\n"); exit(2); }
  return strtod(word, nullptr);
}

static long long read_int(FILE* f) {
  long long v = 0;
  if (fscanf(f, "%lld", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: replan_ticks_check cases.txt\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  char kind[16];
  while (fscanf(f, "%15s", kind) == 1) {
    if (!strcmp(kind, "ticks")) {
      const int n = (int)read_int(f), k = (int)read_int(f);
      const double span = read_double(f);
      if (n < 0 || !auvp::replan_meas_ticks_ok(k)) { fprintf(stderr, "bad ticks case\n"); return 2; }
      std::vector<double> seg((size_t)n * auvp::REPLAN_ROW);  // (exactly n rows: a read past them is the sanitizer's to find)
      for (double& v : seg) v = read_double(f);
      std::vector<double> tau((size_t)k);
      std::vector<int32_t> row((size_t)k);
      auvp::replan_meas_ticks_serial(seg.data(), n, k, span, tau.data(), row.data());
      printf("ticks %d\n", k);
      for (int j = 0; j < k; j++) printf("%a %d\n", tau[(size_t)j], (int)row[(size_t)j]);
    } else if (!strcmp(kind, "plan")) {
      const long long n_pieces = read_int(f);
      const int last_round = (int)read_int(f), n_auvs = (int)read_int(f), n_rows = (int)read_int(f);
      const long long log_rows = read_int(f), k = read_int(f);
      std::vector<auvp::ReplanPiece> pieces((size_t)n_pieces);
      for (auvp::ReplanPiece& p : pieces) {
        p.auv = (int32_t)read_int(f); p.n = (int32_t)read_int(f); p.src = (int64_t)read_int(f); p.round = (int32_t)read_int(f);
        p._pad = 0;
      }
      std::vector<int32_t> members((size_t)n_rows);
      for (int32_t& m : members) m = (int32_t)read_int(f);
      const auvp::ReplanTicksPlan p = auvp::replan_ticks_plan(pieces.data(), pieces.size(), last_round, n_auvs, members.data(), n_rows, log_rows, k);
      printf("plan %d %lld %zu\n", (int)p.status, p.bad, p.seg.size());
      for (const auvp::ReplanMeasSeg& s : p.seg) printf("%lld %d\n", (long long)s.off, (int)s.n);
    } else {
      fprintf(stderr, "unknown case kind %s\n", kind);
      return 2;
    }
  }
  fclose(f);
  return 0;
}

// astar_tables.h -- the top-n table of astar_fixLenSOG's heuristic (get_top_n_prob, astar_fixLenSOG.py:516-531), as a pure host
// function: no HIP, no handle, nothing but <algorithm>.  Three users share this one text: astar_build_world (the world's own
// table), the host route of the probability sets' tables (rows too long for astar_topn_sets_kernel's LDS: astar_host.h) and the
// host test (tests/host/astar_tables_dump.cpp, built with the sanitizers by tests/test_astar_tables_host.py).
//
// Per time bin t:  topn[t][0] = 0.0,  topn[t][i + 1] = topn[t][i] + sorted_desc(prob[t])[i]  -- the additions one after the
// other, in that order, in fp64 (`total = 0; total += probabilities[index]`, :526-530).  Equal values are interchangeable in the
// sort, and as the running sum starts at +0.0 the order of +0.0 and -0.0 cannot show.  A row that holds a nan has no defined
// order (neither in the reference's sorted() nor in std::sort): the caller keeps such rows away.
#ifndef AUVP_ASTAR_TABLES_H
#define AUVP_ASTAR_TABLES_H
#include <algorithm>
#include <cstddef>
#include <vector>

namespace auvp {

// longest row astar_topn_sets_kernel sorts (its row, padded to a power of two, lies in 128 KB of the CU's 160 KB of LDS)
constexpr int ASTAR_TOPN_DEV_MAX_C = 16384;

// prob [T][C] -> topn [T][C + 1]
inline void astar_topn_rows(const double* prob, size_t T, size_t C, double* topn) {
  std::vector<double> tmp(C);
  for (size_t t = 0; t < T; t++) {
    if (C) std::copy(prob + t * C, prob + (t + 1) * C, tmp.begin());
    std::sort(tmp.begin(), tmp.end(), [](double a, double b) { return a > b; });
    double tot = 0.0;  // total = 0; total += probabilities[index]  (astar_fixLenSOG.py:526-530)
    double* row = topn + t * (C + 1);
    row[0] = 0.0;
    for (size_t i = 0; i < C; i++) { tot += tmp[i]; row[i + 1] = tot; }
  }
}

}  // namespace auvp
#endif

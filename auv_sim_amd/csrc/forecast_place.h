// forecast_place.h -- where a forecast's rounds go among a planner's time bins, as data.
//
// A forecast (forecast_kernel.h) is indexed from "now": round 0 is the corrected grid of the moment the filters were read, round
// j the prediction j bins later.  A planner's bins are absolute times.  A forecast made when the fleet stands in bin b is placed
// with first_bin = b: with T planner bins and a forecast of R + 1 rounds
//   bin t of every set reads forecast round  min(max(t - b, 0), R)
// -- the bins before b (which no course reaches any more) repeat round 0, the bins past the forecast's end repeat its last round.
// b = 0 with R + 1 == T is the identity: the forecast's tables are the planner's as they lie.
//
// placed_round is the one formula, for sf_place_kernel (leaf_grid_kernels.hip: the source round of its row) and for the host.
// placed_round_of_bin is the host's plan: pure, no HIP runtime call, no handle; it validates the shape and names the identity.
// tests/test_forecast_place_host.py compiles it with g++ alone.
#ifndef AUVP_FORECAST_PLACE_H
#define AUVP_FORECAST_PLACE_H
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define AUVP_PLACE_HD __host__ __device__ inline
#else
#define AUVP_PLACE_HD inline
#endif

namespace auvp {

// forecast round that bin t reads; R: the forecast's last round (it has R + 1), b: the first bin
AUVP_PLACE_HD int placed_round(int t, int b, int R) {
  const int j = t - b;
  return j < 0 ? 0 : (j > R ? R : j);
}

enum SfPlaceStatus {
  SF_PLACE_OK = 0,
  SF_PLACE_BAD_SHAPE,  // T < 1 or R < 0
  SF_PLACE_BAD_BIN     // b outside 0 .. T - 1
};

struct SfPlacePlan {
  SfPlaceStatus status = SF_PLACE_OK;
  bool identity = false;              // round_of_bin[t] == t for every t and R + 1 == T: no gather is needed
  std::vector<int32_t> round_of_bin;  // [T]
};

inline SfPlacePlan placed_round_of_bin(int T, int R, int b) {
  SfPlacePlan p;
  if (T < 1 || R < 0) { p.status = SF_PLACE_BAD_SHAPE; return p; }
  if (b < 0 || b > T - 1) { p.status = SF_PLACE_BAD_BIN; return p; }
  p.round_of_bin.resize((size_t)T);
  for (int t = 0; t < T; t++) p.round_of_bin[(size_t)t] = placed_round(t, b, R);
  p.identity = b == 0 && R + 1 == T;
  return p;
}

}  // namespace auvp
#endif  // AUVP_FORECAST_PLACE_H

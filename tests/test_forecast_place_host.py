"""Where a forecast's rounds go among a planner's bins (csrc/forecast_place.h), on the host: placed_round_of_bin compiled with
g++ alone into a small program that prints its table for every (T, R, b), against the one-line formula
min(max(t - b, 0), R) -- the identity (b = 0, R + 1 = T), b = T - 1 and R = 0 among them -- and the shapes it refuses; and
rrt_dubins.place_forecast, the numpy form the host path of RRT.set_shark_grids uses."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
MAX_T, MAX_R = 6, 6

PROGRAM = r"""
#include <cstdio>
#include "forecast_place.h"
int main() {
  for (int T = 0; T <= %d; T++)
    for (int R = -1; R <= %d; R++)
      for (int b = -1; b <= T; b++) {
        const auvp::SfPlacePlan p = auvp::placed_round_of_bin(T, R, b);
        std::printf("%%d %%d %%d %%d %%d", T, R, b, (int)p.status, p.identity ? 1 : 0);
        for (int32_t r : p.round_of_bin) std::printf(" %%d", (int)r);
        std::printf("\n");
      }
  return 0;
}
""" % (MAX_T, MAX_R)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("forecast_place")
    src, exe = os.path.join(d, "place.cpp"), os.path.join(d, "place")
    open(src, "w").write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(REPO, "auv_sim_amd", "csrc"), src, "-o", exe],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    rows = {}
    for line in out.splitlines():
        v = [int(x) for x in line.split()]
        rows[tuple(v[:3])] = (v[3], v[4], v[5:])
    return rows


def test_every_shape_up_to_six_bins_and_six_rounds(table):
    OK, BAD_SHAPE, BAD_BIN = 0, 1, 2
    seen_identity = seen_last_bin = seen_one_round = 0
    for T in range(0, MAX_T + 1):
        for R in range(-1, MAX_R + 1):
            for b in range(-1, T + 1):
                status, identity, rounds = table[(T, R, b)]
                if T < 1 or R < 0:
                    assert (status, rounds) == (BAD_SHAPE, []), (T, R, b)
                    continue
                if not 0 <= b <= T - 1:
                    assert (status, rounds) == (BAD_BIN, []), (T, R, b)
                    continue
                assert status == OK and rounds == [min(max(t - b, 0), R) for t in range(T)], (T, R, b, rounds)
                assert identity == int(b == 0 and R + 1 == T), (T, R, b)
                if identity:
                    assert rounds == list(range(T))
                    seen_identity += 1
                seen_last_bin += b == T - 1 and rounds == [0] * T
                seen_one_round += R == 0 and rounds == [0] * T
    assert seen_identity == MAX_T and seen_last_bin > 0 and seen_one_round > 0


def test_numpy_placement_is_the_same_table(table):
    from auv_sim_amd.rrt_dubins import place_forecast
    for (T, R, b), (status, _, rounds) in table.items():
        if status != 0:
            continue
        prob = np.arange(2 * (R + 1) * 3, dtype=np.float64).reshape(2, R + 1, 3)
        got = place_forecast(prob, T, b)
        assert got.shape == (2, T, 3) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, prob[:, rounds, :]), (T, R, b)

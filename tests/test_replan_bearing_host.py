"""replan_atan2_round (csrc/replan_measure.h), the step that turns the particle-filter kernel's atan2 value into the correctly
rounded one for replan_measure_kernel's bearings, compiled with g++ alone: started from libm's value moved by -2 .. +2 ulp it
must return the double nearest to the true angle, which mpmath gives (200 bits); the special operands come back unchanged."""
import math
import os
import shutil
import subprocess

import pytest

from conftest import REPO

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <random>
#include "replan_measure.h"
int main() {
  std::mt19937_64 g(11);
  std::uniform_real_distribution<double> u(-200.0, 200.0), v(-1.0, 1.0);
  auto one = [&](double y, double x, int off) {
    double a0 = std::atan2(y, x);
    for (int k = 0; k < (off < 0 ? -off : off); k++) a0 = std::nextafter(a0, off < 0 ? -10.0 : 10.0);
    std::printf("%a %a %a %a\n", y, x, a0, auvp::replan_atan2_round(y, x, a0));
  };
  for (int i = 0; i < 1500; i++) one(u(g), u(g), i % 5 - 2);
  for (int i = 0; i < 300; i++) one(v(g) * 1e-9, u(g), i % 5 - 2);   // near 0 and near +-pi
  for (int i = 0; i < 300; i++) one(u(g), v(g) * 1e-9, i % 5 - 2);   // near +-pi/2
  for (int i = 0; i < 300; i++) { const double x = u(g); one(x * (1.0 + v(g) * 1e-12), x, i % 5 - 2); }  // near pi/4, -3pi/4
  const double sp[] = {0.0, -0.0, 25.0, -25.0, 1e-9, -1e-9, 30.0};
  for (double y : sp) for (double x : sp) one(y, x, 0);
  return 0;
}
"""


def test_rounds_to_the_nearest_double(tmp_path):
    import mpmath as mp
    src, exe = os.path.join(tmp_path, "bearing.cpp"), os.path.join(tmp_path, "bearing")
    open(src, "w").write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(REPO, "auv_sim_amd", "csrc"), src, "-o", exe],
                   check=True, capture_output=True, text=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == 1500 + 900 + 49
    moved = 0
    with mp.workprec(200):
        for line in lines:
            y, x, a0, r = (float.fromhex(t) for t in line.split())
            if y == 0.0:  # a signed zero: 0, -0, pi or -pi by the signs alone (mpmath knows no -0)
                assert r == a0 == math.atan2(y, x) and math.copysign(1.0, r) == math.copysign(1.0, a0), line
                continue
            true = mp.atan2(mp.mpf(y), mp.mpf(x))
            err = abs(true - mp.mpf(r))
            # the nearest double: no neighbour is closer (a tie does not occur: the true angle is irrational)
            assert err <= abs(true - mp.mpf(math.nextafter(r, math.inf))) and err <= abs(true - mp.mpf(math.nextafter(r, -math.inf))), line
            moved += r != a0
    assert moved > 1000  # (three starts in five were off by one or two ulp)

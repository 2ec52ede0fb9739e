"""RRT.replanning_batch without a GPU: the C-ABI of the per-episode limits is declared and exported, the host's commit step
between rounds restates the reference's splitPath / removeHabitat, the argument checks refuse what the library refuses, and
the two limits kernels cost no more scratch than the kernels they share their bodies with."""
import math
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO


def test_prepare_episodes_declared_and_exported():
    import __graft_entry__ as ge
    ge.build()
    hdr = open(os.path.join(REPO, "include", "auvplan.h")).read()
    assert re.search(r"typedef struct \{\s*double max_traj_time;[^}]*uint64_t habitat_keep;[^}]*\} auvp_rrt_episode;", hdr)
    assert re.search(r"\bint auvp_rrt_prepare_episodes\s*\(", hdr)
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(REPO, "auv_sim_amd", "libauvplan.so")],
                          capture_output=True, text=True, check=True).stdout.split()
    assert "auvp_rrt_prepare_episodes" in syms


class _P:
    def __init__(self, x, y, t):
        self.x, self.y, self.traj_time_stamp = x, y, t


class _H:
    def __init__(self, x, y, size):
        self.x, self.y, self.size = x, y, size


def _split_path(path, shark_interval, traj_time):
    """path_planning/rrt_dubins.py:590-602, restated"""
    bin_list = {}
    for i in range(math.floor(traj_time[1] / shark_interval)):
        bin_list[(traj_time[0] + i * shark_interval, traj_time[0] + (i + 1) * shark_interval)] = []
    for point in path:
        for time_bin in bin_list:
            if point.traj_time_stamp >= time_bin[0] and point.traj_time_stamp <= time_bin[1]:
                bin_list[time_bin].append(point)
                break
    return bin_list


def _remove_habitat(habitats, path):
    """path_planning/rrt_dubins.py:604-610, restated"""
    for point in path:
        for habitat in habitats:
            if math.sqrt((point.x - habitat.x) ** 2 + (point.y - habitat.y) ** 2) <= habitat.size:
                habitats.remove(habitat)
                break
    return habitats


def test_commit_step_restates_split_path_and_remove_habitat():
    """first bucket + keep-mask update (rrt_dubins.first_bucket_commit) against the reference's two helpers on random courses:
    overlapping habitats (a point inside several removes only the first one still listed), a point on the edge the first and
    second buckets share (it belongs to the first), random starting lists"""
    from auv_sim_amd.rrt_dubins import first_bucket_commit
    rng = random.Random(7)
    n_edge = 0
    for case in range(300):
        H = rng.randint(0, 12)
        cx, cy = rng.uniform(-50, 50), rng.uniform(-50, 50)
        hab = [(cx + rng.uniform(-30, 30), cy + rng.uniform(-30, 30), rng.uniform(5, 25)) for _ in range(H)]
        t0 = rng.choice([0.0, 93.00600185, rng.uniform(0, 400)])
        span = rng.choice([100.0, 78.5, rng.uniform(20, 120)])
        mtt = t0 + rng.uniform(span, 4 * span)
        n = rng.randint(1, 150)
        ts = sorted([t0] + [t0 + rng.uniform(0, mtt - t0 + 20) for _ in range(n - 1)])
        if case % 3 == 0:
            ts[len(ts) // 2] = t0 + 1 * span  # on the edge shared by the first two buckets
            ts.sort()
        x, y = cx, cy
        pts = []
        for t in ts:
            x, y = x + rng.uniform(-4, 4), y + rng.uniform(-4, 4)
            pts.append(_P(x, y, t))
        keep = rng.getrandbits(H) if case % 4 else (1 << H) - 1
        listed = [_H(*hab[h]) for h in range(H) if (keep >> h) & 1]
        idx_of = {id(o): h for o, h in zip(listed, [h for h in range(H) if (keep >> h) & 1])}
        buckets = _split_path(pts, span, [t0, mtt])
        first = buckets[next(iter(buckets))]
        left = _remove_habitat(list(listed), first)
        want_keep = sum(1 << idx_of[id(o)] for o in left)
        sel, got_keep = first_bucket_commit([p.traj_time_stamp for p in pts], [(p.x, p.y) for p in pts], t0, mtt, span, keep,
                                            np.array(hab).reshape(-1, 3))
        assert [p for p, s in zip(pts, sel) if s] == first, case
        assert got_keep == want_keep, case
        n_edge += any(p.traj_time_stamp == t0 + 1 * span for p in first)
    assert n_edge > 50
    with pytest.raises(ValueError):  # the reference's next(iter({})) raises as well: no whole bucket in the horizon
        first_bucket_commit([0.0], [(0.0, 0.0)], 0.0, 50.0, 100.0, 0, np.zeros((0, 3)))


def test_episode_limit_checks():
    """the binding refuses what auvp_rrt_prepare_episodes refuses (AUVP_ERR_ARG), before the library is reached"""
    from auv_sim_amd import _lib
    cap, rec = _lib.episode_limits(3, [60.0, 500.0, 137.5], [0, 0b111, 0b100], 3)
    assert cap == 500.0 and rec["max_traj_time"].tolist() == [60.0, 500.0, 137.5] and rec["habitat_keep"].tolist() == [0, 7, 4]
    cap, rec = _lib.episode_limits(2, 200.0, None, 64)  # every habitat of a full table
    assert cap == 200.0 and rec["habitat_keep"].tolist() == [2 ** 64 - 1] * 2
    with pytest.raises(ValueError):
        _lib.episode_limits(2, [100.0, 200.0], None, 3, mode="plantime")
    with pytest.raises(ValueError):
        _lib.episode_limits(2, [100.0, 200.0], None, 3, mode="nn")
    with pytest.raises(ValueError):
        _lib.episode_limits(2, [100.0, 200.0], None, 3, iter_log=True)
    with pytest.raises(ValueError):
        _lib.episode_limits(2, [100.0, 200.0], None, 3, phase_clocks=True)
    for bad in ([0.0, 100.0], [-1.0, 100.0], [float("nan"), 100.0], [float("inf"), 100.0]):
        with pytest.raises(ValueError):
            _lib.episode_limits(2, bad, None, 3)
    with pytest.raises(ValueError):
        _lib.episode_limits(2, 100.0, [1, 0b1000], 3)
    with pytest.raises(ValueError):
        _lib.episode_limits(1, 100.0, [1], 0)
    from auv_sim_amd.rrt_dubins import habitat_keep_bits
    assert habitat_keep_bits(None, 4, 2) == [15, 15]
    assert habitat_keep_bits([5, 0], 4, 2) == [5, 0]
    assert habitat_keep_bits(np.array([[True, False, True, False], [False] * 4]), 4, 2) == [5, 0]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_limits_kernels_use_no_more_scratch():
    """rrt_explore_lim_kernel<J> and rrt_leaf_lim_kernel are the bodies of rrt_explore_kernel<J, 0, false> and rrt_leaf_kernel
    with per-episode limits: no more scratch than those; up to 256 obstacles six wavefronts per SIMD, what the LDS plan of three
    8-wavefront workgroups per CU needs"""
    from test_kernel_resources import _resources
    res = _resources("auvplan.hip")
    for J in (1, 2, 4, 8, 16):
        new, old = res["auvp::rrt_explore_lim_kernel<%d>" % J], res["auvp::rrt_explore_kernel<%d, 0, false>" % J]
        assert new["scratch"] <= old["scratch"] and (J > 4 or new["waves"] >= 6), (J, new, old)
    new, old = res["auvp::rrt_leaf_lim_kernel"], res["auvp::rrt_leaf_kernel"]
    assert new["scratch"] <= old["scratch"], (new, old)

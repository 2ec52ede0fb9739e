"""The team fold of RRT.replanning_batch(teams=...), without a GPU: csrc/replan_teams.h (the pure header replan_team_kernel and
its host side are built from) compiled into tests/host/replan_team_check.cpp with g++ and the address / undefined-behaviour
sanitizers, run on crafted and random label and mask arrays, and compared for exact equality with rrt_dubins.team_csr /
team_fold -- the Python statement of the rule; team_labels' refusals; and replanning_batch's, before it touches a device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import replan_team_cases as tc
from auv_sim_amd.rrt_dubins import RRT, team_csr, team_fold, team_labels

REPO = tc.REPO
ALL = tc.ALL

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """cases -> [(team_off, members, keep)] through the sanitized program"""
    d = tmp_path_factory.mktemp("replan_teams")
    exe = str(d / "replan_team_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "auv_sim_amd", "csrc"), "-o", exe,
                    os.path.join(REPO, "tests", "host", "replan_team_check.cpp")], check=True)
    count = [0]

    def go(cases):
        count[0] += 1
        src, dst = str(d / ("in%d.bin" % count[0])), str(d / ("out%d.bin" % count[0]))
        tc.write_cases(src, cases)
        r = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]  # the sanitizers report on stderr
        return tc.read_results(dst, cases)

    return go


def check(cases, got):
    assert len(got) == len(cases)
    for c, (off, mem, keep) in zip(cases, got):
        e_off, e_mem, e_keep = tc.expected(c)
        assert np.array_equal(off, e_off) and np.array_equal(mem, e_mem), (c["name"], off, mem)
        assert keep == e_keep, (c["name"], [hex(k) for k in keep], [hex(k) for k in e_keep])


# ---- the Python definition by its own expectation ------------------------------------------------------------------------

def test_team_fold_means_what_it_says():
    by = {c["name"]: tc.expected(c) for c in tc.crafted()}
    assert by["n = 1"][0].tolist() == [0] and by["n = 1"][2] == [0x3ff]
    assert by["all labels negative"][0].tolist() == [0] and by["all labels negative"][2] == [1, 2, 3, 4]
    off, mem, keep = by["a team of one next to a team of two"]
    assert off.tolist() == [0, 2] and mem.tolist() == [0, 2] and keep == [0b010, 0b001, 0b010, 0b111]
    assert by["a team of one alone"][1].tolist() == [] and by["a team of one alone"][2] == [ALL]
    off, mem, keep = by["labels 7, 1000000, 0 interleaved"]  # teams in label order: 0, 7, 1000000
    assert off.tolist() == [0, 3, 6, 8] and mem.tolist() == [2, 5, 6, 0, 3, 7, 1, 4]
    assert keep == [0x3c, 0xf00, 0x31, 0x3c, 0xf00, 0x31, 0x31, 0x3c]
    assert by["a mask of 0 empties the team"][2] == [0, 0, 0]
    assert by["masks 2**64 - 1 and 0"][2] == [ALL, ALL, ALL, 0, 0]
    assert by["bit 63 leaves"][2] == [ALL & ~(1 << 63)] * 3
    assert by["bit 63 stays"][2] == [1 << 63, 0, 1 << 63]
    assert by["bits 31, 32, 33 and 63: both halves of the word"][2] == [1 << 63, 1 << 32, 1 << 63, 1 << 32, 77]
    assert by["every member lacks a bit of its own"][2] == [0x3f8] * 4
    assert by["disjoint lists"][2] == [0, 0]
    # the input is not changed, numpy masks are taken too, and folding twice changes nothing
    keep = np.array([6, 3, 9], dtype=np.uint64)
    assert team_fold(keep, [1, 1, -1]) == [2, 2, 9] and keep.tolist() == [6, 3, 9]
    assert team_fold(team_fold([6, 3, 9], [1, 1, -1]), [1, 1, -1]) == [2, 2, 9]
    with pytest.raises(ValueError):
        team_fold([1, 2], [0, 0, 0])


def test_team_labels_checks_its_input():
    lab = team_labels([0, 0, -1, 1000000, np.int64(7), 2.0], 6)
    assert lab.dtype == np.int32 and lab.tolist() == [0, 0, -1, 1000000, 7, 2]
    assert team_labels(np.array([3, -2], dtype=np.int16), 2).tolist() == [3, -2]
    assert team_labels([], 0).tolist() == []
    for bad, n in (([0, 0], 3), ([0, 0, 0, 0], 3), ([0, True, 1], 3), ([np.bool_(False), 0, 1], 3), ([0, 1.5, 1], 3),
                   ([0, "a", 1], 3), ([0, None, 1], 3), ([0, float("nan"), 1], 3), ([0, 2 ** 31, 1], 3), ([0, -2 ** 31 - 1, 1], 3)):
        with pytest.raises(ValueError):
            team_labels(bad, n)


def test_malformed_teams_are_refused_before_any_launch():
    """a planner object without a device context: the refusal comes before replanning_batch reads any of it"""
    rrt = RRT.__new__(RRT)
    starts = [object(), object(), object()]
    for bad in ([0, 0], [0, 0, 1, 1], [0, True, 0], [0, 0.5, 0], [0, "x", 0]):
        for commit in ("host", "device"):
            with pytest.raises(ValueError):
                rrt.replanning_batch(starts, [], 2.0, 150.0, 98.0, [-3, -3, -4], max_iter=10, seeds=[1, 2, 3], commit=commit, teams=bad)
    assert not hasattr(rrt, "_ctx")


# ---- the header ---------------------------------------------------------------------------------------------------------------

@needs_gxx
def test_crafted_cases_equal_team_fold(run):
    cases = tc.crafted()
    names = " | ".join(c["name"] for c in cases)
    for need in ("n = 1", "all labels negative", "a team of one", "7, 1000000, 0", "2**64 - 1 and 0", "bit 63"):
        assert need in names
    check(cases, run(cases))


@needs_gxx
def test_sizes_around_the_wavefront_equal_team_fold(run):
    """one team per size, members interleaved, each team with one member that lacks a bit of its own"""
    sizes = [1, 2, 63, 64, 65, 129, 1000]
    labels = np.concatenate([np.full(s, 10 * k, dtype=np.int32) for k, s in enumerate(sizes)])
    labels = labels[np.random.default_rng(3).permutation(len(labels))]
    keep = [ALL] * len(labels)
    for k in range(len(sizes)):
        keep[int(np.flatnonzero(labels == 10 * k)[-1])] = ALL & ~(1 << (k + 57))
    c = tc.case(labels, keep, "sizes")
    (off, mem, got), = run([c])
    assert np.diff(off).tolist() == sizes[1:]
    assert [got[int(np.flatnonzero(labels == 10 * k)[0])] for k in range(len(sizes))] == \
        [ALL & ~(1 << (k + 57)) for k in range(len(sizes))]  # (the team of one: its own mask)
    check([c], [(off, mem, got)])


@needs_gxx
def test_random_cases_equal_team_fold(run):
    cases = tc.random_cases(500)
    assert {len(c["labels"]) for c in cases} >= {1, 2} and max(len(c["labels"]) for c in cases) > 128
    assert any(len(team_csr(c["labels"])[0]) == 1 for c in cases) and max(len(team_csr(c["labels"])[0]) for c in cases) > 4
    check(cases, run(cases))

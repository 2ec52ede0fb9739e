"""The commit rule of replanning's step between two rounds, without a GPU: csrc/replan_commit.h (the pure header
rrt_commit_kernel is built from) compiled into tests/host/replan_commit_check.cpp with g++ and the address /
undefined-behaviour sanitizers, run on crafted and random cases, and compared for exact equality with
rrt_dubins.first_bucket_commit -- the Python statement of the reference's splitPath first bucket + removeHabitat."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import replan_cases as rc

REPO = rc.REPO

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """cases -> [(sel, rows, keep, last)] through the sanitized program"""
    d = tmp_path_factory.mktemp("replan_commit")
    exe = str(d / "replan_commit_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "auv_sim_amd", "csrc"), "-o", exe,
                    os.path.join(REPO, "tests", "host", "replan_commit_check.cpp")], check=True)
    count = [0]

    def go(cases):
        count[0] += 1
        src, dst = str(d / ("in%d.bin" % count[0])), str(d / ("out%d.bin" % count[0]))
        rc.write_cases(src, cases)
        r = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]  # the sanitizers report on stderr
        return rc.read_results(dst, cases)

    return go


def check(cases, got):
    assert len(got) == len(cases)
    for c, (sel, rows, keep, last) in zip(cases, got):
        e_sel, e_rows, e_keep, e_last = rc.expected(c)
        assert np.array_equal(sel, e_sel), c["name"]
        assert rc.same(rows, e_rows), c["name"]
        assert keep == e_keep, (c["name"], hex(keep), hex(e_keep))
        assert rc.same(last, e_last), c["name"]


def test_crafted_cases_equal_first_bucket_commit(run):
    cases = rc.crafted()
    assert sorted(set(len(c["course"]) for c in cases if c["name"].startswith("length"))) == sorted(rc.LENGTHS)
    check(cases, run(cases))


def test_crafted_cases_mean_what_they_say(run):
    """the seams by their own expectation, not only by the Python definition"""
    by = {c["name"]: r for c, r in zip(rc.crafted(), run(rc.crafted()))}
    sel = by["edges: lo, hi, above hi, nan, below lo, a selected row after unselected ones"][0]
    assert sel.tolist() == [True, True, True, False, False, False, True, False]
    assert [by["edge %d alone" % k][0][1] for k in range(4)] == [True, True, False, False]
    assert by["only row 0 selected"][0].sum() == 1 and by["only row 0 selected"][0][0]
    s = by["alternating selection"]
    assert s[0][:3].all() and not s[0][3::2].any() and s[0][4::2].all() and len(s[1]) == int(s[0].sum())
    assert np.all(np.diff(s[1][1:, 5]) > 0)  # (the course's plan stamps count its rows: the order is kept)
    assert by["row 0 substituted"][2] == 0 and by["row 0 substituted"][1][0, 0] == 100.0
    assert [by["H = %d" % H][2] for H in (0, 1, 33, 64)] == [0, 0, (1 << 32) - 1, (1 << 63) - 1]
    assert by["bits 32 and 63"][2] == ((1 << 64) - 1) & ~(1 << 32) & ~(1 << 63)
    assert by["keep == 0"][2] == 0
    assert by["on the radius"][2] == 0
    assert by["overlapping habitats"][2] == 4
    assert by["inside a habitat that already left"][2] == 4
    # all selected: the new state is the course's last row
    c = [c for c in rc.crafted() if c["name"] == "length 300, all selected"][0]
    assert rc.same(by["length 300, all selected"][3], c["course"][-1]) and len(by["length 300, all selected"][1]) == 300


def test_random_cases_equal_first_bucket_commit(run):
    cases = rc.random_cases(500)
    assert {len(c["hab"]) for c in cases} >= {0, 64} and max(len(c["course"]) for c in cases) > 256
    check(cases, run(cases))

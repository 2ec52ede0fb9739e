"""The team-aware winner selection of RRT.replanning_batch(team_pick="claims"), without a GPU: the Python rule
(rrt_dubins.course_habitat_words / rescore / team_pick_claims) against the CPU checker's habitat_shark_cost_func, bit for bit;
csrc/replan_pick.h (the pure header the two kernels are built from) compiled into tests/host/replan_pick_check.cpp with
g++ -ffp-contract=off, plain and under the address / undefined-behaviour sanitizers, against the Python rule; and
replanning_batch's refusals before it touches a device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import team_pick_cases as pc
from auv_sim_amd.rrt_dubins import RRT, course_habitat_words, rescore, team_csr, team_pick_claims

REPO = pc.REPO
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def cases():
    return pc.crafted(), pc.random_cases(200)


# ---- 1. rescore against the CPU checker ---------------------------------------------------------------------------------------

def test_rescore_equals_the_checkers_cost_under_every_mask(orc, cases):
    """every candidate of every crafted and every random case (a course that occurs twice in a case with the same bins and leaf
    time is taken once), under the full list, the AUV's list, and lists with claims taken out: rescore == orc.cost on a world
    whose habitat list is the masked one, all four doubles bit for bit.  c2 comes from the checker under the full list: it must
    not depend on the list."""
    crafted, rnd = cases
    rng = np.random.default_rng(7)
    n = distinct = 0
    for c in crafted + rnd:
        w = pc.WORLDS[c["world"]]
        hab = w["habitats"]
        H = len(hab)
        full = (1 << H) - 1
        none = np.zeros((0, 3))
        world_of = {}

        def world(mask):
            if mask not in world_of:
                world_of[mask] = orc.WorldArrays(none, hab[[h for h in range(H) if (mask >> h) & 1]].reshape(-1, 3), np.zeros((0, 2)), w["bins"],
                                                 w["cells"], w["prob"])
            return world_of[mask]

        seen = set()
        for e, p in enumerate(c["courses"]):
            if len(p) == 0:
                continue
            lo, hi, lt = c["bin_lo"][e], c["bin_hi"][e], c["leaf_t"][e]
            key = (p.tobytes(), lo, hi, lt)
            if key in seen:
                continue
            seen.add(key)
            distinct += 1
            words = c["words"][e]
            ref_full = orc.cost(world(full), lo, hi, p, lt, c["weights"])
            c2 = float(ref_full[3])
            own = c["keep"][c["active"][e // c["K"]]] & full
            masks = {full, own, own & ~(1 << int(rng.integers(0, 64))), own & int(rng.integers(0, 1 << 62)), 0}
            vis_full = rescore(words, full, c2, lt, c["weights"])[1]
            masks.add(own & ~vis_full)  # (everything the course visits claimed by somebody else)
            for m in masks:
                got, _ = rescore(words, m, c2, lt, c["weights"])
                want = ref_full if m == full else orc.cost(world(m), lo, hi, p, lt, c["weights"])
                assert pc.bits_equal(got, want), (c["name"], e, hex(m), got, want.tolist())
                n += 1
    assert distinct > 2400 and n >= 4 * distinct  # (up to six different masks each; where H == 0 only the empty one)


def test_rescore_and_words_mean_what_they_say():
    hab = np.array([[0.0, 0.0, 5.0], [3.0, 0.0, 5.0], [50.0, 50.0, 5.0]])
    bins = np.array([[0.0, 10.0], [10.0, 20.0]])
    xy = [[1.5, 0.0], [-3.0, 0.0], [50.0, 55.0], [50.0, 55.000001], [1.5, 0.0], [1.5, 0.0]]
    t = [0.0, 10.0, 20.0, 5.0, 20.5, np.nan]
    assert course_habitat_words(xy, t, bins, 0, 2, hab) == [3, 1, 4, 0, 0, 0]
    assert course_habitat_words(xy, t, bins, 1, 2, hab) == [0, 1, 4, 0, 0, 0]  # (t = 10 is in both bins, t = 0 only in bin 0)
    assert course_habitat_words(xy, t, bins, 0, 0, hab) == [0] * 6 and course_habitat_words(xy, t, bins, 0, 2, hab[:0]) == [0] * 6
    words = [3, 1, 4, 0]
    s, vis = rescore(words, 7, -0.5, 10.0, [-3, -3, -4])
    assert vis == 5 and s == [((0.0 + -3 * 2 / 3) + -9 / 10.0) + -0.5, -3 * 2 / 3, -0.9, -0.5]
    s, vis = rescore(words, 6, -0.5, 10.0, [-3, -3, -4])  # habitat 0 claimed: the first point's hit moves to habitat 1
    assert vis == 6 and s[1:] == [-3.0, -6 / 10.0, -0.5]
    s, vis = rescore(words, 0, -0.5, 10.0, [-3, -3, -4])
    assert vis == 0 and s == [-0.5, 0.0, 0.0, -0.5]
    # a non-integer weight is added hit by hit: ten hits of 0.1 are not 1.0
    s, _ = rescore([1] * 10, 1, 0.0, 0.0, [0.0, 0.1, 0.0])
    assert s[2] == 0.1 + 0.1 + 0.1 + 0.1 + 0.1 + 0.1 + 0.1 + 0.1 + 0.1 + 0.1 != 0.1 * 10
    s, _ = rescore([], 1, -0.0, 1.0, [-3.0, -0.0, -4.0])
    assert np.signbit(s[3]) and not np.signbit(s[2]) and not np.signbit(s[0])


def test_the_crafted_cases_hold_what_their_names_say(cases):
    by = {c["name"]: (c, pc.expected(c)) for c in cases[0]}
    c, r = by["bit 63 claimed"]
    assert r[0]["winner"] == 0 and r[1]["claimed"] == 1 << 63 and r[1]["winner"] == 1
    c, r = by["bit 63 not claimed"]
    assert r[1]["claimed"] == 1 << 5 and r[1]["winner"] == 0
    c, r = by["claimed empties the member's mask: H' == 0"]
    assert r[1]["claimed"] == 1 << 3 and r[1]["cost"][1] == 0.0 and r[1]["cost"][2] == 0.0 and r[1]["winner"] == 0
    c, r = by["a member with no leaf in any tree"]
    assert r[1]["winner"] == -1 and r[1]["n_with_leaf"] == 0 and r[1]["cost"] == [np.inf] * 4 and r[2]["claimed"] == r[1]["claimed"] != 0
    c, r = by["a member absent from the round"]
    assert [x["claimed"] == 0 for x in r] == [True, False, True]  # (AUV 3: a loner; AUV 0 comes before AUV 2)
    c, r = by["equal scores: the lower tree wins"]
    assert r[1]["winner"] == 1 and pc.rescore(c["words"][4], c["keep"][1] & ~r[1]["claimed"], -9.0, c["leaf_t"][4], c["weights"])[0] == r[1]["cost"]
    c, r = by["a NaN c2"]
    assert r[0]["winner"] in (1, 2) and r[1]["winner"] in (0, 2)
    c, r = by["every c2 a NaN"]
    assert [x["winner"] for x in r] == [-1, -1] and r[1]["claimed"] == 0
    c, r = by["inside two habitats, the lower one claimed"]
    assert r[1]["claimed"] == 1 and c["words"][2] == [3] * 4 and r[1]["winner"] == 0 and r[1]["cost"][1] == -3.0 / 2
    c, r = by["inside a habitat, in no selected bin"]
    assert c["words"][2] == [0] * 4 and r[1]["winner"] == 1
    c, r = by["w2 = -0.1: repeated addition, not the product"]
    by_adding = 0.0
    for _ in range(11):
        by_adding = by_adding + -0.1
    assert r[0]["winner"] == 1 and r[0]["cost"][2] == by_adding != -0.1 * 11  # (the sum differs from the product in the last bit)
    c, r = by["a leaf time of 0"]
    assert r[0]["cost"][2] == -18.0  # (six hits, not divided)
    c, r = by["teams of 2, 3, 64 and 65 between loners and a team of one"]
    assert sum(x["claimed"] != 0 for x in r) >= 100
    # the invariant: whoever sees claimed == 0 gets the tree's own cost, and rrt_group_best's winner
    for c, r in by.values():
        cands = pc.candidates(c)
        for g, x in enumerate(r):
            if x["claimed"] == 0 and x["winner"] >= 0:
                assert pc.bits_equal(x["cost"], cands[g][x["winner"]]["cost"]), (c["name"], g)
                assert x["winner"] == min((k for k, q in enumerate(cands[g]) if q is not None and q["cost"][0] == x["cost"][0])), (c["name"], g)


# ---- 2. the header --------------------------------------------------------------------------------------------------------------

def _build(d, name, flags):
    exe = str(d / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off"] + flags + ["-I", os.path.join(REPO, "auv_sim_amd", "csrc"), "-o", exe,
                    os.path.join(REPO, "tests", "host", "replan_pick_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("replan_pick")
    return d, _build(d, "replan_pick_check", []), _build(d, "replan_pick_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(d, exe, cases, tag):
    src, dst = str(d / ("in_%s.bin" % tag)), str(d / ("out_%s.bin" % tag))
    pc.write_cases(src, cases)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]  # the sanitizers report on stderr
    return pc.read_results(dst, cases)


def _check(cases, got):
    assert len(got) == len(cases)
    for c, (win, cost, claimed, words) in zip(cases, got):
        want = pc.expected(c)
        assert words == c["words"], c["name"]
        in_team = {int(m) for m in team_csr(c["labels"])[1]}
        for g, a in enumerate(c["active"]):
            if a not in in_team:
                assert win[g] == -2, (c["name"], g)
                continue
            assert win[g] == want[g]["winner"] and claimed[g] == want[g]["claimed"], (c["name"], g, win[g], want[g])
            assert pc.bits_equal(cost[g], want[g]["cost"]), (c["name"], g, cost[g], want[g]["cost"])


@needs_gxx
@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_header_reproduces_team_pick_claims(programs, cases, which):
    d, plain, san = programs
    crafted, rnd = cases
    _check(crafted + rnd, _run(d, plain if which == "plain" else san, crafted + rnd, which))


# ---- 3. the argument errors of team_pick ----------------------------------------------------------------------------------------

def test_team_pick_is_refused_before_any_launch():
    """a planner object without a device context: the refusal comes before replanning_batch reads any of it"""
    rrt = RRT.__new__(RRT)
    starts = [object(), object(), object()]
    args = (starts, [], 2.0, 150.0, 98.0, [-3, -3, -4])
    for commit in ("host", "device"):
        with pytest.raises(ValueError, match="needs teams"):
            rrt.replanning_batch(*args, max_iter=10, seeds=[1, 2, 3], commit=commit, team_pick="claims")
        for bad in ("claim", "", True, 1, "CLAIMS"):
            with pytest.raises(ValueError, match="team_pick"):
                rrt.replanning_batch(*args, max_iter=10, seeds=[1, 2, 3], commit=commit, teams=[0, 0, 1], team_pick=bad)
        with pytest.raises(ValueError):  # (malformed teams are still refused first)
            rrt.replanning_batch(*args, max_iter=10, seeds=[1, 2, 3], commit=commit, teams=[0, 0], team_pick="claims")
    import random
    with pytest.raises(ValueError, match="rngs"):  # (as without team_pick: one generator cannot continue K streams)
        rrt.replanning_batch(*args, max_iter=10, rngs=[random.Random(1)] * 3, trees_per_auv=2, teams=[0, 0, 1], team_pick="claims")
    with pytest.raises(ValueError, match="rngs"):
        rrt.replanning_batch(*args, max_iter=10, rngs=[random.Random(1)] * 3, commit="device", teams=[0, 0, 1], team_pick="claims")
    assert not hasattr(rrt, "_ctx")


def test_team_pick_claims_leaves_its_inputs_alone():
    keep = np.array([7, 7, 7], dtype=np.uint64)
    cands = [[dict(words=[1, 1], cost=[-1.0, -1.0, 0.0, 0.0], leaf_time=2.0)], [dict(words=[1, 2], cost=[-2.0, -2.0, 0.0, 0.0], leaf_time=2.0)]]
    r = team_pick_claims(np.array([0, 0, -1], dtype=np.int32), keep, [1, 0], cands, [-3, -3, -4])
    assert keep.tolist() == [7, 7, 7]
    # group 1 is AUV 0: it goes first and claims habitat 0 and 1; group 0 (AUV 1) sees them
    assert r[1]["claimed"] == 0 and r[0]["claimed"] == 3 and r[0]["winner"] == 0 and r[0]["cost"][1:3] == [0.0, 0.0]

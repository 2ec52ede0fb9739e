"""The winner selection of RRT.replanning_batch(team_separation=d), without a GPU: the Python rule (rrt_dubins.course_ticks /
tick_conflicts / team_pick_separated) on hand-made courses whose tables are written out here, its invariants over every crafted
and random case, csrc/replan_apart.h (the pure header the two kernels are built from) compiled into
tests/host/replan_apart_check.cpp with g++ -ffp-contract=off, plain and under the address / undefined-behaviour sanitizers,
against the Python rule bit for bit; and replanning_batch's refusals before it touches a device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import separation_cases as sc
import team_pick_cases as pc
from auv_sim_amd.rrt_dubins import RRT, course_ticks, team_csr, team_pick_claims, team_pick_separated, tick_conflicts

REPO = sc.REPO
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def cases():
    return sc.crafted(), sc.random_cases(200)


# ---- 1. the rule on hand-made courses -------------------------------------------------------------------------------------------

def _table(t, W, tick=1.0, xy=None):
    """the table of the course whose row i sits at (i, 10 i) unless xy says otherwise: (s_lo, [x of every tick])"""
    xy = [[float(i), 10.0 * i] for i in range(len(t))] if xy is None else xy
    s_lo, out = course_ticks(t, xy, tick, W)
    assert out.shape == (len(out), 2) and all(out[:, 1] == 10.0 * out[:, 0])
    return s_lo, out[:, 0].tolist()


def test_tick_tables_of_hand_made_courses():
    # several rows in one tick: the last one owns it (ticks 5, 6, 7: rows 0, 3, 4)
    assert _table([5.0, 5.2, 5.7, 6.0, 7.0], 8) == (5, [0.0, 3.0, 4.0])
    # one slow row spanning many ticks: row 1 is reached at tick 9 and row 0 owns everything before
    assert _table([2.0, 9.0], 16) == (2, [0.0] * 7 + [1.0])
    # a row beyond the window extends the table to s_hi but owns nothing
    assert _table([0.0, 1.0, 50.0], 4) == (0, [0.0, 1.0, 1.0, 1.0])
    assert _table([0.0, 1.0, 3.0], 4) == (0, [0.0, 1.0, 1.0, 2.0])  # (the last tick of the window is still owned)
    # an infinite time extends the table as well; a NaN time does nothing
    assert _table([0.0, 1.0, INF], 4) == (0, [0.0, 1.0, 1.0, 1.0])
    assert _table([0.0, 1.0, NAN], 4) == (0, [0.0, 1.0])
    assert _table([0.0, NAN, 2.0], 4) == (0, [0.0, 0.0, 2.0])
    # a course of length 1, and W = 1
    assert _table([7.5], 10) == (8, [0.0])
    assert _table([7.5, 7.9, 8.0, 9.0], 1) == (8, [2.0])
    # a non-monotone course: the largest index wins, and a row before s_lo counts as s_lo
    assert _table([5.0, 8.0, 6.0, 7.0], 8) == (5, [0.0, 2.0, 3.0, 3.0])
    assert _table([5.0, 3.0, -INF], 8) == (5, [2.0])
    # the tick index is ceil(t / tick): one division
    assert _table([0.3, 0.6, 0.61, 2.0], 16, tick=0.3) == (1, [0.0, 1.0, 2.0, 2.0, 2.0, 2.0, 3.0])
    assert _table([-3.5, -2.0], 4) == (-3, [0.0, 1.0])
    # nothing to sample
    assert course_ticks([], np.zeros((0, 2)), 1.0, 4)[1].shape == (0, 2)
    assert course_ticks([NAN, 1.0], np.zeros((2, 2)), 1.0, 4)[1].shape == (0, 2)
    assert course_ticks([1e300, 1.0], np.zeros((2, 2)), 1e-3, 4)[1].shape == (0, 2)


def test_conflicts_of_hand_made_tables():
    a = (10, np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [3.0, 0.0]]))
    # exactly d apart: no conflict; one ulp closer: a conflict
    b = (10, np.array([[0.0, 5.0], [1.0, np.nextafter(5.0, 0.0)], [2.0, np.nextafter(5.0, 9.0)], [30.0, 0.0]]))
    assert tick_conflicts(a[0], a[1], [b], 5.0) == 1
    assert tick_conflicts(a[0], a[1], [b], np.nextafter(5.0, 9.0)) == 2
    # only the ticks both tables cover are compared, at the same tick
    assert tick_conflicts(a[0], a[1], [(12, a[1])], 1.5) == 0 and tick_conflicts(a[0], a[1], [(12, a[1])], 2.5) == 2
    assert tick_conflicts(a[0], a[1], [(14, a[1])], 100.0) == 0 and tick_conflicts(a[0], a[1], [(7, a[1])], 100.0) == 1
    # a tick counts once however many tables are close there; a NaN never conflicts
    assert tick_conflicts(a[0], a[1], [a, a, b], 1.0) == 4
    nan = (10, np.array([[NAN, 0.0], [1.0, NAN], [INF, 0.0], [3.0, 0.5]]))
    assert tick_conflicts(a[0], a[1], [nan], 1.0) == 1
    assert tick_conflicts(a[0], a[1], [], 1.0) == 0 and tick_conflicts(0, np.zeros((0, 2)), [a], 1.0) == 0


def test_the_crafted_cases_hold_what_their_names_say(cases):
    by = {c["name"]: c for c in cases[0]}
    for need in ("W = 1", "W = 63", "W = 64", "W = 65", "W = 1024", "K = 1", "K = 4", "K = 65", "teams of 2, 3, 64 and 65", "no leaf", "absent"):
        assert any(need in n for n in by), need
    assert max(len(t[1]) for t in by["W = 1024"]["ticks"]) == 1024 and max(len(t[1]) for t in by["W = 65"]["ticks"]) == 65
    for claims in (False, True):
        r = sc.expected(by["every candidate conflicts: the fewest win"], claims)
        assert r[0]["conflicts"] == 0 and r[1]["winner"] == 2 and r[1]["conflicts"] == 2
        r = sc.expected(by["equal n, different scores"], claims)
        assert r[1]["winner"] == 1 and r[1]["conflicts"] == 0
        r = sc.expected(by["equal n, equal scores: the lowest tree wins"], claims)
        assert r[1]["winner"] == 1 and r[1]["conflicts"] == 0
        c = by["a NaN score with n = 0 must not win"]
        r = sc.expected(c, claims)
        assert np.isnan(c["cost4"][3][0]) and r[1]["winner"] == 2 and r[1]["conflicts"] == 3  # (j * j + (1 + j) ** 2 < 16: j = 0, 1, 2)
        c = by["claims and separation disagree: n decides"]
        r = sc.expected(c, claims)
        assert r[1]["winner"] == 1 and r[1]["conflicts"] == 0 and r[1]["claimed"] == (1 if claims else 0)
        c = by["NaN, infinite and descending times"]
        assert c["ticks"][0][0] == 5 and len(c["ticks"][0][1]) == 16
        r = sc.expected(by["a member with no leaf in any tree"], claims)
        assert r[1]["winner"] == -1 and r[1]["conflicts"] == 0 and r[1]["cost"] == [np.inf] * 4
        r = sc.expected(by["teams of 2, 3, 64 and 65 between loners and a team of one"], claims)
        assert sum(x["conflicts"] > 0 for x in r) >= 20
    c = by["claims and separation disagree: n decides"]
    assert team_pick_claims(c["labels"], c["keep"], c["active"], pc.candidates(c), c["weights"])[1]["winner"] == 0
    r = sc.expected(by["d so small that nothing conflicts"], True)
    assert r[1]["winner"] == 0 and r[1]["conflicts"] == 0


# ---- 2. the invariants ------------------------------------------------------------------------------------------------------------

def _plain_fold(cands):
    out = []
    for row in cands:
        best, win, cost = np.inf, -1, [np.inf] * 4
        for k, c in enumerate(row):
            if c is not None and float(c["cost"][0]) < best:
                best, win, cost = float(c["cost"][0]), k, [float(x) for x in c["cost"]]
        out.append((win, cost))
    return out


def test_invariants_over_all_cases(cases):
    """whoever sees an empty trail chooses as team_pick_claims does (claims on) or as the plain fold does (claims off), the cost
    bits included; and with d so small that no tick conflicts every group equals the run without the option"""
    crafted, rnd = cases
    conflicting = changed = 0
    for c in crafted + rnd:
        cands = sc.candidates(c)
        by_claims, plain = team_pick_claims(c["labels"], c["keep"], c["active"], cands, c["weights"]), _plain_fold(cands)
        team_off, members = team_csr(c["labels"])
        slot_of = {a: g for g, a in enumerate(c["active"])}
        for claims in (False, True):
            r = sc.expected(c, claims)
            none = team_pick_separated(c["labels"], c["keep"], c["active"], cands, c["weights"], 1e-300, claims)
            empty_trail = set(range(len(c["active"])))  # the groups that have no teammate's winner before them in this run
            for t in range(len(team_off) - 1):
                seen = False
                for m in members[team_off[t]:team_off[t + 1]]:
                    g = slot_of.get(int(m))
                    if g is not None:
                        if seen:
                            empty_trail.discard(g)
                        seen = seen or r[g]["winner"] >= 0
            for g in range(len(c["active"])):
                want_w, want_c = (by_claims[g]["winner"], by_claims[g]["cost"]) if claims else plain[g]
                want_m = by_claims[g]["claimed"] if claims else 0
                tag = (c["name"], claims, g)
                assert none[g]["conflicts"] == 0 and none[g]["winner"] == want_w and pc.bits_equal(none[g]["cost"], want_c), tag
                assert none[g]["claimed"] == want_m and r[g]["n_with_leaf"] == by_claims[g]["n_with_leaf"], tag
                if g in empty_trail:
                    assert r[g]["conflicts"] == 0 and r[g]["winner"] == want_w and pc.bits_equal(r[g]["cost"], want_c), tag
                    assert r[g]["claimed"] == want_m, tag
                conflicting += r[g]["conflicts"] > 0
                changed += r[g]["winner"] != none[g]["winner"]
    assert conflicting > 400 and changed > 100


# ---- 3. the header --------------------------------------------------------------------------------------------------------------

def _build(d, name, flags):
    exe = str(d / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off"] + flags + ["-I", os.path.join(REPO, "auv_sim_amd", "csrc"), "-o", exe,
                    os.path.join(REPO, "tests", "host", "replan_apart_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("replan_apart")
    return d, _build(d, "replan_apart_check", []), _build(d, "replan_apart_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@needs_gxx
@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_header_reproduces_team_pick_separated(programs, cases, which):
    d, plain, san = programs
    pairs = [(c, claims) for c in cases[0] + cases[1] for claims in (False, True)]
    src, dst = str(d / ("in_%s.bin" % which)), str(d / ("out_%s.bin" % which))
    sc.write_cases(src, pairs)
    r = subprocess.run([plain if which == "plain" else san, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]  # the sanitizers report on stderr
    got = sc.read_results(dst, pairs)
    assert len(got) == len(pairs)
    for (c, claims), (rec, tables) in zip(pairs, got):
        want = sc.expected(c, claims)
        for e, (s_lo, xy) in enumerate(tables):
            assert s_lo == c["ticks"][e][0] and pc.bits_equal(xy, c["ticks"][e][1]) and xy.shape == c["ticks"][e][1].shape, (c["name"], e)
        in_team = {int(m) for m in team_csr(c["labels"])[1]}
        for g, a in enumerate(c["active"]):
            if a not in in_team:
                assert rec[g]["winner"] == -2, (c["name"], g)
                continue
            tag = (c["name"], claims, g, rec[g], want[g])
            assert int(rec[g]["winner"]) == want[g]["winner"] and int(rec[g]["claimed"]) == want[g]["claimed"], tag
            assert int(rec[g]["conflicts"]) == want[g]["conflicts"] and pc.bits_equal(rec[g]["cost"], want[g]["cost"]), tag


# ---- 4. the argument errors -------------------------------------------------------------------------------------------------------

def test_team_separation_is_refused_before_any_launch():
    """a planner object without a device context: the refusals come before replanning_batch reads any of it but the horizon"""
    rrt = RRT.__new__(RRT)
    starts = [object(), object(), object()]
    args = (starts, [], 2.0, 150.0, 98.0, [-3, -3, -4])
    kw = dict(max_iter=10, seeds=[1, 2, 3])
    for commit in ("host", "device"):
        for pick in (None, "claims"):
            if pick is None:
                with pytest.raises(ValueError, match="team_separation needs teams"):
                    rrt.replanning_batch(*args, commit=commit, team_separation=5.0, **kw)
            k = dict(kw, commit=commit, teams=[0, 0, 1], team_pick=pick)
            for bad in (0.0, -1.0, NAN, INF, True, "5", [5.0]):
                with pytest.raises(ValueError, match="team_separation"):
                    rrt.replanning_batch(*args, team_separation=bad, **k)
                with pytest.raises(ValueError, match="separation_tick"):
                    rrt.replanning_batch(*args, team_separation=5.0, separation_tick=bad, **k)
            for bad in (0, -1, 1025, True, 2.5, "8"):
                with pytest.raises(ValueError, match="separation_ticks"):
                    rrt.replanning_batch(*args, team_separation=5.0, separation_ticks=bad, **k)
            with pytest.raises(ValueError, match="separation_ticks"):  # (the default: ceil(100 / 0.05) = 2000 ticks)
                rrt.replanning_batch(*args, team_separation=5.0, separation_tick=0.05, **k)
            with pytest.raises(ValueError):  # (malformed teams are still refused first)
                rrt.replanning_batch(*args, team_separation=-5.0, **dict(k, teams=[0, 0]))
        with pytest.raises(ValueError, match="team_pick"):  # (and so is another team_pick)
            rrt.replanning_batch(*args, team_separation=5.0, **dict(kw, commit=commit, teams=[0, 0, 1], team_pick="rerank"))
        many = [object()] * 1030
        with pytest.raises(ValueError, match="1025 members"):
            rrt.replanning_batch(many, *args[1:], max_iter=10, seeds=list(range(1030)), commit=commit, teams=[3] * 1025 + [-1] * 5,
                                 team_separation=5.0)
        # the horizon's end against the tick: the one refusal that reads the planner's shark grid
        rrt.sharkGrid = {(0.0, 150.0): {}, (150.0, 2.0 ** 31 * 0.5): {}}
        with pytest.raises(ValueError, match="2\\*\\*31"):
            rrt.replanning_batch(*args, team_separation=5.0, separation_tick=0.5, separation_ticks=8, **dict(kw, commit=commit, teams=[0, 0, 1]))
        del rrt.sharkGrid
    assert not hasattr(rrt, "_ctx")


def test_team_pick_separated_leaves_its_inputs_alone():
    keep = np.array([7, 7, 7], dtype=np.uint64)
    t = (0, np.zeros((3, 2)))
    cands = [[dict(words=[1, 1], cost=[-1.0, -1.0, 0.0, 0.0], leaf_time=2.0, ticks=t)],
             [dict(words=[1, 2], cost=[-2.0, -2.0, 0.0, 0.0], leaf_time=2.0, ticks=t)]]
    r = team_pick_separated(np.array([0, 0, -1], dtype=np.int32), keep, [1, 0], cands, [-3, -3, -4], 1.0, False)
    assert keep.tolist() == [7, 7, 7] and t[1].tolist() == [[0.0, 0.0]] * 3
    # group 1 is AUV 0: it goes first; group 0 (AUV 1) has one candidate, which sits on it at all three ticks
    assert [x["conflicts"] for x in r] == [3, 0] and [x["winner"] for x in r] == [0, 0] and r[0]["cost"] == [-1.0, -1.0, 0.0, 0.0]

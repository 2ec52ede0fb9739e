"""RRT.replanning_batch(teams=..., team_separation=d): rrt_course_ticks_kernel and replan_team_pick_apart_kernel through their
probe entry against rrt_dubins.team_pick_separated, a fleet of ten AUVs in three teams whose members start together (the device
route against the host route, with the claims and without; the run with team_separation=None against the call as it was; the
first members and the loners against the run without the option; every round's choice and conflict count recomputed by the
Python rule from all the candidates; the committed trees and counts against the CPU checker's prediction), and the C-ABI of
auvp_replan_team_pick_apart.  Every comparison is bit for bit."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import separation_cases as sc
import team_pick_cases as pc
from conftest import GOLDEN
from test_gpu_replan_commit import _same_arrays, _world

pytestmark = pytest.mark.gpu

RECORD = 128  # bytes of one auvp_replan_record
N_AUVS, N_ITER, K3 = 10, 400, 3
BUDGET, LENGTH, INTERVAL = 2.0, 150.0, 98.0
WEIGHT = [-3, -3, -4]
TEAMS = [0, 0, 0, 0, 1, 1, 1, -1, -1, 2]
FIRST = [0, 4]        # the first member of each team of two or more
LONERS = [7, 8, 9]    # two AUVs on their own and a team of one
SEEDS = [31 * e + 3 for e in range(N_AUVS)]
SHARK_OF = [e % 2 for e in range(N_AUVS)]
D, TICK = 5.0, 1.0    # metres, seconds; the window is the default, ceil((2 + 98) / 1) = 100 ticks
# team 0 starts at habitat 0 (two members on the point, one a metre east, one a metre north), team 1 at habitat 4 likewise, the
# others each at their own habitat
OFFSET = [(0.0, 0.0), (1.0, 0.0), (0.0, 0.0), (0.0, 1.0), (0.0, 0.0), (1.0, 0.0), (0.0, 0.0), (0.0, 0.0), (0.0, 0.0), (0.0, 0.0)]
HOME = [0, 0, 0, 0, 4, 4, 4, 7, 8, 9]
# the CPU checker's prediction (oracle/orc.py's rrt_explore for every tree + team_pick_separated / team_pick_claims + first_bucket_commit
# + team_fold), made before the device ran: the tree every AUV commits in every round and the winner's conflicts, by team_pick
TREE = {None: [[1, 2, 0, 2, 2], [1, 0, 1, 0, 1], [1, 2, 1, 1, 1], [1, 2, 2, 2, 0], [2, 1, 1, 1, 2], [1, 2, 2, 1, 0], [0, 0, 1, 2, 2],
               [1, 2, 2, 0, 1], [0, 0, 2, 1, 0], [2, 0, 0, 0, 2]],
        "claims": [[1, 2, 0, 2, 2], [1, 0, 1, 0, 1], [1, 1, 1, 2, 0], [1, 0, 1, 2, 2], [2, 1, 1, 1, 1], [1, 2, 2, 0, 1], [1, 2, 0, 2, 2, 1, 1],
                   [1, 2, 2, 0, 1], [0, 0, 2, 1, 0], [2, 0, 0, 0, 2]]}
TREE_WITHOUT = {None: [[1, 0, 1, 0, 1], [1, 0, 0, 2, 2], [0, 0, 2, 1, 1], [2, 1, 0, 2, 1], [2, 1, 1, 1, 2], [0, 0, 0, 1, 1], [0, 0, 1, 0, 0],
                       [1, 2, 2, 0, 1], [0, 0, 2, 1, 0], [2, 0, 0, 0, 2]],
                "claims": [[1, 0, 0, 2, 0], [1, 0, 1, 0, 1], [2, 1, 2, 2, 0], [1, 0, 1, 2, 2], [2, 1, 1, 1, 2], [2, 0, 0, 2, 1], [1, 0, 2, 0, 0, 0],
                           [1, 2, 2, 0, 1], [0, 0, 2, 1, 0], [2, 0, 0, 0, 2]]}
FIRST_ROUND_CONFLICTS = [0, 4, 5, 7, 0, 5, 14, 0, 0, 0]  # (the same with and without the claims; no later round has any)


# ---- 1. the probe entry -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    return _lib.Context(0)


def _probe_args(c):
    return (c["labels"], c["keep"], c["active"], c["K"], c["courses"], c["cost4"], c["leaf_t"], c["length"], c["bin_lo"], c["bin_hi"], c["weights"])


def _probe_equals(ctx, cases):
    w = pc.WORLDS["h10"]
    ctx.set_world(None, w["habitats"], None, w["bins"], w["cells"], w["prob"])
    n = conflicting = 0
    for c in cases:
        assert c["world"] == "h10"
        K = c["K"]
        for claims in (False, True):
            rec, claimed, conflicts = ctx.replan_team_pick_apart_courses(*_probe_args(c), claims, c["d"], c["tick"], c["W"])
            want = sc.expected(c, claims)
            assert len(rec) == len(want) == len(c["active"]) and claimed.dtype == np.uint64 and conflicts.dtype == np.int32
            for g, x in enumerate(want):
                e = g * K + x["winner"]
                tag = (c["name"], claims, g, rec[g], int(conflicts[g]), x)
                assert int(claimed[g]) == x["claimed"] and int(conflicts[g]) == x["conflicts"], tag
                assert int(rec[g]["winner"]) == (e if x["winner"] >= 0 else -1) and int(rec[g]["n_with_leaf"]) == x["n_with_leaf"], tag
                assert int(rec[g]["status"]) == (0 if x["winner"] >= 0 else 1), tag
                assert pc.bits_equal(rec[g]["cost"], x["cost"]), tag
                if x["winner"] >= 0:
                    assert int(rec[g]["path_len"]) == len(c["courses"][e]) and rec[g]["length"] == c["length"][e], tag
                else:
                    assert int(rec[g]["path_len"]) == 0 and rec[g]["length"] == 0.0, tag
                n += 1
                conflicting += x["conflicts"] > 0
    return n, conflicting


def test_probe_crafted_cases_equal_team_pick_separated(ctx):
    n, conflicting = _probe_equals(ctx, sc.crafted())
    assert n > 300 and conflicting > 100


def test_probe_random_cases_equal_team_pick_separated(ctx):
    n, conflicting = _probe_equals(ctx, sc.random_cases(200))
    assert n > 1000 and conflicting > 200


def test_probe_refuses_bad_arguments(ctx):
    from auv_sim_amd._lib import AuvpError
    w = pc.WORLDS["h10"]
    ctx.set_world(None, w["habitats"], None, w["bins"], w["cells"], w["prob"])
    c = sc.crafted()[1]
    args = _probe_args(c)
    good = ctx.replan_team_pick_apart_courses(*args, True, c["d"], c["tick"], c["W"])
    nan, inf = float("nan"), float("inf")
    for d, tick, W in ((0.0, 1.0, 8), (-1.0, 1.0, 8), (nan, 1.0, 8), (inf, 1.0, 8), (4.0, 0.0, 8), (4.0, -2.0, 8), (4.0, nan, 8), (4.0, inf, 8),
                       (4.0, 1.0, 0), (4.0, 1.0, -3), (4.0, 1.0, 1025)):
        with pytest.raises(AuvpError) as err:
            ctx.replan_team_pick_apart_courses(*args, True, d, tick, W)
        assert err.value.code == -1, (d, tick, W)
    big = sc.sep_case(4.0, 1.0, 8, "h10", [3] * 1025, [sc.FULL10] * 1025, [0, 1], 1, [sc.line([0, 0], [5, 0], 6)] * 2, "a team of 1025")
    with pytest.raises(AuvpError) as err:
        ctx.replan_team_pick_apart_courses(*_probe_args(big), False, 4.0, 1.0, 8)
    assert err.value.code == -1
    a = list(args)
    a[2] = [0, 0] + list(c["active"][2:])  # (an AUV named twice: as the claims' probe refuses it)
    with pytest.raises(AuvpError) as err:
        ctx.replan_team_pick_apart_courses(*a, True, c["d"], c["tick"], c["W"])
    assert err.value.code == -1
    again = ctx.replan_team_pick_apart_courses(*args, True, c["d"], c["tick"], c["W"])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(good, again))
    # a team of exactly 1024 members is taken
    cap = sc.sep_case(4.0, 1.0, 8, "h10", [3] * 1024, [sc.FULL10] * 1024, [5, 1000], 1, [sc.line([0, 0], [5, 0], 6)] * 2, "a team of 1024")
    _, _, conflicts = ctx.replan_team_pick_apart_courses(*_probe_args(cap), False, 4.0, 1.0, 8)
    assert conflicts.tolist() == [0, 6]


# ---- 2. the fleet ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fleet():
    """ten AUVs, teammates starting together, three trees each, two shark tables: TEAMS without the option and with it, with
    team_pick=None and "claims", on both routes"""
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    from auv_sim_amd.rrt_dubins import RRT
    g = np.load(os.path.join(GOLDEN, "g13_replan_a.npz"))
    obstacles, habitats, cell_list, grids, poly = _world(g)
    assert len(habitats) == N_AUVS
    rrt = RRT(poly, obstacles, grids[0], cell_list)
    rrt.set_shark_grids(grids)
    starts = [MPS(habitats[HOME[e]].x + OFFSET[e][0], habitats[HOME[e]].y + OFFSET[e][1]) for e in range(N_AUVS)]
    args = (starts, habitats, BUDGET, LENGTH, INTERVAL, WEIGHT)
    kw = dict(max_iter=N_ITER, seeds=SEEDS, as_arrays=True, trees_per_auv=K3, shark_of=SHARK_OF, teams=TEAMS)
    sep = dict(team_separation=D, separation_tick=TICK)
    out = dict(rrt=rrt, starts=starts, habitats=habitats, grids=grids, hab=g["habitats"], golden=g)
    for pick in (None, "claims"):
        out["without", pick, "host"] = rrt.replanning_batch(*args, team_pick=pick, **kw)  # (the call as it was: no keyword at all)
        out["without", pick, "dev"] = rrt.replanning_batch(*args, commit="device", team_pick=pick, **kw)
        out["kernel_plain", pick], out["info_plain", pick] = rrt._ctx.last_rrt_kernel(), rrt._ctx.replan_info()
        out["off", pick, "dev"] = rrt.replanning_batch(*args, commit="device", team_pick=pick, team_separation=None, **kw)
        out["kernel_off", pick], out["info_off", pick] = rrt._ctx.last_rrt_kernel(), rrt._ctx.replan_info()
        out["sep", pick, "host"] = rrt.replanning_batch(*args, team_pick=pick, **sep, **kw)
        out["sep", pick, "dev"] = rrt.replanning_batch(*args, commit="device", team_pick=pick, **sep, **kw)
        out["info_sep", pick] = rrt._ctx.replan_info()
    return out


def test_routes_agree_in_every_array(fleet):
    for pick in (None, "claims"):
        host, dev = fleet["sep", pick, "host"], fleet["sep", pick, "dev"]
        assert all(r is not None and len(r["round_len"]) >= 5 for r in host)
        assert all(r["round_conflicts"].dtype == np.int64 and r["round_conflicts"].shape == r["round_len"].shape for r in host)
        assert all(("round_claimed" in r) == (pick is not None) for r in host)
        _same_arrays(dev, host, "team_separation, team_pick=%r" % (pick,))
        _same_arrays(fleet["without", pick, "dev"], fleet["without", pick, "host"], "no team_separation, team_pick=%r" % (pick,))
        assert all("round_conflicts" not in r for r in fleet["without", pick, "host"] + fleet["off", pick, "dev"])


def test_team_separation_none_is_the_call_as_it_was(fleet):
    """the same arrays, the same expansion kernel and the same counters (commit_ms apart) as the call without the keyword; and
    with the option nothing more than the records crosses the bus either"""
    for pick in (None, "claims"):
        assert fleet["kernel_off", pick] == fleet["kernel_plain", pick] != ""
        _same_arrays(fleet["off", pick, "dev"], fleet["without", pick, "dev"], "team_separation=None")
        a, b = fleet["info_off", pick], fleet["info_plain", pick]
        assert {k: a[k] for k in a if k != "commit_ms"} == {k: b[k] for k in b if k != "commit_ms"}
        d = fleet["info_sep", pick]
        n_records = sum(len(r["round_len"]) for r in fleet["sep", pick, "dev"])
        assert d["bytes_to_host"] - d["bytes_traj"] == n_records * RECORD and d["bytes_traj"] == d["rows"] * 56 and d["commit_ms"] > 0.0


def test_first_members_and_loners_are_unchanged(fleet):
    """an empty trail: round 1 of the first member of each team and every round of the AUVs without a teammate are those of the
    run without the option"""
    for pick in (None, "claims"):
        for route in ("host", "dev"):
            for e in FIRST:
                t, a = fleet["sep", pick, route][e], fleet["without", pick, "host"][e]
                n = int(a["round_len"][0])
                assert int(t["round_conflicts"][0]) == 0 and int(t["round_len"][0]) == n > 0 and np.array_equal(t["traj"][:n], a["traj"][:n]), (route, e)
                assert pc.bits_equal(t["round_cost"][0], a["round_cost"][0]) and int(t["round_tree"][0]) == int(a["round_tree"][0]), (route, e)
            for e in LONERS:
                t, a = dict(fleet["sep", pick, route][e]), fleet["without", pick, "host"][e]
                assert not t.pop("round_conflicts").any(), (route, e)
                _same_arrays([t], [a], "%s, AUV %d" % (route, e))


def test_every_round_is_the_rule_on_all_its_candidates(fleet):
    """every tree of every AUV and round is grown again (one exploring_batch from the rounds' start states, seeds, lists, horizons
    and tables) and comes down through the host route; team_pick_separated on each round's candidates gives round_tree,
    round_cost, round_conflicts (and round_claimed)"""
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    from auv_sim_amd.rrt_dubins import course_habitat_words, course_ticks, team_labels, team_pick_separated
    rrt, habitats, hab = fleet["rrt"], fleet["habitats"], fleet["hab"]
    bins = rrt._bins
    labels = team_labels(TEAMS, N_AUVS)
    for pick in (None, "claims"):
        res = fleet["sep", pick, "dev"]
        inits, seeds, masks, mtts, sets, who = [], [], [], [], [], []
        for e in range(N_AUVS):
            stream = random.Random(SEEDS[e])
            at = 0
            for r in range(len(res[e]["round_len"])):
                row = res[e]["traj"][at - 1] if at else None
                init = fleet["starts"][e] if row is None else MPS(float(row[0]), float(row[1]), theta=float(row[2]), v=float(row[3]),
                                                                  traj_time_stamp=float(row[4]), plan_time_stamp=float(row[5]), length=float(row[6]))
                for k in range(K3):
                    inits.append(init)
                    seeds.append(stream.getrandbits(63))
                    masks.append(int(res[e]["round_keep"][r]))
                    mtts.append(float(res[e]["round_max_traj_time"][r]))
                    sets.append(SHARK_OF[e])
                    who.append((e, r, k))
                at += int(res[e]["round_len"][r])
        plans = rrt.exploring_batch(inits, habitats, 0.5, 5, 2, BUDGET + INTERVAL, traj_time_stamp=True, max_plan_time=BUDGET, max_traj_time=np.array(mtts),
                                    plan_time=True, weights=WEIGHT, max_iter=N_ITER, seeds=seeds, habitat_masks=masks, shark_of=sets)
        cand = {}
        for (e, r, k), plan in zip(who, plans):
            course = plan["path"][0] if plan is not None and plan["path"] else []
            if len(course) == 0:
                cand[e, r, k] = None
                continue
            xy = np.array([[p.x, p.y] for p in course])
            t = np.array([p.traj_time_stamp for p in course])
            cand[e, r, k] = dict(cost=[plan["cost"][0]] + list(plan["cost"][1]), leaf_time=float(t[-1]), ticks=course_ticks(t, xy, TICK, 100),
                                 words=course_habitat_words(xy, t, bins, 0, len(bins), hab))
        conflicting = 0
        for r in range(max(len(x["round_len"]) for x in res)):
            act = [e for e in range(N_AUVS) if r < len(res[e]["round_len"])]
            keep = [int(res[e]["round_keep"][r]) if e in act else 0 for e in range(N_AUVS)]
            want = team_pick_separated(labels, keep, act, [[cand[e, r, k] for k in range(K3)] for e in act], WEIGHT, D, pick is not None)
            for x, e in zip(want, act):
                tag = (pick, e, r, x)
                assert int(res[e]["round_tree"][r]) == x["winner"] and int(res[e]["round_conflicts"][r]) == x["conflicts"], tag
                assert pc.bits_equal(res[e]["round_cost"][r], x["cost"]), tag
                if pick is not None:
                    assert int(res[e]["round_claimed"][r]) == x["claimed"], tag
                conflicting += x["conflicts"] > 0
        assert conflicting >= 5


def test_the_separation_shows(fleet):
    """what keeps this file from being vacuous: the trees the fleet commits and the conflicts it reports are the CPU checker's
    prediction, the option changes committed trees, and a committed winner still has conflicts -- teammates that start on one
    point cannot be 5 m apart at the first ticks, so the least conflicting tree is taken"""
    for pick in (None, "claims"):
        for route in ("host", "dev"):
            got = fleet["sep", pick, route]
            assert [[int(t) for t in r["round_tree"]] for r in got] == TREE[pick], (pick, route)
            assert [int(r["round_conflicts"][0]) for r in got] == FIRST_ROUND_CONFLICTS, (pick, route)
            assert all(not r["round_conflicts"][1:].any() for r in got), (pick, route)
            assert [[int(t) for t in r["round_tree"]] for r in fleet["without", pick, route]] == TREE_WITHOUT[pick], (pick, route)
        differ = [(e, r) for e in range(N_AUVS) for r in range(5) if TREE[pick][e][r] != TREE_WITHOUT[pick][e][r]]
        assert len(differ) >= 3 and (2, 0) in differ and (5, 0) in differ and all(TEAMS[e] in (0, 1) for e, _ in differ)
    assert sum(c > 0 for c in FIRST_ROUND_CONFLICTS) >= 1


def test_generators_with_one_tree_on_the_host_route(fleet):
    """rngs with K = 1 (commit="host" only): a member's one tree is its one candidate, so the fleet commits what it commits
    without the option and the generators end in the same states; only the conflict count is recorded"""
    rrt = fleet["rrt"]
    args = (fleet["starts"], fleet["habitats"], BUDGET, LENGTH, INTERVAL, WEIGHT)

    def run(**kw):
        gens = [random.Random(1000 + e) for e in range(N_AUVS)]
        res = rrt.replanning_batch(*args, max_iter=N_ITER, rngs=gens, as_arrays=True, shark_of=SHARK_OF, teams=TEAMS, **kw)
        return res, [g.getstate() for g in gens]

    none, state_none = run()
    sep, state_sep = run(team_separation=D, separation_tick=TICK)
    assert state_sep == state_none and all(r is not None for r in none)
    counted = 0
    for e, (s, n) in enumerate(zip(sep, none)):
        s = dict(s)
        conflicts = s.pop("round_conflicts")
        _same_arrays([s], [n], "AUV %d" % e)
        if e in FIRST + LONERS:
            assert not conflicts[:1].any() if e in FIRST else not conflicts.any(), e
        counted += int(conflicts[0]) > 0
    assert counted >= 3  # (teammates that start within a metre of each other: the first tick at least)


# ---- 3. the C-ABI ---------------------------------------------------------------------------------------------------------------

def test_cabi_team_pick_apart():
    """six AUVs that start on one point, four of them active, two trees each, on real trees: the state and argument errors, a
    refused call changes nothing, the records equal team_pick_separated on the courses as the host route downloads them, the
    commit behind it carries the conflicts, and a round chosen by rrt_group_best afterwards carries 0"""
    from auv_sim_amd import _lib, synth
    from auv_sim_amd.rrt_dubins import course_habitat_words, course_ticks, team_pick_separated
    w = synth.make_world(seed=12, n_obstacles=64, n_habitats=9)
    ctx = _lib.Context(0)
    ctx.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"])
    N, G, K, n_iter, span = 6, 4, 2, 800, 100.0
    d, tick, W = 6.0, 1.0, 100
    init = np.zeros((G * K, 6))
    init[:, 0], init[:, 1] = w["start"]
    init[2 * K:3 * K, 0] = 1.0e4  # group 2: outside the boundary, no winner
    seeds = np.arange(G * K, dtype=np.uint64) + 21
    start7 = np.zeros((N, 7))
    start7[:, 0], start7[:, 1] = w["start"]
    keep0 = [0x1ff & ~(1 << a) for a in range(N)]
    labels = np.array([4, 4, 4, 9, 9, -1], dtype=np.int32)
    auv_of = [2, 4, 0, 1]
    ip = C.POINTER(C.c_int32)

    def pick(auvs, k=K, claims=1, d=d, tick=tick, W=W):
        a = np.ascontiguousarray(auvs, dtype=np.int32)
        return ctx.L.auvp_replan_team_pick_apart(ctx.h, len(a), a.ctypes.data_as(ip), k, claims, d, tick, W, None)

    def batch():
        return ctx.rrt_explore_batch(init, seeds, n_iter, max_traj_time=np.full(G * K, 100.0),
                                     habitat_keep=np.repeat(np.array([keep0[a] for a in auv_of], dtype=np.uint64), K), weights=[-3, -3, -4])

    assert pick(auv_of) == -4                              # no fleet
    ctx.replan_begin(start7, keep0)
    assert pick(auv_of) == -4                              # no teams
    ctx.replan_set_teams(labels)
    assert pick(auv_of) == -4                              # no batch has run
    summ = batch()
    best0 = ctx.rrt_group_best(np.arange(G + 1) * K)
    paths0 = ctx.group_paths(best0)
    info0 = ctx.replan_info()
    assert pick(auv_of, k=3) == -1 and pick(auv_of[:3]) == -1    # not the batch's size
    assert pick([2, 4, 0, 6]) == -1 and pick([2, 4, -1, 1]) == -1 and pick([2, 4, 2, 1]) == -1
    assert ctx.L.auvp_replan_team_pick_apart(ctx.h, G, None, K, 1, d, tick, W, None) == -1
    assert pick(auv_of, d=0.0) == -1 and pick(auv_of, d=float("nan")) == -1 and pick(auv_of, tick=float("inf")) == -1
    assert pick(auv_of, tick=-1.0) == -1 and pick(auv_of, W=0) == -1 and pick(auv_of, W=1025) == -1
    # the refused calls changed nothing: the group records are there, the fleet is as it was
    assert ctx.group_best_dev() is not None and ctx.replan_info() == info0
    again = ctx.group_paths(best0)
    assert all(np.array_equal(a, b) for a, b in zip(again, paths0))
    # the pick on the batch's trees against the rule on the downloaded courses
    paths = ctx.paths(summ)
    cands = []
    for g, a in enumerate(auv_of):
        row = []
        for k in range(K):
            s, p = summ[g * K + k], paths[g * K + k].copy()
            if s["best_leaf"] < 0:
                row.append(None)
                continue
            p[0] = start7[a]
            row.append(dict(words=course_habitat_words(p[:, :2], p[:, 4], w["bins"], 0, len(w["bins"]), w["habitats"]),
                            cost=[float(x) for x in s["best_cost"]], leaf_time=float(p[-1, 4]), ticks=course_ticks(p[:, 4], p[:, :2], tick, W)))
        cands.append(row)
    for claims in (False, True):
        want = team_pick_separated(labels, keep0, auv_of, cands, [-3, -3, -4], d, claims)
        rec = ctx.replan_team_pick_apart(auv_of, K, claims, d, tick, W)
        assert [int(x) for x in rec["winner"]] == [g * K + x["winner"] if x["winner"] >= 0 else -1 for g, x in enumerate(want)]
        assert int(rec["winner"][2]) == -1 and int(rec["status"][2]) == 1 and sum(int(x) >= 0 for x in rec["winner"]) == 3
        for g, x in enumerate(want):
            assert pc.bits_equal(rec[g]["cost"], x["cost"]) and int(rec[g]["n_with_leaf"]) == x["n_with_leaf"], (g, rec[g], x)
            if x["winner"] >= 0:
                s = summ[g * K + x["winner"]]
                assert int(rec[g]["path_len"]) == int(s["best_path_len"]) and rec[g]["length"] == s["best_length"], g
        assert any(x["conflicts"] for x in want) and (not claims or any(x["claimed"] for x in want))
    # the commit behind it carries the counts and the masks the members saw; nothing but the records came back
    out = ctx.replan_commit(auv_of, span)
    assert [int(x) for x in out["conflicts"]] == [x["conflicts"] for x in want] and not out["_reserved"].any()
    assert [int(x) for x in out["claimed"]] == [x["claimed"] for x in want]
    assert [int(x) for x in out["winner"]] == [int(x) for x in rec["winner"]] and all(pc.bits_equal(a, b) for a, b in zip(out["cost"], rec["cost"]))
    info = ctx.replan_info()
    assert info["rounds"] == 1 and info["bytes_to_host"] == G * RECORD
    # a round chosen by rrt_group_best afterwards, and one chosen by the claims alone: no conflicts in their records
    batch()
    ctx.rrt_group_best(np.arange(G + 1) * K)
    out = ctx.replan_commit(auv_of, span)
    assert not out["conflicts"].any() and not out["claimed"].any()
    batch()
    ctx.replan_team_pick(auv_of, K)
    out = ctx.replan_commit(auv_of, span)
    assert not out["conflicts"].any() and not out["_reserved"].any()
    ctx.replan_set_teams(None)
    assert pick(auv_of) == -4                              # the teams are gone

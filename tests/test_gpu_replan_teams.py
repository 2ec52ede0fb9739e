"""Teams that share one habitat list in RRT.replanning_batch(teams=...): replan_team_kernel through its probe entry against
rrt_dubins.team_fold, a fleet of ten AUVs in three teams (the device route against the host route, every round against the
rule, the final lists against the CPU checker's prediction), and the C-ABI of auvp_replan_set_teams."""
import ctypes as C
import os

import numpy as np
import pytest

import replan_cases as rc
import replan_team_cases as tc
from conftest import GOLDEN
from test_gpu_replan_commit import _rows, _same_arrays, _world

pytestmark = pytest.mark.gpu

ALL = tc.ALL
RECORD = 128  # bytes of one auvp_replan_record
N_AUVS, N_ITER, ROUNDS = 10, 400, 5
BUDGET, LENGTH, INTERVAL = 2.0, 150.0, 98.0
TEAMS = [0, 0, 0, 0, 1, 1, 1, -1, -1, 2]
# the CPU checker's prediction (oracle/orc.py + first_bucket_commit) of every AUV's list at the end of the horizon
KEEP_ALONE = [0x232, 0x368, 0x368, 0x237, 0x369, 0x1cb, 0x337, 0x317, 0xb7, 0x197]
KEEP_TEAMS = [0x0] * 4 + [0x101] * 3 + KEEP_ALONE[7:]
TEAM0_ROUND_KEEP = [0x3ff, 0x360, 0x220, 0x220, 0x220]


# ---- the probe entry ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    return _lib.Context(0)  # (no world: the probe needs none)


def _fold_equals(ctx, c):
    got = ctx.replan_team_fold(c["labels"], c["keep"])
    want = tc.expected(c)[2]
    assert got.dtype == np.uint64 and [int(k) for k in got] == want, c["name"]
    return want


def test_probe_crafted_cases_equal_team_fold(ctx):
    for c in tc.crafted():
        _fold_equals(ctx, c)


def test_probe_team_sizes_around_the_wavefront_in_one_call(ctx):
    """teams of 1, 2, 63, 64, 65, 129 and 1000 members interleaved across the array with loners between them; every mask lacks
    a few bits of its own, so every member counts"""
    sizes = [1, 2, 63, 64, 65, 129, 1000]
    rng = np.random.default_rng(11)
    labels = np.concatenate([np.full(s, 1000 * k + 3, dtype=np.int32) for k, s in enumerate(sizes)] + [np.full(300, -1, dtype=np.int32)])
    labels = labels[rng.permutation(len(labels))]
    keep = []
    for _ in labels:
        w = ALL
        for b in rng.integers(0, 64, size=3):
            w &= ~(1 << int(b))
        keep.append(w)
    c = tc.case(labels, keep, "sizes")
    off, mem, _ = tc.expected(c)
    assert np.diff(off).tolist() == sizes[1:] and np.any(np.diff(mem[off[-2]:off[-1]]) > 1)  # (interleaved)
    want = _fold_equals(ctx, c)
    alone = np.flatnonzero((labels < 0) | (labels == 3))
    assert len(alone) == 301 and all(want[i] == keep[i] for i in alone)  # loners and the team of one keep their masks
    for k in range(1, len(sizes)):
        ms = np.flatnonzero(labels == 1000 * k + 3)
        assert len({want[i] for i in ms}) == 1 and want[ms[0]] != keep[ms[0]]


@pytest.mark.parametrize("at", [0, 63, 64, 4095])
def test_probe_one_team_of_4096_one_member_lacks_one_bit(ctx, at):
    keep = [ALL] * 4096
    keep[at] = ALL & ~(1 << (at % 64))
    got = ctx.replan_team_fold(np.full(4096, 5, dtype=np.int32), keep)
    assert np.all(got == np.uint64(keep[at])), at
    assert tc.expected(tc.case([5] * 4096, keep))[2] == [keep[at]] * 4096


def test_probe_random_cases_equal_team_fold(ctx):
    for c in tc.random_cases(200, seed=99):
        _fold_equals(ctx, c)


def test_probe_refuses_bad_arguments(ctx):
    lab, kp = np.zeros(2, dtype=np.int32), np.array([1, 3], dtype=np.uint64)
    ip, up = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    fold = ctx.L.auvp_replan_team_fold
    assert fold(ctx.h, 0, lab.ctypes.data_as(ip), kp.ctypes.data_as(up)) == -1
    assert fold(ctx.h, -3, lab.ctypes.data_as(ip), kp.ctypes.data_as(up)) == -1
    assert fold(ctx.h, 2, None, kp.ctypes.data_as(up)) == -1
    assert fold(ctx.h, 2, lab.ctypes.data_as(ip), None) == -1
    assert kp.tolist() == [1, 3]
    assert fold(ctx.h, 2, lab.ctypes.data_as(ip), kp.ctypes.data_as(up)) == 0 and kp.tolist() == [1, 1]
    with pytest.raises(ValueError):
        ctx.replan_team_fold([0, 0, 0], [1, 2])


# ---- the fleet ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fleet():
    """ten AUVs, each starting at the centre of its own habitat: without teams, and with TEAMS on both routes"""
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    from auv_sim_amd.rrt_dubins import RRT
    g = np.load(os.path.join(GOLDEN, "g13_replan_a.npz"))
    obstacles, habitats, cell_list, grids, poly = _world(g)
    assert len(habitats) == N_AUVS
    rrt = RRT(poly, obstacles, grids[0], cell_list)
    rrt3 = RRT(poly, obstacles, grids[0], cell_list)
    rrt3.set_shark_grids(grids)
    starts = [MPS(h.x, h.y) for h in habitats]
    seeds = [31 * e + 3 for e in range(N_AUVS)]
    args = (starts, habitats, BUDGET, LENGTH, INTERVAL, [-3, -3, -4])
    kw = dict(max_iter=N_ITER, seeds=seeds)
    k3 = dict(kw, as_arrays=True, trees_per_auv=3, shark_of=[e % 2 for e in range(N_AUVS)], teams=TEAMS)
    out = dict(starts=starts, habitats=habitats, hab=g["habitats"])
    out["alone"] = rrt.replanning_batch(*args, as_arrays=True, **kw)
    out["alone_dev"] = rrt.replanning_batch(*args, as_arrays=True, commit="device", **kw)
    out["host_arr"] = rrt.replanning_batch(*args, as_arrays=True, teams=TEAMS, **kw)
    out["dev_arr"] = rrt.replanning_batch(*args, as_arrays=True, teams=TEAMS, commit="device", **kw)
    out["info"] = rrt._ctx.replan_info()
    out["host_obj"] = rrt.replanning_batch(*args, teams=TEAMS, **kw)
    out["dev_obj"] = rrt.replanning_batch(*args, teams=TEAMS, commit="device", **kw)
    out["host_k3"] = rrt3.replanning_batch(*args, **k3)
    out["dev_k3"] = rrt3.replanning_batch(*args, commit="device", **k3)
    return out


def test_routes_agree_as_arrays(fleet):
    assert all(r is not None and len(r["round_len"]) == ROUNDS for r in fleet["host_arr"])
    _same_arrays(fleet["dev_arr"], fleet["host_arr"], "teams")
    _same_arrays(fleet["alone_dev"], fleet["alone"], "no teams")


def test_routes_agree_as_objects(fleet):
    host, dev, habitats = fleet["host_obj"], fleet["dev_obj"], fleet["habitats"]
    for e in range(N_AUVS):
        h, d = host[e], dev[e]
        assert h is not None and d is not None, e
        assert np.array_equal(_rows(d[0]), _rows(h[0])) and d[0][0] is fleet["starts"][e], e
        assert list(d[1].keys()) == list(h[1].keys()) == list(range(1, ROUNDS + 1)), e
        for k in h[1]:
            assert np.array_equal(_rows(d[1][k][0]), _rows(h[1][k][0])), (e, k)
            assert len(d[1][k][1]) == len(h[1][k][1]) and all(a is b for a, b in zip(d[1][k][1], h[1][k][1])), (e, k)
            # the rounds dict's habitat list is the team's list at the start of the round
            bits = int(fleet["host_arr"][e]["round_keep"][k - 1])
            want = [habitats[i] for i in range(N_AUVS) if (bits >> i) & 1]
            assert len(h[1][k][1]) == len(want) and all(a is b for a, b in zip(h[1][k][1], want)), (e, k)
        assert d[2] == h[2], e
        assert len(d[3]) == len(h[3]) and all(a is b for a, b in zip(d[3], h[3])), e
        want = [habitats[i] for i in range(N_AUVS) if (KEEP_TEAMS[e] >> i) & 1]
        assert len(h[3]) == len(want) and all(a is b for a, b in zip(h[3], want)), e
        # the arrays say the same as the objects
        assert np.array_equal(_rows(h[0]), fleet["host_arr"][e]["traj"]) and h[2][0] == float(fleet["host_arr"][e]["cost"][0]), e


def test_routes_agree_with_k_trees_and_shark_tables(fleet):
    host = fleet["host_k3"]
    assert sum(r is not None for r in host) >= 8
    assert len({int(t) for r in host if r is not None for t in r["round_tree"]}) > 1  # (not always member 0)
    _same_arrays(fleet["dev_k3"], host, "teams, three trees, two tables")
    # the rule holds here too: teammates end with one list
    for t in (0, 1):
        assert len({int(r["keep"]) for r, lab in zip(host, TEAMS) if lab == t and r is not None}) == 1


def test_teams_cost_nothing_when_unused(fleet):
    """two loners and a team of one: exactly the run without teams"""
    for route in ("host_arr", "dev_arr"):
        _same_arrays(fleet[route][7:], fleet["alone"][7:], route)


def test_round_one_is_unchanged(fleet):
    for e, (t, a) in enumerate(zip(fleet["host_arr"], fleet["alone"])):
        n = int(a["round_len"][0])
        assert int(t["round_len"][0]) == n > 0 and np.array_equal(t["traj"][:n], a["traj"][:n]), e
        assert int(t["round_keep"][0]) == int(a["round_keep"][0]) == 0x3ff, e
        assert np.array_equal(t["round_cost"][0], a["round_cost"][0]) and t["round_max_traj_time"][0] == a["round_max_traj_time"][0], e


def test_every_round_follows_the_rule(fleet):
    """round_keep[r] of a member is the AND of the members' own folds of round r - 1, each recomputed here from the member's
    committed rows with first_bucket_commit"""
    from auv_sim_amd.rrt_dubins import first_bucket_commit
    res, hab, span = fleet["host_arr"], fleet["hab"], BUDGET + INTERVAL
    for team in (0, 1):
        ms = [e for e in range(N_AUVS) if TEAMS[e] == team]
        cur = 0x3ff
        for r in range(ROUNDS):
            nxt = ALL
            for e in ms:
                assert int(res[e]["round_keep"][r]) == cur, (team, e, r, hex(int(res[e]["round_keep"][r])), hex(cur))
                a = int(res[e]["round_len"][:r].sum())
                rows = res[e]["traj"][a:a + int(res[e]["round_len"][r])]
                assert len(rows) > 0
                sel, own = first_bucket_commit(rows[:, 4], rows[:, :2], float(rows[0, 4]), float(res[e]["round_max_traj_time"][r]), span,
                                               cur, hab)
                assert sel.all()
                nxt &= own
            cur = nxt
        assert all(int(res[e]["keep"]) == cur for e in ms), (team, hex(cur))


def test_the_sharing_shows(fleet):
    """what keeps this file from being vacuous: a member's second round starts without a habitat only a TEAMMATE has visited"""
    shown = []
    for e in range(N_AUVS):
        mates = [m for m in range(N_AUVS) if m != e and TEAMS[m] >= 0 and TEAMS[m] == TEAMS[e]]
        with_t, alone = int(fleet["host_arr"][e]["round_keep"][1]), int(fleet["alone"][e]["round_keep"][1])
        if with_t != alone and any(not (with_t >> m) & 1 for m in mates):
            shown.append(e)
    print("members whose round 2 starts without a teammate's start habitat:", shown)
    assert shown
    # and the plans diverge from there, not only the lists
    assert any(not np.array_equal(fleet["host_arr"][e]["traj"], fleet["alone"][e]["traj"]) for e in range(7))


def test_final_lists_are_the_checkers(fleet):
    got_alone = [int(r["keep"]) for r in fleet["alone"]]
    got_teams = [int(r["keep"]) for r in fleet["host_arr"]]
    print("without teams:", [hex(k) for k in got_alone])
    print("with teams   :", [hex(k) for k in got_teams])
    print("team 0, round_keep:", [hex(int(k)) for k in fleet["host_arr"][0]["round_keep"]])
    assert got_alone == KEEP_ALONE
    assert got_teams == KEEP_TEAMS
    assert [int(r["keep"]) for r in fleet["dev_arr"]] == KEEP_TEAMS
    for e in range(4):
        assert [int(k) for k in fleet["host_arr"][e]["round_keep"]] == TEAM0_ROUND_KEEP, e


def test_the_team_step_adds_nothing_to_what_crosses_the_bus(fleet):
    info = fleet["info"]
    assert info["n_auvs"] == N_AUVS and info["rounds"] == ROUNDS
    assert 0 < info["bytes_to_host"] - info["bytes_traj"] <= info["rounds"] * N_AUVS * RECORD
    assert info["bytes_traj"] == info["rows"] * 56 and info["commit_ms"] > 0.0


def test_malformed_teams_raise_before_any_launch():
    from auv_sim_amd.rrt_dubins import RRT
    g = np.load(os.path.join(GOLDEN, "g13_replan_a.npz"))
    obstacles, habitats, cell_list, grids, poly = _world(g)
    rrt = RRT(poly, obstacles, grids[0], cell_list)
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    starts = [MPS(h.x, h.y) for h in habitats[:3]]
    for bad in ([0, 0], [0, 0, 0, 0], [0, True, 0], [0, 1.5, 0], [0, "a", 0]):
        for commit in ("host", "device"):
            with pytest.raises(ValueError):
                rrt.replanning_batch(starts, habitats, BUDGET, LENGTH, INTERVAL, [-3, -3, -4], max_iter=50, seeds=[1, 2, 3], commit=commit,
                                     teams=bad)
    assert rrt._ctx.last_rrt_kernel() == "" and rrt._ctx.replan_info()["n_auvs"] == 0


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------

def test_cabi_set_teams():
    """six AUVs with lists of their own from the start (so that a fold shows in the first round), four of them active per
    round; every round's records against first_bucket_commit + team_fold on the host"""
    from auv_sim_amd import _lib, synth
    from auv_sim_amd.rrt_dubins import team_fold
    w = synth.make_world(seed=12, n_obstacles=64, n_habitats=9)
    ctx = _lib.Context(0)
    ctx.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"])
    N, G, K, n_iter, span = 6, 4, 2, 800, 100.0
    init = np.zeros((G * K, 6))
    init[:, 0], init[:, 1] = w["start"]
    init[2 * K:3 * K, 0] = 1.0e4  # group 2: outside the boundary, no winner
    seeds = np.arange(G * K, dtype=np.uint64) + 21
    start7 = np.zeros((N, 7))
    start7[:, 0], start7[:, 1] = w["start"]
    keep0 = [0x1ff & ~(1 << a) for a in range(N)]
    labels = np.array([4, 4, 4, 9, 9, -1], dtype=np.int32)
    ip = C.POINTER(C.c_int32)

    def set_teams(lab, n=None):
        lab = np.ascontiguousarray(lab, dtype=np.int32)
        return ctx.L.auvp_replan_set_teams(ctx.h, len(lab) if n is None else n, lab.ctypes.data_as(ip))

    state = {}

    def begin():
        ctx.replan_begin(start7, keep0)
        state.update(last=start7.copy(), keep=list(keep0))

    def round_(auv_of, lab):
        """one round on the device and on the host; lab: the teams the device is expected to apply (None: none)"""
        ctx.rrt_explore_batch(init, seeds, n_iter, max_traj_time=np.full(G * K, 100.0), habitat_keep=np.full(G * K, 0x1ff, np.uint64),
                              summaries=False)
        best = ctx.rrt_group_best(np.arange(G + 1) * K)
        rec = ctx.replan_commit(auv_of, span)
        paths = ctx.group_paths(best)
        own = list(state["keep"])
        for g, a in enumerate(auv_of):
            _, _, own[a], state["last"][a] = rc.expected(rc.case(paths[g], state["last"][a], state["keep"][a], span, w["habitats"]))
        state["keep"] = own if lab is None else team_fold(own, lab)
        for g, a in enumerate(auv_of):
            assert int(rec["keep"][g]) == state["keep"][a], (g, a, hex(int(rec["keep"][g])), hex(state["keep"][a]), hex(own[a]))
            assert rc.same(rec["last"][g], state["last"][a]), (g, a)
        return own != state["keep"]  # the fold changed something

    assert set_teams(labels) == -4                       # no fleet
    begin()
    assert set_teams(labels, n=5) == -1 and set_teams(np.zeros(7), n=7) == -1   # not the fleet's size
    round_([5, 0, 3, 1], None)                           # the refused calls set nothing
    begin()
    assert set_teams(labels) == 0
    assert set_teams(np.zeros(7), n=7) == -1 and set_teams(np.zeros(5), n=5) == -1
    assert round_([2, 4, 0, 1], labels)                  # the teams are as they were; AUVs 3 and 5 are not part of this round
    round_([5, 3, 1, 4], labels)                         # ... and AUVs 0 and 2 not of this one: their lists are folded all the same
    begin()
    assert set_teams(labels) == 0 and ctx.L.auvp_replan_set_teams(ctx.h, N, None) == 0   # NULL clears them
    round_([0, 1, 2, 3], None)
    ctx.replan_set_teams(labels)
    begin()                                              # a new fleet has no teams
    round_([5, 0, 3, 1], None)
    ctx.replan_set_teams(labels)
    assert round_([1, 2, 3, 4], labels)
    round_([0, 1, 4, 5], labels)
    off, rows = ctx.replan_traj()
    info = ctx.replan_info()
    assert info["rounds"] == 3 and 0 < info["bytes_to_host"] - info["bytes_traj"] <= info["rounds"] * N * RECORD
    # the probe on a handle with a fleet: the fleet is as it was
    assert [int(k) for k in ctx.replan_team_fold([1, 1, 1], [6, 3, 7])] == [2, 2, 2]
    off2, rows2 = ctx.replan_traj()
    info2 = ctx.replan_info()
    assert np.array_equal(off, off2) and np.array_equal(rows, rows2)
    assert info2 == dict(info, bytes_to_host=info["bytes_to_host"] + rows.nbytes, bytes_traj=info["bytes_traj"] + rows.nbytes)
    round_([3, 2, 1, 0], labels)                         # (and the teams are still the fleet's)
    ctx.replan_set_teams(None)

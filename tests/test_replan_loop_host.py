"""The fleet loop (replanning.ReplanSession.round) and the result builder (replanning.replan_results) without a GPU: a scripted
round back end hands the loop hand-written records and rows, and every expectation below is a literal -- since both commit
routes share this loop and this builder, "host route equals device route" no longer checks them against an independent copy.

The fleet: N = 4 AUVs, H = 5 habitats, teams [0, 0, 1, -1], K = 2 trees, rounds of 50 s, a horizon that ends at 200 s, a
traj_time_length of 150 s.  AUV 0 plans three rounds (from 0, 50 and 100 s); AUV 1 commits in round 1 and has no winner in round
2; AUV 2 starts at 120 s -- its only round is clipped to the horizon's end --; AUV 3 starts at 150 s and never plans."""
import random

import numpy as np
import pytest

from auv_sim_amd import _lib
from auv_sim_amd.motion_plan_state import Motion_plan_state
from auv_sim_amd.replanning import ReplanSession

INF = float("inf")
# the rows each AUV commits, round by round: x, y, theta, v, traj_time_stamp, plan_time_stamp, length; a round's first row is the
# state the AUV had
ROWS0 = [[[1.0, 2.0, 0.5, 0.0, 0.0, 0.0, 0.0], [3.0, 2.0, 0.6, 2.0, 20.0, 1.0, 2.5], [5.0, 3.0, 0.7, 2.0, 50.0, 2.0, 5.0]],
         [[5.0, 3.0, 0.7, 2.0, 50.0, 2.0, 5.0], [8.0, 3.0, 0.1, 2.0, 100.0, 3.0, 9.0]],
         [[8.0, 3.0, 0.1, 2.0, 100.0, 3.0, 9.0], [9.0, 9.0, 0.2, 2.0, 150.0, 4.0, 15.0]]]
ROWS2 = [[[20.0, 20.0, 0.0, 0.0, 120.0, 0.0, 0.0], [22.0, 21.0, 0.3, 2.0, 165.0, 1.0, 3.0]]]
LAST1 = [0.0, 1.0, 0.0, 2.0, 50.0, 1.0, 4.0]  # AUV 1 after round 1
# per round: (the AUVs the loop must name, their horizons, then per AUV: winner (episode of the round's batch), n_committed, last,
# keep (as the back end leaves it: folded), cost, claimed, conflicts)
SCRIPT = [
    ([0, 1, 2], [150.0, 150.0, 200.0],
     [(1, 3, ROWS0[0][-1], 0b11101, [-1.0, -0.25, -0.5, -0.25], 0, 0), (2, 2, LAST1, 0b11101, [-2.0, -1.0, -0.5, -0.5], 0b00010, 3),
      (5, 2, ROWS2[0][-1], 0b10101, [-3.0, -1.0, -1.0, -1.0], 0, 0)]),
    ([0, 1], [200.0, 200.0],
     [(0, 2, ROWS0[1][-1], 0b01101, [-4.0, -2.0, -1.0, -1.0], 0b10000, 1), (-1, 0, LAST1, 0b11010, [INF] * 4, 0, 0)]),
    ([0], [200.0], [(1, 2, ROWS0[2][-1], 0b01101, [-5.0, -2.0, -2.0, -1.0], 0, 0)]),
]
SEEDS = [11, 12, 13, 14]


class _Scripted:
    """a round back end that plays SCRIPT and checks what the loop hands it"""

    def __init__(self, session):
        self.session, self.calls = session, 0
        self.streams = [random.Random(s) for s in SEEDS]

    def round(self, act, mtt, seeds):
        want_act, want_mtt, per_auv = SCRIPT[self.calls]
        self.calls += 1
        assert act.tolist() == want_act and mtt.tolist() == want_mtt
        # K = 2 seeds per active AUV from its own stream, in member order; an AUV that sat a round out drew nothing
        assert seeds.dtype == np.uint64 and seeds.tolist() == [self.streams[e].getrandbits(63) for e in want_act for _ in range(2)]
        rec = np.zeros(len(act), dtype=_lib.REPLAN_RECORD_DTYPE)
        for g, (winner, n, last, keep, cost, claimed, conflicts) in enumerate(per_auv):
            rec[g] = (0 if winner >= 0 else 1, winner, n, 9, cost, last, keep, claimed, conflicts, 0)
        return rec

    def rows(self, done):
        assert done == [0, 2, 3]
        blocks = {0: np.array(sum(ROWS0, [])), 2: np.array(sum(ROWS2, [])), 3: np.zeros((0, 7))}
        return {e: blocks[e] for e in done}


class _Ctx:
    """the planner's context: nothing of it may be reached"""
    device, session = 0, None


class _CostCtx:
    """the cost-only context: a trajectory's "cost" is (its rows, its end time, 0.5, -1)"""

    def set_world(self, *a):
        pass

    def cost_paths(self, paths_xyt, bin_lo, bin_hi, total, weights):
        return np.array([[float(len(p)), float(t), 0.5, -1.0] for p, t in zip(paths_xyt, total)]).reshape(-1, 4)


class _Habitat:
    def __init__(self, x):
        self.x, self.y, self.size = x, 0.0, 1.0


def _fleet(traj_time_length=150.0, team_pick=None, sep=None):
    from auv_sim_amd.rrt_dubins import RRT
    rrt = RRT.__new__(RRT)
    rrt._session, rrt._batch, rrt._ctx, rrt._cost_ctx = None, "a batch", _Ctx(), _CostCtx()
    rrt._bins, rrt._cells, rrt._prob, rrt._set_prob = np.zeros((4, 2)), np.zeros((1, 4)), np.zeros((4, 1)), None
    starts = [Motion_plan_state(1.0, 2.0, theta=0.5), Motion_plan_state(0.0, 0.0), Motion_plan_state(20.0, 20.0, traj_time_stamp=120.0),
              Motion_plan_state(30.0, 30.0, traj_time_stamp=150.0)]
    habitats = [_Habitat(float(h)) for h in range(5)]
    session = ReplanSession(rrt, starts, traj_time_length, [-3, -3, -4], all_habitats=habitats, hab=np.zeros((5, 3)), horizon_end=200,
                            round_span=50.0, max_iter=10, seeds=SEEDS, K=2, sets=None, labels=np.array([0, 0, 1, -1], dtype=np.int32),
                            team_pick=team_pick, sep=sep, back_end=_Scripted)
    assert rrt._session is session and rrt._ctx.session is session and rrt._batch is None
    return rrt, starts, habitats, session


@pytest.mark.parametrize("team_pick, sep", [(None, None), ("claims", None), (None, (5.0, 1.0, 50)), ("claims", (5.0, 1.0, 50))])
def test_loop_and_builder_as_arrays(team_pick, sep):
    rrt, starts, habitats, s = _fleet(team_pick=team_pick, sep=sep)
    assert s.active().tolist() == [0, 1, 2]
    out = s.round()
    assert out["auv"].tolist() == [0, 1, 2] and out["winner"].tolist() == [1, 0, 1] and out["keep"].tolist() == [29, 29, 21]
    assert out["last"].tolist() == [ROWS0[0][-1], LAST1, ROWS2[0][-1]] and out["cost"][1].tolist() == [-2.0, -1.0, -0.5, -0.5]
    assert s.round_index == 1 and s.last[:, 4].tolist() == [50.0, 50.0, 165.0, 150.0] and s.keep.tolist() == [29, 29, 21, 31]
    out = s.round()
    assert out["auv"].tolist() == [0, 1] and out["winner"].tolist() == [0, -1]
    assert s.active().tolist() == [0]  # (AUV 1 had no winner: it stops planning)
    assert s.round()["winner"].tolist() == [1]
    assert s.round() is None and s.round_index == 3
    res = s.finish(as_arrays=True)
    assert s.closed and rrt._session is None and rrt._ctx.session is None
    assert len(res) == 4 and res[1] is None
    keys = {"traj", "round_len", "round_keep", "round_max_traj_time", "round_cost", "round_tree", "keep", "cost"}
    keys |= ({"round_claimed"} if team_pick else set()) | ({"round_conflicts"} if sep else set())
    assert all(set(res[e]) == keys for e in (0, 2, 3))
    a = res[0]
    assert a["traj"].tolist() == sum(ROWS0, [])
    assert a["round_len"].tolist() == [3, 2, 2] and a["round_len"].dtype == np.int64
    assert a["round_keep"].tolist() == [31, 29, 13] and a["round_keep"].dtype == np.uint64  # the lists at each round's START
    assert a["round_max_traj_time"].tolist() == [150.0, 200.0, 200.0]  # 150 + 0; 150 + 50; clipped: 100 + 100
    assert a["round_tree"].tolist() == [1, 0, 1] and a["round_tree"].dtype == np.int64
    assert a["round_cost"].tolist() == [[-1.0, -0.25, -0.5, -0.25], [-4.0, -2.0, -1.0, -1.0], [-5.0, -2.0, -2.0, -1.0]]
    assert a["keep"] == 0b01000  # 01101 of AUV 0 & 11010 of AUV 1, which stopped in round 2
    assert a["cost"].tolist() == [7.0, 150.0, 0.5, -1.0]
    if team_pick:
        assert a["round_claimed"].tolist() == [0, 0b10000, 0] and a["round_claimed"].dtype == np.uint64
    if sep:
        assert a["round_conflicts"].tolist() == [0, 1, 0] and a["round_conflicts"].dtype == np.int64
    b = res[2]  # one round, clipped from 120 + 150 to the horizon's end; a team of one keeps its own list
    assert b["traj"].tolist() == sum(ROWS2, []) and b["round_len"].tolist() == [2] and b["round_keep"].tolist() == [31]
    assert b["round_max_traj_time"].tolist() == [200.0] and b["round_tree"].tolist() == [1] and b["keep"] == 0b10101
    assert b["round_cost"].tolist() == [[-3.0, -1.0, -1.0, -1.0]] and b["cost"].tolist() == [2.0, 165.0, 0.5, -1.0]
    c = res[3]  # never planned: no rows, no rounds, the whole list, the cost at its start time
    assert c["traj"].shape == (0, 7) and c["round_len"].tolist() == [] and c["round_keep"].tolist() == []
    assert c["round_max_traj_time"].tolist() == [] and c["round_tree"].tolist() == [] and c["round_cost"].shape == (0, 4)
    assert c["keep"] == 0b11111 and c["cost"].tolist() == [0.0, 150.0, 0.5, -1.0]


def test_loop_and_builder_objects():
    rrt, starts, habitats, s = _fleet()
    res = s.run()
    assert s.closed and rrt._session is None and len(res) == 4 and res[1] is None
    traj, rounds, cost, left = res[0]
    assert len(traj) == 7 and traj[0] is starts[0]  # round 1's first object is the caller's start object itself
    assert traj[3] is traj[2] and traj[5] is traj[4]  # every later round's first object is the previous round's last one
    assert [(m.x, m.y, m.theta, m.v, m.traj_time_stamp, m.plan_time_stamp, m.length) for m in traj[1:]] == [
        tuple(r) for r in sum(ROWS0, [])[1:]]
    assert sorted(rounds) == [1, 2, 3]
    for k, (lo, hi, listed) in {1: (0, 3, [0, 1, 2, 3, 4]), 2: (3, 5, [0, 2, 3, 4]), 3: (5, 7, [0, 2, 3])}.items():
        bucket, listed_objs = rounds[k]  # (the caller's own habitat objects, in the caller's order)
        assert len(bucket) == hi - lo and all(x is y for x, y in zip(bucket, traj[lo:hi]))
        assert len(listed_objs) == len(listed) and all(x is habitats[h] for x, h in zip(listed_objs, listed))
    assert cost == [7.0, [150.0, 0.5, -1.0]]
    assert len(left) == 1 and left[0] is habitats[3]
    traj, rounds, cost, left = res[2]
    assert len(traj) == 2 and traj[0] is starts[2] and traj[1].traj_time_stamp == 165.0 and sorted(rounds) == [1]
    assert all(x is y for x, y in zip(rounds[1][0], traj)) and all(x is y for x, y in zip(rounds[1][1], habitats))
    assert cost == [2.0, [165.0, 0.5, -1.0]] and [habitats.index(x) for x in left] == [0, 2, 4]
    traj, rounds, cost, left = res[3]
    assert traj == [] and rounds == {} and cost == [0.0, [150.0, 0.5, -1.0]]
    assert len(left) == 5 and all(x is y for x, y in zip(left, habitats))


def test_a_horizon_without_a_whole_bucket_raises_before_the_round():
    """30 s of trajectory from 0 s hold no bucket of 50 s: ValueError, and the back end's round is never called"""
    rrt, starts, habitats, s = _fleet(traj_time_length=30.0)
    with pytest.raises(ValueError, match="max_traj_time 30.0 holds no shark-interval bucket of 50.0"):
        s.round()
    assert s._back.calls == 0 and s.round_index == 0 and not s.inside and not s.closed
    with pytest.raises(ValueError):
        s.run()
    assert s._back.calls == 0 and s.closed and rrt._session is None

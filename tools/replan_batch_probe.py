"""RRT.replanning_batch throughput (profiles/replan_batch_probe.md).

    python tools/replan_batch_probe.py [--sizes 256,1024,4096] [--iters 2000] [--seq 4] [--commit host|device] [--runs 1]
                                        [--teams T] [--trees K] [--team-pick claims] [--separation D]

For N AUVs on a G13-style world (synth.make_world(seed=1, n_obstacles=64), the world of tests/golden/g13_replan_a; plan budget
2, horizon 150 s, replan interval 98 s) and `iters` iterations per round: every round's launch (AUVs still planning, expansions
per second of the expansion + leaf pass) and the wall time of the whole batch.  Then a few AUVs through the sequential
RRT.replanning (wall time per AUV, for the ratio), and at each N the same parameters as one uniform batch through the
per-episode-limits kernel and through plain rrt_explore_kernel (options ROWS = DUO = TRIO = 0): the cost of reading the
limits per episode.  One JSON line per measurement.

--commit device: the step between two rounds on the device (rrt_commit_kernel; profiles/replan_device_commit.md); the line
then also carries the commit kernel's own time and, from replan_info, the bytes per round that came back to the host and the
one trajectory download.  --runs R: the batch R times after the warm-up, one line each (the uniform-batch and sequential parts
only with --commit host).  --teams T: AUVs e with the same e // T share one habitat list (replanning_batch's teams;
profiles/replan_teams.md); with --commit device the commit kernel's time then covers replan_team_kernel too.  --trees K:
trees_per_auv.  --team-pick claims: the team-aware winner selection (profiles/replan_team_pick.md); with --commit device
commit_kernel_ms then also covers rrt_course_words_kernel and replan_team_pick_kernel.  --separation D: team_separation=D with
the default tick and window (profiles/replan_team_separation.md); commit_kernel_ms then covers rrt_course_ticks_kernel and
replan_team_pick_apart_kernel."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from auv_sim_amd import _lib, synth  # noqa: E402
from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS  # noqa: E402
from auv_sim_amd.rrt_dubins import RRT  # noqa: E402


class _Cell:
    def __init__(self, b):
        self.bounds = tuple(float(v) for v in b)


class _Poly:
    class _Ext:
        def __init__(self, pts):
            self.coords = list(pts) + [pts[0]]

    def __init__(self, pts):
        self.exterior = _Poly._Ext([tuple(p) for p in pts])


def world_objects(w):
    obstacles = [MPS(o[0], o[1], size=o[2]) for o in w["obstacles"].tolist()]
    habitats = [MPS(h[0], h[1], size=h[2]) for h in w["habitats"].tolist()]
    cells = [_Cell(c) for c in w["cells"].tolist()]
    shark = {(int(b[0]), int(b[1])): {cells[i].bounds: p for i, p in enumerate(w["prob"][t].tolist())}
             for t, b in enumerate(w["bins"].tolist())}
    return obstacles, habitats, cells, shark, _Poly(w["polygon"].tolist())


def starts_near(w, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        x, y = w["start"][0] + rng.uniform(-25, 25), w["start"][1] + rng.uniform(-25, 25)
        if all(math.hypot(x - o[0], y - o[1]) > o[2] + 3.0 for o in w["obstacles"]):
            out.append(MPS(float(x), float(y)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024,4096")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--seq", type=int, default=4)
    ap.add_argument("--commit", choices=("host", "device"), default="host")
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--teams", type=int, default=0)
    ap.add_argument("--trees", type=int, default=1)
    ap.add_argument("--team-pick", default=None)
    ap.add_argument("--separation", type=float, default=None)
    a = ap.parse_args()
    budget, length, interval = 2.0, 150.0, 98.0
    w = synth.make_world(seed=1, n_obstacles=64)
    obstacles, habitats, cells, shark, poly = world_objects(w)
    rrt = RRT(poly, obstacles, shark, cells)
    # every launch of the batch: (AUVs, iterations run, ms of the expansion + leaf pass)
    launches = []
    run = rrt._ctx.rrt_explore_batch

    def timed(*args, **kw):
        s = run(*args, **kw)
        # (the device route leaves the summaries in HBM: every episode runs its whole budget, args[2] iterations)
        n, it = (len(s), int(s["iters_run"].sum())) if s is not None else (len(args[0]), len(args[0]) * int(args[2]))
        launches.append((n, it, rrt._ctx.last_kernel_ms(), rrt._ctx.last_rrt_kernel()))
        return s
    rrt._ctx.rrt_explore_batch = timed
    for N in [int(x) for x in a.sizes.split(",")]:
        starts = starts_near(w, N, N)
        seeds = list(range(1, N + 1))
        tkw = dict(teams=[e // a.teams for e in range(N)]) if a.teams > 0 else {}  # (without --teams: the call as it always was)
        if a.trees > 1:
            tkw["trees_per_auv"] = a.trees
        if a.team_pick:
            tkw["team_pick"] = a.team_pick
        if a.separation is not None:
            tkw["team_separation"] = a.separation
        rrt.replanning_batch(starts[:8], habitats, budget, length, interval, [-3, -3, -4], max_iter=a.iters, seeds=seeds[:8],
                             as_arrays=True, commit=a.commit, **({"trees_per_auv": a.trees} if a.trees > 1 else {}))  # warm-up (code objects, buffers)
        for _ in range(a.runs):
            launches.clear()
            t0 = time.perf_counter()
            res = rrt.replanning_batch(starts, habitats, budget, length, interval, [-3, -3, -4], max_iter=a.iters, seeds=seeds,
                                       as_arrays=True, commit=a.commit, **tkw)
            wall = time.perf_counter() - t0
            rounds = [dict(auvs=n, expansions=it, ms=round(ms, 3), mexp_s=round(it / ms / 1e3, 1), kernel=k) for n, it, ms, k in launches]
            exp = sum(r["expansions"] for r in rounds)
            extra = {}
            if a.commit == "device":
                info = rrt._ctx.replan_info()
                extra = dict(commit_kernel_ms=round(info["commit_ms"], 3), commit_rounds=info["rounds"], rows=info["rows"],
                             bytes_traj=info["bytes_traj"],
                             bytes_per_round=round((info["bytes_to_host"] - info["bytes_traj"]) / max(info["rounds"], 1), 1))
            print(json.dumps(dict(probe="replanning_batch", commit=a.commit, auvs=N, teams_of=a.teams, trees=a.trees, team_pick=a.team_pick, separation=a.separation, iters=a.iters, wall_s=round(wall, 3),
                                  kernel_ms=round(sum(r["ms"] for r in rounds), 3), expansions=exp,
                                  mexp_s_kernel=round(exp / sum(r["ms"] for r in rounds) / 1e3, 1),
                                  mexp_s_wall=round(exp / wall / 1e6, 2), none=sum(r is None for r in res), **extra,
                                  rounds=rounds)), flush=True)
        if a.commit == "device":
            continue
        # the same parameters as one uniform batch: per-episode-limits kernel vs plain rrt_explore_kernel
        ctx = _lib.Context(0)
        ctx.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"])
        init = np.array([[s.x, s.y, 0, 0, 0, 0] for s in starts], dtype=np.float64)
        sd = np.array(seeds, dtype=np.uint64)
        kw = dict(max_plan_time=float(a.iters), weights=(-3, -3, -4))
        for k in ("ROWS", "DUO", "TRIO"):
            ctx.set_option(k, 0)
        out = {}
        for name, mtt in (("lim", [length] * N), ("plain", length)):
            ctx.rrt_explore_batch(init, sd, a.iters, max_traj_time=mtt, **kw)  # warm-up
            ms = []
            for _ in range(3):
                s = ctx.rrt_explore_batch(init, sd, a.iters, max_traj_time=mtt, **kw)
                ms.append(ctx.last_kernel_ms())
            out[name] = dict(kernel=ctx.last_rrt_kernel(), ms=round(min(ms), 3), mexp_s=round(int(s["iters_run"].sum()) / min(ms) / 1e3, 1))
        print(json.dumps(dict(probe="uniform_batch", auvs=N, iters=a.iters, max_traj_time=length, **out,
                              lim_over_plain=round(out["lim"]["ms"] / out["plain"]["ms"], 4))), flush=True)
        ctx.close()
    # sequential replanning, a few AUVs: wall time per AUV
    if a.seq and a.commit == "host":
        starts = starts_near(w, a.seq, 7)
        rrt.replanning(starts[0], list(habitats), budget, length, interval, [-3, -3, -4], max_iter=a.iters, seed=1)  # warm-up
        t0 = time.perf_counter()
        n_ok = 0
        for e in range(a.seq):
            try:
                rrt.replanning(starts[e], list(habitats), budget, length, interval, [-3, -3, -4], max_iter=a.iters, seed=e + 1)
                n_ok += 1
            except TypeError:
                pass
        wall = time.perf_counter() - t0
        print(json.dumps(dict(probe="replanning_sequential", auvs=a.seq, completed=n_ok, iters=a.iters, wall_s=round(wall, 3),
                              s_per_auv=round(wall / a.seq, 4))), flush=True)


if __name__ == "__main__":
    main()

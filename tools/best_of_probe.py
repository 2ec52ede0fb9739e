"""Best-of-K planning: what one replanning round costs and buys (profiles/best_of_probe.md).

    python tools/best_of_probe.py [--sizes 256,1024,4096] [--trees 1,4,8] [--iters 2000] [--reps 3] [--out profiles/best_of_probe.md]

The world and parameters of tools/replan_batch_probe.py (synth.make_world(seed=1, n_obstacles=64), horizon 150 s, starts
within 25 m of the world's start, `iters` iterations per round).  One round = one batch of N AUVs x K trees with per-episode
limits, as RRT.replanning_batch(trees_per_auv=K) launches it: AUV i's members are episodes i*K .. i*K+K-1, tree m of AUV i has
seed 8 i + m + 1 (so the trees of a smaller K are the first trees of a larger one).  Per configuration, after a warm-up, `reps`
times:
  expand + leaf   the handle's event time of the expansion and leaf launches
  select          rrt_group_best + group_paths: the selection launch, the course launch and the winners' courses to the host
                  (host clock; both calls end in a stream synchronise)
  host route      what a caller has to do without the selection kernels: every summary and every episode's course to the
                  host (summaries + paths: both end in a synchronise) and a numpy fold over the groups (host clock)
and the mean winning cost over the AUVs that have a winner.  The two routes must name the same winners (asserted).
A configuration whose buffers do not fit the device is reported as such.  One JSON line per configuration; the table goes to
--out."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from auv_sim_amd import _lib, synth  # noqa: E402


def starts_near(w, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        x, y = w["start"][0] + rng.uniform(-25, 25), w["start"][1] + rng.uniform(-25, 25)
        if all(math.hypot(x - o[0], y - o[1]) > o[2] + 3.0 for o in w["obstacles"]):
            out.append((float(x), float(y)))
    return np.array(out)


def host_fold(summ, K):
    """exploring's rule per group of K on the host: the winners' batch-wide indexes (-1: none)"""
    c = np.where(summ["best_leaf"] >= 0, summ["best_cost"][:, 0], np.inf).reshape(-1, K)
    c = np.where(np.isnan(c), np.inf, c)
    m = np.argmin(c, axis=1)  # (the first of equal minima)
    g = np.arange(len(c))
    return np.where(c[g, m] < np.inf, m + g * K, -1)


def measure(ctx, xy, K, iters, horizon, reps):
    N = len(xy)
    E = N * K
    init = np.zeros((E, 6))
    init[:, :2] = np.repeat(xy, K, axis=0)
    seeds = (np.repeat(np.arange(N, dtype=np.uint64) * 8, K) + np.tile(np.arange(K, dtype=np.uint64), N) + 1)
    off = np.arange(N + 1) * K
    ctx.rrt_prepare(init, seeds, iters, max_traj_time=np.full(E, horizon), weights=(-3, -3, -4), max_plan_time=float(iters))
    rows = []
    for rep in range(reps + 1):  # (the first pass is the warm-up)
        ctx.rrt_run()
        kernel_ms = ctx.last_kernel_ms()
        t0 = time.perf_counter()
        best = ctx.rrt_group_best(off)
        gp = ctx.group_paths(best)
        t1 = time.perf_counter()
        summ = ctx.summaries()
        paths = ctx.paths(summ)
        win = host_fold(summ, K)
        t2 = time.perf_counter()
        assert np.array_equal(win, best["winner"]), "the two routes disagree"
        if rep:
            rows.append((kernel_ms, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    has = best["winner"] >= 0
    g = int(np.flatnonzero(has)[0]) if has.any() else -1
    assert g < 0 or np.array_equal(gp[g], paths[int(best[g]["winner"])])
    a = np.array(rows)
    return dict(auvs=N, trees=K, episodes=E, iters=iters, kernel=ctx.last_rrt_kernel(),
                expand_leaf_ms=[round(float(x), 3) for x in a[:, 0]], select_ms=[round(float(x), 3) for x in a[:, 1]],
                host_route_ms=[round(float(x), 3) for x in a[:, 2]],
                winners=int(has.sum()), mean_winning_cost=round(float(best["cost"][has, 0].mean()), 4) if has.any() else None,
                winner_rows=int(np.where(has, best["path_len"], 0).sum()),
                all_rows=int(np.where(summ["best_leaf"] >= 0, summ["best_path_len"], 0).sum()))


def cell(v):
    lo, hi = min(v), max(v)
    return "%.2f (%.2f - %.2f)" % (float(np.median(v)), lo, hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024,4096")
    ap.add_argument("--trees", default="1,4,8")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "best_of_probe.md"))
    a = ap.parse_args()
    horizon = 150.0
    w = synth.make_world(seed=1, n_obstacles=64)
    ctx = _lib.Context(0)
    ctx.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"])
    results = []
    for N in [int(x) for x in a.sizes.split(",")]:
        xy = starts_near(w, N, N)
        for K in [int(x) for x in a.trees.split(",")]:
            try:
                r = measure(ctx, xy, K, a.iters, horizon, a.reps)
            except _lib.AuvpError as e:
                if e.code not in (-2, -3):  # (capacity / HIP allocation: the batch does not fit)
                    raise
                r = dict(auvs=N, trees=K, episodes=N * K, iters=a.iters, does_not_fit=str(e))
            results.append(r)
            print(json.dumps(r), flush=True)
            if "does_not_fit" in r:
                break  # (a failed allocation leaves the handle without buffers; larger K will not fit either)
    lines = ["# Best-of-K planning: one replanning round (`tools/best_of_probe.py`)", "",
             "Measured on one MI355X (gfx950) with the build of this change: `python tools/best_of_probe.py --sizes %s --trees %s "
             "--iters %d --reps %d`." % (a.sizes, a.trees, a.iters, a.reps),
             "World and parameters of `profiles/replan_batch_probe.md` (`synth.make_world(seed=1, n_obstacles=64)`, horizon 150 s,",
             "%d iterations per round); one round = one batch of N AUVs x K trees with per-episode limits, tree m of AUV i seeded" % a.iters,
             "8 i + m + 1.  Times in ms: median (min - max) of %d runs after a warm-up.  *expand + leaf*: the handle's event time of" % a.reps,
             "the round's launches.  *select*: `rrt_group_best` + `group_paths` (selection launch, course launch, the winners' courses",
             "to the host; host clock, ends in a synchronise).  *host route*: all summaries and all E courses to the host plus a numpy",
             "fold, on the same build (host clock, ends in a synchronise): what a caller without the selection kernels has to do.", "",
             "| AUVs | K | episodes | expand + leaf ms | select ms | host route ms | host route / select | course rows: winners / all | mean winning cost |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        if "does_not_fit" in r:
            lines.append("| %d | %d | %d | does not fit the device's memory (%s) | | | | | |" % (r["auvs"], r["trees"], r["episodes"], r["does_not_fit"]))
            continue
        lines.append("| %d | %d | %d | %s | %s | %s | %.1f | %d / %d | %s |" % (
            r["auvs"], r["trees"], r["episodes"], cell(r["expand_leaf_ms"]), cell(r["select_ms"]), cell(r["host_route_ms"]),
            float(np.median(r["host_route_ms"])) / float(np.median(r["select_ms"])), r["winner_rows"], r["all_rows"],
            "%.4f (%d AUVs)" % (r["mean_winning_cost"], r["winners"]) if r["winners"] else "-"))
    ok = [r for r in results if "does_not_fit" not in r]
    if ok:
        spread = max((max(r[k]) - min(r[k])) / min(r[k]) for r in ok for k in ("expand_leaf_ms",))
        lines += ["", "Run-to-run spread of the expand + leaf time, (max - min) / min over the %d runs: at most %.1f %%; the host-clock columns"
                  % (a.reps, 100.0 * spread), "show their own range.  Lower cost is better (the weights are negative)."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""A shark-occupancy table per episode: what the leaf pass costs with G tables (profiles/shark_grid_sets.md).

    python tools/shark_grids_probe.py [--auvs 4096] [--iters 2000] [--sets 1,8,64] [--grid 200] [--reps 3] [--out profiles/shark_grid_sets.md]

The bench's world at `grid` x `grid` cells (synth.make_world(seed=2, n_obstacles=64), 10 time bins: one table of a 200 x 200
grid is 3.2 MB), one batch of `auvs` episodes with per-episode limits (horizon 200 s, every habitat kept), grown ONCE; every
leaf-pass figure is then an auvp_rrt_rerank of that batch -- the leaf pass alone on the same trees, timed by the handle's
events.  The tables are the world's own plus G - 1 seeded redraws.  After a warm-up of every variant, `reps` rounds that
alternate between the variants:
  lim          no assignment: rrt_leaf_lim_kernel against the world's table
  set 0        rrt_leaf_grid_kernel, every episode on set 0 (the world's table again: the summaries must equal lim's, asserted)
  G sets       rrt_leaf_grid_kernel, episode e on set e % G
and, once per round, a full auvp_rrt_run (expansion + leaf pass) of the same batch.  One JSON line per G; the table goes to
--out."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from auv_sim_amd import _lib, synth  # noqa: E402

FIELDS = ("status", "n_nodes", "n_leaves", "best_leaf", "best_path_len", "best_cost", "best_length", "leaf_elems")


def cell(v):
    return "%.3f (%.3f - %.3f)" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--auvs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--sets", default="1,8,64")
    ap.add_argument("--grid", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "shark_grid_sets.md"))
    a = ap.parse_args()
    E, horizon = a.auvs, 200.0
    half = 0.5 * a.grid * 10.0
    w = synth.make_world(seed=2, n_obstacles=64, box=(-half, -half, half, half), cell=10.0, n_bins=10, bin_len=50, n_habitats=10)
    ctx = _lib.Context(0)
    ctx.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"])
    rng = np.random.default_rng(3)
    init = np.zeros((E, 6))
    init[:, 0] = w["start"][0] + rng.uniform(-20, 20, E)
    init[:, 1] = w["start"][1] + rng.uniform(-20, 20, E)
    seeds = np.arange(E, dtype=np.uint64) + 9000
    table_mb = w["prob"].nbytes / 1e6
    results = []
    for G in [int(x) for x in a.sets.split(",")]:
        tabs = np.stack([w["prob"]] + [np.random.default_rng(100 + g).uniform(0.0, 0.3, w["prob"].shape) for g in range(1, G)])
        ctx.set_prob_sets(tabs)
        del tabs
        ctx.rrt_prepare(init, seeds, a.iters, max_traj_time=np.full(E, horizon), weights=(-3, -3, -4), max_plan_time=float(a.iters))
        ctx.rrt_run()
        variants = {"lim": None, "set0": np.zeros(E, np.int32), "sets": (np.arange(E) % G).astype(np.int32)}
        times = {k: [] for k in list(variants) + ["round", "round_leaf"]}
        for rep in range(a.reps + 1):  # (the first round is the warm-up)
            summ = {}
            for k, v in variants.items():
                ctx.rrt_set_episode_grids(v)
                summ[k] = ctx.rrt_rerank()
                if rep:
                    times[k].append(ctx.last_launch_parts()[1])
            for f in FIELDS:
                assert np.array_equal(summ["lim"][f], summ["set0"][f]), f  # the same table through the other kernel
            ctx.rrt_run()  # (with the G-set assignment in place)
            if rep:
                times["round"].append(ctx.last_kernel_ms())
                times["round_leaf"].append(ctx.last_launch_parts()[1])
        differ = int((summ["sets"]["best_leaf"] != summ["lim"]["best_leaf"]).sum())
        r = dict(auvs=E, iters=a.iters, sets=G, tables_mb=round(G * table_mb, 1), expansion_kernel=ctx.last_rrt_kernel(),
                 leaves=int(summ["lim"]["n_leaves"].sum()), episodes_with_another_best_leaf=differ,
                 **{k + "_ms": [round(float(x), 4) for x in v] for k, v in times.items()})
        results.append(r)
        print(json.dumps(r), flush=True)
    lines = ["# A shark table per episode: the leaf pass against G tables (`tools/shark_grids_probe.py`)", "",
             "Measured on one MI355X (gfx950) with the build of this change: `python tools/shark_grids_probe.py --auvs %d --iters %d "
             "--sets %s --grid %d --reps %d`." % (E, a.iters, a.sets, a.grid, a.reps),
             "The bench's world at %d x %d cells and 10 time bins (one table: %.1f MB); one batch of %d episodes with per-episode limits,"
             % (a.grid, a.grid, table_mb, E),
             "horizon %.0f s, grown once per G; every leaf-pass time is an `auvp_rrt_rerank` of that batch (the leaf pass alone on the same" % horizon,
             "trees, the handle's event time).  Times in ms: median (min - max) of %d rounds after a warm-up round; a round runs the" % a.reps,
             "variants one after the other, so they alternate.  *lim*: `rrt_leaf_lim_kernel`, the world's table.  *set 0*:",
             "`rrt_leaf_grid_kernel`, every episode on set 0 = the world's table (summaries equal to lim's: asserted).  *G sets*:",
             "`rrt_leaf_grid_kernel`, episode e on set e % G.  *full round*: `auvp_rrt_run`, expansion + leaf pass with the G-set assignment.", "",
             "| G | tables MB | lim ms | set 0 ms | set 0 / lim | G sets ms | G sets / lim | full round ms | full round / rerank | episodes whose best leaf differs from lim's |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        m = {k: float(np.median(r[k + "_ms"])) for k in ("lim", "set0", "sets", "round")}
        lines.append("| %d | %.1f | %s | %s | %.3f | %s | %.3f | %s | %.1f | %d of %d |" % (
            r["sets"], r["tables_mb"], cell(r["lim_ms"]), cell(r["set0_ms"]), m["set0"] / m["lim"], cell(r["sets_ms"]),
            m["sets"] / m["lim"], cell(r["round_ms"]), m["round"] / m["sets"], r["episodes_with_another_best_leaf"], r["auvs"]))
    spread = max((max(r[k]) - min(r[k])) / min(r[k]) for r in results for k in ("lim_ms", "set0_ms", "sets_ms"))
    lines += ["", "Run-to-run spread of the leaf-pass times, (max - min) / min over the %d rounds: at most %.1f %%." % (a.reps, 100.0 * spread),
              "Expansion kernel of the full round: `%s`." % results[-1]["expansion_kernel"]]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

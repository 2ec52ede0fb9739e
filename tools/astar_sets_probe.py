"""astar_fixLenSOG with a shark-occupancy table per instance: what the sets launch and the device top-n tables cost
(profiles/astar_shark_sets.md).

    python tools/astar_sets_probe.py [--parent-lib <libauvplan.so of the parent commit>] [--runs 6] [--out profiles/astar_shark_sets.md]

(a) BASELINE config 3 -- 1 024 astar_fixLenSOG instances over bench_sides' world -- as a plain auvp_astar_batch and through
    auvp_astar_batch_sets with ONE set equal to the world's table and set_of = 0 for every instance: the batch's event time
    (search launch + whatever reset the batch needs), `runs` runs each after a warm-up of both, on the same build and handle.
    The summaries of the two must be equal (asserted).  With --parent-lib the plain batch is also timed on that library, in a
    fresh child process (AUVPLAN_LIBRARY).
(b) the same for the first 128 instances: a latency batch, which takes the PAIR form (two wavefronts per instance).
    The table names the form every row ran (512 threads per workgroup: PAIR, 256: one wavefront per instance); (a) is repeated
    with option ASTAR_PAIR = 0, so that the one-wavefront form is timed whatever the library chooses for 1 024 instances.
(c) the top-n tables of F = 64 sets with T = 10 bins and C = 4 096 cells: on the device (astar_topn_sets_kernel: the event time
    of its launch, and the wall time of the call that builds the tables and reads them back), against the route a caller has
    without it -- the tables are on the host (read back), every row is sorted descending and summed one entry after the other
    (here numpy's sort and its cumsum, the same serial additions; the result must equal the device's, asserted), and the result
    is uploaded (here: the upload of an array of the tables' size through set_prob_sets).
One JSON line per part; the table goes to --out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from auv_sim_amd import _astar_lib as al, _lib  # noqa: E402
from bench_sides.astar import astar_inputs  # noqa: E402

WTS = (0, 10, 10, 100)
# (instances, option ASTAR_PAIR): (a), (b) with the library's own choice of the kernel form, and (a) once more with the
# one-wavefront form forced, so that both forms are timed whichever the choice takes
CASES = ((1024, None), (128, None), (1024, 0))


def cell(v):
    return "%.3f (%.3f - %.3f)" % (float(np.median(v)), min(v), max(v))


def batches(n_inst, runs, with_sets, pair=None):
    """event times (ms) of `runs` plain batches and, with_sets, `runs` sets batches of the first n_inst config-3 instances"""
    w, starts, limits = astar_inputs(1024)
    starts, limits = starts[:n_inst], limits[:n_inst]
    ctx = _lib.Context(0)
    ctx.set_option("ASTAR_PAIR", pair)   # (None: the library's own choice)
    ctx.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"])
    if with_sets:
        ctx.set_prob_sets(np.asarray(w["prob"], dtype=np.float64)[None])
    kw = dict(limits=limits, weights=WTS, velocity=1.0, cap_nodes=20000)
    forms = [("plain", None)] + ([("sets", np.zeros(n_inst, np.int32))] if with_sets else [])
    out, summ, block = {}, {}, {}
    for name, so in forms:   # warm-up of every form (the first sets batch builds the top-n tables)
        al.run_batch_arrays(ctx, "astar_fixLenSOG", starts, set_of=so, **kw)
    for name, so in forms:
        ms = []
        for _ in range(runs):
            r = al.run_batch_arrays(ctx, "astar_fixLenSOG", starts, set_of=so, **kw)
            ms.append(float(r["batch_ms"]))
        out[name], summ[name], block[name] = ms, r["summ"], ctx.last_launch()[1]
    if with_sets:
        for f in summ["plain"].dtype.names:
            assert np.array_equal(summ["plain"][f], summ["sets"][f]), f
    assert not (summ["plain"]["status"] < 0).any()
    ctx.close()
    return dict(instances=n_inst, pair_option=pair, threads_per_workgroup=block, **{k + "_ms": [round(x, 4) for x in v] for k, v in out.items()})


def tables(F=64, T=10, C=4096):
    rng = np.random.default_rng(4)
    prob = rng.uniform(0.0, 0.3, (F, T, C))
    bins = np.array([(50.0 * t, 50.0 * t + 50.0) for t in range(T)])
    side = int(round(C ** 0.5))
    cells = np.array([(10.0 * c, 10.0 * r, 10.0 * c + 10.0, 10.0 * r + 10.0) for r in range(C // side) for c in range(side)])
    ctx = _lib.Context(0)
    ctx.set_world(bins=bins, cells=cells, prob=prob[0])
    dev_ms, dev_wall, host_sort, host_up = [], [], [], []
    for rep in range(4):   # (the first round is the warm-up)
        ctx.set_prob_sets(prob)   # (replaces the sets: the tables are stale and the next call builds them)
        t0 = time.perf_counter()
        got = al.sets_topn(ctx)
        t1 = time.perf_counter()
        # (sets_topn's event time is the table kernel's: nothing else was launched since)
        k_ms = ctx.last_kernel_ms()
        t2 = time.perf_counter()
        want = np.zeros((F, T, C + 1))
        np.cumsum(-np.sort(-prob, axis=2), axis=2, out=want[:, :, 1:])
        t3 = time.perf_counter()
        ctx.set_prob_sets(want[:, :, :C])   # an upload of the tables' size
        t4 = time.perf_counter()
        assert np.array_equal(got, want)
        if rep:
            dev_ms.append(k_ms); dev_wall.append(1e3 * (t1 - t0)); host_sort.append(1e3 * (t3 - t2)); host_up.append(1e3 * (t4 - t3))
    ctx.close()
    return dict(F=F, T=T, C=C, device_kernel_ms=[round(x, 4) for x in dev_ms], device_build_and_readback_wall_ms=[round(x, 3) for x in dev_wall],
                host_sort_sum_ms=[round(x, 3) for x in host_sort], host_upload_ms=[round(x, 3) for x in host_up])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--out", default=os.path.join("profiles", "astar_shark_sets.md"))
    ap.add_argument("--child-plain", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_plain:   # the plain batches alone, on whatever library AUVPLAN_LIBRARY names
        print(json.dumps([batches(n, a.runs, False, pr) for n, pr in CASES]))
        return
    parent = None
    if a.parent_lib:
        env = dict(os.environ, AUVPLAN_LIBRARY=os.path.abspath(a.parent_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-plain", "--runs", str(a.runs)], env=env, cwd=REPO,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        parent = json.loads(r.stdout.strip().splitlines()[-1])
    parts = [batches(n, a.runs, True, pr) for n, pr in CASES]
    for i, p in enumerate(parts):
        if parent:
            p["parent_plain_ms"] = parent[i]["plain_ms"]
        print(json.dumps(p), flush=True)
    tb = tables()
    print(json.dumps(tb), flush=True)
    lines = ["# astar_fixLenSOG with a shark table per instance: the sets launch and the device top-n tables (`tools/astar_sets_probe.py`)", "",
             "Measured on one MI355X (gfx950): `python tools/astar_sets_probe.py --runs %d%s`." % (a.runs, " --parent-lib <parent build>" if parent else ""),
             "Batch times are the handle's event time of `auvp_astar_batch` / `auvp_astar_batch_sets` (search launch + the reset the batch",
             "needs), ms: median (min - max) of %d runs after a warm-up of both forms, same build, same handle.  *sets*: one set equal to the" % a.runs,
             "world's table, `set_of = 0` for every instance; its summaries equal the plain batch's (asserted).", "",
             "| instances | ASTAR_PAIR | threads per workgroup | plain ms | sets ms | sets / plain (medians) | plain spread (max - min) / min | plain on the parent build ms |",
             "|---|---|---|---|---|---|---|---|"]
    for p in parts:
        pl, st = p["plain_ms"], p["sets_ms"]
        lines.append("| %d | %s | %d | %s | %s | %.4f | %.2f %% | %s |" % (
            p["instances"], "default" if p["pair_option"] is None else str(p["pair_option"]), p["threads_per_workgroup"]["sets"], cell(pl), cell(st), np.median(st) / np.median(pl),
            100.0 * (max(pl) - min(pl)) / min(pl), cell(p["parent_plain_ms"]) if parent else "not measured"))
    lines += ["", "Top-n tables of F = %d sets, T = %d bins, C = %d cells (ms, median (min - max) of 3 rounds after a warm-up round):" % (tb["F"], tb["T"], tb["C"]), "",
              "| route | ms |", "|---|---|",
              "| device: `astar_topn_sets_kernel`, event time | %s |" % cell(tb["device_kernel_ms"]),
              "| device: wall time of the call that builds the tables and reads them back (%.1f MB) | %s |"
              % (tb["F"] * tb["T"] * (tb["C"] + 1) * 8 / 1e6, cell(tb["device_build_and_readback_wall_ms"])),
              "| host: sort + serial sums of the %d rows (numpy; the tables already read back) | %s |" % (tb["F"] * tb["T"], cell(tb["host_sort_sum_ms"])),
              "| host: upload of the tables | %s |" % cell(tb["host_upload_ms"])]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

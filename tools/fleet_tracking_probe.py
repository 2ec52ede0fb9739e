"""Per-round wall time of tracking.FleetTracker (profiles/fleet_tracking.md).

    python tools/fleet_tracking_probe.py [--auvs 4096] [--trees 4] [--sharks 64] [--particles 1000] [--iters 2000] [--cell 1.0]
                                          [--forecast-rounds 4] [--repeats 2]

A fleet of `auvs` AUVs x `trees` trees tracks `sharks` sharks on synth.make_world(seed=1, n_obstacles=64, cell=`cell`) -- cell 1.0:
40 000 cells, a 201 x 201 forecast grid (large_grids=True) --, plan budget 2, horizon 150 s, replan interval 98 s.  After a
warm-up tracker of 8 x sharks AUVs, `repeats` x (one tracker with measure="device", one with measure="host"), alternating, each
run to its end.  Every step is timed stage by stage on the host clock (every stage ends with a stream synchronisation inside
the library): the measurements and the filter step, the forecast, placing its tables, the round (whose planning launch's own
HIP-event time is listed beside it).  One JSON line per tracker."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from auv_sim_amd import _lib, _pf_lib, synth  # noqa: E402
from auv_sim_amd.rrt_dubins import RRT  # noqa: E402
from auv_sim_amd.sharkForecast import SharkForecast  # noqa: E402
from auv_sim_amd.tracking import FleetTracker, first_bin_of_time, fleet_measurements  # noqa: E402
from replan_batch_probe import starts_near, world_objects  # noqa: E402


class _Box:
    def __init__(self, b):
        self.bounds = tuple(float(v) for v in b)


def run_tracker(rrt, w, cells, habitats, n_auvs, a, measure):
    F = a.sharks
    rng = np.random.default_rng(3)
    x0, y0, x1, y1 = w["box"]
    base = np.column_stack([rng.uniform(x0 + 30, x1 - 30, F), rng.uniform(y0 + 30, y1 - 30, F)])
    tracks = base[:, None, :] + np.arange(8)[None, :, None] * np.array([3.0, -2.0])[None, None, :]
    fctx = _lib.Context(0)
    mts = np.stack([_pf_lib.np_seed_state(100 + f)[0] for f in range(F)])
    filters = _pf_lib.FilterBatch(fctx, F, a.particles).create(tracks[:, 0, :], mts, 624)
    sf = SharkForecast(_Box(w["box"]), a.cell, cells, device_context=fctx)
    shark_of = [e % F for e in range(n_auvs)]
    tr = FleetTracker(rrt, sf, filters, tracks, shark_of, np.ones((sf.n_row, sf.n_col)), a.forecast_rounds, measure=measure,
                      large_grids=True, starts=starts_near(w, n_auvs, n_auvs), habitats=habitats, plan_time_budget=2.0,
                      traj_time_length=150.0, replan_time_interval=98.0, weight=[-3, -3, -4], max_iter=a.iters,
                      seeds=list(range(1, n_auvs + 1)), trees_per_auv=a.trees)
    s, ctx = tr.session, rrt._ctx
    plan_ms = []
    run = ctx.rrt_explore_batch

    def timed(*args, **kw):
        out = run(*args, **kw)
        plan_ms.append(ctx.last_kernel_ms())
        return out
    ctx.rrt_explore_batch = timed
    steps = []
    try:
        while True:
            r = s.round_index
            if r >= tracks.shape[1] or len(s.active()) == 0:
                break
            shark = tracks[:, r, :]
            t0 = time.perf_counter()
            if measure == "device":
                filters.run_dev_meas(ctx.replan_measure(tr.shark_of, tr.A, shark), tr.A, shark[None])
            else:
                filters.run(meas=fleet_measurements(s.last, tr.shark_of, shark), shark_xy=shark[None])
            t1 = time.perf_counter()
            fc = tr._forecast()
            t2 = time.perf_counter()
            s.set_shark_grids(fc, first_bin=first_bin_of_time(rrt._bins, r * s.round_span))
            t3 = time.perf_counter()
            out = s.round()
            t4 = time.perf_counter()
            steps.append(dict(auvs=int(len(out["auv"])), measure_filter_ms=1e3 * (t1 - t0), forecast_ms=1e3 * (t2 - t1),
                              place_ms=1e3 * (t3 - t2), round_ms=1e3 * (t4 - t3), step_ms=1e3 * (t4 - t0), plan_kernel_ms=plan_ms[-1]))
    finally:
        del ctx.rrt_explore_batch
        t0 = time.perf_counter()
        res = s.finish(as_arrays=True)
        finish_ms = 1e3 * (time.perf_counter() - t0)
    fctx.close()
    return dict(probe="fleet_tracking", measure=measure, auvs=n_auvs, trees=a.trees, sharks=F, particles=a.particles, iters=a.iters,
                grid=[sf.n_row, sf.n_col], cells=len(cells), forecast_kernel=sf.last.kernel, rounds=len(steps), finish_ms=round(finish_ms, 1),
                none=sum(x is None for x in res), steps=[{k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()} for st in steps])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--auvs", type=int, default=4096)
    ap.add_argument("--trees", type=int, default=4)
    ap.add_argument("--sharks", type=int, default=64)
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--cell", type=float, default=1.0)
    ap.add_argument("--forecast-rounds", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    w = synth.make_world(seed=1, n_obstacles=64, cell=a.cell)
    obstacles, habitats, cells, shark, poly = world_objects(w)
    rrt = RRT(poly, obstacles, shark, cells)
    warm = run_tracker(rrt, w, cells, habitats, 8 * a.sharks, a, "device")  # (code objects, buffers)
    print(json.dumps(dict(warm, probe="fleet_tracking_warmup")), flush=True)
    for _ in range(a.repeats):
        for measure in ("device", "host"):
            print(json.dumps(run_tracker(rrt, w, cells, habitats, a.auvs, a, measure)), flush=True)


if __name__ == "__main__":
    main()

"""k filter steps per round (FleetTracker(filter_steps=k), option MEAS_TICKS): what the measurement kernel and the whole round
cost (profiles/fleet_tracking_ticks.md).

    python tools/fleet_ticks_probe.py [--auvs 4096] [--trees 4] [--sharks 64] [--particles 1000] [--iters 2000] [--cell 1.0]
                                       [--forecast-rounds 4] [--ticks 1,4,16] [--repeats 2] [--launches 30]

The fleet, world and rounds of tools/fleet_tracking_probe.py.  After a warm-up tracker of 8 x sharks AUVs:
  1. one tracker runs one round, so that every AUV has a committed bucket in the log; then, `launches` times each, alternating:
     replan_measure_kernel (shark_xy [F,2]) and replan_measure_ticks_kernel with k of `ticks` (shark_xy [k,F,2]) on those
     segments -- the kernel's own HIP-event time (auvp_last_kernel_ms) and the call's wall time (uploads, the launch, the
     stream synchronisation); one JSON line with min / median / max of each;
  2. `repeats` x (one tracker per k of `ticks`, measure="device"), alternating, each run to its end with every step timed stage
     by stage on the host clock as tools/fleet_tracking_probe.py times them; one JSON line per tracker."""
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
from auv_sim_amd.tracking import FleetTracker, first_bin_of_time  # noqa: E402
from replan_batch_probe import starts_near, world_objects  # noqa: E402

ROUNDS = 8  # samples of the tracks, in rounds (fleet_tracking_probe.py: 8 samples at one per round)


class _Box:
    def __init__(self, b):
        self.bounds = tuple(float(v) for v in b)


def tracker(rrt, w, cells, habitats, n_auvs, a, k):
    F = a.sharks
    rng = np.random.default_rng(3)
    x0, y0, x1, y1 = w["box"]
    base = np.column_stack([rng.uniform(x0 + 30, x1 - 30, F), rng.uniform(y0 + 30, y1 - 30, F)])
    # the sharks move 3 and -2 metres per round, in k equal parts
    tracks = base[:, None, :] + (np.arange(ROUNDS * k) / k)[None, :, None] * np.array([3.0, -2.0])[None, None, :]
    fctx = _lib.Context(0)
    mts = np.stack([_pf_lib.np_seed_state(100 + f)[0] for f in range(F)])
    filters = _pf_lib.FilterBatch(fctx, F, a.particles).create(tracks[:, 0, :], mts, 624)
    sf = SharkForecast(_Box(w["box"]), a.cell, cells, device_context=fctx)
    tr = FleetTracker(rrt, sf, filters, tracks, [e % F for e in range(n_auvs)], np.ones((sf.n_row, sf.n_col)), a.forecast_rounds,
                      measure="device", large_grids=True, filter_steps=k, starts=starts_near(w, n_auvs, n_auvs), habitats=habitats,
                      plan_time_budget=2.0, traj_time_length=150.0, replan_time_interval=98.0, weight=[-3, -3, -4], max_iter=a.iters,
                      seeds=list(range(1, n_auvs + 1)), trees_per_auv=a.trees)
    return tr, tracks, fctx, sf


def sharks_of_round(tracks, r, k):
    return np.ascontiguousarray(tracks[:, r * k:(r + 1) * k].transpose(1, 0, 2))


def spread(v):
    v = sorted(v)
    return dict(min=round(v[0], 4), median=round(v[len(v) // 2], 4), max=round(v[-1], 4))


def kernel_times(rrt, w, cells, habitats, a, ticks):
    tr, tracks, fctx, _ = tracker(rrt, w, cells, habitats, a.auvs, a, 1)
    ctx, s = rrt._ctx, tr.session
    assert tr.step() is not None
    rows = s.last_segments()
    n = np.array([len(x) for x in rows])
    rng = np.random.default_rng(7)
    forms = [("replan_measure_kernel", None)] + [("replan_measure_ticks_kernel k=%d" % k, k) for k in ticks]
    sharks = {k: np.ascontiguousarray(tracks[:, 1, :][None] + rng.uniform(-1, 1, (k, a.sharks, 2))) for _, k in forms if k}
    kern, wall = {name: [] for name, _ in forms}, {name: [] for name, _ in forms}
    for i in range(a.launches + 2):
        for name, k in forms:
            t0 = time.perf_counter()
            ctx.replan_measure(tr.shark_of, tr.A, tracks[:, 1, :] if k is None else sharks[k])
            t1 = time.perf_counter()
            if i >= 2:  # (the first two of every form: code objects, buffers)
                kern[name].append(ctx.last_kernel_ms())
                wall[name].append(1e3 * (t1 - t0))
    s.finish()
    fctx.close()
    return dict(probe="fleet_ticks_kernels", auvs=a.auvs, sharks=a.sharks, launches=a.launches,
                segment_rows=dict(min=int(n.min()), median=int(np.median(n)), max=int(n.max())),
                kernel_ms={name: spread(v) for name, v in kern.items()}, call_ms={name: spread(v) for name, v in wall.items()})


def run_tracker(rrt, w, cells, habitats, n_auvs, a, k):
    tr, tracks, fctx, sf = tracker(rrt, w, cells, habitats, n_auvs, a, k)
    s, ctx, filters = tr.session, rrt._ctx, tr.filters
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
            if (r + 1) * k > tracks.shape[1] or len(s.active()) == 0:
                break
            shark = sharks_of_round(tracks, r, k)
            t0 = time.perf_counter()
            ptr = ctx.replan_measure(tr.shark_of, tr.A, shark if k > 1 else shark[0])
            meas_kernel_ms = ctx.last_kernel_ms()
            t1 = time.perf_counter()
            filters.run_dev_meas(ptr, tr.A, shark, n_steps=k)
            pf_kernel_ms = fctx.last_kernel_ms()
            t2 = time.perf_counter()
            fc = tr._forecast()
            t3 = time.perf_counter()
            s.set_shark_grids(fc, first_bin=first_bin_of_time(rrt._bins, r * s.round_span))
            t4 = time.perf_counter()
            out = s.round()
            t5 = time.perf_counter()
            steps.append(dict(auvs=int(len(out["auv"])), measure_ms=1e3 * (t1 - t0), measure_kernel_ms=meas_kernel_ms,
                              filter_ms=1e3 * (t2 - t1), filter_kernel_ms=pf_kernel_ms, forecast_ms=1e3 * (t3 - t2),
                              place_ms=1e3 * (t4 - t3), round_ms=1e3 * (t5 - t4), step_ms=1e3 * (t5 - t0), plan_kernel_ms=plan_ms[-1]))
    finally:
        del ctx.rrt_explore_batch
        res = s.finish(as_arrays=True)
    fctx.close()
    return dict(probe="fleet_ticks_round", filter_steps=k, auvs=n_auvs, trees=a.trees, sharks=a.sharks, particles=a.particles,
                iters=a.iters, grid=[sf.n_row, sf.n_col], rounds=len(steps), none=sum(x is None for x in res),
                steps=[{key: (round(v, 3) if isinstance(v, float) else v) for key, v in st.items()} for st in steps])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--auvs", type=int, default=4096)
    ap.add_argument("--trees", type=int, default=4)
    ap.add_argument("--sharks", type=int, default=64)
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--cell", type=float, default=1.0)
    ap.add_argument("--forecast-rounds", type=int, default=4)
    ap.add_argument("--ticks", default="1,4,16")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--launches", type=int, default=30)
    a = ap.parse_args()
    ticks = [int(x) for x in a.ticks.split(",")]
    w = synth.make_world(seed=1, n_obstacles=64, cell=a.cell)
    obstacles, habitats, cells, shark, poly = world_objects(w)
    rrt = RRT(poly, obstacles, shark, cells)
    warm = run_tracker(rrt, w, cells, habitats, 8 * a.sharks, a, max(ticks))  # (code objects, buffers)
    print(json.dumps(dict(warm, probe="fleet_ticks_warmup")), flush=True)
    print(json.dumps(kernel_times(rrt, w, cells, habitats, a, ticks)), flush=True)
    for _ in range(a.repeats):
        for k in ticks:
            print(json.dumps(run_tracker(rrt, w, cells, habitats, a.auvs, a, k)), flush=True)


if __name__ == "__main__":
    main()

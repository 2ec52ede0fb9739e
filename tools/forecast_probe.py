"""Shark-occupancy forecast: what the launch costs next to the host path it replaces (profiles/shark_forecast.md).

    python tools/forecast_probe.py [--filters 512] [--particles 1000] [--side 20] [--rounds 10] [--reps 20] [--host-reps 2]
                                   [--out profiles/shark_forecast.md]

F particle filters x N particles (FilterBatch.create around seeded shark positions, one tracking step), a side x side grid of
10 m cells listed in raster order, a seeded positive prior per filter, method ("ave", 1), R rounds.  After a warm-up, `reps`
times:
  kernel      the handle's event time of sf_forecast_kernel (the particles are read where the filter kernel left them)
  call        SharkForecast.run on the batch, host clock: schedule, uploads of the prior, the launch, grids / prob / counts /
              status to the host (ends in a stream synchronise)
and `host-reps` times the only route the code had before: FilterBatch.particles() (every particle to the host) + counts in
Python + SharkUpdate.correction + R x SharkUpdate.predictOnAve per filter, on the same inputs (host clock).  The two routes
must agree bit for bit (asserted).  One JSON line; the table goes to --out."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from auv_sim_amd import _lib, _pf_lib  # noqa: E402
from auv_sim_amd.sharkEstimate import SharkUpdate  # noqa: E402
from auv_sim_amd.sharkForecast import SharkForecast  # noqa: E402


class Box:
    def __init__(self, *b):
        self.bounds = tuple(float(v) for v in b)


def host_route(batch, su, prior, rounds):
    """download + the SharkUpdate chain per filter -> (counts [F, rows, cols], grids [F, R+1, rows, cols] as lists)"""
    xy = batch.particles()[0][..., 0:2]
    minx, miny = su.boundary.bounds[0], su.boundary.bounds[1]
    all_counts, all_grids = [], []
    for f in range(len(xy)):
        counts = su._blank()
        n_row, n_col = len(counts), len(counts[0])
        for x, y in xy[f].tolist():
            qx, qy = (x - minx) / su.cell_size, (y - miny) / su.cell_size
            if 0 <= qx < n_col and 0 <= qy < n_row:
                counts[int(qy)][int(qx)] += 1
        grids = [su.correction(counts, prior[f].tolist())]
        for _ in range(rounds):
            grids.append(copy.deepcopy(su.predictOnAve(copy.deepcopy(grids[-1]), False, 1, 0.6, 0.1)[1]))
        all_counts.append(counts)
        all_grids.append(grids)
    return all_counts, all_grids


def cell(v, fmt="%.3f"):
    return (fmt + " (" + fmt + " - " + fmt + ")") % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=512)
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--side", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "shark_forecast.md"))
    a = ap.parse_args()
    F, N, side, R, cs = a.filters, a.particles, a.side, a.rounds, 10.0
    half = (side - 1) * cs / 2
    boundary = Box(-half, -half, half, half)
    cells = [Box(-half + c * cs, -half + r * cs, -half + (c + 1) * cs, -half + (r + 1) * cs) for r in range(side) for c in range(side)]
    rng = np.random.default_rng(1)
    prior = rng.uniform(0.01, 1.0, size=(F, side, side))
    ctx = _lib.Context(0)
    mts = np.stack([_pf_lib.np_seed_state(1000 + f)[0] for f in range(F)])
    batch = _pf_lib.FilterBatch(ctx, F, N).create(rng.uniform(-30, 30, size=(F, 2)), mts, 624)
    batch.run(phases=_pf_lib.UPDATE, n_steps=1)
    sf = SharkForecast(boundary, cs, cells)
    assert (sf.n_row, sf.n_col) == (side, side)
    kernel_ms, call_ms = [], []
    for rep in range(a.reps + 1):  # (the first pass is the warm-up)
        t0 = time.perf_counter()
        res = sf.run(batch, prior, R)
        t1 = time.perf_counter()
        if rep:
            kernel_ms.append(res.kernel_ms)
            call_ms.append((t1 - t0) * 1e3)
    host_ms = []
    su = SharkUpdate(boundary, cs, cells)
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        counts, grids = host_route(batch, su, prior, R)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(np.array(counts), res.counts), "the two routes disagree on the counts"
    assert np.array_equal(np.array(grids, dtype=np.float64), res.grids, equal_nan=True), "the two routes disagree on the grids"
    assert not res.status.any()
    try:
        import torch
        gpu = torch.cuda.get_device_name(0)
    except Exception:
        gpu = "device 0"
    r = dict(filters=F, particles=N, grid=[side, side], rounds=R, gpu=gpu, counted=int(res.counts.sum()), launch=list(ctx.last_launch()),
             kernel_ms=[round(x, 4) for x in kernel_ms], call_ms=[round(x, 3) for x in call_ms], host_route_ms=[round(x, 1) for x in host_ms])
    print(json.dumps(r), flush=True)
    lines = ["# Shark-occupancy forecast: the launch and the host path it replaces (`tools/forecast_probe.py`)", "",
             "Measured on one %s (gfx950) with the build of this change: `python tools/forecast_probe.py --filters %d --particles %d "
             "--side %d --rounds %d --reps %d --host-reps %d`." % (gpu, F, N, side, R, a.reps, a.host_reps),
             "%d particle filters x %d particles after one tracking step (%d of the %d particles lie inside the grid), a %d x %d grid of"
             % (F, N, r["counted"], F * N, side, side),
             "10 m cells in raster order (%d levels), one prior per filter, method (\"ave\", 1), %d rounds; grid %d x block %d, %d bytes of"
             % (2 * side - 1, R, r["launch"][0], r["launch"][1], r["launch"][2]),
             "LDS per workgroup.  Times in ms: median (min - max).", "",
             "| what | ms | runs |", "|---|---|---|",
             "| `sf_forecast_kernel`, the handle's event time | %s | %d after a warm-up |" % (cell(kernel_ms, "%.4f"), a.reps),
             "| `SharkForecast.run` on the `FilterBatch`: schedule, prior upload, launch, all outputs to the host (host clock, ends in a "
             "synchronise) | %s | %d after a warm-up |" % (cell(call_ms), a.reps),
             "| host path of the parent commit: `FilterBatch.particles()` + counts in Python + `SharkUpdate.correction` + %d x "
             "`predictOnAve` per filter (host clock) | %s | %d |" % (R, cell(host_ms, "%.1f"), a.host_reps), "",
             "Both routes gave the same counts and the same %d x %d x %d x %d grid values (asserted in the run).  The host path's time is"
             % (F, R + 1, side, side),
             "the Python interpreter's on the host of the GPU machine, a CPU shared with other work; the kernel's spread is the range shown.",
             "Speed is recorded here, not gated by any test."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

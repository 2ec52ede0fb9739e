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
must agree bit for bit (asserted).  One JSON line; the table goes to --out.

    python tools/forecast_probe.py --large --side 201 [--filters-list 1,256,1024] [--rounds 10] [--reps 20] [--host-filters 1]
                                   --out profiles/shark_forecast_wide.md

the forecast on large grids: sf_wide_kernel at four workgroup sizes beside sf_forecast_kernel where the grid fits it and the
Python host chain per filter (`large` below); the tables are APPENDED to --out."""
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


WIDE_BLOCKS = (64, 256, 512, 1024)


def large(a):
    """--large: sf_wide_kernel (SharkForecast.run(large_grids=True, return_grids=False)) on a side x side raster at 64, 256, 512
    and 1 024 threads per workgroup, for every F of --filters-list; where the grid fits it (side x side <= 4096) also
    sf_forecast_kernel, and the wide kernel forced there by option SF_WIDE_MIN = 1.  The variants alternate inside every
    repetition of one run, so that a drift of the machine meets all of them; kernel times are the handle's events.  Beside
    them the Python host chain's time per filter (SharkUpdate.correction + R x predictOnAve on the same inputs), whose prob must
    equal every variant's bit for bit (asserted for the filters it runs).  One JSON line per F; the tables are appended to --out."""
    side, R, N, cs = a.side, a.rounds, a.particles, 10.0
    half = (side - 1) * cs / 2
    boundary = Box(-half, -half, half, half)
    cells = [Box(-half + c * cs, -half + r * cs, -half + (c + 1) * cs, -half + (r + 1) * cs) for r in range(side) for c in range(side)]
    prior = np.random.default_rng(1).uniform(0.01, 1.0, size=(side, side))   # (shared by the filters: F x side x side is not uploaded)
    ctx = _lib.Context(0)
    fits = side * side <= 4096
    variants = ([("sf_forecast_kernel", None)] if fits else []) + [("sf_wide_kernel", b) for b in WIDE_BLOCKS]
    su = SharkUpdate(boundary, cs, cells)
    sf = SharkForecast(boundary, cs, cells, device_context=ctx)
    assert (sf.n_row, sf.n_col) == (side, side)
    try:
        import torch
        gpu = torch.cuda.get_device_name(0)
    except Exception:
        gpu = "device 0"
    out = ["", "## %d x %d raster (%d levels), %d rounds, %d particles per filter, method (\"ave\", 1)" % (side, side, 2 * side - 1, R, N), "",
           "`python tools/forecast_probe.py --large --side %d --rounds %d --particles %d --filters-list %s --reps %d --host-filters %d`"
           % (side, R, N, ",".join(str(f) for f in a.filters_list), a.reps, a.host_filters),
           "on one %s (gfx950).  Kernel times in ms from the handle's events, warm: median (min - max) of %d runs, the variants"
           % (gpu, a.reps), "alternating inside every repetition.", "",
           "| filters | kernel | threads per workgroup | kernel ms |", "|---|---|---|---|"]
    host_ms = []
    for F in a.filters_list:
        xy = np.random.default_rng(100 + F).normal(scale=0.2 * side * cs, size=(F, N, 2))
        times = {v: [] for v in variants}
        prob = {}
        for rep in range(a.reps + 1):  # (the first pass is the warm-up)
            for v in variants:
                name, block = v
                ctx.set_option("SF_WIDE_MIN", 1 if block else None)
                ctx.set_option("SF_WIDE_BLOCK", block)
                res = sf.run(xy, prior, R, large_grids=block is not None, return_grids=False)
                assert res.kernel == name and not res.status.any(), (res.kernel, name)
                if rep:
                    times[v].append(res.kernel_ms)
                else:
                    prob[v] = res.prob[:a.host_filters].copy()
        ctx.set_option("SF_WIDE_MIN", None)
        ctx.set_option("SF_WIDE_BLOCK", None)
        for f in range(min(a.host_filters, F)):
            t0 = time.perf_counter()
            counts = su._blank()
            for x, y in xy[f].tolist():
                qx, qy = (x + half) / cs, (y + half) / cs
                if 0 <= qx < side and 0 <= qy < side:
                    counts[int(qy)][int(qx)] += 1
            grids = [su.correction(counts, prior.tolist())]
            for _ in range(R):
                grids.append(copy.deepcopy(su.predictOnAve(copy.deepcopy(grids[-1]), False, 1, 0.6, 0.1)[1]))
            host_ms.append((time.perf_counter() - t0) * 1e3)
            want = np.array(grids, dtype=np.float64).reshape(R + 1, side * side)   # (raster: list order == grid order)
            for v in variants:
                assert np.array_equal(want, prob[v][f], equal_nan=True), ("the host chain and %s @ %s disagree" % v, f)
        print(json.dumps(dict(large=True, filters=F, particles=N, grid=[side, side], rounds=R, gpu=gpu,
                              kernel_ms={"%s@%s" % v: [round(x, 4) for x in t] for v, t in times.items()},
                              host_chain_ms_per_filter=[round(x, 1) for x in host_ms])), flush=True)
        for v in variants:
            out.append("| %d | `%s` | %s | %s |" % (F, v[0], v[1] or 64, cell(times[v], "%.4f")))
    out += ["", "The Python host chain (counts + `SharkUpdate.correction` + %d x `predictOnAve`) on the same machine: %s ms per filter"
            % (R, cell(host_ms, "%.1f")), "(host clock, %d runs; its prob equals every variant's bit for bit, asserted in the run)." % len(host_ms)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large", action="store_true", help="the sweep of sf_wide_kernel (see large()); appends to --out")
    ap.add_argument("--filters-list", type=lambda s: [int(x) for x in s.split(",")], default=[1, 256, 1024])
    ap.add_argument("--host-filters", type=int, default=1)
    ap.add_argument("--filters", type=int, default=512)
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--side", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "shark_forecast.md"))
    a = ap.parse_args()
    if a.large:
        return large(a)
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

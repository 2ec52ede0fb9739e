#!/usr/bin/env python3
"""What one class of waits costs a trip of rrt_rows_stream_kernel.  Needs a library patched by tools/instrument/rows_wait_stamps_patch.py
and built with -DAUVP_ROWS_WAIT_STAMPS=<class> (see there), loaded through AUVPLAN_LIBRARY: every episode's summary then carries
its wave's stamped shader-clock total in nn_scanned (unused in time-bin mode).  The headline batch, twice (the first batch with a
parameter block sizes the stream); one JSON line: cycles per wave and trip for the class, beside the stamped kernel's time.
Classes 1 .. 9 (the patch tool lists them; 8 = the selection tail, 9 = a steer pass's tail: profiles/rows_trip_lds.md).
usage: AUVPLAN_LIBRARY=... tools/rows_wait_probe.py <class> [episodes] [iterations]"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from auv_sim_amd import _lib  # noqa: E402
from bench_sides.common import RRT_KW, bench_world  # noqa: E402

cls = int(sys.argv[1])
E = int(sys.argv[2]) if len(sys.argv) > 2 else 12288
n_iter = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
world = bench_world(256, 200)
ctx = _lib.Context(0)
ctx.set_world(world["obstacles"], world["habitats"], world["polygon"], world["bins"], world["cells"], world["prob"])
init = np.zeros((E, 6))
init[:, 0], init[:, 1] = world["start"]
seeds = np.arange(E, dtype=np.uint64)
ctx.rrt_explore_batch(init, seeds, n_iter, **RRT_KW)
s = ctx.rrt_explore_batch(init, seeds, n_iter, **RRT_KW)
assert ctx.last_rrt_kernel() == "rrt_rows_stream_kernel", ctx.last_rrt_kernel()
# four episodes share a wave: a class stamped in wave-uniform control flow reports the same total in all four, one stamped under a
# row's own condition (the accepting path) reports each row's share -- the wave's figure is the largest of its four
per_wave = s["nn_scanned"].astype(np.float64)[: (E // 4) * 4].reshape(-1, 4).max(axis=1)
trips = s["iters_run"].astype(np.float64)[: (E // 4) * 4].reshape(-1, 4).max(axis=1)
print(json.dumps({"library": os.environ.get("AUVPLAN_LIBRARY", ""), "class": cls, "episodes": E, "iterations": n_iter,
                  "expand_ms": ctx.last_launch_parts()[0], "cycles_per_wave_and_trip": float((per_wave / trips).mean()),
                  "min": float((per_wave / trips).min()), "max": float((per_wave / trips).max()),
                  "nodes_per_episode": float(s["n_nodes"].mean())}))

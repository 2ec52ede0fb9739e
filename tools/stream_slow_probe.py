#!/usr/bin/env python3
"""How often does rrt_rows_stream_kernel's ring run dry?  Needs a library built with -DAUVP_STREAM_COUNT_SLOW=1
(python __graft_entry__.py variant exp/libauvplan_slow.so -DAUVP_STREAM_COUNT_SLOW=1), loaded through AUVPLAN_LIBRARY: the
kernel then reports every episode's slow-path entries of stream_ensure in the summary's nn_scanned (unused in time-bin mode).
The headline batch, twice (the first batch with a parameter block sizes the stream); one JSON line.
usage: AUVPLAN_LIBRARY=... tools/stream_slow_probe.py [episodes] [iterations]"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from auv_sim_amd import _lib  # noqa: E402
from bench_sides.common import RRT_KW, bench_world  # noqa: E402

E = int(sys.argv[1]) if len(sys.argv) > 1 else 12288
n_iter = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
world = bench_world(256, 200)
ctx = _lib.Context(0)
ctx.set_world(world["obstacles"], world["habitats"], world["polygon"], world["bins"], world["cells"], world["prob"])
init = np.zeros((E, 6))
init[:, 0], init[:, 1] = world["start"]
seeds = np.arange(E, dtype=np.uint64)
ctx.rrt_explore_batch(init, seeds, n_iter, **RRT_KW)
s = ctx.rrt_explore_batch(init, seeds, n_iter, **RRT_KW)
assert ctx.last_rrt_kernel() == "rrt_rows_stream_kernel", ctx.last_rrt_kernel()
slow = s["nn_scanned"].astype(np.float64)
print(json.dumps({"library": os.environ.get("AUVPLAN_LIBRARY", ""), "episodes": E, "iterations": n_iter, "mirror": ctx.last_stream_mirror(),
                  "expand_ms": ctx.last_launch_parts()[0], "slow_entries": float(slow.sum()), "slow_per_episode_mean": float(slow.mean()),
                  "slow_per_episode_max": float(slow.max()), "slow_per_1000_iterations": float(1000.0 * slow.sum() / s["iters_run"].sum())}))

#!/usr/bin/env python3
"""Randomised sweep of the paired A* kernel (astar_kernel<3, true>: a second wavefront per astar_fixLenSOG instance, the popped
node and eight neighbours' rows handed over through an LDS box) against the portable checker: random worlds, cell sizes (edge
tables in LDS / in memory), obstacle counts around the 256 kept in LDS, 1 .. 20 time bins, both velocities, starts on and off
the 10 m lattice, partial and full workgroups.  Every case runs twice paired (the relative speed of the two wavefronts differs
from launch to launch) and once on the one-wavefront kernel, on one context; every summary field, the expansion log, the
paths, the habitat list and the visited array of every instance (auvp_astar_get_visited) are compared bit for bit.  With a
diagnostic build (AUVPLAN_LIBRARY=auv_sim_amd/libauvplan_diag.so) AUVP_DIAG_JITTER delays the hand-overs of the searching
wavefronts ("2,4,0,U,seed") or of their partners ("2,4,1,U,seed") and AUVP_DIAG_SPIN makes the bounded waits run out: the
instances auvp_astar_batch searched again on the one-wavefront kernel are counted in the last line.
usage: python tests/experiments/soak_astar_pair.py <cases> <seed>

tests/test_gpu_astar_pair.py imports gpu_batch / checker / first_difference from here."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from auv_sim_amd import _astar_lib as al, _lib, synth  # noqa: E402
from oracle import orc_astar as oa  # noqa: E402
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import env_options  # noqa: E402  (tests/env_options.py: AUVP_<NAME> in os.environ steers live contexts -- this process only)
env_options.install()

VARIANT = "astar_fixLenSOG"
WEIGHTS = (0, 10, 10, 100)
WORLD_KEYS = ("obstacles", "habitats", "polygon", "bins", "cells", "prob")
STATUS_TO_CHECKER = {-1: -2, -2: -1}  # the C-ABI numbers capacity / argument errors the other way round from the checker
SCALARS = ("found", "n_nodes", "n_expansions", "n_children", "visited_count")
ARRAYS = ("path", "cost_list", "node_path", "smooth_path", "hab_left", "visited")


def gpu_batch(ctx, starts, limits, velocity=1.0, cap_nodes=20000):
    """one astar_fixLenSOG batch over ctx's world: run_batch's per-instance dicts with the expansion log, and the visited array
    of every instance read back with auvp_astar_get_visited (run_batch reads it only for an array the caller uploaded, which
    switches the pairing off)"""
    res = al.run_batch(ctx, VARIANT, starts, limits=limits, velocity=velocity, weights=WEIGHTS, cap_nodes=cap_nodes, exp_log=True)
    L = al._bind()
    for e, r in enumerate(res):
        vb = np.zeros((600, 600), dtype=np.uint8)
        ctx._chk(L.auvp_astar_get_visited(ctx.h, e, vb.ctypes.data_as(C.POINTER(C.c_uint8))))
        r["visited"] = vb
    return res


def checker(world, starts, limits, velocity=1.0, cap_nodes=20000, visited=None):
    """the portable checker, one search per start, each on a visited array of its own (zeros, or visited[e])"""
    zeros = np.zeros((600, 600), np.uint8)
    return [oa.run(VARIANT, starts[e], kind="portable", limit=float(limits[e]), velocity=velocity, weights=WEIGHTS,
                   cap_nodes=cap_nodes, visited=zeros if visited is None else visited[e], **{k: world[k] for k in WORLD_KEYS})
            for e in range(len(starts))]


def first_difference(r, o):
    """name of the first field in which a GPU result differs from the checker's (None: equal).  A declared error (the reference
    raises) is compared by its status and the expansions before it, as tests/test_gpu_astar_limits.py::_assert_same does: the
    reference has created some of the failing expansion's children by then, the kernel none."""
    if STATUS_TO_CHECKER.get(r["status"], r["status"]) != o["status"]:
        return "status (%d, checker %d)" % (r["status"], o["status"])
    if not np.array_equal(r["expansions"], o["expansions"]):
        return "expansions"
    if o["status"] != 0:
        return None
    for f in SCALARS:
        if r[f] != o[f]:
            return "%s (%s, checker %s)" % (f, r[f], o[f])
    for f in ARRAYS:
        if not np.array_equal(r[f], o[f]):
            return f
    return None


def same_results(a, b):
    """two GPU results of one search, every field (error exits included: both forms of the kernel leave at the same point)"""
    return all(a[f] == b[f] for f in ("status",) + SCALARS) and all(np.array_equal(a[f], b[f]) for f in ARRAYS + ("expansions",))


def launch_as_asked(ctx, paired):
    """the last batch ran on the kernel that was asked for: 512 threads per workgroup is the paired launch, 256 the one-wavefront
    kernel -- which a paired batch may end on only when the pipeline fallback redid it"""
    block, redone = ctx.last_launch()[1], ctx.pipeline_fallbacks()[0]
    if paired:
        return (block == 512 and redone == 0) or (block == 256 and redone > 0)
    return block == 256 and redone == 0


def draw_case(rng):
    cell = float(rng.choice([10.0, 14.0, 2.5]))       # 2.5: 2 * (80 + 80) edge entries do not fit ASTAR_LDS_GRID
    n_obst = int(rng.choice([0, 32, 256, 257, 600]))  # past 256 the obstacle arrays are read from memory
    n_bins = int(rng.choice([1, 8, 9, 20]))           # more than 8: the partner's `t0 = 8` loop
    velocity = float(rng.choice([1.0, 0.7]))
    E = int(rng.choice([1, 3, 4, 5, 8, 9]))
    limits = rng.integers(60, 201, E).astype(np.float64)
    # the bins end just past the largest time stamp a child can get (pathLen < limit + 10 sqrt 2), so the last ones are reached
    bin_len = int((limits.max() + 15.0) / velocity / n_bins) + 1
    # (14 m cells: a box of 15 x 15 of them, so that the cells cover the boundary polygon and their edges miss the 10 m lattice)
    box = (-305.0, -105.0, -95.0, 105.0) if cell == 14.0 else (-300.0, -100.0, -100.0, 100.0)
    world = synth.make_world(seed=int(rng.integers(1, 10_000)), n_obstacles=n_obst, box=box, cell=cell, n_bins=n_bins, bin_len=bin_len)
    starts = np.array([(-200.0 + 10.0 * rng.integers(-4, 5), 10.0 * rng.integers(-4, 5)) for _ in range(E)])
    offset = bool(rng.integers(0, 2))
    if offset:  # off the lattice: a step's squared length is no longer exactly 100 / 200 (the auvp_sqrt branch)
        starts = starts + rng.uniform(0.0, 10.0, (E, 2))
    label = "cell=%g O=%d T=%d v=%g E=%d offset=%d limits=%s world=%d" % (cell, n_obst, n_bins, velocity, E, offset,
                                                                          limits.astype(int).tolist(), world["seed"])
    return world, starts, limits, velocity, label


def main():
    n_cases, seed = int(sys.argv[1]), int(sys.argv[2])
    rng = np.random.default_rng(seed)
    ctx = _lib.Context(0)
    bad = fallbacks = n_inst = n_err = 0
    for c in range(n_cases):
        world, starts, limits, velocity, label = draw_case(rng)
        ctx.set_world(*[world[k] for k in WORLD_KEYS])
        ref = checker(world, starts, limits, velocity)
        n_inst += len(ref)
        n_err += sum(o["status"] != 0 for o in ref)
        why = None
        for run, pair in (("paired", 1), ("paired again", 1), ("one wavefront", 0)):
            ctx.set_option("ASTAR_PAIR", pair)
            res = gpu_batch(ctx, starts, limits, velocity)
            fallbacks += ctx.pipeline_fallbacks()[0]
            if not launch_as_asked(ctx, pair) and why is None:
                why = "%s: launched with %d threads per workgroup, %d redone" % (run, ctx.last_launch()[1], ctx.pipeline_fallbacks()[0])
            for e, (r, o) in enumerate(zip(res, ref)):
                d = first_difference(r, o)
                if d is not None and why is None:
                    why = "%s, instance %d: %s" % (run, e, d)
        if why is not None:
            bad += 1
            print("MISMATCH case %d (%s) %s" % (c, label, why))
    ctx.close()
    print("%d instances, %d of them declared errors in the checker too" % (n_inst, n_err))
    print("%d cases, %d mismatches, %d instances redone by the pipeline fallback" % (n_cases, bad, fallbacks))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

"""What the launch query says is what a handle launches (csrc/launch_plan.h: the handle's launches and
auvp_rrt_choose_launch / auvp_prrt_choose_launch go through the same functions; tests/test_launch_plan.py pins the rules).

Every kernel kind of RRT.exploring and Planner_RRT on one small batch each, asked for through options: the kernel name, the launch
geometry, the LDS bytes and the stream's form and length the handle reports equal the query's answer for the device's own CU
count and the same options -- and one episode per kind is checked against the portable checker, so that a launch of the wrong
shape cannot pass by its name."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E, N_ITER = 9, 200   # (a partial last workgroup / wavefront in every kind)
OFF = dict(ROWS=0, DUO=0, TRIO=0)
RRT_CASES = [  # kind, options, per-episode limits  (the stream first: no earlier batch of this context sizes it)
    ("rows_stream", dict(OFF, ROWS=1, ROWS_STREAM=1), False),
    ("rows", dict(OFF, ROWS=1, ROWS_STREAM=0), False),
    ("trio", dict(OFF, TRIO=1), False),
    ("trio", dict(OFF, TRIO=1, QUAD=0), False),
    ("duo", dict(OFF, DUO=1), False),
    ("explore", dict(OFF), False),
    ("explore_lim", dict(ROWS=1, TRIO=1), True),  # (whatever the options say)
]


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _obst_area(obstacles):
    x, y = obstacles[:, 0], obstacles[:, 1]
    a = (x.max() - x.min()) * (y.max() - y.min())
    return float(a) if len(obstacles) > 1 and math.isfinite(a) else 0.0


def test_rrt_exploring_launches_what_the_query_says(orc):
    from auv_sim_amd import _lib, synth
    world = synth.make_world(seed=1, n_obstacles=64)
    init = np.zeros((E, 6))
    init[:, 0], init[:, 1] = world["start"]
    init[:, 2] = np.linspace(-1.0, 1.0, E)
    seeds = np.arange(E, dtype=np.uint64) + 70
    w = orc.WorldArrays(world["obstacles"], world["habitats"], world["polygon"], world["bins"], world["cells"], world["prob"])
    e_ref = E - 1
    ref = orc.rrt_explore(w, int(seeds[e_ref]), N_ITER, init=init[e_ref], kind="portable")
    about = dict(n_cu=_n_cu(), max_iter=N_ITER, K=100, freq=30.0, dist_to_end=2.0, O=len(world["obstacles"]), H=len(world["habitats"]),
                 V=len(world["polygon"]), T=len(world["bins"]), obst_area=_obst_area(np.asarray(world["obstacles"], dtype=np.float64)))
    ctx = _lib.Context(0)
    seen = set()
    try:
        ctx.set_world(world["obstacles"], world["habitats"], world["polygon"], world["bins"], world["cells"], world["prob"])
        for kind, opts, lim in RRT_CASES:
            want = _lib.rrt_choose_launch(E, lim=lim, options=opts, **about)
            assert (want["status"], want["kind"]) == (0, kind), (kind, opts, want)
            for k, v in opts.items():
                ctx.set_option(k, v)
            try:
                summ = ctx.rrt_explore_batch(init, seeds, N_ITER, habitat_keep=[(1 << about["H"]) - 1] * E if lim else None)
                got = dict(name=ctx.last_rrt_kernel(), launch=ctx.last_launch(), mirror=ctx.last_stream_mirror(),
                           stream_len=ctx.last_stream_len(), redone=ctx.pipeline_fallbacks()[0])
                tree = ctx.tree(e_ref, summ[e_ref])
            finally:
                for k in opts:
                    ctx.set_option(k, None)
            assert got["redone"] == 0
            assert got["name"] == want["name"], (kind, got, want)
            assert got["launch"] == (want["grid"], want["block"], want["lds"]), (kind, got, want)
            assert got["mirror"] == (want["mirror"] if kind == "rows_stream" else -1), (kind, got, want)
            assert got["stream_len"] == want["stream_len"], (kind, got, want)
            if kind == "rows_stream":
                assert want["stream_len"] == (int(46.5 * N_ITER) + 4096 + 63) // 64 * 64 and want["stream_waves"] == 1
            # the geometry covers the batch: episodes per workgroup x workgroups
            per_wg = {"rows": want["block"] // 16, "rows_stream": want["block"] // 16, "trio": want["block"] // (256 if want["quad"] else 192),
                      "duo": want["block"] // 128}.get(kind, want["block"] // 64)
            assert (want["grid"] - 1) * per_wg < E <= want["grid"] * per_wg, (kind, want)
            s = summ[e_ref]
            assert (s["status"], s["n_nodes"], s["n_points"]) == (ref["status"], ref["n_nodes"], ref["n_points"]), kind
            assert s["rng_after"] == ref["rng_after"], kind
            assert np.array_equal(tree["parent"], ref["parent"]) and np.array_equal(tree["nodes"], ref["nodes"]), kind
            assert np.array_equal(tree["points"], ref["points"]), kind
            assert np.array_equal(np.array(s["best_cost"]), ref["best_cost"]), kind
            seen.add(want["name"])
    finally:
        ctx.close()
    assert seen == {"rrt_rows_stream_kernel", "rrt_rows_kernel", "rrt_trio_kernel<4 wavefronts>", "rrt_trio_kernel", "rrt_duo_kernel",
                    "rrt_explore_kernel", "rrt_explore_lim_kernel"}


PRRT_CASES = [  # kernel, draw wave, options
    ("prrt_kernel", 0, dict(PRRT_ROWS=0, PRRT_PIPE=0)),
    ("prrt_pipe_kernel", 1, dict(PRRT_ROWS=0, PRRT_PIPE=1)),
    ("prrt_pipe_kernel", 0, dict(PRRT_ROWS=0, PRRT_PIPE=1, PRRT_PIPE_DRAW=0)),
    ("prrt_rows_kernel", 0, dict(PRRT_ROWS=1, PRRT_LAT=0)),
]


def test_planner_rrt_launches_what_the_query_says():
    from auv_sim_amd import _lib, synth
    from auv_sim_amd._prrt_lib import PlannerBatch
    from oracle import orc_planner
    pw = synth.make_rect_world(seed=3, n_obstacles=64, size=100.0, start=(10.0, 10.0), goal=(85.0, 80.0), obst_radius=(2.0, 5.0),
                               origin=(-30.0, 12.5))
    PE, max_step, freq, cell, subs = 6, 100, 10, 5, 2
    starts = np.tile(np.array([pw["start"][0], pw["start"][1], 0.0, 0.0]), (PE, 1))
    starts[:, 2] = np.linspace(-2.0, 2.0, PE)
    goals = np.tile(pw["goal"], (PE, 1))
    pseeds = np.arange(PE, dtype=np.uint64) + 40
    pref = [orc_planner.planning(pw["obstacles"], pw["rect"], starts[e], goals[e], int(pseeds[e]), max_step, freq, cell, subs, kind="portable")
            for e in range(PE)]
    ctx = _lib.Context(0)
    try:
        ctx.set_world(obstacles=pw["obstacles"])
        for name, draw, opts in PRRT_CASES:
            for k, v in opts.items():
                ctx.set_option(k, v)
            try:
                pb = PlannerBatch(ctx, starts, goals, pw["rect"], max_step, seeds=pseeds, freq=freq, cell=cell, subs=subs)
                want = _lib.prrt_choose_launch(PE, n_cu=_n_cu(), O=len(pw["obstacles"]), freq=freq, max_step=max_step,
                                               n_buckets=pb.rows * pb.cols * pb.subs, options=opts)
                ps = pb.plan()
                got = (ctx.prrt_last_kernel(), ctx.last_launch(), ctx.pipeline_fallbacks()[0])
                trees = [pb.tree(e, ps[e]) for e in range(PE)]
            finally:
                for k in opts:
                    ctx.set_option(k, None)
            assert (want["status"], want["name"], want["draw_wave"]) == (0, name, draw), (opts, want)
            assert got == (want["name"], (want["grid"], want["block"], want["lds"]), 0), (got, want)
            assert want["grid"] == (1 if name == "prrt_rows_kernel" else PE)
            for e in range(PE):
                r = pref[e]
                assert (ps[e]["status"], ps[e]["steps"], ps[e]["n_nodes"]) == (0, r["steps"], r["n_nodes"]), (name, e)
                assert np.array_equal(trees[e]["nodes"], r["nodes"][:, :4]) and np.array_equal(trees[e]["node_bucket"], r["node_bucket"])
                assert ps[e]["rng_after"] == r["rng_after"]
    finally:
        ctx.close()

"""The time-bin append of the four-episode RRT kernels where it can go wrong: member lists that outgrow their direct-mapped head
(AUVP_BIN_HEAD = 128 members per bin) and go on in 64-entry chunks -- the chunk's index is written at a chunk crossing and read
back at every later append, and `bin_member` reads it again for every parent drawn from beyond the head.

Four time bins (max_traj_time 20, bin_interval 5), 64 obstacles, at 600 and at 1 800 iterations.  Nearly every iteration accepts a
node, but a node whose time stamp lies past the horizon joins no list: at 600 iterations the longest list of an episode has 55
to 94 members (printed by the test) and stays inside its head -- that case checks the head's own appends and the equalities --
and it takes the 1 800-iteration case to get what this file is about: there the test asserts on the reported bin sizes that
every episode has lists beyond the head and that lists cross a chunk boundary (more than 128 + 64 members).

rrt_rows_stream_kernel, rrt_rows_kernel and the one-episode kernel (which appends through the shared helper of
rrt_explore_kernel.h) must agree bit for bit: every summary field, every node record and path point, the size of every bin.
The library has no accessor for the member lists themselves; they are compared through what they decide: every parent is the
member at a uniformly drawn index of a drawn bin, so a member stored in or read from a wrong slot is a different `parent`
array (one draw per iteration, in the long case most of them from lists beyond their head).  The portable checker, which keeps
plain lists, is run on a sample.

A run of 1 800 iterations that ends in status -2 (point capacity: a points_per_iter below what the steers append) stops the
episodes after their lists have passed the head; the three kernels report the same stop and the same tree up to it (the checker
has no capacities)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(max_traj_time=20.0, bin_interval=5)
N_ITERS = (600, 1800)
HEAD, CHUNK = 128, 64
FORMS = {"rrt_rows_stream_kernel": dict(ROWS=1, ROWS_STREAM=1, DUO=0, TRIO=0),
         "rrt_rows_kernel": dict(ROWS=1, ROWS_STREAM=0, DUO=0, TRIO=0),
         "rrt_explore_kernel": dict(ROWS=0, DUO=0, TRIO=0)}
TREE_KEYS = ("nodes", "parent", "pt_off", "pt_cnt", "points")
# (E, ROWS_WG_WAVES or None for the host's choice)
SHAPES = [(8, None), (96, 2), (96, 12)]


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(ctx):
    from auv_sim_amd import synth
    w = synth.make_world(seed=1, n_obstacles=64)
    ctx.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"])
    return w


def _batch(world, E):
    init = np.zeros((E, 6))
    init[:, 0], init[:, 1] = world["start"]
    init[:, 2] = np.linspace(-3.0, 3.0, E)
    return init, np.arange(7300, 7300 + E, dtype=np.uint64)


def _run(ctx, form, waves, init, seeds, n_iter, **kw):
    opts = dict(FORMS[form])
    if waves is not None and form != "rrt_explore_kernel":
        opts["ROWS_WG_WAVES"] = waves
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        summ = ctx.rrt_explore_batch(init, seeds, n_iter, **kw).copy()
        assert ctx.last_rrt_kernel() == form and ctx.pipeline_fallbacks()[0] == 0, (ctx.last_rrt_kernel(), form)
        if waves is not None and form != "rrt_explore_kernel":
            assert ctx.last_launch()[1] == 64 * waves
        E = len(init)
        return dict(summ=summ, trees=[ctx.tree(e, summ[e]) for e in range(E)], bins=[ctx.bin_sizes(e) for e in range(E)])
    finally:
        for k in opts:
            ctx.set_option(k, None)


def _same(a, b, what):
    failed = a["summ"]["status"] < 0
    for f in a["summ"].dtype.names:
        if f == "n_candidates":  # (a diagnostic of the cull, which the one-episode kernel makes with another box)
            continue
        # (an episode stopped by a capacity error reports where it stopped; its stream position there depends on how the kernel
        # cuts a steer into passes and is not part of the contract: tests/test_gpu_rows_kernel.py)
        keep = ~failed if f in ("rng_after", "n_draw32") else np.ones(len(failed), bool)
        assert np.array_equal(a["summ"][f][keep], b["summ"][f][keep]), (what, f)
    for e, (ta, tb) in enumerate(zip(a["trees"], b["trees"])):
        for k in TREE_KEYS:
            assert np.array_equal(ta[k], tb[k]), (what, e, k)
        assert np.array_equal(a["bins"][e], b["bins"][e]), (what, e)


@pytest.mark.parametrize("n_iter", N_ITERS)
@pytest.mark.parametrize("E,waves", SHAPES)
def test_lists_beyond_the_head_and_over_chunk_boundaries(ctx, orc, world, E, waves, n_iter):
    init, seeds = _batch(world, E)
    got = {form: _run(ctx, form, waves, init, seeds, n_iter, **KW) for form in FORMS}
    first = got["rrt_rows_stream_kernel"]
    assert (first["summ"]["status"] >= 0).all()
    largest = np.array([b.max() for b in first["bins"]])
    print("largest list per episode:", largest.tolist())
    if n_iter == 1800:
        assert (largest > HEAD).all()               # every episode appends (and draws parents) beyond the direct-mapped head
        assert (largest > HEAD + CHUNK).any()       # ... and some lists go on into a second chunk
        # more than one list of an episode beyond the head: their chunks interleave in the episode's chunk pool
        assert any((b > HEAD).sum() >= 2 for b in first["bins"])
    for form in ("rrt_rows_kernel", "rrt_explore_kernel"):
        _same(first, got[form], form)
    # n_candidates: the two four-episode kernels share the cull
    assert np.array_equal(first["summ"]["n_candidates"], got["rrt_rows_kernel"]["summ"]["n_candidates"])
    w = orc.WorldArrays(world["obstacles"], world["habitats"], world["polygon"], world["bins"], world["cells"], world["prob"])
    for e in sorted({0, 3, E // 2, E - 1}):   # (the last episode: row 3 of the last live wave)
        r = orc.rrt_explore(w, int(seeds[e]), n_iter, init=init[e], kind="portable", **KW)
        s, t = first["summ"][e], first["trees"][e]
        assert (s["status"], s["n_nodes"], s["n_points"], s["n_leaves"]) == (r["status"], r["n_nodes"], r["n_points"], r["n_leaves"]), e
        assert s["rng_after"] == r["rng_after"] and int(s["n_draw32"]) == int(r["n_draw32"]), e
        for k in TREE_KEYS:
            assert np.array_equal(t[k], r[k]), (e, k)
        assert np.array_equal(first["bins"][e], r["bin_sizes"]), e


def test_capacity_error_after_the_lists_passed_the_head(ctx, world):
    E, n_iter = 8, 1800
    init, seeds = _batch(world, E)
    # an accepted node keeps some 10 points here and nearly every iteration accepts one: 6 per iteration run out after about
    # 1 100 nodes, when the longest lists have some 170 members
    kw = dict(KW, points_per_iter=6.0)
    got = {form: _run(ctx, form, None, init, seeds, n_iter, **kw) for form in FORMS}
    first = got["rrt_rows_stream_kernel"]
    print("status", first["summ"]["status"].tolist(), "n_nodes", first["summ"]["n_nodes"].tolist())
    assert (first["summ"]["status"] == -2).all()
    assert (first["summ"]["iters_run"] < n_iter).all()
    assert all(b.max() > HEAD for b in first["bins"])   # the stop came after the lists had passed the head
    for form in ("rrt_rows_kernel", "rrt_explore_kernel"):
        _same(first, got[form], form)

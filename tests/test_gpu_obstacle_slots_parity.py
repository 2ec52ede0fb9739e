"""The obstacle slot tables grouped by median splits (csrc/world_tables.h: build_obstacle_slots) under the kernels that read them:
rrt_rows_kernel and both ring forms of rrt_rows_stream_kernel against rrt_explore_kernel, which reads the obstacles in list order
and no slot table; and one Planner_RRT batch on prrt_rows_kernel against the checker.  A slot's box is only a prefilter, so every
summary field, node record and path point must be rrt_explore_kernel's, bit for bit, however the slots are grouped.

Shape, as tests/test_gpu_rows_theta_parity.py: E = 9 (three wavefronts, the last with one live row), 400 iterations, freq = 30 and
freq = 8; both instances of the cull (option TIGHT_CULL = 1 / 0, set for the reference as well).

Worlds in which collisions are frequent, so that the exact test behind the prefilter decides trees: the boundary lies so far out
that a rejected steer was rejected by a collision, and an iteration in four and more ends without a node (asserted below; the
checker puts the accepted share at 0.2 - 0.7 per batch, under 0.9 in every episode):
  dense  256 obstacles of radius 2 - 6 m round the start (the world of tests/test_gpu_rows_thresholds.py)
  few    17 obstacles of radius up to 14 m in a ring 18 - 50 m round the start: two slots of the Z-curve runs, 16 groups of
         one or two under the median split
  line   255 obstacles of radius 3 - 7 m, 40 of them on the first split's line (ties across the cut), 20 duplicates of others

n_candidates (obstacles that passed the cull) is compared too: with the cull instance set alike for both, the one-episode kernel
tests an obstacle's cull square against the same box (the reach square, or the tight box of the steer's points), and a slot's box
holds the cull squares of its obstacles, so the four-episode kernels must let exactly the same obstacles through."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TREE_KEYS = ("nodes", "parent", "pt_off", "pt_cnt", "points")
E, N_ITER = 9, 400
GROW = 150.0   # how far the boundary lies outside the obstacles' box: a steer moves less than freq x dist_to_end = 60 m


def make_world(name):
    from auv_sim_amd import synth
    seed, n, radius = {"dense": (71, 256, (2.0, 6.0)), "few": (72, 17, (8.0, 14.0)), "line": (73, 255, (3.0, 7.0))}[name]
    w = synth.make_world(seed=seed, n_obstacles=n, obst_radius=radius)
    x0, y0, x1, y1 = w["box"]
    w["polygon"] = np.array([(x0 - GROW, y0 - GROW), (x1 + GROW, y0 - GROW), (x1 + GROW, y1 + GROW), (x0 - GROW, y1 + GROW)])
    if name == "few":
        # the 17 drawn close round the start: a ring of centres 18 - 50 m from it (none within its radius + 5 m of the start)
        rng = np.random.default_rng(72)
        ob, (sx, sy) = w["obstacles"], w["start"]
        d, a = rng.uniform(18.0, 50.0, n), rng.uniform(0.0, 2.0 * np.pi, n)
        ob[:, 0], ob[:, 1] = sx + d * np.cos(a), sy + d * np.sin(a)
        ob[:, 2] = np.minimum(ob[:, 2], d - 5.0)
    if name == "line":
        ob = w["obstacles"]
        ob[200:220] = ob[20:40]                       # 20 duplicates
        xm = float(np.median(ob[:, 0]))
        ob[100:140, 0] = xm                           # 40 on one vertical line, where the first split cuts
        sx, sy = w["start"]
        near = (np.abs(ob[:, 0] - sx) < 12.0) & (np.abs(ob[:, 1] - sy) < 12.0)
        ob[near, 1] += 30.0                           # (none on top of the start)
        below = int((ob[:, 0] < xm).sum())
        assert below < 128 < below + int((ob[:, 0] == xm).sum())   # the cut at ceil(255 / 2) runs through the ties
    return w


def _run(ctx, init, seeds, options, **kw):
    for k, v in options.items():
        ctx.set_option(k, v)
    try:
        summ = ctx.rrt_explore_batch(init, seeds, N_ITER, **kw).copy()
        return dict(summ=summ, kernel=ctx.last_rrt_kernel(), mirror=ctx.last_stream_mirror(), redone=ctx.pipeline_fallbacks()[0],
                    trees=[ctx.tree(e, summ[e]) for e in range(E)], paths=ctx.paths(summ))
    finally:
        for k in options:
            ctx.set_option(k, None)


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=["dense", "few", "line"])
def world(ctx, request):
    w = make_world(request.param)
    ctx.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"])
    return request.param, w


@pytest.fixture(scope="module", params=[(30, 1), (30, 0), (8, 1), (8, 0)], ids=["freq30-tight", "freq30-plain", "freq8-tight", "freq8-plain"])
def reference(ctx, world, request):
    """the batch on rrt_explore_kernel, once per world, freq and cull"""
    name, w = world
    freq, tight = request.param
    init = np.zeros((E, 6))
    init[:, 0], init[:, 1] = w["start"]
    init[:, 2] = np.linspace(-3.0, 3.0, E)
    seeds = np.arange(8300, 8300 + E, dtype=np.uint64) * 7
    ref = _run(ctx, init, seeds, dict(ROWS=0, DUO=0, TRIO=0, TIGHT_CULL=tight), freq=freq)
    s = ref["summ"]
    assert ref["kernel"].startswith("rrt_explore_kernel") and (s["status"] >= 0).all()
    rate = (s["n_nodes"] - 1) / s["iters_run"]
    print("%s freq %d: accepted steers per iteration %s" % (name, freq, np.round(rate, 3).tolist()))
    assert (s["n_nodes"] > 20).all() and (rate < 0.9).all() and rate.mean() < 0.75, (name, freq, s["n_nodes"].tolist())
    return name, freq, tight, init, seeds, ref


@pytest.mark.parametrize("form", ["classic", "mirrored", "masked"])
def test_the_four_episode_kernels_equal_the_one_episode_kernel(ctx, reference, form):
    name, freq, tight, init, seeds, ref = reference
    cap = int(ref["summ"]["n_draw32"].max()) // 2 + 64     # a stream as long as the busiest episode needs
    options = {"classic": dict(ROWS=1, DUO=0, TRIO=0, ROWS_STREAM=0),
               "mirrored": dict(ROWS=1, DUO=0, TRIO=0, ROWS_STREAM=1, ROWS_STREAM_CAP=cap, ROWS_STREAM_MIRROR=1),
               "masked": dict(ROWS=1, DUO=0, TRIO=0, ROWS_STREAM=1, ROWS_STREAM_CAP=cap, ROWS_STREAM_MIRROR=0)}[form]
    got = _run(ctx, init, seeds, dict(options, TIGHT_CULL=tight), freq=freq)
    want = {"classic": ("rrt_rows_kernel", -1), "mirrored": ("rrt_rows_stream_kernel", 1), "masked": ("rrt_rows_stream_kernel", 0)}[form]
    assert (got["kernel"], got["mirror"]) == want and got["redone"] == 0, (got["kernel"], got["mirror"], got["redone"])
    print("%s freq %d %s %s: n_candidates %s" % (name, freq, "tight" if tight else "plain", form, got["summ"]["n_candidates"].tolist()))
    for f in got["summ"].dtype.names:
        assert np.array_equal(got["summ"][f], ref["summ"][f]), f
    assert got["summ"]["n_candidates"].sum() > 0
    for e in range(E):
        for k in TREE_KEYS:
            assert np.array_equal(got["trees"][e][k], ref["trees"][e][k]), (e, k)
        assert np.array_equal(got["paths"][e], ref["paths"][e]), e


@pytest.fixture
def planner_ctx():
    """a context of its own: the module's keeps the world of the parametrised tests round it"""
    from auv_sim_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def test_planner_rows_kernel_on_a_dense_world_equals_the_checker(planner_ctx, orc):
    """prrt_rows_kernel reads the same slot tables: five episodes, freq 3, planning(150) -- the smallest shape of
    tests/test_gpu_planner_rows.py -- in 256 obstacles of radius 2 - 5 m on 200 m x 200 m, every episode against the checker"""
    from auv_sim_amd import synth
    from auv_sim_amd._prrt_lib import PlannerBatch
    from oracle import orc_planner as op
    ctx = planner_ctx
    w = synth.make_rect_world(seed=3, n_obstacles=256, obst_radius=(2.0, 5.0))
    ctx.set_world(obstacles=w["obstacles"])
    n_ep, freq, max_step = 5, 3, 150
    rng = np.random.default_rng(n_ep)
    starts = np.tile(np.array([w["start"][0], w["start"][1], 0.0, 0.0]), (n_ep, 1))
    starts[:, 2] = rng.uniform(-3.0, 3.0, n_ep)
    goals = np.column_stack([rng.uniform(w["rect"][0] + 5, w["rect"][2] - 5, n_ep), rng.uniform(w["rect"][1] + 5, w["rect"][3] - 5, n_ep)])
    seeds = np.arange(n_ep, dtype=np.uint64) + 11
    opts = dict(PRRT_ROWS=1, PRRT_LAT=0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        pb = PlannerBatch(ctx, starts, goals, w["rect"], max_step, seeds=seeds, freq=freq, cell=5, subs=2)
        s = pb.plan().copy()
    finally:
        for k in opts:
            ctx.set_option(k, None)
    assert ctx.prrt_last_kernel() == "prrt_rows_kernel"
    assert s["n_nodes"].sum() < 0.95 * s["steps"].sum()   # steers were rejected: the exact test decided
    for e in range(n_ep):
        r = op.planning(w["obstacles"], w["rect"], starts[e], goals[e], int(seeds[e]), max_step, freq, 5, 2, kind="portable")
        t = pb.tree(e, s[e])
        assert (s[e]["status"], s[e]["steps"], bool(s[e]["done"]), s[e]["n_nodes"], s[e]["n_points"]) == \
            (0, r["steps"], bool(r["done"]), r["n_nodes"], r["n_points"]), e
        assert np.array_equal(t["nodes"], r["nodes"][:, :4]) and np.array_equal(t["node_bucket"], r["node_bucket"]), e
        assert s[e]["rng_after"] == r["rng_after"], e

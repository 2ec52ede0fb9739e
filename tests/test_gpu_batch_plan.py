"""The refusals of csrc/batch_plan.h through a live handle: batches whose sizing used to be undefined (a NaN horizon, an infinite
freq, INT_MAX iterations, a buffer past 2^62 bytes) raise AuvpError with the ARG code and change nothing -- the handle's prepared
batch still runs, and the next batch on it equals, bit for bit, the same batch on a fresh handle.  bin_sizes() reports the plan's K.

The plans themselves (every capacity, by hand) are tests/test_batch_plan_host.py's; this file only needs small batches."""
import ctypes as C
import math

import numpy as np
import pytest

from auv_sim_amd import _lib, _prrt_lib, synth

pytestmark = pytest.mark.gpu

ERR_ARG = -1
INT_MAX = 2147483647
E, N_ITER = 3, 60


@pytest.fixture(scope="module")
def world():
    return synth.make_world(seed=1, n_obstacles=64)


def new_context(world):
    ctx = _lib.Context(0)
    ctx.set_world(world["obstacles"], world["habitats"], world["polygon"], world["bins"], world["cells"], world["prob"])
    return ctx


def rrt_inputs(world):
    init = np.zeros((E, 6))
    init[:, 0], init[:, 1] = world["start"]
    return init, np.arange(E, dtype=np.uint64) + 11


def rrt_results(ctx, world, **kw):
    init, seeds = rrt_inputs(world)
    ctx.set_world(world["obstacles"], world["habitats"], world["polygon"], world["bins"], world["cells"], world["prob"])
    summ = ctx.rrt_explore_batch(init, seeds, N_ITER, **kw)
    return summ, ctx.paths(summ)


def assert_same_rrt(got, want):
    """(summaries, courses) of a batch, RRT.exploring's or the planner's: every field, every byte"""
    assert all(np.array_equal(got[0][n], want[0][n], equal_nan=True) for n in want[0].dtype.names)
    assert len(got[1]) == len(want[1]) and all(a.tobytes() == b.tobytes() for a, b in zip(got[1], want[1]))


@pytest.fixture(scope="module")
def fresh_rrt(world):
    """the batch every handle must still run after a refusal, from a handle that has seen nothing else"""
    out = rrt_results(new_context(world), world)
    assert (out[0]["status"] >= 0).all() and (out[0]["n_nodes"] > 10).all()
    return out


RRT_REFUSALS = [
    (dict(max_traj_time=math.nan), "max_traj_time / bin_interval"),
    (dict(max_traj_time=1.1e10), "max_traj_time / bin_interval"),
    (dict(max_traj_time=1.0, bin_interval=1e-300), "max_traj_time / bin_interval"),
    (dict(freq=math.inf), "freq"),
    (dict(freq=1e300), "freq"),
    (dict(n_iter=INT_MAX), "max_iter"),
    (dict(points_per_iter=math.nan), "points_per_iter"),
    (dict(n_iter=1000000, freq=1000.0, n_episodes=INT_MAX), "points"),
    (dict(max_traj_time=[3.0e10, 5.0, 5.0], bin_interval=10.0), "episode 0: max_traj_time / bin_interval"),
]


def refused_prepare(ctx, world, n_iter=N_ITER, n_episodes=None, **kw):
    init, seeds = rrt_inputs(world)
    if n_episodes is None:
        return ctx.rrt_prepare(init, seeds, n_iter, **kw)
    # (more episodes than there are inputs: the sizes are refused before a single input is read)
    p = _lib.RRTParams()
    p.dist_to_end, p.diff_max, p.freq, p.min_dist, p.bin_interval, p.v, p.max_traj_time = 2.0, 0.5, float(kw.get("freq", 30)), 0.5, 5.0, 2.0, 500.0
    p.max_plan_time, p.mode, p.max_iter, p.points_per_iter = float(n_iter), _lib.MODES["timebin"], int(n_iter), 0.0
    return ctx._chk(ctx.L.auvp_rrt_prepare(ctx.h, n_episodes, _lib._p(init), seeds.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(p), 0))


@pytest.fixture(scope="module")
def shared_context(world):
    """one handle for every refusal of this file: each is followed by the batch a fresh handle ran, so none may leave a trace"""
    return new_context(world)


@pytest.mark.parametrize("kw, names", RRT_REFUSALS)
def test_rrt_refusal_names_the_field_and_leaves_the_handle_as_it_was(shared_context, world, fresh_rrt, kw, names):
    ctx = shared_context
    init, seeds = rrt_inputs(world)
    ctx.set_world(world["obstacles"], world["habitats"], world["polygon"], world["bins"], world["cells"], world["prob"])
    ctx.rrt_prepare(init, seeds, N_ITER)
    with pytest.raises(_lib.AuvpError) as err:
        refused_prepare(ctx, world, **kw)
    assert err.value.code == ERR_ARG and names in str(err.value), str(err.value)
    ctx.rrt_run()                # the batch prepared before the refusal is still the handle's
    summ = ctx.summaries()
    assert_same_rrt((summ, ctx.paths(summ)), fresh_rrt)
    assert_same_rrt(rrt_results(ctx, world), fresh_rrt)


def test_refusals_there_have_always_been_keep_their_messages(shared_context, world, fresh_rrt):
    ctx = shared_context
    for kw, message in ((dict(max_traj_time=5242881.0), "too many time bins (1048577)"), (dict(points_per_iter=1.0e9), "point capacity too large"),
                        (dict(n_iter=2000000, max_traj_time=5242880.0), "time-bin lists too large (K=1048576, max_iter=2000000)"),
                        (dict(freq=-1.0), "bad params"), (dict(bin_interval=0.0), "bin_interval <= 0")):
        with pytest.raises(_lib.AuvpError) as err:
            refused_prepare(ctx, world, **kw)
        assert err.value.code == ERR_ARG and str(err.value).endswith(": " + message), str(err.value)
    assert_same_rrt(rrt_results(ctx, world), fresh_rrt)


def test_bin_sizes_report_the_plans_k(shared_context, world):
    ctx = shared_context
    summ, _ = rrt_results(ctx, world, max_traj_time=52.0, bin_interval=7.0)      # K = ceil(52 / 7)
    assert (summ["status"] >= 0).all()
    for e in range(E):
        assert len(ctx.bin_sizes(e)) == 8
    summ, _ = rrt_results(ctx, world, max_traj_time=[52.0, 7.0, 7.5], bin_interval=7.0)
    assert (summ["status"] >= 0).all() and [len(ctx.bin_sizes(e)) for e in range(E)] == [8, 1, 2]


# ---- Planner_RRT ------------------------------------------------------------------------------------------------------------------

RECT = (0.0, 0.0, 100.0, 100.0)


def planner_inputs():
    starts = np.tile(np.array([10.0, 10.0, 0.0, 0.0]), (E, 1))
    starts[:, 2] = np.linspace(-1.0, 1.0, E)
    return starts, np.tile(np.array([85.0, 80.0]), (E, 1)), np.arange(E, dtype=np.uint64) + 40


def planner_results(ctx, pworld):
    ctx.set_world(obstacles=pworld["obstacles"])
    starts, goals, seeds = planner_inputs()
    pb = _prrt_lib.PlannerBatch(ctx, starts, goals, RECT, N_ITER, seeds=seeds, freq=10, cell=5, subs=2)
    summ = pb.plan()
    return summ, pb.paths(summ)


@pytest.fixture(scope="module")
def pworld():
    return synth.make_rect_world(seed=3, n_obstacles=64, size=100.0, start=(10.0, 10.0), goal=(85.0, 80.0), obst_radius=(2.0, 5.0))


@pytest.fixture(scope="module")
def fresh_planner(pworld):
    out = planner_results(_lib.Context(0), pworld)
    assert (out[0]["status"] >= 0).all() and (out[0]["n_nodes"] > 5).all()
    return out


def refused_planner(ctx, rect=RECT, cell=5.0, max_step=N_ITER, freq=10.0, n_episodes=E):
    """auvp_prrt_create_batch itself: PlannerBatch takes int() of the rect and the cell first, which raises on its own for nan / inf"""
    starts, goals, seeds = planner_inputs()
    p = _prrt_lib.PrrtParams()
    for i in range(4):
        p.rect[i] = float(rect[i])
    p.exp_rate, p.dist_to_end, p.diff_max, p.freq, p.cell_side_length, p.subsections, p.max_step = 1.0, 2.0, 0.5, float(freq), float(cell), 2, max_step
    L = _prrt_lib._bind()
    return ctx._chk(L.auvp_prrt_create_batch(ctx.h, n_episodes, _lib._p(starts), _lib._p(goals), C.byref(p),
                                             seeds.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, 0))


@pytest.mark.parametrize("kw, names", [
    (dict(cell=math.nan), "cell_side_length"), (dict(cell=math.inf), "cell_side_length"), (dict(cell=3.0e9), "cell_side_length"),
    (dict(rect=(0.0, 0.0, math.inf, 100.0)), "rect"), (dict(rect=(0.0, math.nan, 100.0, 100.0)), "rect"),
    (dict(rect=(-2.0e9, 0.0, 2.0e9, 100.0)), "rect"),
    (dict(freq=math.inf), "freq"), (dict(max_step=INT_MAX), "max_step"),
    (dict(n_episodes=INT_MAX, max_step=1 << 23, freq=200.0), "points"),
])
def test_planner_refusal_names_the_field_and_leaves_the_handle_as_it_was(shared_context, pworld, fresh_planner, kw, names):
    ctx = shared_context
    ctx.set_world(obstacles=pworld["obstacles"])
    starts, goals, seeds = planner_inputs()
    pb = _prrt_lib.PlannerBatch(ctx, starts, goals, RECT, N_ITER, seeds=seeds, freq=10, cell=5, subs=2)
    with pytest.raises(_lib.AuvpError) as err:
        refused_planner(ctx, **kw)
    assert err.value.code == ERR_ARG and names in str(err.value), str(err.value)
    summ = pb.plan()             # the batch created before the refusal is still the handle's
    assert_same_rrt((summ, pb.paths(summ)), fresh_planner)
    assert_same_rrt(planner_results(ctx, pworld), fresh_planner)

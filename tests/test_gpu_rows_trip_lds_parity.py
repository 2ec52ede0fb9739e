"""The three kernels built from rrt_rows_body.h -- rrt_rows_kernel, rrt_rows_stream_kernel with the mirrored ring and with the
masked one -- take a steer pass's end state (x, y, t, length, theta) from the ends of the pass's five chains (rows_sums_chain /
rows_pass_ends_dpp, auv_sim_amd/csrc/rrt_rows_kernel.h: lanes past the pass's n sub-arcs add -0.0, entry 15 of an LDS row is never
added) instead of reading the prefix values of sub-arc n - 1 back.  rrt_explore_kernel (one episode per wavefront) uses none of
it.  The shape of tests/test_gpu_rows_theta_parity.py: E = 9 (three wavefronts, the last with one live row), 400 iterations; every
summary field, node record and path point must be rrt_explore_kernel's, bit for bit (n_candidates as there: a diagnostic of the
cull box, which differs by design).  freq:
  30  most steers take the second pass;
   8  none does;
  17  a steer has 0 .. 16 sub-arcs: the second pass runs with n = 1, its last sub-arc on lane 0;
  16  a steer has 0 .. 15 sub-arcs: the second pass never runs, the first one can be full (n = 15, last sub-arc on lane 14).
What the reference run shows of the second pass is asserted: accepted steers of more than 15 points (freq 30), none above 7 (freq
8).  At freq 17 and 16 the accepted steers do not tell (a steer of 16 points is rare and the ones here are rejected), so the
witness is the CPU checker's record of every iteration's path on the same episodes -- after its node counts are held against the
reference run's: a path of 17 (16 points + the parent's end) at freq 17, paths of 16 and none longer at freq 16.
The first iterations of every episode have one non-empty time bin of K: selections of several rounds, with winners at every try
0 .. 13 of a round.  n_draw32 (compared like every field, and once more by name) pins the stream position after every selection
and pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TREE_KEYS = ("nodes", "parent", "pt_off", "pt_cnt", "points")
E, N_ITER = 9, 400


def _world():
    from auv_sim_amd import synth
    return synth.make_world(seed=51, n_obstacles=64)


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    c = _lib.Context(0)
    w = _world()
    c.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"])
    yield c
    c.close()


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


def _checker_paths(init, seeds, freq):
    """len(new.path) of every iteration and the node count, per episode, from the CPU checker"""
    from oracle import orc
    w = _world()
    wa = orc.WorldArrays(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"])
    runs = [orc.rrt_explore(wa, int(seeds[e]), N_ITER, init=init[e], freq=freq, kind="portable") for e in range(E)]
    return np.array([r["it_npath"].max() for r in runs]), np.array([r["n_nodes"] for r in runs])


@pytest.fixture(scope="module", params=[30, 8, 17, 16])
def reference(ctx, request):
    """the batch on rrt_explore_kernel, once per freq"""
    freq = request.param
    init = np.zeros((E, 6))
    init[:, 0], init[:, 1] = _world()["start"]
    init[:, 2] = np.linspace(-3.0, 3.0, E)
    seeds = np.arange(7100, 7100 + E, dtype=np.uint64) * 13
    ref = _run(ctx, init, seeds, dict(ROWS=0, DUO=0, TRIO=0), freq=freq)
    assert ref["kernel"].startswith("rrt_explore_kernel") and (ref["summ"]["status"] >= 0).all()
    assert (ref["summ"]["n_nodes"] > 100).all()
    most = np.array([t["pt_cnt"].max() for t in ref["trees"]])
    if freq == 30:
        assert (most > 15).all(), most      # the second pass ran in every episode
    elif freq == 8:
        assert (most < 8).all(), most       # it cannot
    else:
        longest, nodes = _checker_paths(init, seeds, freq)
        assert np.array_equal(nodes, ref["summ"]["n_nodes"])    # (the checker ran what the reference ran)
        if freq == 17:
            assert longest.max() == 17, longest         # a steer of 16 sub-arcs, all taken: the second pass ran with n = 1
        else:
            assert longest.max() == 16, longest         # a full first pass (n = 15), and never a second one
        assert (most <= 15).all(), most
    return freq, init, seeds, ref


@pytest.mark.parametrize("form", ["classic", "mirrored", "masked"])
def test_the_four_episode_kernels_equal_the_one_episode_kernel(ctx, reference, form):
    freq, init, seeds, ref = reference
    cap = int(ref["summ"]["n_draw32"].max()) // 2 + 64     # a stream as long as the busiest episode needs
    options = {"classic": dict(ROWS=1, DUO=0, TRIO=0, ROWS_STREAM=0),
               "mirrored": dict(ROWS=1, DUO=0, TRIO=0, ROWS_STREAM=1, ROWS_STREAM_CAP=cap, ROWS_STREAM_MIRROR=1),
               "masked": dict(ROWS=1, DUO=0, TRIO=0, ROWS_STREAM=1, ROWS_STREAM_CAP=cap, ROWS_STREAM_MIRROR=0)}[form]
    got = _run(ctx, init, seeds, options, freq=freq)
    want = {"classic": ("rrt_rows_kernel", -1), "mirrored": ("rrt_rows_stream_kernel", 1), "masked": ("rrt_rows_stream_kernel", 0)}[form]
    assert (got["kernel"], got["mirror"]) == want and got["redone"] == 0, (got["kernel"], got["mirror"], got["redone"])
    assert np.array_equal(got["summ"]["n_draw32"], ref["summ"]["n_draw32"])
    for f in got["summ"].dtype.names:
        if f == "n_candidates":
            assert (got["summ"][f] <= ref["summ"][f]).all()
            continue
        assert np.array_equal(got["summ"][f], ref["summ"][f]), f
    for e in range(E):
        for k in TREE_KEYS:
            assert np.array_equal(got["trees"][e][k], ref["trees"][e][k]), (e, k)
        assert np.array_equal(got["paths"][e], ref["paths"][e]), e

"""The three kernels built from rrt_rows_body.h -- rrt_rows_kernel, rrt_rows_stream_kernel with the mirrored ring and with the
masked one -- take a steer pass's angles from rows_theta_chain_dpp; rrt_explore_kernel (one episode per wavefront) does not use
the helper.  The smallest batch that runs both steer passes and a part-filled wavefront: E = 9 (three wavefronts, the last with one
live row), 400 iterations, freq = 30 (most steers take the second pass) and freq = 8 (none does).  Every summary field, node record
and path point must be rrt_explore_kernel's, bit for bit.  (n_candidates is a diagnostic of the cull box, which differs between the
four-episode kernels and the one-episode kernel by design: tests/test_gpu_rows_kernel.py.)"""
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


@pytest.fixture(scope="module", params=[30, 8])
def reference(ctx, request):
    """the batch on rrt_explore_kernel, once per freq"""
    freq = request.param
    init = np.zeros((E, 6))
    init[:, 0], init[:, 1] = _world()["start"]
    init[:, 2] = np.linspace(-3.0, 3.0, E)
    seeds = np.arange(7100, 7100 + E, dtype=np.uint64) * 13
    ref = _run(ctx, init, seeds, dict(ROWS=0, DUO=0, TRIO=0), freq=freq)
    assert ref["kernel"].startswith("rrt_explore_kernel") and (ref["summ"]["status"] >= 0).all()
    # freq = 30: accepted steers that left more than 15 points (so the second pass ran) in every episode; freq = 8: none can
    most = np.array([t["pt_cnt"].max() for t in ref["trees"]])
    assert (ref["summ"]["n_nodes"] > 100).all() and ((most > 15).all() if freq == 30 else (most < 8).all()), (freq, most)
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
    for f in got["summ"].dtype.names:
        if f == "n_candidates":
            assert (got["summ"][f] <= ref["summ"][f]).all()
            continue
        assert np.array_equal(got["summ"][f], ref["summ"][f]), f
    for e in range(E):
        for k in TREE_KEYS:
            assert np.array_equal(got["trees"][e][k], ref["trees"][e][k]), (e, k)
        assert np.array_equal(got["paths"][e], ref["paths"][e]), e

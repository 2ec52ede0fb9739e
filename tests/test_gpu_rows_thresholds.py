"""The four-episode RRT kernels read an obstacle's collision threshold through the scalar data path: in a round of the
candidate loop each row of the wavefront that has a candidate loads the threshold of ITS obstacle and keeps it by a per-lane
select.  The risk is a row taking another row's threshold when several rows have candidates in the same round, so the world
here is dense -- 256 obstacles with pairwise different radii, i.e. pairwise different thresholds -- and every sampled episode
is compared with the portable checker: a wrong threshold changes a collision, the tree and everything after it.

Kernels: rrt_rows_stream_kernel (mirrored ring), rrt_rows_stream_masked_kernel (ROWS_STREAM_MIRROR = 0) and rrt_rows_kernel;
workgroups of one and of twelve wavefronts (ROWS_WG_WAVES); the tight cull, which the host picks by itself in a world this
dense, and the plain one (TIGHT_CULL = 0).

What is compared: status, node count, point count, parents and the generator's position exactly; nodes and points to 1e-9.
n_candidates (obstacles that passed the conservative cull) is a diagnostic of these kernels that the checker does not have:
its reference is tests/golden/rows_thresholds_ncand.json, what the kernels reported for this very batch BEFORE thresholds went
through the scalar path (recorded once per cull form; both stream kernels and rrt_rows_kernel agreed on it).

The world must not be lenient: the boundary is pushed out so far that no steer can leave it (asserted below from the checker's
tree: a steer moves less than freq x dist_to_end from its parent), so every steer the checker rejects is rejected by a
collision -- and that must be at least one steer in ten on every sampled episode (it is two in three and more)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "rows_thresholds_ncand.json")

E, N_ITER = 53, 1000          # two twelve-wave workgroups (48 episodes each), the second one partly filled
FREQ, DIST_TO_END = 30, 2     # rrt_explore_batch's defaults, named because the boundary margin below is derived from them
GROW = 150.0                  # how far the boundary lies outside the obstacles' box


def make_case():
    from auv_sim_amd import synth
    world = synth.make_world(seed=71, n_obstacles=256, obst_radius=(2.0, 6.0))
    x0, y0, x1, y1 = world["box"]
    world["polygon"] = np.array([(x0 - GROW, y0 - GROW), (x1 + GROW, y0 - GROW), (x1 + GROW, y1 + GROW), (x0 - GROW, y1 + GROW)])
    init = np.zeros((E, 6))
    init[:, 0], init[:, 1] = world["start"]
    init[:, 2] = np.linspace(-3.0, 3.0, E)
    seeds = np.arange(4000, 4000 + E, dtype=np.uint64)
    return world, init, seeds


def run_case(ctx, init, seeds, kernel, waves, tight):
    """kernel: 'stream' / 'masked' / 'classic'; tight: None (the host's choice) or 0"""
    opts = {"ROWS": 1, "ROWS_STREAM": 0 if kernel == "classic" else 1, "ROWS_WG_WAVES": waves, "TIGHT_CULL": tight,
            "ROWS_STREAM_MIRROR": {"stream": 1, "masked": 0, "classic": None}[kernel],
            # (a steer in a world this dense is rejected two times in three, and a rejected steer's numbers buy no node: the
            # episodes draw more than the default stream holds for a parameter block the context has not seen yet)
            "ROWS_STREAM_CAP": None if kernel == "classic" else 160 * N_ITER}
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        summ = ctx.rrt_explore_batch(init, seeds, N_ITER).copy()
        name, mirror, block = ctx.last_rrt_kernel(), ctx.last_stream_mirror(), ctx.last_launch()[1]
        redone = ctx.pipeline_fallbacks()[0]
        trees = {e: ctx.tree(e, summ[e]) for e in SAMPLE}
    finally:
        for k in opts:
            ctx.set_option(k, None)
    return summ, trees, name, mirror, block, redone


SAMPLE = sorted({0, 1, 2, 3, E // 2, 47, 48, E - 1})   # a whole wavefront's four rows, a workgroup's last and next first episode


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def reference(orc):
    """the portable checker on the sampled episodes, and the proof that the world is not lenient"""
    world, init, seeds = make_case()
    radii = world["obstacles"][:, 2]
    assert len(radii) == 256 and len(set(radii.tolist())) == 256
    w = orc.WorldArrays(world["obstacles"], world["habitats"], world["polygon"], world["bins"], world["cells"], world["prob"])
    px0, py0 = world["polygon"].min(axis=0)
    px1, py1 = world["polygon"].max(axis=0)
    ref = {}
    for e in SAMPLE:
        r = orc.rrt_explore(w, int(seeds[e]), N_ITER, init=init[e], kind="portable")
        n = r["nodes"]
        # a steer's sub-arcs are each at most dist_to_end long and there are fewer than freq of them: from no node of the tree
        # can a steer reach the boundary, so a rejected steer was rejected by a collision
        margin = min((n[:, 0] - px0).min(), (px1 - n[:, 0]).min(), (n[:, 1] - py0).min(), (py1 - n[:, 1]).min())
        assert margin > FREQ * DIST_TO_END, (e, margin)
        tried = r["it_parent"] >= 0
        rejected = tried & (r["it_accepted"] == 0)
        print("episode %d: %d steers, %d rejected by collision (%.3f), %d nodes" % (e, tried.sum(), rejected.sum(),
                                                                                 rejected.sum() / tried.sum(), r["n_nodes"]))
        assert tried.sum() >= N_ITER // 2 and rejected.sum() * 10 >= tried.sum(), (e, int(tried.sum()), int(rejected.sum()))
        ref[e] = r
    return ref


@pytest.mark.parametrize("tight", [None, 0], ids=["tight_cull", "plain_cull"])
@pytest.mark.parametrize("waves", [1, 12])
@pytest.mark.parametrize("kernel", ["stream", "masked", "classic"])
def test_every_row_tests_its_candidate_against_its_own_threshold(ctx, reference, kernel, waves, tight):
    world, init, seeds = make_case()
    ctx.set_world(world["obstacles"], world["habitats"], world["polygon"], world["bins"], world["cells"], world["prob"])
    summ, trees, name, mirror, block, redone = run_case(ctx, init, seeds, kernel, waves, tight)
    assert name == ("rrt_rows_kernel" if kernel == "classic" else "rrt_rows_stream_kernel") and redone == 0
    assert mirror == {"stream": 1, "masked": 0, "classic": -1}[kernel] and block == 64 * waves
    golden = json.load(open(GOLDEN))["plain_cull" if tight == 0 else "tight_cull"]
    print("n_candidates", summ["n_candidates"].tolist())
    assert summ["n_candidates"].tolist() == golden
    # (the tight box never lets more obstacles through than the reach square, and in a world this dense it lets fewer through)
    plain = json.load(open(GOLDEN))["plain_cull"]
    assert all(a <= b for a, b in zip(golden, plain)) and (tight == 0 or sum(golden) < sum(plain))
    for e in SAMPLE:
        r, s, t = reference[e], summ[e], trees[e]
        assert (s["status"], s["n_nodes"], s["n_points"], s["n_leaves"]) == (r["status"], r["n_nodes"], r["n_points"], r["n_leaves"]), e
        assert s["rng_after"] == r["rng_after"] and int(s["n_draw32"]) == int(r["n_draw32"]), e
        assert np.array_equal(t["parent"], r["parent"]), e
        assert np.array_equal(t["pt_off"], r["pt_off"]) and np.array_equal(t["pt_cnt"], r["pt_cnt"]), e
        dn, dp = np.abs(t["nodes"] - r["nodes"]).max(), np.abs(t["points"] - r["points"]).max()
        print("episode %d: max |nodes - checker| %.3g, max |points - checker| %.3g" % (e, dn, dp))
        assert dn <= 1e-9 and dp <= 1e-9, (e, dn, dp)

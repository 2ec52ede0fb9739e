"""Planner_RRT on rectangles whose origin is not (0, 0) -- round 6 (VERDICT r5 missing #2).

The reference's bucket grid ignores the boundary's origin (gym_rrt/envs/rrt_dubins.py:115-116: int(y / cell), int(x / cell) of
the ABSOLUTE position): nodes land in "wrong" cells, negative indexes wrap to the far end of the Python lists, indexes past the
grid return without inserting (:118-124) and indexes below -len raise IndexError (:127).  The device takes that arithmetic from
ONE helper (csrc/planner_rrt_kernel.h prrt_bucket_of); here every planner kernel runs the translated worlds:

  g2_org_*  (the reference completes)  x  prrt_kernel / prrt_rows_kernel / prrt_pipe_kernel, generate_one_node stepping,
            the drop-in class, RRTEnvBatch.step:  decisions exact and floats <= 1e-9 vs the golden, bit-for-bit vs the checker
  g2e_*     (the reference raises IndexError: in __init__, at the first random.choice of an empty occupied list, in the
            middle of planning())  ->  the episode's status is AUVP_ERR_ARG and its record stops where the reference stopped
"""
import glob
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ORG = sorted(glob.glob(os.path.join(GOLDEN, "g2_org_*.npz")))
ERR = sorted(glob.glob(os.path.join(GOLDEN, "g2e_*.npz")))
ST = ("st_bucket", "st_picked", "st_accepted", "st_done", "st_npath", "st_arc_n", "st_arc_free")
# kernel -> (options that force it, keeps the step log)
KERNELS = {"prrt_kernel": (dict(PRRT_ROWS=0, PRRT_PIPE=0), True), "prrt_rows_kernel": (dict(PRRT_ROWS=1, PRRT_LAT=0), False),
           # (the pipeline with the draw wavefront -- five per episode, round 6 -- and in its four-wavefront form)
           "prrt_pipe_kernel": (dict(PRRT_ROWS=0, PRRT_PIPE=1, PRRT_PIPE_DRAW=1), False),
           "prrt_pipe_kernel/4": (dict(PRRT_ROWS=0, PRRT_PIPE=1, PRRT_PIPE_DRAW=0), False)}
MAX_FREQ = {"prrt_kernel": 10 ** 9, "prrt_rows_kernel": 15, "prrt_pipe_kernel": 30, "prrt_pipe_kernel/4": 30}  # PRW_MAX_FREQ, DUO_MAX_FREQ


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _ids(paths):
    return [os.path.basename(p)[:-4] for p in paths]


def _batch(ctx, g, kernel, E, seeds, step_log):
    from auv_sim_amd._prrt_lib import PlannerBatch
    opts, log_ok = KERNELS[kernel]
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        ctx.set_world(obstacles=g["obstacles"])
        st = list(g["start"]) + [0.0] * (4 - len(g["start"]))
        starts = np.tile(np.array(st, dtype=np.float64), (E, 1))
        goals = np.tile(np.asarray(g["goal"], dtype=np.float64), (E, 1))
        pb = PlannerBatch(ctx, starts, goals, g["rect"], int(g["max_step"]), seeds=seeds, freq=int(g["freq"]), cell=int(g["cell"]),
                          subs=int(g["subs"]), exp_rate=float(g["exp_rate"]), dist_to_end=float(g["dist_to_end"]),
                          diff_max=float(g["diff_max"]), step_log=step_log and log_ok)
        # (a failing start is reported by the batch's first summaries; plan() then leaves such an episode alone)
        summ = pb.plan().copy()
        assert ctx.L.auvp_prrt_last_kernel(ctx.h).decode() == kernel.split("/")[0]
        assert ctx.pipeline_fallbacks()[0] == 0
    finally:
        for k in opts:
            ctx.set_option(k, None)
    return pb, summ


def _oracle(g, seed=None, kind="portable"):
    from oracle import orc_planner as op
    return op.planning(g["obstacles"], g["rect"], g["start"], g["goal"], int(g["seed"]) if seed is None else seed, int(g["max_step"]),
                       int(g["freq"]), int(g["cell"]), int(g["subs"]), float(g["exp_rate"]), float(g["dist_to_end"]),
                       float(g["diff_max"]), kind=kind)


def _same_as_oracle(pb, s, e, r, paths):
    assert s["status"] == 0 and r["status"] == 0
    assert (s["steps"], bool(s["done"]), s["n_nodes"], s["n_points"]) == (r["steps"], r["done"], r["n_nodes"], r["n_points"])
    t = pb.tree(e, s)
    assert np.array_equal(t["parent"], r["parent"])
    assert np.array_equal(t["nodes"], r["nodes"][:, :4])
    assert np.array_equal(t["points"], r["points"])
    assert np.array_equal(t["node_bucket"], r["node_bucket"])
    assert np.array_equal(t["pt_off"], r["pt_off"]) and np.array_equal(t["pt_cnt"], r["pt_cnt"])
    occ, cnt = pb.grid(e)
    assert np.array_equal(occ, r["occupied"]) and np.array_equal(cnt, r["bucket_counts"])
    assert s["rng_after"] == r["rng_after"] and int(s["n_draw32"]) == int(r["n_draw32"])
    if r["done"]:
        assert np.array_equal(paths[e], r["path"])
    return t


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("path", ORG, ids=_ids(ORG))
def test_translated_world_vs_golden_and_oracle(ctx, orc, path, kernel):
    """episode 0 = the golden's seed; the others (other seeds, same world) against the checker: the batch shapes of the three
    kernels (four episodes per wavefront, one per wavefront, four wavefronts per episode) all see wrapped and missing buckets"""
    g = np.load(path)
    if int(g["freq"]) > MAX_FREQ[kernel]:
        pytest.skip("freq %d is beyond %s's steer width" % (int(g["freq"]), kernel))
    E = 6
    seeds = np.array([int(g["seed"])] + [1000 + 17 * e for e in range(1, E)], dtype=np.uint64)
    pb, summ = _batch(ctx, g, kernel, E, seeds, step_log=True)
    paths = pb.paths(summ)
    # the golden: decisions exact, floats within 1e-9
    s = summ[0]
    assert s["status"] == 0
    assert s["steps"] == int(g["steps"]) and bool(s["done"]) == bool(g["done"]) and s["n_nodes"] == len(g["nodes"])
    t = pb.tree(0, s)
    assert np.array_equal(t["parent"], g["parent"])
    assert np.array_equal(t["pt_cnt"][1:] + 1, g["npath"][1:])
    np.testing.assert_allclose(t["nodes"], g["nodes"][:, :4], rtol=1e-9, atol=1e-9)
    if "points" in g.files:
        np.testing.assert_allclose(t["points"], g["points"], rtol=1e-9, atol=1e-9)
    occ, cnt = pb.grid(0)
    assert np.array_equal(occ, g["occupied"]) and np.array_equal(cnt, g["bucket_counts"])
    # nodes the reference left out of every bucket ("out of the habitat environment bound") are left out here
    assert int((t["node_bucket"] < 0).sum()) == len(g["nodes"]) - int(g["bucket_counts"].sum())
    assert s["rng_after"] == float(g["rng_after"])
    if KERNELS[kernel][1]:
        log = pb.step_log(0, int(s["steps"]))
        for i, k in enumerate(ST):
            assert np.array_equal(log[:, i], g[k].astype(np.int32)), k
    if "path" in g.files:
        assert paths[0].shape == g["path"].shape
        np.testing.assert_allclose(paths[0], g["path"], rtol=1e-9, atol=1e-9)
    # the checker on the same portable math: bit for bit, every episode
    for e in range(E):
        _same_as_oracle(pb, summ[e], e, _oracle(g, int(seeds[e])), paths)


@pytest.mark.parametrize("path", ORG, ids=_ids(ORG))
def test_translated_world_generate_one_node_stepping(ctx, path):
    """planning() as the loop the reference runs -- random.choice(occupied) on the host, generate_one_node on the device with
    Python's global stream handed over for the step -- reproduces the golden's buckets on a translated world"""
    from auv_sim_amd._prrt_lib import PlannerBatch
    g = np.load(path)
    random.seed(int(g["seed"]))

    def state():
        ver, internal, _ = random.getstate()
        return np.array(internal[:624], dtype=np.uint32).reshape(1, 624), np.array([internal[624]], dtype=np.int32)

    ctx.set_world(obstacles=g["obstacles"])
    st = list(g["start"]) + [0.0] * (4 - len(g["start"]))
    pb = PlannerBatch(ctx, [st], [list(g["goal"])], g["rect"], int(g["max_step"]), mt_states=state(), freq=int(g["freq"]),
                      cell=int(g["cell"]), subs=int(g["subs"]), exp_rate=float(g["exp_rate"]), dist_to_end=float(g["dist_to_end"]),
                      diff_max=float(g["diff_max"]))
    occupied = [int(b) for b in pb.grid(0)[0]]
    n_steps = min(int(g["steps"]), 500)
    for i in range(n_steps):
        b = random.choice(occupied)
        assert b == int(g["st_bucket"][i]), i
        s = pb.step([b], mt_states=state())[0]
        assert s["status"] == 0
        n = int(s["n_draw32"])
        if n:
            random.getrandbits(32 * n)
        assert bool(s["last_accepted"]) == bool(g["st_accepted"][i]), i
        assert bool(s["done"]) == bool(g["st_done"][i]), i
        if s["last_accepted"]:
            occupied = [int(x) for x in pb.grid(0)[0]]
    s = pb.summaries()[0]
    n_acc = int(g["st_accepted"][:n_steps].sum())
    assert s["n_nodes"] == 1 + n_acc
    t = pb.tree(0, s)
    assert np.array_equal(t["parent"], g["parent"][:1 + n_acc])
    np.testing.assert_allclose(t["nodes"], g["nodes"][:1 + n_acc, :4], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("name", ["g2_org_m50_m30", "g2_org_p30_p20", "g2_org_frac"])
def test_translated_world_dropin_class(name):
    """the reference-signature class (auv_sim_amd.planner_rrt.Planner_RRT) on a translated world: planning() under
    random.seed, then the Python mirror of the bucket grid (env_grid / occupied_grid_cells_array) against the golden"""
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    from auv_sim_amd.planner_rrt import Planner_RRT
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    obs = [MPS(o[0], o[1], size=o[2]) for o in g["obstacles"].tolist()]
    rect = g["rect"]
    bnd = [MPS(rect[0], rect[1]), MPS(rect[2], rect[3])]
    st = g["start"]
    s = MPS(float(st[0]), float(st[1]), z=-5.0, theta=float(st[2]) if len(st) > 2 else 0.0)
    goal = MPS(float(g["goal"][0]), float(g["goal"][1]), z=-5.0, theta=0.0)
    rrt = Planner_RRT(s, goal, bnd, obs, [], exp_rate=float(g["exp_rate"]), dist_to_end=float(g["dist_to_end"]),
                      diff_max=float(g["diff_max"]), freq=int(g["freq"]), cell_side_length=int(g["cell"]),
                      subsections_in_cell=int(g["subs"]))
    random.seed(int(g["seed"]))
    path, step, _ = rrt.planning(max_step=int(g["max_step"]))
    assert step == int(g["steps"])
    assert random.random() == float(g["rng_after"])
    assert len(rrt.mps_list) == len(g["nodes"])
    got = np.array([[n.x, n.y, n.theta, n.traj_time_stamp] for n in rrt.mps_list])
    np.testing.assert_allclose(got, g["nodes"][:, :4], rtol=1e-9, atol=1e-9)
    ncols, subs = len(rrt.env_grid[0]), int(g["subs"])
    occ = [(r * ncols + c) * subs + k for r, c, k in rrt.occupied_grid_cells_array]
    assert occ == g["occupied"].tolist()
    counts = [len(sub.node_array) for row in rrt.env_grid for gc in row for sub in gc.subsection_cells]
    assert counts == g["bucket_counts"].tolist()
    if bool(g["done"]):
        arr = np.array([[p.x, p.y, p.theta, p.traj_time_stamp] for p in path])
        np.testing.assert_allclose(arr, g["path"][:, :4], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("path", ERR, ids=_ids(ERR))
def test_reference_indexerror_is_a_declared_status(ctx, orc, path, kernel):
    """where the reference raises IndexError the episode ends with AUVP_ERR_ARG (-1) and its record holds what the reference
    had built when it raised: the steps completed, the tree incl. the node whose insertion failed (mps_list.append precedes
    add_node_to_grid: :229-230), the generator position.  The neighbours in the batch (a world-compatible start) are untouched."""
    g = np.load(path)
    stage = str(g["error_stage"])
    E = 5
    seeds = np.array([int(g["seed"])] * E, dtype=np.uint64)
    pb, summ = _batch(ctx, g, kernel, E, seeds, step_log=False)
    r = _oracle(g)
    assert r["status"] == -2  # ORC_ERR_ARG (oracle/orc_api.h): the checker's name for the IndexError
    for e in range(E):
        s = summ[e]
        assert s["status"] == -1
        assert s["steps"] == int(g["steps"]) == r["steps"] and not s["done"]
        if stage == "init":
            continue
        assert s["n_nodes"] == len(g["nodes"]) == r["n_nodes"]
        t = pb.tree(e, s)
        assert np.array_equal(t["parent"], g["parent"])
        np.testing.assert_allclose(t["nodes"], g["nodes"][:, :4], rtol=1e-9, atol=1e-9)
        assert np.array_equal(t["nodes"], r["nodes"][:, :4]) and np.array_equal(t["points"], r["points"])
        assert np.array_equal(t["node_bucket"], r["node_bucket"])
        occ, cnt = pb.grid(e)
        assert np.array_equal(occ, g["occupied"]) and np.array_equal(cnt, g["bucket_counts"])
        assert s["rng_after"] == float(g["rng_after"]) == r["rng_after"]


@pytest.mark.parametrize("name", [os.path.basename(p)[:-4] for p in ERR])
def test_reference_indexerror_through_the_dropin_class(name):
    """the drop-in raises what the reference raises, where it raises it"""
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    from auv_sim_amd.planner_rrt import Planner_RRT
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    obs = [MPS(o[0], o[1], size=o[2]) for o in g["obstacles"].tolist()]
    rect = g["rect"]
    bnd = [MPS(rect[0], rect[1]), MPS(rect[2], rect[3])]
    s = MPS(float(g["start"][0]), float(g["start"][1]), z=-5.0, theta=0.0)
    goal = MPS(float(g["goal"][0]), float(g["goal"][1]), z=-5.0, theta=0.0)
    kw = dict(exp_rate=float(g["exp_rate"]), dist_to_end=float(g["dist_to_end"]), diff_max=float(g["diff_max"]), freq=int(g["freq"]),
              cell_side_length=int(g["cell"]), subsections_in_cell=int(g["subs"]))
    if str(g["error_stage"]) == "init":
        with pytest.raises(IndexError):
            Planner_RRT(s, goal, bnd, obs, [], **kw)
        return
    rrt = Planner_RRT(s, goal, bnd, obs, [], **kw)
    random.seed(int(g["seed"]))
    with pytest.raises(IndexError):
        rrt.planning(max_step=int(g["max_step"]))
    assert random.random() == float(g["rng_after"])
    assert len(rrt.mps_list) == len(g["nodes"])  # the node whose insertion raised is in mps_list (:229)
    got = np.array([[n.x, n.y, n.theta, n.traj_time_stamp] for n in rrt.mps_list])
    np.testing.assert_allclose(got, g["nodes"][:, :4], rtol=1e-9, atol=1e-9)

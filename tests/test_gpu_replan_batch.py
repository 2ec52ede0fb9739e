"""RRT.replanning_batch and the per-episode limits under it (auvp_rrt_prepare_episodes: rrt_explore_lim_kernel +
rrt_leaf_lim_kernel): every AUV of a batch plans with its own horizon and its own habitat list.  Checked against the
reference's own multi-round runs (G13), against sequential RRT.replanning calls, against the CPU checker run on a world that
holds only the episode's habitats, and against plain uniform-parameter batches at full-chip size."""
import ctypes as C
import math
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


class _Cell:
    def __init__(self, b):
        self.bounds = tuple(float(v) for v in b)


class _Poly:
    class _Ext:
        def __init__(self, pts):
            self.coords = list(pts) + [pts[0]]

    def __init__(self, pts):
        self.exterior = _Poly._Ext([tuple(p) for p in pts])


def _inputs(g):
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    obstacles = [MPS(o[0], o[1], size=o[2]) for o in g["obstacles"].tolist()]
    habitats = [MPS(h[0], h[1], size=h[2]) for h in g["habitats"].tolist()]
    cell_list = [_Cell(c) for c in g["cells"].tolist()]
    shark = {}
    for t, b in enumerate(g["bins"].tolist()):
        shark[(int(b[0]), int(b[1]))] = {cell_list[i].bounds: p for i, p in enumerate(g["prob"][t].tolist())}
    return obstacles, habitats, cell_list, shark, _Poly(g["polygon"].tolist())


def _free_starts(rng, g, n):
    """n start points inside the boundary and outside every obstacle (with a margin)"""
    poly, obst = g["polygon"], g["obstacles"]
    x0, y0, x1, y1 = poly[:, 0].min(), poly[:, 1].min(), poly[:, 0].max(), poly[:, 1].max()
    out = []
    while len(out) < n:
        x, y = rng.uniform(x0 + 10, x1 - 10), rng.uniform(y0 + 10, y1 - 10)
        if all(math.hypot(x - o[0], y - o[1]) > o[2] + 3.0 for o in obst):
            out.append((x, y))
    return out


def _rows(objs):
    return np.array([[p.x, p.y, p.theta, p.v, p.traj_time_stamp, p.plan_time_stamp, p.length] for p in objs]).reshape(-1, 7)


@pytest.mark.parametrize("name", ["g13_replan_a", "g13_replan_b"])
def test_batch_reproduces_reference_replanning(name):
    """33 AUVs in one batch; AUVs 0, 16 and 32 start where the reference's run started and continue the reference's global
    stream (rngs = random.Random(seed)); the others start elsewhere with seeds of their own.  Each golden AUV equals the
    reference round for round, and its generator ends where the reference's global stream ended; seeded AUVs of the same
    batch equal their sequential calls."""
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    from auv_sim_amd.rrt_dubins import RRT
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    obstacles, habitats, cell_list, shark, poly = _inputs(g)
    rrt = RRT(poly, obstacles, shark, cell_list)
    rng = random.Random(99)
    pts = _free_starts(rng, g, 33)
    golden_ids = (0, 16, 32)
    starts, rngs, seeds = [], [], []
    for e in range(33):
        if e in golden_ids:
            starts.append(MPS(float(g["start"][0]), float(g["start"][1])))
            rngs.append(random.Random(int(g["seed"])))
            seeds.append(None)
        else:
            starts.append(MPS(*pts[e]))
            rngs.append(None)
            seeds.append(1000 + e)
    before = [(h.x, h.y, h.size) for h in habitats]
    res = rrt.replanning_batch(starts, habitats, float(g["plan_time_budget"]), float(g["traj_time_length"]),
                               float(g["replan_time_interval"]), [-3, -3, -4], max_iter=int(g["iters_per_round"][0]),
                               seeds=seeds, rngs=rngs)
    assert [(h.x, h.y, h.size) for h in habitats] == before  # the caller's list is not mutated
    for e in golden_ids:
        traj, rounds, cost, _ = res[e]
        got = _rows(traj)[:, [0, 1, 2, 3, 4, 6]]
        assert got.shape == g["traj"].shape
        np.testing.assert_allclose(got, g["traj"], rtol=1e-9, atol=1e-9)
        assert list(rounds.keys()) == list(range(1, len(g["round_len"]) + 1))
        assert [len(rounds[k][0]) for k in rounds] == g["round_len"].tolist()
        assert [len(rounds[k][1]) for k in rounds] == g["round_habitats"].tolist()
        assert rngs[e].random() == float(g["rng_after"])
        np.testing.assert_allclose([cost[0]] + list(cost[1]), g["cost"], rtol=0, atol=1e-6)
        assert [[h.x, h.y, h.size] for h in res[e][3]] == g["habitats_left"].tolist()
        assert all(any(h is x for x in habitats) for h in res[e][3])  # the caller's own objects
    # the same AUVs as arrays: per-round horizon, cost and the habitats left
    rngs2 = [random.Random(int(g["seed"])) if e in golden_ids else None for e in range(33)]
    arr = rrt.replanning_batch(starts, habitats, float(g["plan_time_budget"]), float(g["traj_time_length"]),
                               float(g["replan_time_interval"]), [-3, -3, -4], max_iter=int(g["iters_per_round"][0]),
                               seeds=seeds, rngs=rngs2, as_arrays=True)
    H = len(habitats)
    for e in golden_ids:
        a = arr[e]
        np.testing.assert_allclose(a["traj"][:, [0, 1, 2, 3, 4, 6]], g["traj"], rtol=1e-9, atol=1e-9)
        assert a["round_len"].tolist() == g["round_len"].tolist()
        assert [bin(int(k)).count("1") for k in a["round_keep"]] == g["round_habitats"].tolist()
        np.testing.assert_allclose(a["round_max_traj_time"], g["round_max_traj_time"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(a["round_cost"], g["round_cost"], rtol=0, atol=1e-6)
        left = np.array([g["habitats"][h] for h in range(H) if (a["keep"] >> h) & 1]).reshape(-1, 3)
        assert left.tolist() == g["habitats_left"].tolist()
        np.testing.assert_allclose(a["cost"], g["cost"], rtol=0, atol=1e-6)
        assert rngs2[e].random() == float(g["rng_after"])
    # the seeded AUVs of this mixed batch ran from host-seeded generator states (the batch also holds generators): each still
    # equals its sequential replanning(seed=...) call
    for e in (1, 15, 17, 31):
        b = res[e]
        try:
            seq = rrt.replanning(starts[e], list(habitats), float(g["plan_time_budget"]), float(g["traj_time_length"]),
                                 float(g["replan_time_interval"]), [-3, -3, -4], max_iter=int(g["iters_per_round"][0]),
                                 seed=seeds[e])
        except TypeError:  # a round without a qualifying leaf: the batch's entry is None
            assert b is None, e
            continue
        assert np.array_equal(_rows(seq[0]), _rows(b[0])), e
        assert [len(v[0]) for v in seq[1].values()] == [len(v[0]) for v in b[1].values()], e
        assert [v[1] for v in seq[1].values()] == [v[1] for v in b[1].values()], e
        assert seq[2] == b[2], e


def test_batch_equals_sequential_replanning():
    """24 AUVs with distinct starts and seeds, one of them starting late enough that its first round's horizon is clipped at
    the shark grid's end: element for element the 24 sequential RRT.replanning(seed=...) calls."""
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    from auv_sim_amd.rrt_dubins import RRT
    g = np.load(os.path.join(GOLDEN, "g13_replan_a.npz"))
    obstacles, habitats, cell_list, shark, poly = _inputs(g)
    rrt = RRT(poly, obstacles, shark, cell_list)
    pts = _free_starts(random.Random(5), g, 24)
    horizon_end = float(g["bins"][-1][1])
    budget, length, interval, n_iter = 2.0, 150.0, 98.0, 400
    starts = [MPS(x, y) for x, y in pts]
    starts[7].traj_time_stamp = horizon_end - 120.0  # 380 + 150 > 500: clipped in its first round, one round only
    seeds = [31 * e + 3 for e in range(24)]
    batch = rrt.replanning_batch(starts, habitats, budget, length, interval, [-3, -3, -4], max_iter=n_iter, seeds=seeds)
    clipped = 0
    for e in range(24):
        hl = list(habitats)
        b = batch[e]
        try:
            seq = rrt.replanning(starts[e], hl, budget, length, interval, [-3, -3, -4], max_iter=n_iter, seed=seeds[e])
        except TypeError:  # a round without a qualifying leaf: the batch's entry is None
            assert b is None, e
            continue
        assert np.array_equal(_rows(seq[0]), _rows(b[0])), e
        assert list(seq[1].keys()) == list(b[1].keys())
        for k in seq[1]:
            assert np.array_equal(_rows(seq[1][k][0]), _rows(b[1][k][0])), (e, k)
            assert seq[1][k][1] == b[1][k][1], (e, k)  # the same habitat objects, same order
        assert seq[2] == b[2], e
        assert hl == b[3], e  # the habitats left: the same objects as the list the sequential call shortened
        clipped += 1 if (e == 7 and len(seq[1]) == 1) else 0
    assert clipped == 1


def _limits_world(seed=12, n_habitats=9):
    from auv_sim_amd import synth
    return synth.make_world(seed=seed, n_obstacles=64, n_habitats=n_habitats)


@pytest.mark.parametrize("no_grid", [False, True])
def test_limits_kernel_equals_checker_per_episode(orc, no_grid):
    """600 episodes with horizons from 60 to 500 s (and a few of 1 500 s) and keep masks that include none, all and single
    habitats, some without a qualifying leaf (a start outside the boundary): each equals the CPU checker run on a world holding
    only its kept habitats, with its own max_traj_time -- status, node / leaf counts, generator draws, best cost and best path;
    bin_sizes() reports the episode's own K.  600 episodes are more than two per CU, so workgroups carry several wavefronts
    whose K differ (asserted on the launch shape).  no_grid: the world without its habitat mask grid (option NO_HABITAT_GRID):
    the leaf pass takes the habitat scan instead."""
    from auv_sim_amd import _lib
    w = _limits_world()
    H = len(w["habitats"])
    ctx = _lib.Context(0)
    if no_grid:
        ctx.set_option("NO_HABITAT_GRID", 1)  # (read when the habitats are set)
    ctx.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"])
    rng = random.Random(3)
    E, n_iter = 600, 350
    mtt = np.array([rng.choice([60.0, 75.5, 100.0, 137.0, 200.0, 260.0, 333.0, 420.0, 500.0]) for _ in range(E)])
    mtt[[4, 9, 17, 30, 301]] = 1500.0  # the longest horizon, K = 300
    keep = [0, (1 << H) - 1, 1, 1 << (H - 1)] + [1 << rng.randrange(H) for _ in range(6)] + \
           [rng.getrandbits(H) for _ in range(E - 10)]
    init = np.zeros((E, 6))
    init[:, 0], init[:, 1] = w["start"]
    init[[5, 9, 22, 450], 0] = 1.0e4  # outside the boundary: every steer is rejected, no qualifying leaf
    seeds = np.arange(E, dtype=np.uint64) * 7 + 11
    summ = ctx.rrt_explore_batch(init, seeds, n_iter, max_traj_time=mtt, habitat_keep=np.array(keep, dtype=np.uint64))
    assert ctx.last_rrt_kernel() == "rrt_explore_lim_kernel"
    grid, block, _ = ctx.last_launch()
    assert block >= 2 * 64 and grid * block // 64 >= E, (grid, block)  # several episodes, several K, per workgroup
    paths = ctx.paths(summ)
    no_leaf = 0
    for e in range(E):
        sub = w["habitats"][[h for h in range(H) if (keep[e] >> h) & 1]].reshape(-1, 3)
        wa = orc.WorldArrays(w["obstacles"], sub, w["polygon"], w["bins"], w["cells"], w["prob"])
        r = orc.rrt_explore(wa, int(seeds[e]), n_iter, init=init[e], max_traj_time=float(mtt[e]), kind="portable")
        s = summ[e]
        assert (int(s["status"]), int(s["n_nodes"]), int(s["n_points"]), int(s["n_leaves"])) == \
               (r["status"], r["n_nodes"], r["n_points"], r["n_leaves"]), e
        assert int(s["n_draw32"]) == r["n_draw32"] and s["rng_after"] == r["rng_after"], e
        assert np.array_equal(np.array(s["best_cost"]), r["best_cost"]), (e, s["best_cost"], r["best_cost"])
        assert int(s["best_leaf"]) == r["best_leaf"], e
        if r["best_leaf"] >= 0:
            assert np.array_equal(paths[e], r["path"]), e
        else:
            no_leaf += 1
        assert ctx.bin_sizes(e).tolist() == r["bin_sizes"].tolist() and len(ctx.bin_sizes(e)) == math.ceil(mtt[e] / 5)
    assert 0 < no_leaf < E


def test_limits_full_chip_equals_uniform_batches():
    """2 100 episodes (more than eight per CU: full RRT_X_WAVES workgroups, every workgroup mixing all eight horizons) at 300
    iterations in eight (horizon, habitat mask) groups: every episode's summary and best path equal the same group run as a
    plain uniform-parameter batch on a world holding only the group's habitats."""
    from auv_sim_amd import _lib
    w = _limits_world(seed=21, n_habitats=10)
    H = len(w["habitats"])
    groups = [(60.0, 0b1111111111), (95.0, 0b0000000001), (150.0, 0), (210.0, 0b1010101010), (275.0, 0b1000000000),
              (330.0, 0b0111001100), (415.0, 0b0000011111), (500.0, 0b1111111111)]
    E, n_iter = 2100, 300
    grp = np.arange(E) % len(groups)
    rng = np.random.default_rng(4)
    init = np.zeros((E, 6))
    init[:, 0] = w["start"][0] + rng.uniform(-20, 20, E)
    init[:, 1] = w["start"][1] + rng.uniform(-20, 20, E)
    seeds = np.arange(E, dtype=np.uint64) + 5000
    ctx = _lib.Context(0)
    ctx.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"])
    mtt = np.array([groups[k][0] for k in grp])
    keep = np.array([groups[k][1] for k in grp], dtype=np.uint64)
    summ = ctx.rrt_explore_batch(init, seeds, n_iter, max_traj_time=mtt, habitat_keep=keep)
    assert ctx.last_rrt_kernel() == "rrt_explore_lim_kernel" and ctx.last_launch()[1] == 8 * 64
    paths = ctx.paths(summ)
    fields = ("status", "n_nodes", "n_points", "n_leaves", "best_leaf", "best_path_len", "iters_run", "best_cost",
              "best_length", "rng_after", "leaf_elems", "n_draw32")
    ref = _lib.Context(0)
    ref.set_world(w["obstacles"], None, w["polygon"], w["bins"], w["cells"], w["prob"])
    for k, (h, m) in enumerate(groups):
        ids = np.flatnonzero(grp == k)
        ref.set_habitats(w["habitats"][[i for i in range(H) if (m >> i) & 1]].reshape(-1, 3))
        rs = ref.rrt_explore_batch(init[ids], seeds[ids], n_iter, max_traj_time=h)
        rp = ref.paths(rs)
        for j, e in enumerate(ids):
            for f in fields:
                assert np.array_equal(np.asarray(summ[e][f]), np.asarray(rs[j][f])), (k, e, f)
            assert np.array_equal(paths[e], rp[j]), (k, e)


def test_prepare_episodes_argument_checks():
    """auvp_rrt_prepare_episodes refuses (AUVP_ERR_ARG) another mode than time-bin, the iteration log / phase clocks, a
    horizon above the cap or not above zero, and keep bits at or above n_habitats; the leaf log is allowed"""
    from auv_sim_amd import _lib
    w = _limits_world()
    H = len(w["habitats"])
    ctx = _lib.Context(0)
    ctx.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"])
    E = 2
    init = np.zeros((E, 6))
    seeds = np.array([1, 2], dtype=np.uint64)

    def call(mode=0, flags=0, mtt=(100.0, 200.0), keep=(1, 3), cap=200.0):
        p = _lib.RRTParams()
        p.dist_to_end, p.diff_max, p.freq, p.min_dist, p.bin_interval, p.v = 2.0, 0.5, 30.0, 0.5, 5.0, 2.0
        p.max_traj_time, p.max_plan_time, p.mode, p.max_iter = cap, 50.0, mode, 50
        for i in range(3):
            p.w[i] = -3.0
        rec = np.zeros(E, dtype=_lib.EPISODE_DTYPE)
        rec["max_traj_time"], rec["habitat_keep"] = mtt, np.array(keep, dtype=np.uint64)
        return ctx.L.auvp_rrt_prepare_episodes(ctx.h, E, init.ctypes.data_as(C.POINTER(C.c_double)),
                                               seeds.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, C.byref(p),
                                               rec.ctypes.data_as(C.c_void_p), flags)
    assert call() == 0
    assert call(flags=_lib.FLAG_LEAF_LOG) == 0
    assert call(mode=1) == -1 and call(mode=2) == -1
    assert call(flags=_lib.FLAG_ITER_LOG) == -1 and call(flags=_lib.FLAG_PHASE_CLOCKS) == -1
    assert call(mtt=(100.0, 200.5)) == -1 and call(mtt=(0.0, 100.0)) == -1 and call(mtt=(-5.0, 100.0)) == -1
    assert call(keep=(1, 1 << H)) == -1 and call(keep=(1 << 63, 0)) == -1
    assert call(keep=(0, (1 << H) - 1)) == 0
    # the Python binding refuses the same before the library is reached
    with pytest.raises(ValueError):
        ctx.rrt_prepare(init, seeds, 50, mode="nn", max_traj_time=[100.0, 200.0])
    with pytest.raises(ValueError):
        ctx.rrt_prepare(init, seeds, 50, habitat_keep=[1, 1 << H])

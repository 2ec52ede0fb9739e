"""The A* kernel at the limits of what it keeps in LDS, HIP against the portable checker, bit for bit:

  * obstacle lists around and past the 256 it stages in LDS (astar_kernel.h ASTAR_LDS_OBST; beyond it the collision tests
    read the obstacle arrays from memory), for all four variants, each world built so that the obstacles a kernel could drop
    decide the result;
  * the world tables at their caps (64 habitats -- the 64-bit closed mask --, a 64-vertex boundary, 64 time bins), the
    smallest ones, and an odd mix, with routes that consume the last habitat and time stamps in the last bins."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LDS_OBST = 256  # astar_kernel.h ASTAR_LDS_OBST
CAP = 20000


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _checker(v, start, kw):
    from oracle import orc_astar as oa
    return oa.run(v, start, kind="portable", cap_nodes=CAP, **kw)


def _gpu(ctx, v, starts, kw):
    from auv_sim_amd import _astar_lib as al
    ctx.set_world(kw.get("obstacles"), kw.get("habitats"), kw.get("polygon"), kw.get("bins"), kw.get("cells"), kw.get("prob"))
    E = len(starts)
    goals = np.tile(np.asarray(kw["goal"], dtype=np.float64), (E, 1)) if "goal" in kw else None
    limits = np.full(E, kw["limit"]) if "limit" in kw else None
    return al.run_batch(ctx, v, starts, goals=goals, limits=limits, box=kw.get("box", (0, 0, 0, 0)),
                        velocity=kw.get("velocity", 1.0), weights=kw.get("weights", (0, 0, 0, 0)), cap_nodes=CAP, exp_log=True)


def _key(r):
    return (r["status"], r["found"], r["n_nodes"], r["n_children"], r["expansions"].tobytes(), r["path"].tobytes(),
            r["cost_list"].tobytes(), r["smooth_path"].tobytes(), r["hab_left"].tobytes(), r["visited_count"])


def _assert_same(r, o, e):
    """the fields test_astar_batch_vs_oracle compares.  A declared error (the reference raises) is compared by its status and
    the expansions before it; the C-ABI numbers capacity / argument errors the other way round from the checker."""
    st = {-1: -2, -2: -1}.get(r["status"], r["status"])
    assert st == o["status"], (e, r["status"], o["status"])
    assert np.array_equal(r["expansions"], o["expansions"]), e
    if o["status"] != 0:
        return
    assert r["found"] == o["found"] and r["n_nodes"] == o["n_nodes"] and r["n_children"] == o["n_children"], e
    assert np.array_equal(r["path"], o["path"]) and np.array_equal(r["cost_list"], o["cost_list"]), e
    assert np.array_equal(r["node_path"], o["node_path"]), e
    assert np.array_equal(r["smooth_path"], o["smooth_path"]), e
    assert np.array_equal(r["hab_left"], o["hab_left"]) and r["visited_count"] == o["visited_count"], e


def count_world(variant, n):
    """a world of n obstacles and nine starts (three workgroups, the last one partial) whose LAST obstacle lies on the middle
    node of instance 0's path without it"""
    from auv_sim_amd import synth
    rng = np.random.default_rng(1000 + n)
    if variant == "astar":
        w = synth.make_lattice_world(seed=n, n_obstacles=n - 1, r_range=(1, 4) if n <= 600 else (1, 2))
        starts = np.array([(10.0 * rng.integers(0, 6), 10.0 * rng.integers(0, 6)) for _ in range(9)])
        kw = dict(obstacles=w["obstacles"], goal=(490.0, 490.0), box=w["box"])
        last_r = 2.0
    else:
        starts = np.array([(-290.0 + 10.0 * rng.integers(0, 6), -90.0 + 10.0 * rng.integers(0, 6)) for _ in range(9)])
        w = synth.make_world(seed=n, n_obstacles=n - 1, obst_radius=(0.5, 2.5) if n <= 600 else (0.3, 1.2), start=starts[0],
                             n_habitats=8, hab_radius=(10.0, 25.0))
        kw = dict(obstacles=w["obstacles"], polygon=w["polygon"])
        if variant == "astar_real":
            kw["goal"] = (-120.0, 80.0)
        else:
            kw.update(habitats=w["habitats"], limit=150.0, weights=(0, 10, 10, 100))
            if variant == "astar_fixLenSOG":
                kw.update(bins=w["bins"], cells=w["cells"], prob=w["prob"], velocity=1.0)
        last_r = 1.5
    first = _checker(variant, starts[0], kw)
    assert first["found"], (variant, n)
    p = first["path"][len(first["path"]) // 2]
    kw["obstacles"] = np.vstack([kw["obstacles"], [[p[0], p[1], last_r]]])
    return kw, starts


@pytest.mark.parametrize("n", [255, 256, 257, 263, 600, 2048])
@pytest.mark.parametrize("variant,pair", [("astar", None), ("astar_real", None), ("astar_fixLen", None),
                                          ("astar_fixLenSOG", "1"), ("astar_fixLenSOG", "0")])
def test_obstacle_counts_around_the_lds_limit(ctx, orc, variant, pair, n, monkeypatch):
    """255 / 256: every obstacle in LDS, 256 filling it; 257 and up: the arrays in memory -- 263 leaves a partial last trip of
    the four-wide collision loop (its clamped index), 600 and 2 048 several 64-lane trips of the smoothing pass's point test.
    A batch of nine and a batch of one (the latency form), both equal to the checker.  The world must discriminate: without
    its last obstacle (n <= 257) and with its first 256 alone (n > 256) the checker finds another result for some instance."""
    if pair is not None:
        monkeypatch.setenv("AUVP_ASTAR_PAIR", pair)
    kw, starts = count_world(variant, n)
    ref = [_checker(variant, s, kw) for s in starts]
    cuts = ([n - 1] if n <= LDS_OBST + 1 else []) + ([LDS_OBST] if n > LDS_OBST else [])
    for m in cuts:
        cut = dict(kw, obstacles=kw["obstacles"][:m])
        assert any(_key(_checker(variant, s, cut)) != _key(o) for s, o in zip(starts, ref)), m
    res = _gpu(ctx, variant, starts, kw)
    for e, (r, o) in enumerate(zip(res, ref)):
        _assert_same(r, o, e)
    assert sum(o["found"] for o in ref) > 0
    one = _gpu(ctx, variant, starts[:1], kw)[0]
    _assert_same(one, ref[0], "latency")


def table_world(variant, H, V, T):
    """a V-gon inside the cell grid, H habitats around the starts (the search closes the last ones), T time bins that hold
    every child's time stamp, the final ones reached by the longest paths"""
    from auv_sim_amd import synth
    # children are at most limit - 10 + 10 sqrt 2 long when the search stops (|pathLen - limit| <= 10): the bins hold them, and the
    # node that stops it lies past the start of bin 8 (T = 9) or 56 (T = 64)
    bin_len, limit = {64: (3, 183.0), 9: (16, 139.0), 1: (300, 100.0)}[T]
    w = synth.make_world(seed=80 + H + V + T, n_obstacles=60, box=(-350.0, -150.0, -50.0, 150.0), obst_radius=(0.5, 2.0), n_bins=T,
                         bin_len=bin_len, n_habitats=0)
    rng = np.random.default_rng(H * 10000 + V * 100 + T)
    cx, cy = -200.0, 0.0
    ang = 2.0 * np.pi * np.arange(V) / V
    poly = np.stack([cx + 145.0 * np.cos(ang), cy + 145.0 * np.sin(ang)], axis=1)  # inside the 300 x 300 m grid of cells
    hab = np.column_stack([cx + rng.uniform(-45.0, 45.0, H), cy + rng.uniform(-45.0, 45.0, H), rng.uniform(8.0, 20.0, H)])
    starts = np.array([(cx + 10.0 * rng.integers(-3, 4), cy + 10.0 * rng.integers(-3, 4)) for _ in range(9)])
    kw = dict(obstacles=w["obstacles"], polygon=poly)
    if variant == "astar_real":
        kw["goal"] = (cx + 30.0, cy + 20.0)
    else:
        kw.update(habitats=hab.reshape(-1, 3), limit=limit, weights=(0, 10, 10, 100))
        if variant == "astar_fixLenSOG":
            kw.update(bins=w["bins"], cells=w["cells"], prob=w["prob"], velocity=1.0)
    return kw, starts


@pytest.mark.parametrize("H,V,T", [(64, 64, 64), (0, 3, 1), (33, 17, 9)])
@pytest.mark.parametrize("variant", ["astar_real", "astar_fixLen", "astar_fixLenSOG"])
def test_world_tables_at_their_limits(ctx, orc, variant, H, V, T, monkeypatch):
    """the shared LDS tables sized by the world, as test_gpu_edge_cases.py::test_exploring_table_sizes does for RRT: the largest
    world auvp_world_set accepts, the smallest, an odd one.  fixLen closes the last habitat (bit H - 1 of the closed mask); SOG
    time stamps reach bin 8 and up (56 and up with 64 bins), both forms of its kernel"""
    kw, starts = table_world(variant, H, V, T)
    ref = [_checker(variant, s, kw) for s in starts]
    assert any(o["status"] == 0 and o["found"] for o in ref)
    if variant == "astar_fixLen" and H:
        assert any(o["status"] == 0 and H - 1 not in o["hab_left"].tolist() for o in ref)
    if variant == "astar_fixLenSOG" and T > 8:
        # the time bin of a time stamp is the first one that holds it (astar_fixLenSOG.py:520-527)
        bins = kw["bins"]
        tb = max(min(t for t in range(T) if bins[t][0] <= ts <= bins[t][1])
                 for o in ref if o["status"] == 0 and o["found"] for ts in o["node_path"][:, 7])
        assert tb >= (56 if T == 64 else 8), tb
    for pair in (("1", "0") if variant == "astar_fixLenSOG" else (None,)):
        if pair is not None:
            monkeypatch.setenv("AUVP_ASTAR_PAIR", pair)
        res = _gpu(ctx, variant, starts, kw)
        for e, (r, o) in enumerate(zip(res, ref)):
            _assert_same(r, o, (pair, e))
        _assert_same(_gpu(ctx, variant, starts[:1], kw)[0], ref[0], (pair, "latency"))

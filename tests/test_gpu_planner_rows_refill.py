"""prrt_rows_kernel rows that take a SECOND episode (and a third, a ninth ...).

The kernel is persistent: a row that finishes its episode stores it, pulls the next id from a device counter and reloads the
generator state, the record and the LDS copy of the occupied list (planner_rows_kernel.h).  The host launches
min(ceil(E / 16), 3 per CU) workgroups of 16 rows, so below 48 episodes per CU every episode has a row of its own and whether
any row refills is a matter of timing.  Option PRRT_ROWS_GRID caps the workgroups: with 16 or 32 rows for 100 / 130 episodes
every row must refill, several times, and every episode is compared with prrt_kernel (bit for bit: records, trees, bucket
lists, paths) and with the checker -- in all four LDS plans of the kernel (obstacle tile in LDS or not x occupied list in LDS
or in memory), two of which no other test launches.  Step mode: many launches on one batch, each of which starts from the
counter value the launches before it left (work_base), with steps whose first 16 pulls are all skipped episodes and a step
that skips every episode."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_OBST = 200
TILE_BYTES = 256 * (8 + 8 + 4) + 16 * 32   # the obstacle slot tables as an LDS tile
EP_BYTES = 624 * 4                         # generator state per episode


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _fields_equal(a, b):
    return all(np.array_equal(a[n], b[n]) for n in a.dtype.names)


def _batch(n_ep):
    """world and batch of test_gpu_planner_rows.py::test_rows_equals_one_episode_kernel"""
    from auv_sim_amd import synth
    w = synth.make_rect_world(seed=3, n_obstacles=N_OBST)
    rng = np.random.default_rng(n_ep)
    starts = np.tile(np.array([w["start"][0], w["start"][1], 0.0, 0.0]), (n_ep, 1))
    starts[:, 2] = rng.uniform(-3.0, 3.0, n_ep)
    # goals all over the box: some are reached within a few steps, some never
    goals = np.column_stack([rng.uniform(w["rect"][0] + 5, w["rect"][2] - 5, n_ep), rng.uniform(w["rect"][1] + 5, w["rect"][3] - 5, n_ep)])
    goals[0] = [w["start"][0] + 6.0, w["start"][1] + 1.0]
    seeds = np.arange(n_ep, dtype=np.uint64) + 11
    return w, starts, goals, seeds


_REF = {}


def _reference(ctx, orc, monkeypatch, n_ep, max_step, cell, subs):
    """the batch on prrt_kernel (records, trees, bucket lists, paths) and in the checker: once per batch, shared by its cases"""
    key = (n_ep, max_step, cell, subs)
    if key not in _REF:
        from auv_sim_amd._prrt_lib import PlannerBatch
        from oracle import orc_planner as op
        w, starts, goals, seeds = _batch(n_ep)
        ctx.set_world(obstacles=w["obstacles"])
        monkeypatch.setenv("AUVP_PRRT_ROWS", "0")
        monkeypatch.setenv("AUVP_PRRT_LAT", "0")
        pa = PlannerBatch(ctx, starts, goals, w["rect"], max_step, seeds=seeds, freq=10, cell=cell, subs=subs)
        a = pa.plan().copy()
        assert ctx.prrt_last_kernel() == "prrt_kernel"
        trees = [pa.tree(e, a[e]) for e in range(n_ep)]
        grids = [pa.grid(e) for e in range(n_ep)]
        paths = [p.copy() for p in pa.paths(a)]
        chk = [op.planning(w["obstacles"], w["rect"], starts[e], goals[e], int(seeds[e]), max_step, 10, cell, subs, kind="portable")
               for e in range(n_ep)]
        _REF[key] = (a, trees, grids, paths, chk)
    return _REF[key]


# (tile, occupied list in LDS): the four LDS plans of the kernel.  The tile goes where three granule-rounded workgroups still fit
# a CU beside it (max_step 200 and 450: yes, 300: no); the occupied list's copy is 16-bit and at most 832 bytes (max_step < 416,
# at most 65 535 buckets).  The last case reaches "occupied list in memory" the second way: 200 x 200 cells x 2 = 80 000 buckets
CASES = [
    pytest.param(1, 1, 130, 200, 5, {}, id="tile-occ_lds"),
    pytest.param(0, 1, 130, 300, 5, {}, id="no_tile-occ_lds"),
    pytest.param(1, 0, 130, 450, 5, {}, id="tile-occ_mem"),
    pytest.param(0, 0, 130, 450, 5, {"AUVP_PRRT_OBST_LDS": "0"}, id="no_tile-occ_mem"),
    pytest.param(1, 0, 100, 200, 1, {}, id="tile-occ_mem-80000_buckets"),
]


@pytest.mark.parametrize("rows_grid", [1, 2])
@pytest.mark.parametrize("tile, occ_lds, n_ep, max_step, cell, env", CASES)
def test_refilled_rows_equal_one_episode_kernel_and_checker(ctx, orc, monkeypatch, tile, occ_lds, n_ep, max_step, cell, env, rows_grid):
    from auv_sim_amd import _lib
    from auv_sim_amd._prrt_lib import PlannerBatch
    subs = 2
    a, ta, ga, paths_a, chk = _reference(ctx, orc, monkeypatch, n_ep, max_step, cell, subs)
    w, starts, goals, seeds = _batch(n_ep)
    ctx.set_world(obstacles=w["obstacles"])
    monkeypatch.setenv("AUVP_PRRT_ROWS", "1")
    monkeypatch.setenv("AUVP_PRRT_LAT", "0")
    monkeypatch.setenv("AUVP_PRRT_ROWS_GRID", str(rows_grid))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pb = PlannerBatch(ctx, starts, goals, w["rect"], max_step, seeds=seeds, freq=10, cell=cell, subs=subs)
    b = pb.plan().copy()
    assert ctx.prrt_last_kernel() == "prrt_rows_kernel"
    # fewer rows than episodes: rows refilled, whatever the timing
    grid, block, lds = ctx.last_launch()
    assert (grid, block) == (rows_grid, 256) and grid * 16 < n_ep
    # ... in the LDS plan the case is about (the host's own answer for this batch, and what it says of the two tables)
    n_buckets = (200 // cell) * (200 // cell) * subs
    plan = _lib.prrt_choose_launch(n_ep, O=N_OBST, freq=10.0, max_step=max_step, n_buckets=n_buckets, rows=True,
                                   options=dict(PRRT_ROWS_GRID=rows_grid, **{k[5:]: int(v) for k, v in env.items()}))
    assert (plan["name"], plan["grid"], plan["lds"], plan["obst_lds"]) == ("prrt_rows_kernel", grid, lds, tile)
    occ_bytes = (lds - tile * TILE_BYTES) // 16 - EP_BYTES
    assert occ_bytes == ((((max_step + 1) * 2 + 15) & ~15) if occ_lds else 0)

    assert (a["status"] == 0).all() and _fields_equal(a, b)
    assert (a["done"] == 1).any() and (a["done"] == 0).any()  # both kinds of episode are in the batch
    assert a["steps"].min() == 1 and a["steps"].max() == max_step
    paths_b = pb.paths(b)
    bad = []
    for e in range(n_ep):
        tb = pb.tree(e, b[e])
        gb = pb.grid(e)
        # the one-episode kernel: every tree array, the occupied list and the counts, the path
        for k in ta[e]:
            if not np.array_equal(ta[e][k], tb[k]):
                bad.append((e, "prrt_kernel", k))
        if not (np.array_equal(ga[e][0], gb[0]) and np.array_equal(ga[e][1], gb[1])):
            bad.append((e, "prrt_kernel", "grid"))
        if not np.array_equal(paths_a[e], paths_b[e]):
            bad.append((e, "prrt_kernel", "path"))
        # the checker, every episode
        r, s = chk[e], b[e]
        if (s["status"], s["steps"], bool(s["done"]), s["n_nodes"], s["n_points"]) != (r["status"], r["steps"], r["done"], r["n_nodes"], r["n_points"]):
            bad.append((e, "checker", "record"))
        if s["rng_after"] != r["rng_after"]:
            bad.append((e, "checker", "rng_after"))
        if not (np.array_equal(tb["parent"], r["parent"]) and np.array_equal(tb["nodes"], r["nodes"][:, :4])
                and np.array_equal(tb["node_bucket"], r["node_bucket"])):
            bad.append((e, "checker", "tree"))
        if r["done"] and not np.array_equal(paths_b[e], r["path"]):
            bad.append((e, "checker", "path"))
    print("refill %s grid %d: %d episodes on %d rows, %d finished, %d mismatches" % (
        (tile, occ_lds), grid, n_ep, grid * 16, int((b["done"] == 1).sum()), len(bad)))
    assert not bad, bad[:10]


def test_step_mode_on_sixteen_rows_over_many_launches(ctx, monkeypatch):
    """generate_one_node stepping of 45 episodes on ONE workgroup (16 rows): every launch hands out ids from where the launches
    before it left the counter (45 episodes + 16 empty pulls each).  Recipe of test_gpu_planner_rows.py's step-mode test (caller-
    chosen buckets, empty buckets, one episode sitting out per step) plus two kinds of step: episodes 0..41 sit out -- the first
    pull of all 16 rows is a skipped episode, so every wavefront draws again without a live row -- and every episode sits out."""
    from auv_sim_amd import synth
    from auv_sim_amd._prrt_lib import PlannerBatch
    w = synth.make_rect_world(seed=5, n_obstacles=128)
    ctx.set_world(obstacles=w["obstacles"])
    E, n_steps = 45, 60
    first_rows_skip, all_skip = (7, 23, 41), (12, 24, 52)
    starts = np.tile(np.array([w["start"][0], w["start"][1], 0.3, 0.0]), (E, 1))
    goals = np.tile(w["goal"], (E, 1))
    seeds = np.arange(E, dtype=np.uint64)
    monkeypatch.setenv("AUVP_PRRT_LAT", "0")
    monkeypatch.setenv("AUVP_PRRT_ROWS_GRID", "1")  # (prrt_kernel does not read it)
    out = {}
    for rows in (False, True):
        monkeypatch.setenv("AUVP_PRRT_ROWS", "1" if rows else "0")
        pb = PlannerBatch(ctx, starts, goals, w["rect"], n_steps + 4, seeds=seeds, freq=10, cell=5, subs=1)
        rng = np.random.default_rng(2)
        log = []
        prev = pb.summaries().copy()
        for i in range(n_steps):
            buckets = np.array([int(rng.choice(pb.grid(e)[0])) if rng.random() < 0.8 else int(rng.integers(0, pb.rows * pb.cols))
                                for e in range(E)], dtype=np.int32)
            buckets[i % E] = -1  # this episode sits the step out
            if i in first_rows_skip:
                buckets[:42] = -1
            if i in all_skip:
                buckets[:] = -1
            out_eps = np.flatnonzero(buckets < 0)
            before = [pb.tree(e, prev[e]) for e in out_eps] if (i in first_rows_skip or i in all_skip) else None
            s = pb.step(buckets).copy()
            assert ctx.prrt_last_kernel() == ("prrt_rows_kernel" if rows else "prrt_kernel")
            if rows:
                assert ctx.last_launch()[:2] == (1, 256)  # 16 rows for 45 episodes
            # the episodes that sit out are untouched: their records, and in the two new kinds of step their trees
            assert _fields_equal(s[out_eps], prev[out_eps]), i
            if before is not None:
                for e, t0 in zip(out_eps, before):
                    t1 = pb.tree(e, s[e])
                    assert all(np.array_equal(t0[k], t1[k]) for k in t0), (i, e)
            if i not in all_skip:
                live = np.flatnonzero((buckets >= 0) & (prev["done"] == 0) & (prev["status"] == 0))
                assert (s["steps"][live] == prev["steps"][live] + 1).all(), i  # ... and every other episode took its step
            log.append(s)
            prev = s
        out[rows] = (log, [pb.tree(e, log[-1][e]) for e in range(E)])
    assert all((s["status"] == 0).all() for s in out[False][0])
    assert out[False][0][-1]["n_nodes"].sum() > 10 * E  # trees grew
    for i, (sa, sb) in enumerate(zip(out[False][0], out[True][0])):
        assert _fields_equal(sa, sb), i
    for ta, tb in zip(out[False][1], out[True][1]):
        for k in ta:
            assert np.array_equal(ta[k], tb[k]), k

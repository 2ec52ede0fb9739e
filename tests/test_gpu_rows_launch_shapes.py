"""The four-episode RRT.exploring kernels (rrt_rows_kernel, rrt_rows_stream_kernel) at the launch shapes the headline runs.

A workgroup of w waves holds 4 w episodes: episode e sits in workgroup e // (4 w), wave (e % (4 w)) // 4, row e % 4, and its LDS
slice is slice (wave, row) of the workgroup's plan, with the obstacle tile after the last slice.  The host sizes w from the batch
(ceil(E / (4 CUs)), at most 12), so only full-chip batches get w > 1; option ROWS_WG_WAVES forces w, and small batches here run
at 2, 7 and 12 waves with a partial last workgroup (whole waves of it exit early).

  a) forced shapes: every episode = the same batch at one wave per workgroup, bit for bit; the checker on every (wave, row) slot
  b) the largest time-bin count the 12-wave plan admits (the last episode's bin counters next to the tile, LDS within 1 KiB of
     160 KiB): the next count falls back to the one-episode kernel
  c) the reference's rectangular time-bin goldens at slot 0 and slot 47 (wave 11, row 3) of a 12-wave workgroup
  d) the shape the host derives at full chip size (12 325 episodes: 12 waves, a workgroup more than the CUs, a partial last one)
  e) bench.py, unchanged, at the shape it times: its dumped results against 1-wave batches and the checker
"""
import json
import os
import subprocess
import sys
from multiprocessing.pool import ThreadPool

import numpy as np
import pytest

from conftest import GOLDEN, golden_world

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from bench_sides.common import RRT_KW, bench_world  # noqa: E402

# (DUO / TRIO off: small batches would otherwise get the latency kernels where a form cannot run)
FORMS = {"rrt_rows_kernel": dict(ROWS=1, ROWS_STREAM=0, DUO=0, TRIO=0),
         "rrt_rows_stream_kernel": dict(ROWS=1, ROWS_STREAM=1, DUO=0, TRIO=0)}
WORKERS = min(16, os.cpu_count() or 1)   # (the checker is a ctypes call: it releases the GIL)
TREE_KEYS = ("nodes", "parent", "pt_off", "pt_cnt", "points")
LDS_LIMIT = 160 * 1024


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _derived_waves(E, n_cu):
    return max(1, min(12, -(-E // (4 * n_cu))))


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _set_world(ctx, w):
    ctx.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"])


def _run(ctx, init, seeds, n_iter, options, named=(), **kw):
    """one batch under `options`: summaries, the kernel and launch it ran, trees of the `named` episodes, every best path"""
    for k, v in options.items():
        ctx.set_option(k, v)
    try:
        summ = ctx.rrt_explore_batch(init, seeds, n_iter, **kw).copy()
        out = dict(summ=summ, kernel=ctx.last_rrt_kernel(), launch=ctx.last_launch(), redone=ctx.pipeline_fallbacks()[0],
                   trees={e: ctx.tree(e, summ[e]) for e in named}, paths=ctx.paths(summ))
    finally:
        for k in options:
            ctx.set_option(k, None)
    return out


def _assert_launch(r, kernel, E, w):
    assert r["kernel"] == kernel and r["redone"] == 0, (r["kernel"], r["redone"])
    grid, block, lds = r["launch"]
    assert (grid, block) == (-(-E // (4 * w)), 64 * w), (r["launch"], E, w)
    assert 0 < lds <= LDS_LIMIT


def _same(a, b, named):
    """every summary field of every episode; trees of the named episodes; every best path -- bit for bit"""
    for f in a["summ"].dtype.names:
        assert np.array_equal(a["summ"][f], b["summ"][f]), f
    for e in named:
        for k in TREE_KEYS:
            assert np.array_equal(a["trees"][e][k], b["trees"][e][k]), (e, k)
    assert len(a["paths"]) == len(b["paths"])
    for e, (pa, pb) in enumerate(zip(a["paths"], b["paths"])):
        assert np.array_equal(pa, pb), e


def _checker(orc, world, seeds, init, n_iter, eps, **kw):
    """the portable checker on episodes `eps`, in a thread pool -> {episode: result}"""
    w = orc.WorldArrays(world["obstacles"], world["habitats"], world["polygon"], world["bins"], world["cells"], world["prob"])
    eps = list(eps)
    with ThreadPool(min(WORKERS, len(eps))) as pool:
        res = pool.map(lambda e: orc.rrt_explore(w, int(seeds[e]), n_iter, init=init[e], kind="portable", **kw), eps)
    return dict(zip(eps, res))


def _same_as_checker(s, r, tree=None, path=None, where=None):
    assert (s["status"], s["n_nodes"], s["n_points"], s["n_leaves"]) == (r["status"], r["n_nodes"], r["n_points"], r["n_leaves"]), where
    assert s["rng_after"] == r["rng_after"] and int(s["n_draw32"]) == int(r["n_draw32"]), where
    if r["status"] == 0:
        assert s["best_leaf"] == r["best_leaf"] and s["best_length"] == r["best_length"], where
        assert np.array_equal(np.asarray(s["best_cost"], dtype=np.float64), r["best_cost"]), where
        if path is not None:
            assert np.array_equal(path, r["path"]), where
    if tree is not None:
        for k in TREE_KEYS:
            assert np.array_equal(tree[k], r[k]), (where, k)


def _slot_sample(E, w, wgs):
    """one live episode per (wave, row) slot of a 4w-episode workgroup, the slots dealt round the workgroups `wgs`"""
    per = 4 * w
    out = []
    for s in range(per):
        live = [g for g in wgs if g * per + s < E]
        out.append(live[s % len(live)] * per + s)
    return out


def _init(world, E, heading=True):
    init = np.zeros((E, 6))
    init[:, 0], init[:, 1] = world["start"]
    if heading:
        init[:, 2] = np.linspace(-3.0, 3.0, E)
    return init


# ---- a) forced shapes at small batches ----------------------------------------------------------------------------------
# w -> E: the last workgroup partial (w = 12: 29 episodes, the last live one wave 7 row 0: waves 8-11 exit early)
SHAPES = {12: 2 * 48 + 29, 7: 28 + 3, 2: 8 * 3 + 6}


def _few_obstacles_world():
    from auv_sim_amd import synth
    return synth.make_world(seed=61, n_obstacles=12)


WORLDS = {"bench_o256": lambda: bench_world(256, 200), "few_o12": _few_obstacles_world}
N_ITER_A = {"bench_o256": 700, "few_o12": 400}
_ref_cache = {}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("w", list(SHAPES))
@pytest.mark.parametrize("wname", list(WORLDS))
def test_forced_waves_equal_one_wave_and_the_checker(ctx, orc, wname, w, form):
    world = WORLDS[wname]()
    _set_world(ctx, world)
    E, n_iter = SHAPES[w], N_ITER_A[wname]
    assert world["obstacles"].shape[0] == (256 if wname == "bench_o256" else 12)
    init = _init(world, E)
    seeds = np.arange(9100, 9100 + E, dtype=np.uint64) * 7919
    n_wg = -(-E // (4 * w))
    sample = sorted(set(_slot_sample(E, w, list(range(n_wg)))) | {0, E - 1})
    last_wg = (n_wg - 1) * 4 * w
    assert any(e >= last_wg for e in sample) and any(e < 4 * w for e in sample)
    got = _run(ctx, init, seeds, n_iter, dict(FORMS[form], ROWS_WG_WAVES=w), named=sample)
    _assert_launch(got, form, E, w)
    one = _run(ctx, init, seeds, n_iter, dict(FORMS[form], ROWS_WG_WAVES=1), named=sample)
    _assert_launch(one, form, E, 1)
    _same(got, one, sample)
    key = (wname, w)
    if key not in _ref_cache:
        _ref_cache[key] = _checker(orc, world, seeds, init, n_iter, sample)
    ref = _ref_cache[key]
    for e in sample:
        _same_as_checker(got["summ"][e], ref[e], got["trees"][e], got["paths"][e], where=(e, e // (4 * w), (e % (4 * w)) // 4, e % 4))


# ---- b) the largest time-bin count the 12-wave plan accepts ---------------------------------------------------------------
def test_largest_bin_count_of_the_twelve_wave_plan(ctx, orc):
    world = bench_world(256, 200)
    _set_world(ctx, world)
    E, w = 48, 12
    init = _init(world, E)
    seeds = np.arange(500, 500 + E, dtype=np.uint64)
    probe = dict(FORMS["rrt_rows_kernel"], ROWS_WG_WAVES=w)
    kw = dict(RRT_KW)
    # from the bench's 100 bins up, one bin at a time (max_traj_time = 5 K at bin_interval = 5), until the host gives up the rows kernel
    K, last = int(round(kw["max_traj_time"] / kw["bin_interval"])), None
    for _ in range(64):
        kw["max_traj_time"] = kw["bin_interval"] * K
        r = _run(ctx, init, seeds, 20, probe, **kw)
        if r["kernel"] != "rrt_rows_kernel":
            break
        last = (K, r["launch"])
        K += 1
    assert last is not None and r["kernel"] == "rrt_explore_kernel", (last, r["kernel"])
    K_max, (_, _, lds) = last
    assert LDS_LIMIT - 1024 < lds <= LDS_LIMIT, (K_max, lds)
    kw["max_traj_time"] = kw["bin_interval"] * K_max
    n_iter, named = 600, [0, 23, 47]
    ref = _checker(orc, world, seeds, init, n_iter, named, **kw)
    for form in FORMS:
        got = _run(ctx, init, seeds, n_iter, dict(FORMS[form], ROWS_WG_WAVES=w), named=named, **kw)
        _assert_launch(got, form, E, w)
        if form == "rrt_rows_kernel":
            assert got["launch"][2] == lds
        one = _run(ctx, init, seeds, n_iter, dict(FORMS[form], ROWS_WG_WAVES=1), named=named, **kw)
        _assert_launch(one, form, E, 1)
        _same(got, one, named)
        for e in named:
            _same_as_checker(got["summ"][e], ref[e], got["trees"][e], got["paths"][e], where=(form, e))


# ---- c) the reference's goldens at slots 0 and 47 of a 12-wave workgroup ----------------------------------------------------
G3_ROWS = ["g3_tb_o64_i500", "g3_tb_o64_i2000", "g3_tb_o256_i500", "g3_tb_o256_i10000", "g3_tb_c40000", "g3_tb_binreset",
           "g3_tb_short_traj", "g3_tb_dense"]


def _g3_args(g):
    return dict(mode=str(g["mode"]), freq=int(g["freq"]), bin_interval=int(g["bin_interval"]), v=int(g["v"]),
                max_traj_time=float(g["max_traj_time"]), weights=g["weights"], dist_to_end=float(g["dist_to_end"]),
                diff_max=float(g["diff_max"]))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", G3_ROWS)
def test_golden_at_the_first_and_last_slot_of_a_twelve_wave_workgroup(ctx, name, form):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    gw = golden_world(g)
    _set_world(ctx, gw)
    E, w, slots = 48, 12, (0, 47)
    init = np.zeros((E, 6))
    init[:, 0], init[:, 1] = g["start"]
    init[:, 2] = np.linspace(-2.5, 2.5, E)
    seeds = np.array([7000 + 13 * e for e in range(E)], dtype=np.uint64)
    for e in slots:
        init[e, 2] = 0.0
        seeds[e] = int(g["seed"])
    n_iter = int(g["n_iter"])
    got = _run(ctx, init, seeds, n_iter, dict(FORMS[form], ROWS_WG_WAVES=w), named=slots, **_g3_args(g))
    _assert_launch(got, form, E, w)
    bins = {e: ctx.bin_sizes(e) for e in slots}
    for e in slots:
        s, t, p = got["summ"][e], got["trees"][e], got["paths"][e]
        assert s["status"] == 0 and s["n_nodes"] == len(g["nodes"]), e
        assert np.array_equal(t["parent"], g["parent"]), e
        assert np.array_equal(t["pt_cnt"][1:] + 1, g["npath"][1:]), e
        assert s["rng_after"] == float(g["rng_after"]), e
        assert s["n_leaves"] == len(g["leaf_iter"]), e
        np.testing.assert_allclose(t["nodes"], g["nodes"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(np.array(s["best_cost"]), g["res_cost"], rtol=0, atol=1e-6)
        assert abs(s["best_length"] - float(g["res_path_length"])) <= 1e-9 * max(1.0, abs(float(g["res_path_length"])))
        assert p.shape == g["res_path"].shape
        np.testing.assert_allclose(p, g["res_path"], rtol=1e-9, atol=1e-9)
        if "bin_sizes" in g.files:
            assert np.array_equal(bins[e], g["bin_sizes"][:len(bins[e])]), e
    one = _run(ctx, init, seeds, n_iter, dict(FORMS[form], ROWS_WG_WAVES=1), named=slots, **_g3_args(g))
    _assert_launch(one, form, E, 1)
    _same(got, one, slots)


# ---- d) the derived shape at full chip size -------------------------------------------------------------------------------
def test_derived_full_chip_shape_both_forms():
    from auv_sim_amd import _lib
    from oracle import orc
    orc.build()
    world = bench_world(256, 200)
    n_cu = _n_cu()
    E, n_iter = 12325, 1000
    w = _derived_waves(E, n_cu)
    per = 4 * w
    n_wg = -(-E // per)
    init = _init(world, E)
    seeds = np.arange(E, dtype=np.uint64) * 3 + 11
    wgs = sorted({0, 1, n_wg // 2, n_wg - 2, n_wg - 1})
    if n_cu == 256:
        assert (w, n_wg, E - (n_wg - 1) * per, wgs) == (12, 257, 37, [0, 1, 128, 255, 256])
    sample = _slot_sample(E, w, wgs)
    assert len(set(e % per for e in sample)) == per
    ctx = _lib.Context(0)     # (a context of its own: no earlier batch with these parameters sizes a stream)
    try:
        _set_world(ctx, world)
        first = _run(ctx, init, seeds, n_iter, dict(ROWS=1), named=sample, **RRT_KW)
        _assert_launch(first, "rrt_rows_kernel", E, w)
        second = _run(ctx, init, seeds, n_iter, dict(ROWS=1), named=sample, **RRT_KW)
        _assert_launch(second, "rrt_rows_stream_kernel", E, w)
        _same(first, second, sample)
        del second
        # the same seeds in batches of at most 1 024 episodes, one wave per workgroup
        for b0 in range(0, E, 1024):
            b1 = min(E, b0 + 1024)
            mine = [e - b0 for e in sample if b0 <= e < b1]
            part = _run(ctx, init[b0:b1], seeds[b0:b1], n_iter, dict(FORMS["rrt_rows_kernel"], ROWS_WG_WAVES=1), named=mine, **RRT_KW)
            _assert_launch(part, "rrt_rows_kernel", b1 - b0, 1)
            for f in first["summ"].dtype.names:
                assert np.array_equal(first["summ"][f][b0:b1], part["summ"][f]), (b0, f)
            for e in mine:
                for k in TREE_KEYS:
                    assert np.array_equal(first["trees"][b0 + e][k], part["trees"][e][k]), (b0 + e, k)
            for e in range(b1 - b0):
                assert np.array_equal(first["paths"][b0 + e], part["paths"][e]), b0 + e
    finally:
        ctx.close()
    ref = _checker(orc, world, seeds, init, n_iter, sample, **RRT_KW)
    for e in sample:
        _same_as_checker(first["summ"][e], ref[e], first["trees"][e], first["paths"][e], where=(e, e // per, (e % per) // 4, e % 4))


# ---- e) bench.py's own results at the shape it times ------------------------------------------------------------------------
def test_bench_dump_at_the_headline_shape(tmp_path):
    from auv_sim_amd import _lib
    from oracle import orc
    orc.build()
    sides, dump = tmp_path / "bench_sides.json", tmp_path / "dump"
    env = dict(os.environ, AUVP_BENCH_SIDES=str(sides))
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    rec = json.load(open(sides))
    E, n_iter = int(rec["config"]["episodes_per_gpu"]), int(rec["config"]["iters"])
    assert n_iter == 10000 and (E == 12288 or E % 6144 == 0), E
    w = _derived_waves(E, _n_cu())
    per = 4 * w
    n_wg = -(-E // per)
    roof = rec["roofline"]
    assert roof["kernel"] == "rrt_rows_stream_kernel"
    assert (roof["launch_grid"], roof["launch_block"]) == (n_wg, 64 * w), (roof["launch_grid"], roof["launch_block"], E, w)
    dumped = {f: np.load(dump / ("summary_%s.npy" % f)) for f in _lib.SUMMARY_DTYPE.names}
    p_eps = np.load(dump / "best_path_episodes.npy").astype(np.int64)
    p_off = np.load(dump / "best_path_offsets.npy").astype(np.int64)
    p_all = np.load(dump / "best_paths.npy")
    dumped_path = {int(e): p_all[p_off[i]:p_off[i + 1]] for i, e in enumerate(p_eps)}
    world = bench_world(256, 200)
    init = _init(world, E, heading=False)
    seeds = np.arange(E, dtype=np.uint64)
    # the same seeds in process: batches of at most 1 024 episodes, one wave per workgroup, the generator inside the kernel
    ctx = _lib.Context(0)
    try:
        _set_world(ctx, world)
        for b0 in range(0, E, 1024):
            b1 = min(E, b0 + 1024)
            part = _run(ctx, init[b0:b1], seeds[b0:b1], n_iter, dict(FORMS["rrt_rows_kernel"], ROWS_WG_WAVES=1), **RRT_KW)
            _assert_launch(part, "rrt_rows_kernel", b1 - b0, 1)
            for f in _lib.SUMMARY_DTYPE.names:
                assert dumped[f].dtype == np.float64
                assert np.array_equal(dumped[f][b0:b1], part["summ"][f].astype(np.float64)), (b0, f)
            for e in range(b0, b1):
                if e in dumped_path:
                    assert np.array_equal(dumped_path[e], part["paths"][e - b0]), e
    finally:
        ctx.close()
    sample = _slot_sample(E, w, sorted({0, n_wg // 2, n_wg - 1}))
    assert len(set(e % per for e in sample)) == per
    ref = _checker(orc, world, seeds, init, n_iter, sample, **RRT_KW)
    for e in sample:
        for f in ("status", "n_nodes", "n_points", "n_leaves", "rng_after", "n_draw32"):
            assert dumped[f][e] == float(ref[e][f]), (e, f, dumped[f][e], ref[e][f])
        if ref[e]["status"] == 0:
            for f in ("best_leaf", "best_length"):
                assert dumped[f][e] == float(ref[e][f]), (e, f, dumped[f][e], ref[e][f])
            assert np.array_equal(dumped["best_cost"][e], ref[e]["best_cost"]), e
            if e in dumped_path:
                assert np.array_equal(dumped_path[e], ref[e]["path"]), e

"""Which kernel a batch gets, and at what shape, asked of the library without a GPU (auvp_rrt_choose_launch /
auvp_prrt_choose_launch: the pure host functions of csrc/launch_plan.h that the handle's own launches go through).

Every expectation is a rule of the host code with its measured threshold: 18 episodes per CU for the four-episode RRT kernels,
8 per CU for two wavefronts per episode, 4 per CU for three, one per CU for the fourth; 12 per CU between Planner_RRT's latency
and throughput batches, 4 per CU for its pipeline.  256 compute units unless a case says otherwise."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from auv_sim_amd import _lib  # noqa: E402

ITER_LOG, LEAF_LOG, PHASE_CLOCKS = _lib.FLAG_ITER_LOG, _lib.FLAG_LEAF_LOG, _lib.FLAG_PHASE_CLOCKS
WORLD = dict(O=256, H=10, V=4, T=10)
BIG = 12288  # 48 episodes per CU: twelve waves of four episodes


def rrt(E, **kw):
    args = dict(WORLD, max_iter=10000, K=100, freq=30.0)
    args.update(kw)
    return _lib.rrt_choose_launch(E, **args)


def round64(n):
    return (max(n, 64) + 63) // 64 * 64


# ---- RRT.exploring: the default choice by batch size ----

@pytest.mark.parametrize("E, name, grid, block", [
    (1, "rrt_trio_kernel<4 wavefronts>", 1, 256),
    (256, "rrt_trio_kernel<4 wavefronts>", 256, 256),
    (257, "rrt_trio_kernel", 129, 384),          # two episodes per workgroup, three wavefronts each
    (1024, "rrt_trio_kernel", 256, 768),
    (1025, "rrt_duo_kernel", 257, 4 * 128),        # five per CU asked for, four per workgroup at most
    (2048, "rrt_duo_kernel", 512, 512),
    (2049, "rrt_explore_kernel", 257, 8 * 64),   # 8 waves per workgroup
    (4608, "rrt_explore_kernel", 576, 8 * 64),
    (4609, "rrt_rows_kernel", 231, 5 * 64),      # 5 waves per workgroup: 20 episodes
    (BIG, "rrt_rows_kernel", 256, 768),
])
def test_rrt_default_by_batch_size(E, name, grid, block):
    p = rrt(E)
    assert (p["status"], p["name"], p["grid"], p["block"]) == (0, name, grid, block)
    assert p["J"] == 4 and p["kflags"] & ~_lib.KFLAG_TIGHT_CULL == 0
    assert p["lds"] <= p["lds_max"] <= 160 * 1024
    assert p["quad"] == (1 if "<4" in name else 0)
    assert (p["stream_len"], p["stream_waves"]) == (0, 0)


def test_rrt_small_explore_batches_get_small_workgroups():
    # the one-episode kernel below eight episodes per CU (forced: by default such batches get two / three wavefronts per episode)
    off = dict(DUO=0, TRIO=0)
    assert [rrt(E, options=off)["block"] for E in (1, 256, 257, 1024, 2048, 2049)] == [64, 64, 128, 256, 512, 512]
    assert rrt(1024, options=off)["grid"] == 256


# ---- the stream form ----

def test_rrt_stream_after_a_batch_was_seen():
    most = 456789
    p = rrt(BIG, seen_E=BIG, seen_most=most)
    assert p["name"] == "rrt_rows_stream_kernel" and p["kind"] == "rows_stream"
    assert p["stream_len"] == round64(most + most * 3 // 100 + 1024)
    waves, mirror, lds = _lib.rows_stream_shape(100, WORLD["H"], WORLD["V"], WORLD["T"], waves_wanted=12)
    assert (p["stream_waves"], bool(p["mirror"]), p["lds"], p["lds_max"]) == (waves, mirror, lds, lds)
    assert (p["grid"], p["block"]) == ((BIG + 4 * waves - 1) // (4 * waves), 64 * waves)
    # a figure from a batch less than a quarter the size does not count
    assert rrt(BIG, seen_E=BIG // 4, seen_most=most)["name"] == "rrt_rows_stream_kernel"
    assert rrt(BIG, seen_E=BIG // 4 - 1, seen_most=most)["name"] == "rrt_rows_kernel"
    # short runs keep the generator inside
    assert rrt(BIG, seen_E=BIG, seen_most=most, max_iter=1000)["name"] == "rrt_rows_stream_kernel"
    assert rrt(BIG, seen_E=BIG, seen_most=most, max_iter=999)["name"] == "rrt_rows_kernel"
    assert rrt(BIG, seen_E=BIG, seen_most=most, no_stream=True)["name"] == "rrt_rows_kernel"
    assert rrt(BIG, seen_E=BIG, seen_most=most, no_stream=True, options=dict(ROWS_STREAM=1))["name"] == "rrt_rows_kernel"


def test_rrt_classic_rows_attribute_is_the_twelve_wave_plan():
    full, part = rrt(BIG), rrt(4609)
    assert full["lds"] == full["lds_max"] == part["lds_max"] and part["lds"] < part["lds_max"]


# ---- the limits of the four-episode and the pipeline kernels ----

ROWS_ONLY_LIMITS = (dict(max_iter=65534), dict(K=200))  # 16-bit node ids; the twelve-wave plan would need more than 160 KiB


@pytest.mark.parametrize("kw", [dict(mode="plantime", K=0), dict(mode="nn", K=0), dict(O=257), dict(freq=31.5), dict(flags=ITER_LOG),
                                dict(flags=PHASE_CLOCKS)] + list(ROWS_ONLY_LIMITS))
def test_rrt_limits_give_the_one_episode_kernel(kw):
    # (an option forces a kernel only where its limits allow; max_iter and K limit the four-episode kernel alone)
    for opts in (None, dict(ROWS=1) if kw in ROWS_ONLY_LIMITS else dict(ROWS=1, DUO=1, TRIO=1)):
        p = rrt(BIG, options=opts, **kw)
        assert (p["status"], p["name"], p["kind"], p["block"]) == (0, "rrt_explore_kernel", "explore", 512), (kw, opts, p)
        assert p["J"] == (8 if kw.get("O") == 257 else 4)
        p = rrt(8, options=dict(opts, ROWS=0) if opts else None, **kw)
        if kw in ROWS_ONLY_LIMITS:  # (limits of the four-episode kernel alone)
            assert p["name"].startswith("rrt_trio_kernel")
        else:
            assert (p["status"], p["name"], p["block"]) == (0, "rrt_explore_kernel", 64), (kw, opts, p)


@pytest.mark.parametrize("O, J", [(0, 1), (64, 1), (65, 2), (128, 2), (129, 4), (256, 4), (257, 8), (512, 8), (513, 16), (1024, 16)])
def test_rrt_obstacles_per_lane(O, J):
    for E in (8, BIG):
        p = rrt(E, O=O, options=dict(ROWS=0, DUO=0, TRIO=0))
        assert (p["name"], p["J"]) == ("rrt_explore_kernel", J)
    if O <= 256:
        assert rrt(8, O=O)["name"].startswith("rrt_trio_kernel") and rrt(8, O=O)["J"] == J
        assert rrt(8, O=O, options=dict(DUO=1))["J"] == J


def test_rrt_leaf_log_keeps_the_four_episode_kernel():
    """the leaf log is a diagnostic of the leaf pass: it keeps a latency batch off the two- / three-wavefront kernels, but not a
    large batch off the four-episode kernel (only the iteration log and the phase clocks do that)"""
    assert rrt(8, flags=LEAF_LOG)["name"] == "rrt_explore_kernel"
    assert rrt(8, flags=LEAF_LOG, options=dict(TRIO=1))["name"] == "rrt_explore_kernel"
    assert rrt(BIG, flags=LEAF_LOG)["name"] == "rrt_rows_kernel"
    assert rrt(BIG, flags=LEAF_LOG | ITER_LOG)["name"] == "rrt_explore_kernel"


def test_rrt_duo_trio_need_a_sub_arc():
    assert rrt(8, freq=0.5)["name"] == "rrt_explore_kernel"   # floor(freq) = 0
    assert rrt(8, freq=1.0)["name"].startswith("rrt_trio_kernel")


def test_rrt_per_episode_limits_force_their_kernel():
    for E in (8, 2000, BIG):
        for opts in (None, dict(ROWS=1), dict(DUO=1), dict(TRIO=1, QUAD=1), dict(ROWS_STREAM=1, ROWS=1)):
            p = rrt(E, lim=True, options=opts)
            assert (p["name"], p["kind"], p["J"]) == ("rrt_explore_lim_kernel", "explore_lim", 4)
    assert rrt(8, lim=True, O=600)["J"] == 16


def test_rrt_one_wave_only_never_a_pipeline():
    for E in (1, 8, 1024, 2048):
        for opts in (None, dict(DUO=1), dict(TRIO=1), dict(DUO=1, TRIO=1)):
            assert rrt(E, one_wave_only=True, options=opts)["name"] == "rrt_explore_kernel"
    assert rrt(BIG, one_wave_only=True)["name"] == "rrt_rows_kernel"


def test_rrt_lds_over_the_limit_is_a_status():
    """auvp_rrt_run fails with "LDS need ... > 160 KiB": of the one-episode kernel's plan for every batch, of the two- /
    three-wavefront plan where that kernel is chosen"""
    p = rrt(8, K=60000)  # one wave per workgroup: (K + 2) * 4 bytes of bins
    assert p["status"] == -1 and p["lds_need"] > 160 * 1024
    assert rrt(8, K=60000, options=dict(ROWS=1))["status"] == -1
    p = rrt(1024, K=5500, options=dict(DUO=0, TRIO=0))
    assert (p["status"], p["name"]) == (0, "rrt_explore_kernel") and p["lds"] <= 160 * 1024
    p = rrt(1024, K=5500)  # four three-wavefront episodes per workgroup
    assert p["status"] == -1 and p["lds_need"] > 160 * 1024


# ---- options, both ways ----

def test_rrt_option_rows():
    p = rrt(8, options=dict(ROWS=1))
    assert (p["name"], p["grid"], p["block"]) == ("rrt_rows_kernel", 2, 64)
    assert rrt(BIG, options=dict(ROWS=0))["name"] == "rrt_explore_kernel"
    # rows excludes the pipelines
    assert rrt(8, options=dict(ROWS=1, DUO=1, TRIO=1))["name"] == "rrt_rows_kernel"


def test_rrt_options_duo_trio_quad():
    assert rrt(8, options=dict(DUO=1))["name"] == "rrt_duo_kernel"          # an explicit DUO = 1 turns trio's default off
    assert rrt(8, options=dict(DUO=1, TRIO=1))["name"].startswith("rrt_trio_kernel")
    assert rrt(8, options=dict(DUO=0))["name"].startswith("rrt_trio_kernel")
    assert rrt(2048, options=dict(DUO=0))["name"] == "rrt_explore_kernel"
    assert rrt(4096, options=dict(DUO=1))["name"] == "rrt_duo_kernel"
    assert rrt(8, options=dict(TRIO=0))["name"] == "rrt_duo_kernel"
    assert rrt(8, options=dict(TRIO=0, DUO=0))["name"] == "rrt_explore_kernel"
    p = rrt(2048, options=dict(TRIO=1))
    assert (p["name"], p["grid"], p["block"]) == ("rrt_trio_kernel", 512, 768)
    p = rrt(1, options=dict(QUAD=0))
    assert (p["name"], p["quad"], p["block"]) == ("rrt_trio_kernel", 0, 192)
    p = rrt(1024, options=dict(QUAD=1))
    assert (p["name"], p["quad"], p["grid"], p["block"]) == ("rrt_trio_kernel<4 wavefronts>", 1, 256, 1024)
    assert rrt(8, options=dict(DUO=1, QUAD=1))["quad"] == 0


def test_rrt_options_of_the_stream():
    seen = dict(seen_E=BIG, seen_most=450000)
    p = rrt(BIG, options=dict(ROWS_STREAM=1))
    assert p["name"] == "rrt_rows_stream_kernel" and p["stream_len"] == round64(int(46.5 * 10000) + 4096)
    assert rrt(BIG, max_iter=16, options=dict(ROWS_STREAM=1))["name"] == "rrt_rows_stream_kernel"
    assert rrt(BIG, max_iter=15, options=dict(ROWS_STREAM=1))["name"] == "rrt_rows_kernel"
    assert rrt(BIG, options=dict(ROWS_STREAM=0), **seen)["name"] == "rrt_rows_kernel"
    assert rrt(8, options=dict(ROWS_STREAM=1))["name"].startswith("rrt_trio_kernel")  # (a form of the four-episode kernel only)
    assert rrt(BIG, options=dict(ROWS_STREAM_CAP=5000), **seen)["stream_len"] == 5056
    assert rrt(BIG, options=dict(ROWS_STREAM_CAP=1), **seen)["stream_len"] == 64
    assert rrt(BIG, options=dict(ROWS_STREAM_CAP=1 << 31), **seen)["name"] == "rrt_rows_kernel"  # positions are 32-bit
    # ROWS_STREAM_WAVES caps the stream form only, ROWS_WG_WAVES feeds both
    p = rrt(BIG, options=dict(ROWS_STREAM_WAVES=6), **seen)
    assert (p["stream_waves"], p["grid"], p["block"]) == (6, 512, 384)
    assert rrt(BIG, options=dict(ROWS_STREAM_WAVES=6))["block"] == 768
    p = rrt(BIG, options=dict(ROWS_WG_WAVES=3), **seen)
    assert (p["stream_waves"], p["grid"], p["block"]) == (3, 1024, 192)
    p = rrt(BIG, options=dict(ROWS_WG_WAVES=3))
    assert (p["name"], p["grid"], p["block"]) == ("rrt_rows_kernel", 1024, 192)
    assert rrt(8, options=dict(ROWS=1, ROWS_WG_WAVES=12))["block"] == 768
    assert rrt(BIG, options=dict(ROWS_WG_WAVES=99))["block"] == 768
    assert rrt(BIG, options=dict(ROWS_WG_WAVES=8, ROWS_STREAM_WAVES=6), **seen)["stream_waves"] == 6
    for force in (0, 1):
        p = rrt(BIG, options=dict(ROWS_STREAM_MIRROR=force), **seen)
        waves, mirror, lds = _lib.rows_stream_shape(100, WORLD["H"], WORLD["V"], WORLD["T"], waves_wanted=12, force=force)
        assert (p["stream_waves"], p["mirror"], p["lds"]) == (waves, force, lds) and mirror == bool(force)


def test_rrt_cull_flags():
    # reach = freq * dist_to_end / 4 = 15; lam = 4 reach^2 O / area = 900 * 256 / area: 0.5 at an area of 460 800
    dense, sparse = dict(obst_area=460000.0), dict(obst_area=461000.0)
    for E in (8, BIG):
        assert rrt(E, **dense)["kflags"] == _lib.KFLAG_TIGHT_CULL
        assert rrt(E, **sparse)["kflags"] == 0
        assert rrt(E, options=dict(TIGHT_CULL=0), **dense)["kflags"] == 0
        assert rrt(E, options=dict(TIGHT_CULL=1), **sparse)["kflags"] == _lib.KFLAG_TIGHT_CULL
        assert rrt(E, options=dict(NN_EXACT=1), **sparse)["kflags"] == _lib.KFLAG_NN_EXACT
        assert rrt(E, options=dict(NN_EXACT=0), **sparse)["kflags"] == 0
    assert rrt(8, obst_area=0.0)["kflags"] == _lib.KFLAG_TIGHT_CULL       # a degenerate box with obstacles: dense
    assert rrt(8, obst_area=0.0, O=0)["kflags"] == 0


def test_rrt_thresholds_follow_the_cu_count():
    assert rrt(304, n_cu=304)["name"] == "rrt_trio_kernel<4 wavefronts>"
    p = rrt(305, n_cu=304)
    assert (p["name"], p["grid"], p["block"]) == ("rrt_trio_kernel", 153, 384)
    assert rrt(18 * 304, n_cu=304)["name"] == "rrt_explore_kernel"
    p = rrt(18 * 304 + 1, n_cu=304)
    assert (p["name"], p["block"]) == ("rrt_rows_kernel", 5 * 64)
    assert rrt(8 * 304, n_cu=304)["name"] == "rrt_duo_kernel" and rrt(8 * 304 + 1, n_cu=304)["name"] == "rrt_explore_kernel"


def test_unknown_option_and_bad_sizes_are_refused():
    with pytest.raises(_lib.AuvpError):
        rrt(8, options=dict(NO_SUCH_OPTION=1))
    with pytest.raises(_lib.AuvpError):
        rrt(0)
    with pytest.raises(_lib.AuvpError):
        _lib.prrt_choose_launch(8, options=dict(AUVP_PRRT_ROWS=1))
    assert set(_lib.OPTION_NAMES) >= {"ROWS", "PRRT_ROWS"}
    for name in _lib.OPTION_NAMES:  # every option of the binding's list is one the library knows
        rrt(8, options={name: 0})


# ---- Planner_RRT ----

def prrt(E, **kw):
    args = dict(O=64, freq=10.0, max_step=300, n_buckets=800)
    args.update(kw)
    return _lib.prrt_choose_launch(E, **args)


@pytest.mark.parametrize("E, name, grid, block, lat", [
    (512, "prrt_pipe_kernel", 256, 640, 1),    # two five-wavefront episodes per workgroup
    (768, "prrt_pipe_kernel", 256, 960, 1),    # three
    (769, "prrt_pipe_kernel", 193, 1024, 1),   # four episodes of four wavefronts
    (1024, "prrt_pipe_kernel", 256, 1024, 1),
    (1025, "prrt_kernel", 257, 256, 1),
    (3072, "prrt_kernel", 768, 256, 1),
    (3073, "prrt_rows_kernel", 193, 256, 0),
    (16384, "prrt_rows_kernel", 768, 256, 0),  # min(ceil(E / 16), three workgroups per CU)
])
def test_prrt_default_by_batch_size(E, name, grid, block, lat):
    p = prrt(E)
    assert (p["status"], p["name"], p["grid"], p["block"], p["lat"]) == (0, name, grid, block, lat)
    assert p["J"] == 1 and p["lds"] <= 160 * 1024
    assert p["draw_wave"] == (1 if name == "prrt_pipe_kernel" and E <= 768 else 0)
    assert p["rows"] == (1 if name == "prrt_rows_kernel" else 0)
    if name == "prrt_pipe_kernel":
        assert (p["next_lds"], p["bk_lds"]) == (1, 1)


def test_prrt_latency_batches_get_small_workgroups():
    assert [prrt(E, options=dict(PRRT_PIPE=0))["block"] for E in (1, 256, 257, 512, 768, 1024)] == [64, 64, 128, 128, 192, 256]


def test_prrt_pipeline_only_where_the_call_plans_and_waits():
    assert prrt(512, step_mode=1)["name"] == "prrt_kernel"
    assert prrt(512, waits=False)["name"] == "prrt_kernel"
    assert prrt(512, step_mode=1, waits=False, options=dict(PRRT_PIPE=1))["name"] == "prrt_kernel"
    assert prrt(512, one_wave_only=True, options=dict(PRRT_PIPE=1))["name"] == "prrt_kernel"
    assert prrt(512, flags=ITER_LOG)["name"] == "prrt_kernel"
    assert prrt(512, O=257)["name"] == "prrt_kernel" and prrt(512, O=256)["J"] == 4
    assert prrt(512, freq=31.0)["name"] == "prrt_kernel"
    assert prrt(512, rows=True)["name"] == "prrt_rows_kernel"


def test_prrt_rows_limits_and_the_frozen_choice():
    for kw in (dict(freq=16.0), dict(O=257), dict(flags=ITER_LOG)):
        for opts in (None, dict(PRRT_ROWS=1)):
            p = prrt(4096, options=opts, **kw)
            assert (p["name"], p["rows"], p["lat"], p["grid"], p["block"]) == ("prrt_kernel", 0, 0, 1024, 256), (kw, opts)
    assert [prrt(4096, O=O, options=dict(PRRT_ROWS=0))["J"] for O in (64, 65, 128, 129, 256)] == [1, 2, 2, 4, 4]
    assert [prrt(512, O=O)["J"] for O in (64, 65, 128, 129, 256)] == [1, 2, 2, 4, 4]  # (the pipeline's)
    assert [prrt(4096, O=O)["J"] for O in (257, 512, 513, 1024)] == [8, 8, 16, 16]
    # the batch's choice is frozen when it is created: a launch is told, whatever the options say by then
    assert prrt(4096, rows=False)["name"] == "prrt_kernel"
    assert prrt(4096, rows=False, options=dict(PRRT_ROWS=1))["name"] == "prrt_kernel"
    assert prrt(512, rows=True, options=dict(PRRT_ROWS=0))["name"] == "prrt_rows_kernel"


def _rows_lds(max_step, tile):
    occ = ((max_step + 1) * 2 + 15) & ~15
    return 16 * (624 * 4 + (occ if occ <= 832 else 0)) + (256 * (8 + 8 + 4) + 16 * 32 if tile else 0)


def test_prrt_obstacle_tile_where_three_granule_rounded_workgroups_fit():
    def three_fit(b):
        return 3 * ((b + 1279) // 1280 * 1280) <= 160 * 1024
    assert three_fit(_rows_lds(255, True)) and not three_fit(_rows_lds(256, True))  # 53 760 B / 54 016 B: 42 / 43 granules
    p = prrt(4096, max_step=255)
    assert (p["obst_lds"], p["lds"]) == (1, _rows_lds(255, True)) and p["lds"] == 53760
    p = prrt(4096, max_step=256)
    assert (p["obst_lds"], p["lds"]) == (0, _rows_lds(256, False))
    assert prrt(4096, max_step=255, options=dict(PRRT_OBST_LDS=0))["lds"] == _rows_lds(255, False)
    p = prrt(4096, max_step=256, options=dict(PRRT_OBST_LDS=1))
    assert (p["obst_lds"], p["lds"]) == (1, _rows_lds(256, True))
    # the occupied list's LDS copy: 16-bit entries, at most 832 bytes
    assert prrt(4096, max_step=500)["lds"] == _rows_lds(500, True) == 16 * 624 * 4 + 5632
    assert prrt(4096, max_step=255, n_buckets=65536)["lds"] == 16 * 624 * 4 + 5632


def test_prrt_options():
    p = prrt(512, options=dict(PRRT_LAT=0))
    assert (p["name"], p["lat"], p["rows"]) == ("prrt_rows_kernel", 0, 1)
    p = prrt(4096, options=dict(PRRT_LAT=1))
    assert (p["name"], p["lat"], p["grid"], p["block"]) == ("prrt_kernel", 1, 1024, 256)
    assert prrt(512, options=dict(PRRT_ROWS=1))["name"] == "prrt_rows_kernel"
    p = prrt(4096, options=dict(PRRT_ROWS=0))
    assert (p["name"], p["lat"]) == ("prrt_kernel", 0)
    p = prrt(512, options=dict(PRRT_PIPE=0))
    assert (p["name"], p["grid"], p["block"]) == ("prrt_kernel", 256, 128)
    p = prrt(2048, options=dict(PRRT_PIPE=1))
    assert (p["name"], p["eps_wg"], p["grid"], p["block"]) == ("prrt_pipe_kernel", 4, 512, 1024)
    assert prrt(4096, options=dict(PRRT_PIPE=1, PRRT_ROWS=0))["name"] == "prrt_kernel"  # (a latency batch's kernel)
    assert prrt(4096, options=dict(PRRT_PIPE=1, PRRT_LAT=1))["name"] == "prrt_pipe_kernel"
    p = prrt(512, options=dict(PRRT_PIPE_DRAW=0))
    assert (p["draw_wave"], p["block"]) == (0, 512)
    assert prrt(1024, options=dict(PRRT_PIPE_DRAW=1))["draw_wave"] == 0  # (five wavefronts x four episodes: over 1 024 threads)
    full = prrt(512)
    no_next, no_bk = prrt(512, options=dict(PRRT_NEXT_LDS=0)), prrt(512, options=dict(PRRT_BUCKET_LDS=0))
    assert (no_next["next_lds"], no_next["bk_lds"]) == (0, 1) and (no_bk["next_lds"], no_bk["bk_lds"]) == (1, 0)
    assert full["lds"] - no_next["lds"] == 2 * ((301 * 4 + 15) & ~15)
    assert full["lds"] - no_bk["lds"] == 2 * (800 * 8 + ((301 * 4 + 15) & ~15))
    for k in ("PRRT_NEXT_LDS", "PRRT_BUCKET_LDS"):
        assert prrt(512, options={k: 1})["lds"] == full["lds"]
    # where the tables do not fit beside the slots they stay in memory, option or not
    big = prrt(512, n_buckets=20000, options=dict(PRRT_BUCKET_LDS=1))
    assert (big["next_lds"], big["bk_lds"]) == (1, 0)


def test_prrt_rows_grid_option_only_lowers_the_grid():
    """PRRT_ROWS_GRID: at most that many workgroups for prrt_rows_kernel, at least one (tests: fewer rows than episodes, so that
    every batch refills its rows from the work counter); nothing else of the plan moves, and the other kernels ignore it"""
    full, small = prrt(16384), prrt(3073)
    assert (full["grid"], small["grid"]) == (768, 193)
    p = prrt(16384, options=dict(PRRT_ROWS_GRID=2))
    assert p["grid"] == 2 and {k: v for k, v in p.items() if k != "grid"} == {k: v for k, v in full.items() if k != "grid"}
    assert prrt(3073, options=dict(PRRT_ROWS_GRID=192))["grid"] == 192
    # a cap at or above the default leaves it
    for cap in (768, 769, 100000, 1 << 40):
        assert prrt(16384, options=dict(PRRT_ROWS_GRID=cap)) == full
    for cap in (193, 194, 768):
        assert prrt(3073, options=dict(PRRT_ROWS_GRID=cap)) == small
    # below 1 counts as 1
    for cap in (1, 0, -3):
        assert prrt(16384, options=dict(PRRT_ROWS_GRID=cap))["grid"] == 1
        assert prrt(3073, options=dict(PRRT_ROWS_GRID=cap))["grid"] == 1
    # forced rows batches, step mode and enqueue-only launches: the same rule
    assert prrt(130, options=dict(PRRT_ROWS=1, PRRT_LAT=0))["grid"] == 9
    assert prrt(130, options=dict(PRRT_ROWS=1, PRRT_LAT=0, PRRT_ROWS_GRID=2))["grid"] == 2
    assert prrt(45, rows=True, step_mode=1, options=dict(PRRT_ROWS_GRID=1))["grid"] == 1
    assert prrt(40, rows=True, step_mode=1, waits=False, options=dict(PRRT_ROWS_GRID=1))["grid"] == 1
    assert prrt(100000, n_cu=304, options=dict(PRRT_ROWS_GRID=5000))["grid"] == 3 * 304
    # prrt_kernel / prrt_pipe_kernel plans do not read it
    for E in (512, 769, 1025, 3072):
        for cap in (1, 0, 2):
            assert prrt(E, options=dict(PRRT_ROWS_GRID=cap)) == prrt(E), (E, cap)
    assert prrt(4096, options=dict(PRRT_ROWS=0, PRRT_ROWS_GRID=1)) == prrt(4096, options=dict(PRRT_ROWS=0))
    assert "PRRT_ROWS_GRID" in _lib.OPTION_NAMES


def test_prrt_thresholds_follow_the_cu_count():
    assert prrt(12 * 304, n_cu=304)["name"] == "prrt_kernel" and prrt(12 * 304 + 1, n_cu=304)["name"] == "prrt_rows_kernel"
    assert prrt(4 * 304, n_cu=304)["name"] == "prrt_pipe_kernel" and prrt(4 * 304 + 1, n_cu=304)["name"] == "prrt_kernel"
    assert prrt(100000, n_cu=304)["grid"] == 3 * 304

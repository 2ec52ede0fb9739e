"""The two forms of rrt_rows_stream_kernel's LDS ring (option ROWS_STREAM_MIRROR; rrt_rows_stream_kernel.h):

mirrored  the ring's first 48 entries a second time behind it: a lane keeps one LDS address per window and reads at immediates;
masked    every read forms (position + j) & 255.
Same numbers at the same places of the algorithm: both must equal rrt_rows_kernel (the generator inside the kernel) bit for bit,
summaries (n_draw32, rng_after, iters_run among them) and trees, also for episodes that stop early -- a row that fails inside a
steer pass reports the stream position it had before the pass."""
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

TREE_KEYS = ("nodes", "parent", "pt_off", "pt_cnt", "points")
FORMS = {"mirrored": 1, "masked": 0}


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _set_world(ctx, w):
    ctx.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"])


def _run(ctx, init, seeds, n_iter, options, named, **kw):
    opts = dict(ROWS=1, DUO=0, TRIO=0)
    opts.update(options)
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        summ = ctx.rrt_explore_batch(init, seeds, n_iter, **kw).copy()
        return dict(summ=summ, kernel=ctx.last_rrt_kernel(), mirror=ctx.last_stream_mirror(), launch=ctx.last_launch(),
                    redone=ctx.pipeline_fallbacks()[0], trees={e: ctx.tree(e, summ[e]) for e in named})
    finally:
        for k in opts:
            ctx.set_option(k, None)


def _same(a, b, named, what):
    for f in a["summ"].dtype.names:
        assert np.array_equal(a["summ"][f], b["summ"][f]), (what, f)
    for e in named:
        for k in TREE_KEYS:
            assert np.array_equal(a["trees"][e][k], b["trees"][e][k]), (what, e, k)


def _three_ways(ctx, init, seeds, n_iter, named, extra=None, **kw):
    """the batch on rrt_rows_kernel, then on the stream kernel with the mirrored and with the masked ring (the stream as long as
    the busiest episode needs, + 64): the three results, compared"""
    extra = dict(extra or {})
    classic = _run(ctx, init, seeds, n_iter, dict(extra, ROWS_STREAM=0), named, **kw)
    assert classic["kernel"] == "rrt_rows_kernel" and classic["mirror"] == -1
    cap = int(classic["summ"]["n_draw32"].max()) // 2 + 64
    out = {"classic": classic}
    for form, flag in FORMS.items():
        r = _run(ctx, init, seeds, n_iter, dict(extra, ROWS_STREAM=1, ROWS_STREAM_CAP=cap, ROWS_STREAM_MIRROR=flag), named, **kw)
        assert r["kernel"] == "rrt_rows_stream_kernel" and r["redone"] == 0 and r["mirror"] == flag, (form, r["kernel"], r["redone"], r["mirror"])
        _same(r, classic, named, form)
        out[form] = r
    return out


def _init(world, E):
    init = np.zeros((E, 6))
    init[:, 0], init[:, 1] = world["start"]
    init[:, 2] = np.linspace(-3.0, 3.0, E)
    return init


# ---- 1. mirrored = masked = rrt_rows_kernel ---------------------------------------------------------------------------------
# freq = 1 looks at the leaves after every iteration (~92 numbers per iteration: the ring wraps most often), 30 runs two full passes
@pytest.mark.parametrize("freq", [1, 8, 15, 30])
@pytest.mark.parametrize("E", [37, 400])
def test_both_ring_forms_equal_the_classic_kernel(ctx, E, freq):
    from auv_sim_amd import synth
    world = synth.make_world(seed=51, n_obstacles=64)
    _set_world(ctx, world)
    n_iter = 700 if E == 37 else 300
    seeds = np.arange(6000, 6000 + E, dtype=np.uint64) * 31
    named = sorted(set(range(0, E, 29)) | {E - 1})
    r = _three_ways(ctx, _init(world, E), seeds, n_iter, named, freq=freq)
    assert (r["classic"]["summ"]["status"] >= 0).all()
    per_iter = r["classic"]["summ"]["n_draw32"].mean() / 2 / n_iter
    if freq == 1:
        assert per_iter > 60, per_iter


def test_both_ring_forms_at_twelve_waves_and_the_largest_bin_count_the_host_admits(ctx):
    """the host runs the four-episode kernels where rrt_rows_kernel's twelve-wave plan fits, and its generator state is larger than
    the mirrored ring: no world the host gives to this kernel makes its rule fall back to the masked form
    (tests/test_stream_ring_plan.py checks the rule itself beyond that).  So: the largest K the host admits, twelve-wave
    workgroups -- the rule's choice is the mirror, within the LDS limit; the masked form by option; both equal the classic kernel"""
    from auv_sim_amd import _lib
    from bench_sides.common import RRT_KW, bench_world
    world = bench_world(256, 200)
    _set_world(ctx, world)
    E = 48 + 37
    init, seeds = _init(world, E), np.arange(E, dtype=np.uint64) + 77
    kw = dict(RRT_KW)
    K = int(round(kw["max_traj_time"] / kw["bin_interval"]))
    probe = dict(ROWS=1, ROWS_STREAM=0, DUO=0, TRIO=0, ROWS_WG_WAVES=12)
    last = None
    for _ in range(64):
        kw["max_traj_time"] = kw["bin_interval"] * K
        if _run(ctx, init, seeds, 20, probe, (), **kw)["kernel"] != "rrt_rows_kernel":
            break
        last = K
        K += 1
    assert last is not None
    kw["max_traj_time"] = kw["bin_interval"] * last
    named = [0, 47, 48, E - 1]
    r = _three_ways(ctx, init, seeds, 400, named, extra=dict(ROWS_WG_WAVES=12), **kw)
    auto = _run(ctx, init, seeds, 400, dict(ROWS_STREAM=1, ROWS_WG_WAVES=12), named, **kw)
    assert auto["kernel"] == "rrt_rows_stream_kernel" and auto["mirror"] == 1
    assert auto["launch"][:2] == (2, 12 * 64) and auto["launch"][2] <= 160 * 1024
    assert auto["launch"] == r["mirrored"]["launch"] and r["masked"]["launch"][2] == auto["launch"][2] - 48 * 48 * 8
    ws = ctx.world_sizes
    assert _lib.rows_stream_shape(last, ws["H"], ws["V"], ws["T"], 12) == (12, True, auto["launch"][2])
    _same(auto, r["classic"], named, "auto")


@pytest.mark.parametrize("consumed", [77, 312])
def test_both_ring_forms_on_a_continued_generator(ctx, consumed):
    from auv_sim_amd import synth
    world = synth.make_world(seed=59, n_obstacles=64)
    _set_world(ctx, world)
    E = 9
    words, idx = [], []
    for e in range(E):
        rnd = random.Random(900 + e)
        for _ in range(consumed + 3 * e):
            rnd.random()
        if e % 2 == 1:
            rnd.getrandbits(32)
        st = rnd.getstate()[1]
        words.append(st[:624])
        idx.append(st[624])
    seeds = (np.array(words, dtype=np.uint32), np.array(idx, dtype=np.int32))
    _three_ways(ctx, _init(world, E), seeds, 700, list(range(E)))


# ---- 2. the host's choice at the headline's parameters -------------------------------------------------------------------------
def test_the_headline_shape_takes_the_mirrored_ring():
    from auv_sim_amd import _lib
    from bench_sides.common import RRT_KW, bench_world
    import torch
    world = bench_world(256, 200)
    E, n_iter = 12288, 24
    ctx = _lib.Context(0)
    try:
        _set_world(ctx, world)
        init = np.zeros((E, 6))
        init[:, 0], init[:, 1] = world["start"]
        seeds = np.arange(E, dtype=np.uint64)
        named = [0, 47, 6000, E - 1]
        a = _run(ctx, init, seeds, n_iter, dict(ROWS_STREAM=1), named, **RRT_KW)
        w = max(1, min(12, -(-E // (4 * torch.cuda.get_device_properties(0).multi_processor_count))))
        assert a["kernel"] == "rrt_rows_stream_kernel" and a["mirror"] == 1 and a["redone"] == 0
        grid, block, lds = a["launch"]
        assert (grid, block) == (-(-E // (4 * w)), 64 * w) and 0 < lds <= 160 * 1024
        if w == 12:
            ws = ctx.world_sizes
            assert lds == _lib.rows_stream_shape(100, ws["H"], ws["V"], ws["T"], 12)[2] <= 163840
        b = _run(ctx, init, seeds, n_iter, dict(ROWS_STREAM=0), named, **RRT_KW)
        _same(a, b, named, "headline")
    finally:
        ctx.close()


# ---- 3. episodes that stop early report the position the classic kernel reports ------------------------------------------------
def test_capacity_stops_report_the_classic_position(ctx):
    """(the parameters of test_gpu_rows_stream.py's point_capacity_overflow) the point store of an episode overflows inside a steer
    pass: status -2, and the stream position reported is the one before that pass"""
    from auv_sim_amd import synth
    world = synth.make_world(seed=58, n_obstacles=8)
    _set_world(ctx, world)
    E = 6
    r = _three_ways(ctx, _init(world, E), np.arange(4000, 4000 + E, dtype=np.uint64), 400, list(range(E)), points_per_iter=3.0)
    s = r["classic"]["summ"]
    assert (s["status"] == -2).any() and (s["iters_run"][s["status"] == -2] < 400).all()
    for form in FORMS:
        for f in ("status", "n_draw32", "rng_after", "iters_run"):
            assert np.array_equal(r[form]["summ"][f], s[f]), (form, f)


def _untemper(y):
    """the 32-bit state word MT19937 tempers to y"""
    y ^= y >> 18
    y ^= (y << 15) & 0xEFC60000
    t = y
    for _ in range(5):
        t = y ^ ((t << 7) & 0x9D2C5680)
    y = t & 0xFFFFFFFF
    t = y
    for _ in range(3):
        t = y ^ (t >> 11)
    return t & 0xFFFFFFFF


def test_key_errors_report_the_classic_position(ctx):
    """A bin key beyond K (the reference's KeyError, status -5) needs int(1 + K u) = K + 1: with K = 4 the largest random(),
    u = 1 - 2^-53, gives 1 + (4 - 2^-51) = 5 - 2^-51, a tie that rounds to 5.  Generators handed over with that number planted at
    draw 0, 1 and 5 of the first selection round (the draws before it land in empty bins), beside ordinary episodes."""
    from auv_sim_amd import synth
    world = synth.make_world(seed=51, n_obstacles=64)
    _set_world(ctx, world)
    top, mid = _untemper(0xFFFFFFFF), _untemper(0x80000000)
    E, planted = 8, {0: 0, 1: 1, 2: 5}
    words, idx = [], []
    for e in range(E):
        rnd = random.Random(300 + e)
        st = list(rnd.getstate()[1])
        if e in planted:
            w = st[:624]
            for d in range(planted[e]):
                w[2 * d], w[2 * d + 1] = mid, mid      # u = 0.5 + 2^-28: bin 3, empty at the first iteration
            w[2 * planted[e]], w[2 * planted[e] + 1] = top, top
            check = random.Random()
            check.setstate((3, tuple(w) + (0,), None))
            got = [check.random() for _ in range(planted[e] + 1)]
            assert got[-1] == 1.0 - 2.0 ** -53 and all(int(1.0 + 4.0 * g) == 3 for g in got[:-1])
            assert int(1.0 + 4.0 * got[-1]) == 5
            words.append(w)
            idx.append(0)
        else:
            rnd.random()
            st = rnd.getstate()[1]      # (a state that has been twisted once: index < 624)
            words.append(list(st[:624]))
            idx.append(st[624])
    seeds = (np.array(words, dtype=np.uint32), np.array(idx, dtype=np.int32))
    r = _three_ways(ctx, _init(world, E), seeds, 300, list(range(E)), max_traj_time=20.0, bin_interval=5)
    s = r["classic"]["summ"]
    for e in planted:
        assert s["status"][e] == -5 and s["iters_run"][e] == 0 and s["n_draw32"][e] == 0, (e, s[e])
    assert (s["status"][len(planted):] != -5).all()
    for form in FORMS:
        for f in ("status", "n_draw32", "rng_after", "iters_run"):
            assert np.array_equal(r[form]["summ"][f], s[f]), (form, f)

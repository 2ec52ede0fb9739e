"""k filter steps per round, measured along the bucket every AUV committed last: replan_measure_ticks_kernel (option MEAS_TICKS,
Context.replan_measure with shark_xy [k,F,2]) and FleetTracker(filter_steps=k), on the fleet of test_gpu_fleet_tracker.py --
eight AUVs, two sharks x four trackers, 64 particles, 300 iterations, three rounds -- with k = 3.
  * the table [3,F,A,5], downloaded after every round, against tracking.fleet_measurements_ticks on the downloaded trajectory:
    x, y, theta and range bit for bit, the bearings too (below); the last tick is the committed state; round 0 measures from
    the start states at every tick;
  * shark_xy[None] (option set to 1, the new kernel) against the plain call (the old kernel), all five columns bit for bit;
  * an AUV that plans round 0 only repeats its last state at every tick from round 2 on;
  * FleetTracker(measure="device", filter_steps=3) against measure="host" after every step and at the end, and filter_steps=1
    against the argument left out, bit for bit;
  * the refusals leave the option and the last table as they were.
The sharks stand still during round 0 (its k samples are the start position), so that the special start positions of that fleet
-- an AUV at its shark, the shark due west, a hair north of the cut -- keep their exact values at every tick; from then on they
move a third of the fleet's step per sample.

The bearings are compared bit for bit with math.atan2, as test_gpu_fleet_tracker.py does (its docstring: this libm's last bit is
off for about 7 pairs in 10 000); every test prints how many of its bearings differed before it asserts."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_fleet_tracker import (A, BUDGET, F, INTERVAL, LENGTH, N, N_ITER, N_PARTICLES, R_FORECAST, ROUNDS, SEEDS, SHARK_OF, T_START,
                                    _B, _bits, _free, _ulps)
from test_gpu_replan_commit import _same_arrays, _world

pytestmark = pytest.mark.gpu

K_TICKS = 3
T_LATE = 350.0  # an AUV that starts here commits up to t = 450 in round 0, and 450 + 100 is past the horizon's end (500)
SPAN = BUDGET + INTERVAL


def _setup_ticks(measure, K=1, filter_steps=K_TICKS, late=None):
    """test_gpu_fleet_tracker._setup with (ROUNDS + 1) * k samples per track (k = filter_steps, 1 where it is None: the argument is
    left out) and, with late = e, AUV e starting at T_LATE"""
    from auv_sim_amd import _lib, _pf_lib
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    from auv_sim_amd.rrt_dubins import RRT
    from auv_sim_amd.sharkForecast import SharkForecast
    from auv_sim_amd.tracking import FleetTracker
    k = filter_steps or 1
    g = np.load(os.path.join(GOLDEN, "g13_replan_a.npz"))
    obstacles, habitats, cell_list, grids, poly = _world(g)
    rng = np.random.default_rng(5)
    base = []
    while len(base) < F:
        x, y = rng.uniform(-260, -140), rng.uniform(-60, 60)
        if all(_free(g, x + dx, y + dy) for dx in (-30.0, 0.0, 25.0, 25.0) for dy in (0.0, 1e-9)):
            base.append((x, y))
    # sample s: the sharks stand still for the k samples of round 0, then move 4 / k and 3 / k metres per sample
    moved = [max(0, s - (k - 1)) / k for s in range((ROUNDS + 1) * k)]
    tracks = np.array([[(bx + 4.0 * m, by - 3.0 * m * (1 - 2 * f)) for m in moved] for f, (bx, by) in enumerate(base)])
    starts = [None] * N
    sx, sy = tracks[0, 0]
    for e, (dx, dy) in zip((1, 3, 4, 7), ((0.0, 0.0), (25.0, 0.0), (25.0, 1e-9), (-30.0, 0.0))):
        starts[e] = MPS(sx + dx, sy + dy, theta=0.0, traj_time_stamp=T_START)
    for e in range(N):
        if starts[e] is None:
            h = g["habitats"][e]
            starts[e] = MPS(h[0], h[1], theta=0.3 * e, traj_time_stamp=T_LATE if e == late else T_START)
    rrt = RRT(poly, obstacles, grids[0], cell_list)
    fctx = _lib.Context(0)
    mts = np.stack([_pf_lib.np_seed_state(100 + f)[0] for f in range(F)])
    filters = _pf_lib.FilterBatch(fctx, F, N_PARTICLES).create(tracks[:, 0, :], mts, 624)
    sf = SharkForecast(_B(-300, -100, -100, 100), 10, cell_list, device_context=fctx)
    extra = {} if filter_steps is None else dict(filter_steps=filter_steps)
    tr = FleetTracker(rrt, sf, filters, tracks, SHARK_OF, np.ones((sf.n_row, sf.n_col)), R_FORECAST, measure=measure,
                      starts=starts, habitats=habitats, plan_time_budget=BUDGET, traj_time_length=LENGTH, replan_time_interval=INTERVAL,
                      weight=[-3, -3, -4], max_iter=N_ITER, seeds=SEEDS, trees_per_auv=K, **extra)
    return tr, tracks


def _sharks(tracks, r, k=K_TICKS):
    return np.ascontiguousarray(tracks[:, r * k:(r + 1) * k].transpose(1, 0, 2))


def _measured_rounds(late=None):
    """ROUNDS rounds of the session with, before each, the table with k = 3, the definition on the downloaded trajectory, and the
    two k = 1 forms at the round's last sample"""
    from auv_sim_amd.tracking import fleet_measurements_ticks
    tr, tracks = _setup_ticks("device", late=late)
    ctx, s = tr.rrt._ctx, tr.session
    out = []
    for r in range(ROUNDS):
        shark = _sharks(tracks, r)
        assert ctx.replan_measure(SHARK_OF, A, shark)
        got = ctx.replan_meas()
        segs = s.last_segments()
        want = fleet_measurements_ticks(segs, s.last, SHARK_OF, shark, s.round_span)
        assert ctx.replan_measure(SHARK_OF, A, shark[-1])
        plain = ctx.replan_meas()
        assert ctx.replan_measure(SHARK_OF, A, shark[-1:])
        one = ctx.replan_meas()
        out.append(dict(got=got, want=want, plain=plain, one=one, last=s.last.copy(), n=[len(x) for x in segs], shark=shark,
                        option=ctx.get_option("MEAS_TICKS")))
        rec = s.round()
        assert rec is not None
        out[-1]["auv"] = rec["auv"]
    s.finish()
    return out


@pytest.fixture(scope="module")
def rounds():
    return _measured_rounds()


def _compare_tables(rs, tag):
    bad, worst, total = 0, 0, 0
    for r, d in enumerate(rs):
        assert d["got"].shape == d["want"].shape == (K_TICKS, F, A, 5), (tag, r)
        assert np.array_equal(_bits(d["got"][..., :4]), _bits(d["want"][..., :4])), (tag, r)  # x, y, theta, range
        u = _ulps(d["got"][..., 4], d["want"][..., 4])
        bad, worst, total = bad + int((u != 0).sum()), max(worst, int(u.max())), total + u.size
    print("%s: bearings that differ from math.atan2: %d of %d, at most %d ulp" % (tag, bad, total, worst))
    for r, d in enumerate(rs):
        assert np.array_equal(_bits(d["got"]), _bits(d["want"])), (tag, r)


def test_table_equals_the_definition(rounds):
    _compare_tables(rounds, "k = 3")
    assert rounds[0]["n"] == [0] * N and all(max(d["n"]) > 1 for d in rounds[1:])  # nothing committed yet; then whole buckets
    g0 = rounds[0]["got"]
    for j in range(K_TICKS):  # round 0: every tick from the start states -- at the shark; due west; a hair north; west of it
        assert np.array_equal(_bits(g0[j, ..., :3]), _bits(g0[0, ..., :3]))
        assert g0[j, 0, 0, 3] == 0.0 and g0[j, 0, 0, 4] == 0.0 and g0[j, 0, 1, 4] == np.pi and g0[j, 0, 3, 4] == 0.0
        assert -np.pi < g0[j, 0, 2, 4] < -3.14159
    # later rounds: the ticks are different rows of the bucket (an AUV that moves is not where it ends for the whole round)
    assert any(not np.array_equal(_bits(d["got"][0, ..., :2]), _bits(d["got"][K_TICKS - 1, ..., :2])) for d in rounds[1:])


def test_the_last_tick_is_the_committed_state(rounds):
    from auv_sim_amd.tracking import shark_members
    mem = shark_members(SHARK_OF, F)
    for r, d in enumerate(rounds):
        assert np.array_equal(_bits(d["got"][K_TICKS - 1, ..., :3]), _bits(d["last"][mem][..., :3])), r


def test_k_1_through_the_option_equals_the_plain_call(rounds):
    for r, d in enumerate(rounds):
        assert d["option"] is None  # (back to unset after every call)
        assert d["plain"].shape == (F, A, 5) and d["one"].shape == (1, F, A, 5)
        assert np.array_equal(_bits(d["one"][0]), _bits(d["plain"])), r
        # ... and both are the k = 3 table's last step: the same state against the same sample
        assert np.array_equal(_bits(d["plain"]), _bits(d["got"][K_TICKS - 1])), r


def test_a_stopped_auv_repeats_its_last_state():
    from auv_sim_amd.tracking import shark_members
    e = 0
    rs = _measured_rounds(late=e)
    _compare_tables(rs, "one AUV stopped")
    f, a = [(int(f), int(a)) for f, a in zip(*np.nonzero(shark_members(SHARK_OF, F) == e))][0]
    assert e in rs[0]["auv"] and all(e not in d["auv"] for d in rs[1:])  # it plans round 0 only
    assert rs[1]["n"][e] >= 1  # before round 1 its segment is round 0's
    for d in rs[2:]:
        assert d["n"][e] == 0
        for j in range(K_TICKS):
            assert np.array_equal(_bits(d["got"][j, f, a, :3]), _bits(d["last"][e, :3]))
    assert len(rs[2:]) >= 1 and np.array_equal(_bits(rs[1]["last"][e]), _bits(rs[2]["last"][e]))


def _same_step(a, b, dev, host):
    pa, pb = dev.filters.particles(), host.filters.particles()
    return (np.array_equal(_bits(pa[0]), _bits(pb[0])) and np.array_equal(pa[1], pb[1])
            and sorted(a.keys()) == sorted(b.keys())
            and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a if k.startswith("estimates"))
            and all(np.array_equal(x, y) for x, y in zip(dev.filters.rng_state(), host.filters.rng_state()))
            and all(np.array_equal(a[k], b[k]) for k in ("auv", "last", "keep", "winner", "cost")))


@pytest.mark.parametrize("K", [1, 2])
def test_device_loop_equals_host_loop(K):
    dev, tracks = _setup_ticks("device", K)
    host, _ = _setup_ticks("host", K)
    steps, first_diff = 0, None
    while True:
        a, b = dev.step(), host.step()
        assert (a is None) == (b is None)
        if a is None:
            break
        steps += 1
        if not _same_step(a, b, dev, host) and first_diff is None:
            first_diff = steps
            print("K = %d: the two loops differ from step %d on" % (K, steps))
        assert a["estimates"].shape == (F, 2) and a["estimates_all"].shape == (K_TICKS, F, 2)
        assert np.array_equal(_bits(a["estimates"]), _bits(a["estimates_all"][-1]))
    assert ROUNDS <= steps <= ROUNDS + 1  # (as in test_gpu_fleet_tracker.py; the tracks hold ROUNDS + 1 rounds of samples)
    ra, rb = dev.session.finish(as_arrays=True), host.session.finish(as_arrays=True)
    assert first_diff is None
    _same_arrays(ra, rb, "device against host, filter_steps = 3")


def test_filter_steps_1_equals_the_argument_left_out():
    one, _ = _setup_ticks("device", filter_steps=1)
    none, _ = _setup_ticks("device", filter_steps=None)
    steps = 0
    while True:
        a, b = one.step(), none.step()
        assert (a is None) == (b is None)
        if a is None:
            break
        steps += 1
        assert "estimates_all" not in a and _same_step(a, b, one, none), steps
    assert ROUNDS <= steps <= ROUNDS + 1
    _same_arrays(one.session.finish(as_arrays=True), none.session.finish(as_arrays=True), "filter_steps = 1 against none")


def test_refusals_leave_the_option_and_the_table():
    from auv_sim_amd import _lib
    tr, tracks = _setup_ticks("device")
    ctx = tr.rrt._ctx
    shark = _sharks(tracks, 0)
    assert ctx.replan_measure(SHARK_OF, A, shark)
    prev = ctx.replan_meas()
    assert prev.shape == (K_TICKS, F, A, 5)

    def unchanged(option):
        assert ctx.get_option("MEAS_TICKS") == option
        assert np.array_equal(_bits(ctx.replan_meas()), _bits(prev))

    bad_shapes = (np.zeros((0, F, 2)), np.zeros((65, F, 2)), np.zeros((3, F + 1, 2)), np.zeros((3, F, 3)), np.zeros((2, F, 1)),
                  np.zeros((F, 3)))
    for option in (None, 2):
        ctx.set_option("MEAS_TICKS", option)
        for bad in bad_shapes:
            with pytest.raises(ValueError):
                ctx.replan_measure(SHARK_OF, A, bad)
            unchanged(option)
        with pytest.raises(ValueError):
            ctx.replan_measure([0] * 5 + [1] * 3, A, shark)  # unequal trackers
        unchanged(option)
    # a caller's own setting survives a good call too; with it set the [F,2] form is refused (the library would read k x F rows)
    assert ctx.replan_measure(SHARK_OF, A, shark) and ctx.get_option("MEAS_TICKS") == 2
    with pytest.raises(ValueError):
        ctx.replan_measure(SHARK_OF, A, shark[0])
    unchanged(2)
    # the library's own refusal: a k outside 1 .. 64 is AUVP_ERR_ARG, nothing is launched, the last table stays
    so = np.array(SHARK_OF, dtype=np.int32)
    room = np.zeros((65, F, 2))
    for k in (0, 65, -3):
        ctx.set_option("MEAS_TICKS", k)
        assert ctx.L.auvp_replan_measure(ctx.h, _lib._p(so), A, _lib._p(room), None) == -1
        unchanged(k)
    ctx.set_option("MEAS_TICKS", None)
    unchanged(None)
    tr.session.finish()

"""tracking.FleetTracker: measure -> filter -> forecast -> plan, closed on the device.  Eight AUVs track two sharks (four each,
interleaved) on the world of the replanning goldens, 64 particles per filter, three rounds.
  * replan_measure_kernel's table, downloaded, against tracking.fleet_measurements -- the definition -- bit for bit;
  * FleetTracker(measure="device") against measure="host": the filters' particles, estimates and random streams after every
    step and every returned field at the end, bit for bit.
In round 0 one AUV sits exactly at its shark (dx = dy = 0), one has its shark due west on its own latitude (bearing pi), one a
hair north of that line (bearing just under -pi ... the other side of the cut) and one lies due west of the shark.

The bearing: the kernel rounds the particle-filter kernel's atan2 value to the nearest double (replan_atan2_round,
tests/test_replan_bearing_host.py); math.atan2 of this libm is that double for all but about 7 argument pairs in 10 000 (3 737
of 5 000 121 pairs counted on the host, where arbitrary precision says libm's last bit is the one that is off), so the
comparison is bit for bit and the tests print how many of their bearings differ, and by how many ulp, before they assert."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_replan_commit import _same_arrays, _world

pytestmark = pytest.mark.gpu

N, F, A, N_PARTICLES, N_ITER, ROUNDS, R_FORECAST = 8, 2, 4, 64, 300, 3, 4
BUDGET, LENGTH, INTERVAL, T_START = 2.0, 150.0, 98.0, 150.0
SHARK_OF = [1, 0, 1, 0, 0, 1, 1, 0]
SEEDS = [17 * e + 5 for e in range(N)]


class _B:
    def __init__(self, *b):
        self.bounds = tuple(float(v) for v in b)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _ulps(a, b):
    return np.abs(_bits(a).astype(np.int64) - _bits(b).astype(np.int64))


def _free(g, x, y):
    return all(np.hypot(x - o[0], y - o[1]) > o[2] + 3.0 for o in g["obstacles"])


def _setup(measure, K=1):
    from auv_sim_amd import _lib, _pf_lib
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    from auv_sim_amd.rrt_dubins import RRT
    from auv_sim_amd.sharkForecast import SharkForecast
    from auv_sim_amd.tracking import FleetTracker
    g = np.load(os.path.join(GOLDEN, "g13_replan_a.npz"))
    obstacles, habitats, cell_list, grids, poly = _world(g)
    # two sharks that wander a few metres per round, at points free of obstacles
    rng = np.random.default_rng(5)
    base = []
    while len(base) < F:
        x, y = rng.uniform(-260, -140), rng.uniform(-60, 60)
        if all(_free(g, x + dx, y + dy) for dx in (-30.0, 0.0, 25.0, 25.0) for dy in (0.0, 1e-9)):
            base.append((x, y))
    tracks = np.array([[(bx + 4.0 * s, by - 3.0 * s * (1 - 2 * f)) for s in range(ROUNDS + 1)] for f, (bx, by) in enumerate(base)])
    # shark 0's trackers (AUVs 1, 3, 4, 7): at the shark, the shark due west, a hair north of that line, west of the shark
    starts = [None] * N
    sx, sy = tracks[0, 0]
    for e, (dx, dy) in zip((1, 3, 4, 7), ((0.0, 0.0), (25.0, 0.0), (25.0, 1e-9), (-30.0, 0.0))):
        starts[e] = MPS(sx + dx, sy + dy, theta=0.0, traj_time_stamp=T_START)
    for e in range(N):
        if starts[e] is None:
            h = g["habitats"][e]
            starts[e] = MPS(h[0], h[1], theta=0.3 * e, traj_time_stamp=T_START)
    rrt = RRT(poly, obstacles, grids[0], cell_list)
    fctx = _lib.Context(0)
    mts = np.stack([_pf_lib.np_seed_state(100 + f)[0] for f in range(F)])
    filters = _pf_lib.FilterBatch(fctx, F, N_PARTICLES).create(tracks[:, 0, :], mts, 624)
    sf = SharkForecast(_B(-300, -100, -100, 100), 10, cell_list, device_context=fctx)
    tr = FleetTracker(rrt, sf, filters, tracks, SHARK_OF, np.ones((sf.n_row, sf.n_col)), R_FORECAST, measure=measure,
                      starts=starts, habitats=habitats, plan_time_budget=BUDGET, traj_time_length=LENGTH, replan_time_interval=INTERVAL,
                      weight=[-3, -3, -4], max_iter=N_ITER, seeds=SEEDS, trees_per_auv=K)
    return tr, tracks


def test_measurement_table_equals_the_host_definition():
    from auv_sim_amd.tracking import fleet_measurements
    tr, tracks = _setup("device")
    ctx, s = tr.rrt._ctx, tr.session
    bad, worst = 0, 0
    checked = []
    for r in range(ROUNDS):
        ptr = ctx.replan_measure(SHARK_OF, A, tracks[:, r])
        assert ptr
        got, want = ctx.replan_meas(), fleet_measurements(s.last, SHARK_OF, tracks[:, r])[0]
        assert got.shape == want.shape == (F, A, 5)
        assert np.array_equal(_bits(got[..., :4]), _bits(want[..., :4])), r  # x, y, theta, range
        d = _ulps(got[..., 4], want[..., 4])
        bad, worst = bad + int((d != 0).sum()), max(worst, int(d.max()))
        checked.append((got, want))
        if r == 0:
            assert got[0, 0, 3] == 0.0 and got[0, 1, 4] == np.pi and got[0, 3, 4] == 0.0  # at the shark; due west; west of it
        assert s.round() is not None
    print("bearings that differ from math.atan2: %d of %d, at most %d ulp" % (bad, ROUNDS * N, worst))
    s.finish()
    for got, want in checked:
        assert np.array_equal(_bits(got), _bits(want))
    with pytest.raises(ValueError):
        ctx.replan_measure([0] * 5 + [1] * 3, A, tracks[:, 0])  # unequal trackers


def test_unequal_trackers_are_refused_before_the_session_opens():
    from auv_sim_amd.tracking import FleetTracker, shark_members
    with pytest.raises(ValueError):
        shark_members([0, 0, 0, 0, 0, 1, 1, 1], F)

    class _Filters:
        F = 2

    with pytest.raises(ValueError):
        FleetTracker(None, None, _Filters(), np.zeros((F, 3, 2)), [0, 0, 0, 0, 0, 1, 1, 1], None, 2)


@pytest.mark.parametrize("K", [1, 2])
def test_device_loop_equals_host_loop(K):
    dev, tracks = _setup("device", K)
    host, _ = _setup("host", K)
    steps, first_diff = 0, None
    while True:
        a, b = dev.step(), host.step()
        assert (a is None) == (b is None)
        if a is None:
            break
        steps += 1
        pa, pb = dev.filters.particles(), host.filters.particles()
        same = (np.array_equal(_bits(pa[0]), _bits(pb[0])) and np.array_equal(pa[1], pb[1])
                and np.array_equal(_bits(a["estimates"]), _bits(b["estimates"]))
                and all(np.array_equal(x, y) for x, y in zip(dev.filters.rng_state(), host.filters.rng_state()))
                and all(np.array_equal(a[k], b[k]) for k in ("auv", "last", "keep", "winner", "cost")))
        if not same and first_diff is None:
            first_diff = steps
            print("K = %d: the two loops differ from step %d on; particles differ by at most %g" % (K, steps, np.abs(pa[0] - pb[0]).max()))
        assert a["estimates"].shape == (F, 2)
    assert ROUNDS <= steps <= ROUNDS + 1  # (an AUV whose third round ends before t = 400 plans a fourth)
    ra, rb = dev.session.finish(as_arrays=True), host.session.finish(as_arrays=True)
    assert first_diff is None
    _same_arrays(ra, rb, "device against host")

"""tracking.fleet_measurements, the host definition of a fleet's range / bearing measurements from its committed states
(replan_measure_kernel is held to it on the GPU): shapes, the member order of interleaved shark_of lists, the refusals, and
agreement with tracking.range_bearing_measurements where the AUVs sit at that function's fixed offsets."""
import math

import numpy as np
import pytest

from auv_sim_amd.tracking import first_bin_of_time, fleet_measurements, range_bearing_measurements, shark_members


def _fleet(n, seed=3):
    rng = np.random.default_rng(seed)
    last = np.zeros((n, 7))
    last[:, 0], last[:, 1] = rng.uniform(-300, -100, n), rng.uniform(-100, 100, n)
    last[:, 2] = rng.uniform(-math.pi, math.pi, n)
    last[:, 3:] = rng.uniform(0, 50, (n, 4))
    return last


def test_shapes_and_member_order_with_interleaved_sharks():
    shark_of = [1, 0, 1, 0, 0, 1, 1, 0]
    assert shark_members(shark_of).tolist() == [[1, 3, 4, 7], [0, 2, 5, 6]]
    last = _fleet(8)
    shark = np.array([[-210.0, 15.0], [-150.5, -60.25]])
    meas = fleet_measurements(last, shark_of, shark)
    assert meas.shape == (1, 2, 4, 5) and meas.dtype == np.float64
    for f, row in enumerate([[1, 3, 4, 7], [0, 2, 5, 6]]):
        for a, e in enumerate(row):
            x, y, th = last[e, :3]
            dx, dy = shark[f, 0] - x, shark[f, 1] - y
            want = [x, y, th, math.sqrt(dx * dx + dy * dy), math.atan2(dy, dx) - th]
            assert meas[0, f, a].tolist() == want, (f, a)


def test_an_auv_at_its_shark_and_one_with_the_shark_due_west():
    last = np.zeros((2, 7))
    last[0, :3] = [-200.0, 10.0, 0.4]  # at the shark: range 0, atan2(0, 0) = 0
    last[1, :3] = [-150.0, 10.0, 0.0]  # the shark due west: bearing pi
    meas = fleet_measurements(last, [0, 0], [[-200.0, 10.0]])
    assert meas[0, 0, 0].tolist() == [-200.0, 10.0, 0.4, 0.0, -0.4]
    assert meas[0, 0, 1].tolist() == [-150.0, 10.0, 0.0, 50.0, math.pi]


def test_unequal_trackers_and_bad_labels_are_refused():
    last = _fleet(6)
    shark = np.zeros((2, 2))
    for bad in ([0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0], [0, 1, 2, 0, 1, 2], [0, 1, -1, 0, 1, 1], [0, 1, 0.5, 0, 1, 1],
                [0, 1, True, 0, 1, 1]):
        with pytest.raises(ValueError):
            fleet_measurements(last, bad, shark)
    with pytest.raises(ValueError):
        fleet_measurements(last, [0, 1, 0, 1], shark)  # a wrong length
    with pytest.raises(ValueError):
        shark_members([])
    assert shark_members([0, 1, 2, 0, 1, 2]).tolist() == [[0, 3], [1, 4], [2, 5]]
    assert shark_members([0, 0], 1).tolist() == [[0, 1]]


def test_agrees_with_range_bearing_measurements_at_its_fixed_offsets():
    """AUV a of filter f at tracks[f, 0] + offsets[a] with theta 0: the two functions describe the same sensor.  The positions
    and theta are equal exactly; range and bearing to the last few ulps (numpy's ** 2 and arctan2 against math's)"""
    rng = np.random.default_rng(11)
    F, S = 3, 5
    tracks = rng.uniform(-50, 50, (F, S, 2))
    offsets = [(60.0, -40.0), (-50.0, 70.0)]
    want, shark = range_bearing_measurements(tracks, offsets)
    A = len(offsets)
    last = np.zeros((F * A, 7))
    shark_of = []
    for f in range(F):
        for a in range(A):
            last[f * A + a, :2] = tracks[f, 0] + np.array(offsets[a])
            shark_of.append(f)
    for s in range(S):
        got = fleet_measurements(last, shark_of, shark[s])
        assert got.shape == (1, F, A, 5)
        assert np.array_equal(got[0, ..., :3], want[s, ..., :3])
        assert np.allclose(got[0, ..., 3:], want[s, ..., 3:], rtol=4 * np.finfo(float).eps, atol=0.0)


def test_first_bin_of_time():
    bins = [(0, 50), (50, 100), (100, 150), (150, 200)]
    assert [first_bin_of_time(bins, t) for t in (0.0, 49.9, 50.0, 100.0, 120.0, 200.0, 200.1, 1e9)] == [0, 0, 0, 1, 2, 3, 3, 3]

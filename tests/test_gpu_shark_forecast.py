"""sf_forecast_kernel (csrc/forecast_kernel.h) through SharkForecast.run: the per-filter chain counts -> correction -> R rounds
of prediction1 / prediction2, one wavefront per filter, against the host methods it must reproduce bit for bit.

The reference of every case is `_host_chain`: the counts made with plain Python (cellToIndex's expression per particle), then
`auv_sim_amd.sharkEstimate.SharkUpdate.correction` and `predictOnAve` / `predictOnHist` (= prediction1 / prediction2 with the
P_inf grid they build) chained round by round -- the methods tests/golden/g14_shark_update.json pins to the reference.  Every
round is deep-copied, because prediction2 rewrites its argument's rows.  All comparisons are np.array_equal with nan positions
equal, and additionally the sign of every non-nan entry (array_equal alone takes -0.0 for 0.0).  No tolerance appears in
this file.

Grids: geometry chosen so that every coordinate the cases need is exact in binary (cell sizes 0.5, 1, 2, 10; origins on
quarters).  N in {1, 63, 64, 65, 2048} crosses the wavefront's width; norm stays the reference's 1000 whatever N is."""
import copy
import math
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_CAPACITY, ERR_STATE = -1, -2, -4


class _B:
    """anything with .bounds (the boundary, a cell)"""

    def __init__(self, *b):
        self.bounds = tuple(float(v) for v in b)


class _Geom:
    """a rows x cols grid as SharkUpdate sizes it: the boundary spans (cols - 1) x (rows - 1) cells, the `+ 1` row and column
    lie on its far edge"""

    def __init__(self, rows, cols, cs, origin):
        self.rows, self.cols, self.cs = rows, cols, cs
        self.minx, self.miny = origin
        self.boundary = _B(self.minx, self.miny, self.minx + (cols - 1) * cs, self.miny + (rows - 1) * cs)

    def cell(self, r, c):
        cs = self.cs
        return _B(self.minx + c * cs, self.miny + r * cs, self.minx + (c + 1) * cs, self.miny + (r + 1) * cs)

    def cells(self, rcs):
        return [self.cell(r, c) for r, c in rcs]


def _raster(g):
    return [(r, c) for r in range(g.rows) for c in range(g.cols)]


def _snake(g):
    return [(r, c) for r in range(g.rows) for c in (range(g.cols) if r % 2 == 0 else range(g.cols - 1, -1, -1))]


def _shuffled(g, seed=3):
    rcs = _raster(g)
    random.Random(seed).shuffle(rcs)
    return rcs


def _l_shape(g):
    """the left column and the bottom row, shuffled: most of the grid is unlisted"""
    rcs = [(r, c) for r, c in _raster(g) if c == 0 or r == g.rows - 1]
    random.Random(8).shuffle(rcs)
    return rcs


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    return _lib.Context(0)


def _xy(g, F, N, seed, keep=None):
    """[F, N, 2] particle coordinates: uniform over the grid and a margin around it, a third snapped exactly onto cell edges,
    and -- where N leaves room -- the special places: minx / miny, interior edges, the far edge (the `+ 1` row and column, and
    the first coordinate past them), just outside on every side, nan.  keep = (r, c): the LAST position of every filter is the
    centre of that cell (so that a prior with one non-zero cell meets a particle)."""
    rng = np.random.default_rng(seed)
    cs, w, h = g.cs, g.cols * g.cs, g.rows * g.cs
    xy = np.empty((F, N, 2))
    xy[..., 0] = g.minx + rng.uniform(-0.1 * w, 1.1 * w, size=(F, N))
    xy[..., 1] = g.miny + rng.uniform(-0.1 * h, 1.1 * h, size=(F, N))
    snap = rng.random((F, N)) < 1 / 3
    xy[..., 0] = np.where(snap, g.minx + cs * rng.integers(-1, g.cols + 2, size=(F, N)), xy[..., 0])
    snap = rng.random((F, N)) < 1 / 3
    xy[..., 1] = np.where(snap, g.miny + cs * rng.integers(-1, g.rows + 2, size=(F, N)), xy[..., 1])
    x_in, y_in = g.minx + 0.25 * cs, g.miny + 0.25 * cs
    x_far, y_far = g.minx + g.cols * cs, g.miny + g.rows * cs      # the first coordinates past the `+ 1` column / row
    special = [
        (g.minx, g.miny), (g.minx, y_in), (x_in, g.miny),                                     # on minx / miny
        (g.minx + cs, g.miny + cs), (g.minx + cs, y_in),                                      # interior edges
        (g.boundary.bounds[2], g.boundary.bounds[3]),                                         # maxx, maxy: the `+ 1` column and row
        (np.nextafter(x_far, -np.inf), np.nextafter(y_far, -np.inf)),                         # their last coordinates
        (x_far, y_in), (x_in, y_far),                                                         # exactly past them: outside
        (np.nextafter(g.minx, -np.inf), y_in), (x_in, np.nextafter(g.miny, -np.inf)),         # just outside, low sides
        (np.nextafter(x_far, np.inf), y_in), (x_in, np.nextafter(y_far, np.inf)),             # just outside, high sides
        (np.nan, y_in), (x_in, np.nan), (np.nan, np.nan),
    ]
    n_sp = min(len(special), N // 2)
    for f in range(F):
        for i in range(n_sp):
            xy[f, i] = special[(i + f) % len(special)]
    if keep is not None:
        xy[:, N - 1, 0] = g.minx + (keep[1] + 0.5) * cs
        xy[:, N - 1, 1] = g.miny + (keep[0] + 0.5) * cs
    return xy


def _prior(g, F, kind, seed, keep=None):
    rng = np.random.default_rng(seed + 1000)
    p = rng.uniform(0.01, 1.0, size=(F, g.rows, g.cols))
    if kind == "one":          # all zero except one cell: usability has to spread from it along the list
        p[:] = 0.0
        p[:, keep[0], keep[1]] = 0.7
    elif kind == "negzero":
        p[:, keep[0], keep[1]] = -0.0
        p[:, 0, 0] = -0.0
    elif kind == "nan":
        p[0, keep[0], keep[1]] = np.nan     # (filter 0 only: the other filters of the batch stay finite)
    return p


def _host_chain(su, xy_f, prior_f, rounds, method, hist, stay, k):
    """(counts, [G_0 .. G_R]) of one filter by the host methods; the grids are None where correction raises ZeroDivisionError"""
    counts = su._blank()
    n_row, n_col = len(counts), len(counts[0])
    minx, miny = su.boundary.bounds[0], su.boundary.bounds[1]
    for x, y in xy_f.tolist():
        qx, qy = (x - minx) / su.cell_size, (y - miny) / su.cell_size
        if 0 <= qx < n_col and 0 <= qy < n_row:
            counts[int(qy)][int(qx)] += 1
    try:
        grids = [su.correction(counts, prior_f.tolist())]
    except ZeroDivisionError:
        return counts, None
    for _ in range(rounds):
        start = copy.deepcopy(grids[-1])
        if method[0] == "ave":
            nxt = su.predictOnAve(start, False, method[1], stay, k)[1]
        else:
            nxt = su.predictOnHist(start, False, method[1], copy.deepcopy(hist), stay, k)[1]
        grids.append(copy.deepcopy(nxt))
    return counts, grids


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(a, b, equal_nan=True):
        return False
    ok = ~np.isnan(a)
    return bool(np.array_equal(np.signbit(a[ok]), np.signbit(b[ok])))


def _check(ctx, g, rcs, F, N, rounds, method, stay=0.6, k=0.1, prior_kind="pos", shared=False, seed=0, xy=None, prior=None):
    """run the batch, compare every filter with the host chain; returns (result, number of filters with status 1)"""
    from auv_sim_amd.sharkEstimate import SharkUpdate
    from auv_sim_amd.sharkForecast import SharkForecast
    cells = g.cells(rcs)
    su = SharkUpdate(g.boundary, g.cs, cells)
    assert (len(su._blank()), len(su._blank()[0])) == (g.rows, g.cols)
    keep = rcs[len(rcs) // 2]
    xy = _xy(g, F, N, seed, keep) if xy is None else xy
    if prior is None:
        prior = _prior(g, 1 if shared else F, prior_kind, seed, keep)
    hist = None
    if method[0] == "hist":
        hist = np.random.default_rng(seed + 7).uniform(0.0, 0.2, size=(g.rows, g.cols)).tolist()
    sf = SharkForecast(g.boundary, g.cs, cells, device_context=ctx)
    res = sf.run(xy, prior[0] if shared else prior, rounds, method=method, hist=hist, stay_prob=stay, k=k)
    assert res.grids.shape == (F, rounds + 1, g.rows, g.cols) and res.prob.shape == (F, rounds + 1, len(rcs))
    assert res.counts.shape == (F, g.rows, g.cols) and res.counts.dtype == np.int32 and res.status.shape == (F,)
    n_zero = 0
    for f in range(F):
        counts, grids = _host_chain(su, xy[f], prior[0] if shared else prior[f], rounds, method, hist, stay, k)
        assert np.array_equal(res.counts[f], np.array(counts)), (f, "counts")
        if grids is None:
            n_zero += 1
            assert res.status[f] == 1, (f, "status")
            assert not res.grids[f].any() and not res.prob[f].any(), (f, "a filter without a total keeps zero grids")
            continue
        assert res.status[f] == 0, (f, "status")
        assert _same(grids, res.grids[f]), (f, "grids")
        assert _same([[gr[r][c] for r, c in rcs] for gr in grids], res.prob[f]), (f, "prob")
    return res, n_zero


G32 = _Geom(3, 2, 2.0, (-3.0, 5.0))
G75 = _Geom(7, 5, 0.5, (-1.25, 10.5))
G64 = _Geom(64, 64, 1.0, (100.0, -32.0))

CASES = {
    # id: (geometry, list order, F, N, rounds, method, stay_prob, prior, shared prior)
    "3x2-ave1": (G32, _raster, 3, 63, 1, ("ave", 1), 0.6, "pos", False),
    "3x2-no-rounds": (G32, _raster, 3, 64, 0, ("ave", 1), 0.6, "pos", False),
    "3x2-hist2-one-particle": (G32, _raster, 3, 1, 1, ("hist", 2), 0.6, "pos", True),
    "7x5-raster-ave1": (G75, _raster, 3, 64, 12, ("ave", 1), 0.6, "pos", False),
    "7x5-raster-ave2": (G75, _raster, 3, 65, 12, ("ave", 2), 0.6, "pos", False),
    "7x5-shuffled-hist1-one-cell": (G75, _shuffled, 3, 65, 12, ("hist", 1), 0.6, "one", False),
    "7x5-shuffled-hist2": (G75, _shuffled, 3, 2048, 12, ("hist", 2), 0.6, "pos", True),
    "7x5-snake-ave1-one-cell": (G75, _snake, 3, 63, 12, ("ave", 1), 0.6, "one", True),
    "7x5-snake-ave1-stay1": (G75, _snake, 1, 2048, 12, ("ave", 1), 1.0, "pos", False),
    "7x5-raster-ave1-stay1-one-cell": (G75, _raster, 3, 64, 1, ("ave", 1), 1.0, "one", False),
    "7x5-L-ave1": (G75, _l_shape, 3, 65, 12, ("ave", 1), 0.6, "pos", False),
    "7x5-L-ave2": (G75, _l_shape, 3, 63, 1, ("ave", 2), 0.6, "pos", False),
    "7x5-L-hist2": (G75, _l_shape, 1, 64, 12, ("hist", 2), 0.6, "pos", False),
    "7x5-negzero-ave1": (G75, _shuffled, 3, 2048, 12, ("ave", 1), 0.6, "negzero", False),
    "7x5-negzero-ave2": (G75, _raster, 1, 65, 1, ("ave", 2), 0.6, "negzero", True),
    "7x5-nan-ave1": (G75, _raster, 3, 64, 1, ("ave", 1), 0.6, "nan", False),
    "7x5-nan-hist2": (G75, _shuffled, 3, 63, 12, ("hist", 2), 0.6, "nan", False),
    "64x64-raster-ave1": (G64, _raster, 1, 2048, 12, ("ave", 1), 0.6, "pos", False),
    "64x64-shuffled-hist2": (G64, _shuffled, 1, 2048, 1, ("hist", 2), 0.6, "pos", False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_forecast_equals_the_host_chain(ctx, name):
    g, order, F, N, rounds, method, stay, prior_kind, shared = CASES[name]
    res, n_zero = _check(ctx, g, order(g), F, N, rounds, method, stay=stay, prior_kind=prior_kind, shared=shared, seed=len(name))
    assert n_zero == 0   # (every filter has a particle in a cell with a prior: the cases are about the chain)
    if prior_kind == "nan":
        assert np.isnan(res.grids[0]).all() and not np.isnan(res.grids[1:]).any()
    if prior_kind == "one":
        assert np.count_nonzero(res.grids[:, 0]) == F   # the corrected grid: all mass in the one cell
        if method[1] == 1 and stay == 1.0:
            assert np.count_nonzero(res.grids[:, -1]) == F   # nothing moves


def test_usability_spreads_along_the_list_only(ctx):
    """the host rule the kernel's levels must keep, on the smallest example: a 1 x 3 row, all mass in the middle cell.  In list
    order (middle, left, right) both ends see the filled middle cell; in raster order the left end is filled BEFORE the middle
    and stays 0"""
    g = _Geom(1, 3, 1.0, (0.0, 0.0))
    xy = np.array([[[1.5, 0.5]] * 5 + [[0.5, 0.5]] * 2])            # five particles in the middle cell, two in the left one
    prior = np.array([[[0.0, 1.0, 0.0]]])
    for rcs, want in (([(0, 1), (0, 0), (0, 2)], [0.4, 0.6, 0.4]), ([(0, 0), (0, 1), (0, 2)], [0.0, 0.6, 0.4])):
        res, n_zero = _check(ctx, g, rcs, 1, 7, 1, ("ave", 1), xy=xy, prior=prior)
        assert n_zero == 0 and res.counts[0].tolist() == [[2, 5, 0]]
        assert res.grids[0, 0].tolist() == [[0.0, 1.0, 0.0]] and res.grids[0, 1].tolist() == [want]


def test_300_filters_one_of_them_without_a_total(ctx):
    """more workgroups than compute units; filter 137's particles all miss the one cell its prior is non-zero in: status 1 and
    zero grids for it, its neighbours in the batch exact"""
    g, F, N, bad = G75, 300, 64, 137
    rcs = _shuffled(g, 11)
    xy = _xy(g, F, N, 21, rcs[len(rcs) // 2])
    prior = _prior(g, F, "pos", 21)
    prior[bad] = 0.0
    prior[bad, 0, 0] = 0.9
    xy[bad, :, 0] = g.minx + 2.25 * g.cs      # every particle of the filter in cell (3, 2)
    xy[bad, :, 1] = g.miny + 3.25 * g.cs
    res, n_zero = _check(ctx, g, rcs, F, N, 1, ("ave", 1), xy=xy, prior=prior)
    assert n_zero == 1 and res.status[bad] == 1 and res.counts[bad, 3, 2] == N
    assert res.status.sum() == 1
    with pytest.raises(ZeroDivisionError):
        res.shark_grid(bad, (0, 10), 10)


def test_capacity_and_list_errors(ctx):
    from auv_sim_amd import _lib
    from auv_sim_amd.sharkForecast import SharkForecast
    xy = np.zeros((1, 4, 2))
    g = _Geom(17, 241, 1.0, (0.0, 0.0))       # 4097 grid entries
    with pytest.raises(_lib.AuvpError) as e:
        SharkForecast(g.boundary, g.cs, g.cells([(0, 0)]), device_context=ctx).run(xy, np.ones((17, 241)), 1)
    assert e.value.code == ERR_CAPACITY
    g = G32
    for cells in (g.cells([(0, 0), (1, 1), (0, 0)]),                 # listed twice
                  g.cells([(0, 0), (3, 0)]), g.cells([(0, 2)]),       # past the grid (IndexError in the reference)
                  g.cells([(-1, 0)]), g.cells([(0, -2)])):            # negative index (wraps silently in the reference)
        with pytest.raises(_lib.AuvpError) as e:
            SharkForecast(g.boundary, g.cs, cells, device_context=ctx).run(xy, np.ones((3, 2)), 1)
        assert e.value.code == ERR_ARG


def test_particles_read_on_the_device_from_the_filter_batch():
    """FilterBatch(2, 100) after two steps: the forecast from the particles where they lie (NULL xy) == the forecast of the
    downloaded particles passed as xy == the host chain.  No filter batch on the handle: AUVP_ERR_STATE"""
    from auv_sim_amd import _lib, _pf_lib
    from auv_sim_amd.sharkEstimate import SharkUpdate
    from auv_sim_amd.sharkForecast import SharkForecast
    ctx = _lib.Context(0)
    F, N, rounds = 2, 100, 3
    g = _Geom(41, 41, 10.0, (-200.0, -200.0))
    rcs = _raster(g)
    cells = g.cells(rcs)
    sf = SharkForecast(g.boundary, g.cs, cells)
    prior = _prior(g, F, "pos", 5)
    with pytest.raises(_lib.AuvpError) as e:
        sf.run(_pf_lib.FilterBatch(ctx, F, N), prior, rounds)
    assert e.value.code == ERR_STATE
    rng = np.random.default_rng(9)
    mts = np.stack([_pf_lib.np_seed_state(s)[0] for s in (31, 32)])
    batch = _pf_lib.FilterBatch(ctx, F, N).create(np.array([[20.0, -10.0], [-35.0, 40.0]]), mts, 624)
    meas = np.zeros((2, F, 1, 5))
    meas[..., 0:2] = rng.uniform(-200, 200, size=(2, F, 1, 2))
    meas[..., 2] = rng.uniform(-np.pi, np.pi, size=(2, F, 1))
    meas[..., 3] = rng.uniform(0, 300, size=(2, F, 1))
    meas[..., 4] = rng.uniform(-np.pi, np.pi, size=(2, F, 1))
    batch.run(meas=meas, shark_xy=rng.uniform(-30, 30, size=(2, F, 2)))
    assert not batch.status()[0].any()
    on_device = sf.run(batch, prior, rounds)
    xy = np.ascontiguousarray(batch.particles()[0][..., 0:2])
    from_host = sf.run(xy, prior, rounds)
    for name in ("grids", "prob", "counts", "status"):
        assert np.array_equal(getattr(on_device, name), getattr(from_host, name), equal_nan=True), name
    assert on_device.counts.sum() > 0 and not on_device.status.any()
    su = SharkUpdate(g.boundary, g.cs, cells)
    for f in range(F):
        counts, grids = _host_chain(su, xy[f], prior[f], rounds, ("ave", 1), None, 0.6, 0.1)
        assert np.array_equal(on_device.counts[f], np.array(counts)) and _same(grids, on_device.grids[f])
    with pytest.raises(_lib.AuvpError) as e:      # the batch's own shape or nothing
        sf.run(_pf_lib.FilterBatch(ctx, F, N + 1), prior, rounds)
    assert e.value.code == ERR_ARG


class _Pt:
    def __init__(self, x, y, t):
        self.x, self.y, self.traj_time_stamp = x, y, t


def test_forecast_feeds_the_cost_function(ctx):
    """shark_grid -> pack_shark_grid -> habitat_shark_cost_batch: every listed cell in every bin, in list order, zeros included;
    the cost's shark term of a three-point path == the term summed by hand from .prob"""
    from auv_sim_amd.cost import habitat_shark_cost_batch
    from auv_sim_amd.rrt_dubins import pack_shark_grid
    from auv_sim_amd.sharkForecast import SharkForecast
    g = _Geom(7, 5, 0.5, (0.0, 0.0))
    rcs = _shuffled(g, 4)
    cells = g.cells(rcs)
    sf = SharkForecast(g.boundary, g.cs, cells, device_context=ctx)
    prior = _prior(g, 2, "pos", 2)
    prior[:, 6, :] = 0.0                         # a row of zeros: those cells must still be in the dict
    res = sf.run(_xy(g, 2, 500, 2), prior, 2)
    assert not res.status.any()
    grid = sf.shark_grid(0, (0, 10), 10)
    assert list(grid) == [(0, 10), (10, 20), (20, 30)]
    for j, key in enumerate(grid):
        assert list(grid[key]) == [c.bounds for c in cells]
        assert list(grid[key].values()) == res.prob[0, j].tolist()
    assert 0.0 in grid[(0, 10)].values()
    bins, pcells, prob = pack_shark_grid(grid)
    assert np.array_equal(prob, res.prob[0]) and np.array_equal(pcells, np.array([c.bounds for c in cells]))
    # points on the diagonal cells (the cost function's cell test compares x with the cell's maxy, as the reference does)
    pts = [(0.2, 0.3, 5.0, (0, 0)), (1.2, 1.3, 15.0, (2, 2)), (2.2, 2.1, 12.0, (4, 4))]
    w3, total = -4.0, 20.0
    out = habitat_shark_cost_batch([[_Pt(x, y, t) for x, y, t, _ in pts]], [total], [], grid, [-3.0, -3.0, w3], device_context=ctx)
    term = 0.0
    for x, y, t, rc in pts:
        p = res.prob[0, int(t // 10), rcs.index(rc)]
        assert p != 0.0
        term = term + w3 * p
    assert out[0, 3] == term / total and out[0, 0] == ((0.0 + 0.0) + 0.0) + term / total

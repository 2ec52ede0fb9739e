"""sf_wide_kernel (csrc/forecast_wide_kernel.h) through SharkForecast.run(large_grids=True): the forecast on grids of more than
4 096 entries, one workgroup per filter with the grids in HBM, against the host methods it must reproduce bit for bit.

The reference of every case is test_gpu_shark_forecast's `_host_chain` (plain-Python counts, then SharkUpdate.correction and
predictOnAve / predictOnHist chained round by round), computed once per case and shared where several tests need it.  All
comparisons are `_same`: np.array_equal with nan positions equal, plus the sign of every non-nan entry.  No tolerance appears
in this file.

Shapes: 17 x 241 (4 097 entries: the first grid past the one-wavefront kernel's cap), 65 x 64 (the first square-ish one; as
raster 128 levels, as snake one cell per level, as L-shape most of the grid unlisted), 201 x 201 (the planners' 200 x 200
world as SharkUpdate sizes it), and every case of test_gpu_shark_forecast sent to the wide kernel by option SF_WIDE_MIN = 1 at
64, 256 and 1 024 threads (levels narrower and wider than the workgroup, grids smaller than one)."""
import functools
import math
import random

import numpy as np
import pytest

from test_gpu_shark_forecast import (CASES, _Geom, _host_chain, _l_shape, _prior, _raster, _same, _shuffled, _snake, _xy)

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_CAPACITY = -1, -2
ONE, WIDE = "sf_forecast_kernel", "sf_wide_kernel"

G17 = _Geom(17, 241, 1.0, (-8.0, 3.0))          # 4 097 entries
G65 = _Geom(65, 64, 2.0, (100.0, -32.0))        # 4 160
G201 = _Geom(201, 201, 2.0, (-200.0, -200.0))   # 40 401: a 200 x 200 world of 2 m cells


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    return _lib.Context(0)


def _inputs(g, rcs, F, N, method, prior_kind, shared, seed):
    keep = rcs[len(rcs) // 2]
    xy = _xy(g, F, N, seed, keep)
    prior = _prior(g, 1 if shared else F, prior_kind, seed, keep)
    hist = None
    if method[0] == "hist":
        hist = np.random.default_rng(seed + 7).uniform(0.0, 0.2, size=(g.rows, g.cols)).tolist()
    return xy, prior, hist


def _reference(g, rcs, xy, prior, shared, rounds, method, hist, stay=0.6, k=0.1):
    """[(counts, grids or None)] per filter, by the host chain"""
    from auv_sim_amd.sharkEstimate import SharkUpdate
    su = SharkUpdate(g.boundary, g.cs, g.cells(rcs))
    assert (len(su._blank()), len(su._blank()[0])) == (g.rows, g.cols)
    return [_host_chain(su, xy[f], prior[0] if shared else prior[f], rounds, method, hist, stay, k) for f in range(len(xy))]


def _compare(res, ref, rcs, grids=True):
    """every filter of a Forecast against the host chain; returns the number of filters without a total"""
    n_zero = 0
    for f, (counts, want) in enumerate(ref):
        assert np.array_equal(res.counts[f], np.array(counts)), (f, "counts")
        if want is None:
            n_zero += 1
            assert res.status[f] == 1, (f, "status")
            assert not res.prob[f].any() and (not grids or not res.grids[f].any()), (f, "a filter without a total keeps zero grids")
            continue
        assert res.status[f] == 0, (f, "status")
        if grids:
            assert _same(want, res.grids[f]), (f, "grids")
        assert _same([[gr[r][c] for r, c in rcs] for gr in want], res.prob[f]), (f, "prob")
    return n_zero


def _forecast(ctx, g, rcs):
    from auv_sim_amd.sharkForecast import SharkForecast
    return SharkForecast(g.boundary, g.cs, g.cells(rcs), device_context=ctx)


# ---- 1. above the cap ----
_SHAPES = {"17x241-shuffled": (G17, _shuffled), "65x64-raster": (G65, _raster), "65x64-snake": (G65, _snake), "65x64-L": (G65, _l_shape)}
_METHODS = [("ave", 1), ("ave", 2), ("hist", 1), ("hist", 2)]
# per (shape, method): (N, rounds, prior, shared prior) -- every shape meets N in {1, 65, 2048}, 0 / 1 / 3 rounds and the
# negzero / nan / one priors, and a shared prior once
_VARIANTS = {
    "17x241-shuffled": [(2048, 3, "negzero", False), (65, 1, "nan", False), (1, 3, "one", False), (65, 0, "pos", True)],
    "65x64-raster": [(65, 3, "one", False), (2048, 0, "negzero", True), (2048, 3, "nan", False), (1, 1, "pos", False)],
    "65x64-snake": [(1, 1, "nan", False), (2048, 3, "one", True), (65, 0, "pos", False), (65, 3, "negzero", False)],
    "65x64-L": [(2048, 0, "pos", False), (65, 3, "negzero", False), (1, 1, "one", True), (2048, 3, "nan", False)],
}
ABOVE = {"%s-%s%d" % (s, m[0], m[1]): (s, m) + _VARIANTS[s][i] for s in _SHAPES for i, m in enumerate(_METHODS)}


@pytest.mark.parametrize("name", list(ABOVE))
def test_above_the_cap_equals_the_host_chain(ctx, name):
    shape, method, N, rounds, prior_kind, shared = ABOVE[name]
    g, order = _SHAPES[shape]
    rcs, F, seed = order(g), 3, len(name)
    xy, prior, hist = _inputs(g, rcs, F, N, method, prior_kind, shared, seed)
    res = _forecast(ctx, g, rcs).run(xy, prior[0] if shared else prior, rounds, method=method, hist=hist, large_grids=True)
    assert res.kernel == WIDE
    assert res.grids.shape == (F, rounds + 1, g.rows, g.cols) and res.prob.shape == (F, rounds + 1, len(rcs))
    assert res.counts.shape == (F, g.rows, g.cols) and res.counts.dtype == np.int32 and res.status.shape == (F,)
    assert _compare(res, _reference(g, rcs, xy, prior, shared, rounds, method, hist), rcs) == 0
    if prior_kind == "nan":
        assert np.isnan(res.grids[0]).all() and not np.isnan(res.grids[1:]).any()
    if prior_kind == "one":
        assert np.count_nonzero(res.grids[:, 0]) == F   # the corrected grid: all mass in the one cell


# ---- 2. the headline world ----
def test_the_200_x_200_world(ctx):
    """201 x 201 grid entries, the 40 000 cells of the world listed (the far row and column are not), raster; with and without
    the grids on the host"""
    g, F, N, rounds = G201, 2, 2048, 2
    rcs = [(r, c) for r in range(200) for c in range(200)]
    xy, prior, _ = _inputs(g, rcs, F, N, ("ave", 1), "pos", False, 4)
    sf = _forecast(ctx, g, rcs)
    res = sf.run(xy, prior, rounds, large_grids=True)
    assert res.kernel == WIDE and res.grids.shape == (F, rounds + 1, 201, 201) and res.prob.shape == (F, rounds + 1, 40000)
    assert _compare(res, _reference(g, rcs, xy, prior, False, rounds, ("ave", 1), None), rcs) == 0
    assert not res.grids[:, :, 200, :].any() and not res.grids[:, :, :, 200].any()      # unlisted: never filled
    lean = sf.run(xy, prior, rounds, large_grids=True, return_grids=False)
    assert lean.grids is None and lean.kernel == WIDE
    for name in ("prob", "counts", "status"):
        assert _same(getattr(lean, name), getattr(res, name)), name


# ---- 3. the wide kernel on small grids ----
@functools.lru_cache(maxsize=None)
def _small_case(name):
    """inputs and host chain of one of test_gpu_shark_forecast's cases, once for the three block sizes"""
    g, order, F, N, rounds, method, stay, prior_kind, shared = CASES[name]
    rcs = order(g)
    xy, prior, hist = _inputs(g, rcs, F, N, method, prior_kind, shared, len(name))
    return rcs, xy, prior, hist, _reference(g, rcs, xy, prior, shared, rounds, method, hist, stay=stay)


@pytest.fixture(scope="module")
def one_wave(ctx):
    """name -> the Forecast of sf_forecast_kernel for a small case (every one fits it), made on first use"""
    made = {}

    def get(name):
        if name not in made:
            g, order, F, N, rounds, method, stay, prior_kind, shared = CASES[name]
            rcs, xy, prior, hist, _ = _small_case(name)
            made[name] = _forecast(ctx, g, rcs).run(xy, prior[0] if shared else prior, rounds, method=method, hist=hist, stay_prob=stay)
            assert made[name].kernel == ONE
        return made[name]
    return get


@pytest.mark.parametrize("block", [64, 256, 1024])
@pytest.mark.parametrize("name", list(CASES))
def test_small_grids_on_the_wide_kernel(ctx, one_wave, name, block):
    g, order, F, N, rounds, method, stay, prior_kind, shared = CASES[name]
    rcs, xy, prior, hist, ref = _small_case(name)
    base = one_wave(name)
    ctx.set_option("SF_WIDE_MIN", 1)
    ctx.set_option("SF_WIDE_BLOCK", block)
    try:
        res = _forecast(ctx, g, rcs).run(xy, prior[0] if shared else prior, rounds, method=method, hist=hist, stay_prob=stay,
                                         large_grids=True)
        assert res.kernel == WIDE and ctx.last_launch()[:2] == (F, block)
    finally:
        ctx.set_option("SF_WIDE_MIN", None)
        ctx.set_option("SF_WIDE_BLOCK", None)
    assert _compare(res, ref, rcs) == 0
    for field in ("grids", "prob", "counts", "status"):
        assert _same(getattr(res, field), getattr(base, field)), field


def test_a_bad_block_is_err_arg(ctx):
    from auv_sim_amd import _lib
    g, rcs = G65, _l_shape(G65)
    xy, prior, _ = _inputs(g, rcs, 1, 4, ("ave", 1), "pos", False, 1)
    ctx.set_option("SF_WIDE_BLOCK", 100)
    try:
        with pytest.raises(_lib.AuvpError) as e:
            _forecast(ctx, g, rcs).run(xy, prior, 1, large_grids=True)
    finally:
        ctx.set_option("SF_WIDE_BLOCK", None)
    assert e.value.code == ERR_ARG


# ---- 4. a filter without a total ----
def test_a_filter_without_a_total_among_others(ctx):
    """filter 2's particles all miss the one cell its prior is non-zero in: status 1 and zero grids for it, taken by its whole
    workgroup; its neighbours in the batch exact"""
    g, F, N, bad, rounds = G65, 5, 65, 2, 1
    rcs = _shuffled(g, 11)
    xy, prior, _ = _inputs(g, rcs, F, N, ("ave", 1), "pos", False, 21)
    prior[bad] = 0.0
    prior[bad, 0, 0] = 0.9
    xy[bad, :, 0] = g.minx + 2.25 * g.cs      # every particle of the filter in cell (3, 2)
    xy[bad, :, 1] = g.miny + 3.25 * g.cs
    res = _forecast(ctx, g, rcs).run(xy, prior, rounds, large_grids=True)
    assert res.kernel == WIDE
    assert _compare(res, _reference(g, rcs, xy, prior, False, rounds, ("ave", 1), None), rcs) == 1
    assert res.status.tolist() == [0, 0, 1, 0, 0] and res.counts[bad, 3, 2] == N
    assert not res.grids[bad].any() and not res.prob[bad].any()
    with pytest.raises(ZeroDivisionError):
        res.shark_grid(bad, (0, 10), 10)


# ---- 5. particles read where a FilterBatch keeps them ----
def test_particles_read_on_the_device_from_the_filter_batch():
    from auv_sim_amd import _lib, _pf_lib
    ctx = _lib.Context(0)
    F, N, rounds = 2, 100, 2
    g = _Geom(65, 64, 10.0, (-320.0, -320.0))
    rcs = _raster(g)
    sf = _forecast(None, g, rcs)
    prior = _prior(g, F, "pos", 5)
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
    on_device = sf.run(batch, prior, rounds, large_grids=True)
    xy = np.ascontiguousarray(batch.particles()[0][..., 0:2])
    from_host = sf.run(xy, prior, rounds, large_grids=True)
    assert on_device.kernel == WIDE and from_host.kernel == WIDE
    for name in ("grids", "prob", "counts", "status"):
        assert _same(getattr(on_device, name), getattr(from_host, name)), name
    assert on_device.counts.sum() > 0 and not on_device.status.any()
    assert _compare(on_device, _reference(g, rcs, xy, prior, False, rounds, ("ave", 1), None), rcs) == 0


# ---- 6. capacity ----
def test_capacity(ctx):
    from auv_sim_amd import _lib
    xy = np.zeros((1, 4, 2))
    g = _Geom(2049, 2048, 1.0, (0.0, 0.0))            # 2**22 + 2 048 grid entries
    with pytest.raises(_lib.AuvpError) as e:
        _forecast(ctx, g, [(0, 0)]).run(xy, np.ones((2049, 2048)), 1, large_grids=True)
    assert e.value.code == ERR_CAPACITY
    with pytest.raises(_lib.AuvpError) as e:         # the default call keeps its cap at 4 096
        _forecast(ctx, G17, [(0, 0)]).run(xy, np.ones((17, 241)), 1)
    assert e.value.code == ERR_CAPACITY


# ---- 7. hand-off ----
def test_large_forecast_tables_reach_the_planner():
    """a 65 x 64 world of 4 m cells, all 4 160 entries listed, R = 9: set_shark_grids(forecast) while the forecast is its context's
    latest (device to device), and from a Forecast without a context (its host copy): exploring_batch(shark_of) gives the same
    results in every field"""
    from test_gpu_shark_sets import _Poly, _same_result
    from auv_sim_amd import _lib
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    from auv_sim_amd.rrt_dubins import RRT
    from auv_sim_amd.sharkForecast import Forecast
    F, R = 3, 9
    g = _Geom(65, 64, 4.0, (0.0, 0.0))               # the boundary: 252 x 256
    rcs = _raster(g)
    cells = g.cells(rcs)
    rng = np.random.default_rng(8)
    xy = np.stack([rng.normal(loc=m, scale=35.0, size=(200, 2)) for m in ((80.0, 90.0), (170.0, 150.0), (120.0, 50.0))])
    sf = _forecast(_lib.Context(0), g, rcs)
    assert (sf.n_row, sf.n_col, len(cells)) == (65, 64, 4160)
    fc = sf.run(xy, np.ones((65, 64)), R, large_grids=True)
    assert fc.kernel == WIDE and not fc.status.any() and fc.prob.shape == (F, R + 1, 4160)
    poly = _Poly([(0.0, 0.0), (252.0, 0.0), (252.0, 256.0), (0.0, 256.0)])
    orng = random.Random(2)
    obstacles = [MPS(orng.uniform(10, 240), orng.uniform(10, 240), size=orng.uniform(2, 6)) for _ in range(12)]
    obstacles = [o for o in obstacles if math.hypot(o.x - 120, o.y - 120) > 15]
    habitats = [MPS(orng.uniform(20, 230), orng.uniform(20, 230), size=orng.uniform(8, 15)) for _ in range(5)]
    own = fc.shark_grid(0, (0, 20), 20)
    E, shark_of = 6, [0, 1, 2, 2, 0, 1]
    initials = [MPS(120.0, 120.0) for _ in range(E)]
    seeds = [50 + 3 * e for e in range(E)]
    args = (habitats, 0.5, 20, 2, 50.0, True, 2.0, 90.0, True, [-3, -3, -4])
    got = []
    for forecast, on_device in ((fc, True), (Forecast(None, fc.prob, fc.counts, fc.status, fc.cell_bounds, fc.kernel_ms), False)):
        fleet = RRT(poly, obstacles, own, cells)
        calls, upload = [], fleet._ctx.set_prob_sets
        fleet._ctx.set_prob_sets = lambda *a, _c=calls, _u=upload, **k: (_c.append((a, k)), _u(*a, **k))[1]
        fleet.set_shark_grids(forecast)
        assert len(calls) == 1 and fleet.n_shark_sets == F
        if on_device:
            assert not calls[0][0] and calls[0][1]["prob_dev"] == sf._ctx.sf_prob_dev()[0]
        else:
            assert calls[0][0] and "prob_dev" not in calls[0][1]
        got.append(fleet.exploring_batch(initials, *args, max_iter=350, seeds=seeds, shark_of=shark_of))
    for e in range(E):
        _same_result(got[0][e], got[1][e], e)
    assert any(r is not None for r in got[0])      # (the comparison is of results, not of failures)

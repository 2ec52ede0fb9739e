"""A forecast placed at the planner's absolute bins on the device (auvp_world_set_prob_sets_placed, sf_place_kernel): the sets
read back from HBM against the same tables placed by numpy and uploaded through the host path, bit for bit, with the per-set
constants; for first bins 0, 1 and T - 1 and forecasts of 1, T - 1, T and T + 2 rounds on the 400-cell world of the replanning
goldens (T = 10), and on a 9-cell world (an odd row length: rows that start on an odd element, and source and destination rows
of different phase)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
F = 3


class _B:
    def __init__(self, *b):
        self.bounds = tuple(float(v) for v in b)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def worlds():
    """per world: the planner's context (bins, cells and a table of its own), a second one for the host path, the forecaster"""
    from auv_sim_amd import _lib
    from auv_sim_amd.sharkForecast import SharkForecast
    g = np.load(os.path.join(GOLDEN, "g13_replan_a.npz"))
    out = {}
    for name, box, cells, bins in (("g13", (-300, -100, -100, 100), g["cells"], g["bins"]),
                                   ("odd", (0, 0, 30, 30), np.array([(10 * c, 10 * r, 10 * c + 10, 10 * r + 10) for r in range(3) for c in range(3)],
                                                                    dtype=np.float64), np.array([(20 * t, 20 * t + 20) for t in range(4)], dtype=np.float64))):
        ctxs = []
        for _ in range(2):
            ctx = _lib.Context(0)
            ctx.set_world(None, None, None, bins, cells, np.zeros((len(bins), len(cells))))
            ctxs.append(ctx)
        sf = SharkForecast(_B(*box), 10, [_B(*c) for c in cells.tolist()], device_context=_lib.Context(0))
        rng = np.random.default_rng(len(cells))
        cx, cy, half = 0.5 * (box[0] + box[2]), 0.5 * (box[1] + box[3]), 0.5 * (box[2] - box[0])
        xy = np.stack([rng.normal(loc=(cx + 0.3 * half * (f - 1), cy - 0.2 * half * (f - 1)), scale=0.3 * half, size=(200, 2)) for f in range(F)])
        out[name] = dict(planner=ctxs[0], host=ctxs[1], sf=sf, xy=xy, bins=bins, cells=cells, T=len(bins))
    return out


def _place(w, R1, b):
    """the forecast of R1 rounds onto the planner's sets at first bin b, by the device and by the host path; both read back"""
    from auv_sim_amd.rrt_dubins import place_forecast, put_shark_tables
    sf = w["sf"]
    fc = sf.run(w["xy"], np.ones((sf.n_row, sf.n_col)), R1 - 1)
    assert not fc.status.any() and fc.prob.shape == (F, R1, len(w["cells"])) and len(np.unique(fc.prob)) > R1
    ctx = w["planner"]
    calls = dict(placed=0, plain=0)
    placed, plain = ctx.set_prob_sets_placed, ctx.set_prob_sets
    ctx.set_prob_sets_placed = lambda *a, **k: (calls.__setitem__("placed", calls["placed"] + 1), placed(*a, **k))[1]
    ctx.set_prob_sets = lambda *a, **k: (calls.__setitem__("plain", calls["plain"] + 1), plain(*a, **k))[1]
    try:
        host_copy = put_shark_tables(ctx, w["bins"], w["cells"], fc, first_bin=b)
    finally:
        del ctx.set_prob_sets_placed, ctx.set_prob_sets
    want = place_forecast(fc.prob, w["T"], b)
    assert np.array_equal(_bits(host_copy), _bits(want))
    w["host"].set_prob_sets(want)  # the host path: numpy's placement, uploaded
    return fc, calls, ctx.prob_sets(), w["host"].prob_sets(), want


@pytest.mark.parametrize("b", [0, 1, "T-1"])
@pytest.mark.parametrize("R1", [1, "T-1", "T", "T+2"])
def test_placed_sets_equal_the_host_path(worlds, R1, b):
    w = worlds["g13"]
    T = w["T"]
    R1, b = {1: 1, "T-1": T - 1, "T": T, "T+2": T + 2}[R1], {0: 0, 1: 1, "T-1": T - 1}[b]
    fc, calls, dev, host, want = _place(w, R1, b)
    identity = b == 0 and R1 == T
    assert calls == (dict(placed=0, plain=1) if identity else dict(placed=1, plain=0))  # (the identity: today's hand-over)
    assert dev.shape == (F, T, 400)
    assert np.array_equal(_bits(dev), _bits(want)) and np.array_equal(_bits(host), _bits(want))
    for f in range(F):
        for t in range(T):
            assert np.array_equal(_bits(dev[f, t]), _bits(fc.prob[f, min(max(t - b, 0), R1 - 1)])), (f, t)
    a, s = w["planner"].prob_set_stats()
    a2, s2 = w["host"].prob_set_stats()
    assert np.array_equal(_bits(a), _bits(a2)) and s.tolist() == s2.tolist()


@pytest.mark.parametrize("R1,b", [(3, 1), (1, 0), (6, 3), (2, 0)])
def test_odd_row_length(worlds, R1, b):
    """C = 9: every other row of the sets and of the forecast starts on an odd element -- a peeled first element, a last one
    left over, and rows whose source has the other phase (copied element by element)"""
    w = worlds["odd"]
    fc, calls, dev, host, want = _place(w, R1, b)
    assert calls == dict(placed=1, plain=0) and dev.shape == (F, 4, 9)
    assert np.array_equal(_bits(dev), _bits(want)) and np.array_equal(_bits(host), _bits(want))
    phases = {((f * R1 + min(max(t - b, 0), R1 - 1)) * 9 % 2, (f * 4 + t) * 9 % 2) for f in range(F) for t in range(4)}
    if (R1, b) == (3, 1):
        assert phases == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_refusals_keep_the_sets(worlds):
    """AUVP_ERR_ARG for a first bin outside the bins, another cell count, no rounds, a null pointer; the sets stay"""
    import ctypes as C
    w = worlds["g13"]
    fc, _, dev, _, _ = _place(w, 4, 2)
    ctx, src = w["planner"], w["sf"]._ctx
    ptr = src.sf_prob_dev()[0]
    call = ctx.L.auvp_world_set_prob_sets_placed
    for args in ((ptr, F, 4, 400, -1), (ptr, F, 4, 400, 10), (ptr, F, 4, 399, 0), (ptr, F, 0, 400, 0), (ptr, 0, 4, 400, 0), (None, F, 4, 400, 0)):
        assert call(ctx.h, C.c_void_p(args[0]), *args[1:]) == -1, args
    assert np.array_equal(_bits(ctx.prob_sets()), _bits(dev))
    from auv_sim_amd import _lib
    bare = _lib.Context(0)
    assert call(bare.h, C.c_void_p(ptr), F, 4, 400, 0) == -4  # no world

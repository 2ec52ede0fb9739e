"""Shark-occupancy forecast of many particle filters on the MI355X: the link between `FilterBatch` and the planners'
time-binned occupancy table that the reference left unfinished (`path_planning/sharkEstimate.py`; `RRT.replanning` builds a
`SharkUpdate` and never reads it, and `SharkUpdate.update` raises on its second round).

For every filter f, in ONE launch (libauvplan.so `auvp_sf_forecast`, one wavefront per filter):

    counts_f  = particles per grid cell                               (cellToIndex's expression per particle)
    G_0       = SharkUpdate.correction(counts_f, prior_f)
    G_{j+1}   = SharkUpdate.prediction1(G_j, stay_prob)               method 1
              | SharkUpdate.prediction2(G_j, k, P_inf)                method 2, P_inf "ave" (1 / len(cell_list)) or "hist"

Every single step is bit for bit the host method of `sharkEstimate.SharkUpdate` (which `tests/golden/g14_shark_update.json`
pins to the reference).  Feeding each round's prediction into the next is NEW ground: it is what `SharkUpdate.update`'s
docstring intends ("one prediction per time bin of the trajectory") and what its code fails to do -- it stores the pair
[initial, prediction] under the next key and dies when that pair is fed back in.

Limits, documented: rows x cols <= 4096 (`AUVP_ERR_CAPACITY` above), or <= 2**22 with `run(large_grids=True)`: above 4096
entries `sf_wide_kernel` runs, one workgroup per filter with the grids in HBM (the 200 x 200 world of the planners' benchmark
is a 201 x 201 grid; method 1 then costs one workgroup barrier per level of the list's schedule and round); a cell may be listed once (the reference would visit
it twice and see neighbours that come later in the list; `AUVP_ERR_ARG` here); a cell outside the grid is `AUVP_ERR_ARG`
(the reference: IndexError, or a silently wrapped negative index).  The particles are read where `FilterBatch` keeps them in
HBM (or from an [F, N, 2] host array); the forecast comes back to the host, and goes to a planner in one of two ways: one
filter's table as the dict `shark_grid` builds, through `RRT(...)`, or ALL F tables at once through
`RRT.set_shark_grids(forecast)` -- the device copy of `prob` is handed from this context to the planner's without leaving
HBM (`auvp_sf_prob_dev` -> `auvp_world_set_prob_sets`), and `shark_of=[...]` on `exploring_batch` / `exploring_best_of` /
`replanning_batch` then plans every AUV of a batch against its own shark's forecast in the same launch.  A world still keeps
ONE grid of its own (the constructor's); the F tables are probability sets beside it, over the same bins and cells.  No CPU
path: raises without the library / a GPU.
"""
import math

import numpy as np

from . import _lib

ZERO_TOTAL = 1  # per-filter status: the correction's total is 0 (the reference's ZeroDivisionError)
MAX_GRID, MAX_GRID_LARGE = 4096, 1 << 22  # rows x cols at most: `run`, and `run(large_grids=True)` (csrc/forecast_launch.h)


class Forecast:
    """what `SharkForecast.run` returns: grids [F, R+1, rows, cols] (None with return_grids=False), prob [F, R+1, C] (the same values in cell_list order: the
    planners' layout), counts [F, rows, cols] int32, status [F] (0, or ZERO_TOTAL: that filter's grids are all zeros)"""

    def __init__(self, grids, prob, counts, status, cell_bounds, kernel_ms, ctx=None, serial=None, kernel=None):
        self.grids, self.prob, self.counts, self.status = grids, prob, counts, status
        self.cell_bounds, self.kernel_ms = cell_bounds, kernel_ms
        self.kernel = kernel  # "sf_forecast_kernel" or "sf_wide_kernel" (auvp_sf_last_kernel)
        # the context that holds prob's device copy while `serial` is still its latest forecast (RRT.set_shark_grids)
        self.ctx, self.serial = ctx, serial

    def shark_grid(self, f, curr, bin_interval):
        """filter f's forecast as the planners' dict {(t0 + j*bin, t1 + j*bin): {cell.bounds: prob}}, j = 0 .. rounds, curr =
        (t0, t1).  EVERY listed cell appears in every bin, zeros included, in cell_list order (`pack_shark_grid` needs the
        same cell order per bin).  ZeroDivisionError where the reference's correction raises it (status[f] == ZERO_TOTAL)."""
        if self.status[f] == ZERO_TOTAL:
            raise ZeroDivisionError("float division by zero")
        out = {}
        for j in range(self.prob.shape[1]):
            key = (curr[0] + j * bin_interval, curr[1] + j * bin_interval)
            out[key] = {b: float(p) for b, p in zip(self.cell_bounds, self.prob[f, j])}
        return out


class SharkForecast:
    """`SharkForecast(boundary, cell_size, cell_list)`: the arguments of `SharkUpdate`; `boundary` and the cells only need
    `.bounds`.  `device_context`: the `_lib.Context` to run on (a `FilterBatch` handed to `run` brings its own)."""

    def __init__(self, boundary, cell_size, cell_list, device_context=None):
        self.boundary, self.cell_size, self.cell_list = boundary, cell_size, cell_list
        self._ctx = device_context
        minx, miny, maxx, maxy = boundary.bounds
        # SharkUpdate._blank: ceil BEFORE the division, + 1
        self.n_col = int(math.ceil(maxx - minx) / cell_size) + 1
        self.n_row = int(math.ceil(maxy - miny) / cell_size) + 1
        self.cell_bounds = [tuple(c.bounds) for c in cell_list]
        self.last = None

    def _context(self, filters):
        ctx = getattr(filters, "ctx", None)
        if ctx is not None:
            if self._ctx is not None and self._ctx is not ctx:
                raise ValueError("the FilterBatch lives on another context than this forecast's")
            self._ctx = ctx
            return ctx
        if self._ctx is None:
            self._ctx = _lib.Context(0)
        return self._ctx

    def run(self, filters_or_xy, prior, rounds, method=("ave", 1), hist=None, stay_prob=0.6, k=0.1, norm=1000, large_grids=False,
            return_grids=True):
        """filters_or_xy: a `FilterBatch` (its particles are read on the device) or an [F, N, 2] array of x, y; prior
        [rows, cols] (shared by all filters) or [F, rows, cols]; method = ("ave" | "hist", 1 | 2) as `SharkUpdate.update`
        takes it, `hist` [rows, cols] = P_inf of "hist"; norm: the particle count `correction` divides by (the reference
        assumes 1000 whatever N is).  large_grids: take grids of more than 4096 entries too (`auvp_sf_forecast_large`: up to
        2**22, on `sf_wide_kernel`; the same results bit for bit).  return_grids=False: `grids` is not copied to the host and
        `Forecast.grids` is None (F x (R + 1) x rows x cols x 8 bytes; `prob` is what the planners take).  Returns a `Forecast`."""
        kind, which = method
        if kind not in ("ave", "hist") or which not in (1, 2):
            raise ValueError("method must be ('ave' | 'hist', 1 | 2), not %r" % (method,))
        ctx = self._context(filters_or_xy)
        L = ctx.L
        forecast = L.auvp_sf_forecast_large if large_grids else L.auvp_sf_forecast
        rows, cols, n_cells = self.n_row, self.n_col, len(self.cell_bounds)
        if hasattr(filters_or_xy, "ctx"):
            F, N, xy = filters_or_xy.F, filters_or_xy.N, None
        else:
            xy = _lib._f64(filters_or_xy)
            if xy.ndim != 3 or xy.shape[2] != 2:
                raise ValueError("particle coordinates must be [F, N, 2]")
            F, N = xy.shape[0], xy.shape[1]
        pr = _lib._f64(prior)
        if pr.shape == (rows, cols):
            shared = 1
        elif pr.shape == (F, rows, cols):
            shared = 0
        else:
            raise ValueError("prior must be [%d, %d] or [%d, %d, %d], not %r" % (rows, cols, F, rows, cols, pr.shape))
        p_inf = None
        if kind == "hist":
            if hist is None:
                raise ValueError("method 'hist' needs the historical grid")
            p_inf = _lib._f64(hist)
            if p_inf.shape != (rows, cols):
                raise ValueError("hist must be [%d, %d]" % (rows, cols))
        R = int(rounds)
        box = _lib._f64(self.boundary.bounds, (4,))
        cells = _lib._f64(self.cell_bounds if n_cells else [], (-1, 4))
        # (above the entry point's cap the call fails before anything is written)
        n_grid = max(rows * cols, 1) if rows * cols <= (MAX_GRID_LARGE if large_grids else MAX_GRID) else 1
        grids = np.zeros((max(F, 1), max(R, 0) + 1, n_grid)) if return_grids else None
        prob = np.zeros((max(F, 1), max(R, 0) + 1, max(n_cells, 1)))
        counts = np.zeros((max(F, 1), n_grid), dtype=np.int32)
        status = np.zeros(max(F, 1), dtype=np.int32)
        ctx._chk(forecast(ctx.h, _lib._p(box), rows, cols, float(self.cell_size), _lib._p(cells), n_cells, int(F),
                          _lib._p(xy) if xy is not None else None, int(N), _lib._p(pr), shared, int(which),
                          _lib._p(p_inf) if p_inf is not None else None, float(stay_prob), float(k), float(norm), R,
                          _lib._p(grids) if grids is not None else None, _lib._p(prob), _lib._p(counts), _lib._p(status)))
        self.last = Forecast(grids.reshape(F, R + 1, rows, cols) if grids is not None else None, prob.reshape(F, R + 1, n_cells),
                             counts.reshape(F, rows, cols), status, self.cell_bounds, ctx.last_kernel_ms(), ctx,
                             getattr(ctx, "sf_serial", 0) + 1, ctx.sf_last_kernel())
        ctx.sf_serial = self.last.serial
        return self.last

    def shark_grid(self, f, curr, bin_interval):
        """`Forecast.shark_grid` of the last `run`"""
        if self.last is None:
            raise RuntimeError("no forecast has run")
        return self.last.shark_grid(f, curr, bin_interval)

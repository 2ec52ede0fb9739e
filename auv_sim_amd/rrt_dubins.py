"""Drop-in for path_planning/rrt_dubins.py: class RRT with the reference's constructor and
`exploring` / `replanning` signatures (rrt_dubins.py:26,51,92), running on the MI355X through
libauvplan.so.  Same inputs (Motion_plan_state lists, shapely-like boundary polygon, sharkGrid dict,
cell_list) and same outputs (dict with "path length" / "path" / "cost"; Motion_plan_state objects
linked by .parent/.path), so `robotSim`-style callers and `performance.summary_1` (:65-73) can switch
the import and nothing else.

Additive, non-reference keyword arguments:
  max_iter  iteration budget.  The reference loops until a wall-clock deadline (:116-118); here the
            budget is the virtual clock of SURVEY.md 8(c): exactly max_iter loop iterations and
            plan_time_stamp == 0-based iteration index.  Default: max_plan_time * RRT.iters_per_second.
  seed      None (default): continue Python's global `random` stream exactly where it stands -- so
            `random.seed(k); RRT(...).exploring(...)` draws what the reference would draw -- and
            advance it by the number of outputs consumed.  int: a private random.Random(seed) stream.
  device    HIP device index (constructor).

There is no CPU path: without libauvplan.so or a GPU the constructor raises.
"""
import math
import random

import numpy as np

from . import _lib
from .motion_plan_state import Motion_plan_state
# fleet replanning lives in replanning.py; its names stay importable from here
from .replanning import (MAX_SEPARATION_TEAM, MAX_SEPARATION_TICKS, TREE_FAILED, DeviceRounds, HostRounds, ReplanSession,  # noqa: F401
                         course_habitat_words, course_ticks, first_bucket_commit, raise_bad_status, replan_args, replan_costs,
                         replan_results, rescore, separation_args, team_csr, team_fold, team_labels, team_pick_claims,
                         team_pick_separated, tick_conflicts)


def _polygon_vertices(boundary):
    """accepts a shapely Polygon (or look-alike with .exterior.coords), a list of (x, y) pairs, or a
    list of Motion_plan_state-like objects"""
    if hasattr(boundary, "exterior"):
        pts = [(float(p[0]), float(p[1])) for p in boundary.exterior.coords]
    else:
        pts = [(float(p.x), float(p.y)) if hasattr(p, "x") else (float(p[0]), float(p[1])) for p in boundary]
    if len(pts) > 1 and pts[0] == pts[-1]:
        pts = pts[:-1]
    return np.array(pts, dtype=np.float64).reshape(-1, 2)


def _circles(objs):
    return np.array([(float(o.x), float(o.y), float(o.size)) for o in objs], dtype=np.float64).reshape(-1, 3)


def pack_shark_grid(sharkGrid):
    """{(t0,t1): {cell.bounds: prob}} -> bins [T,2], cells [C,4], prob [T,C].  The inner dicts' key
    order is the scan order of the cost function (path_planning/cost.py:181), so it defines the cell
    order; every bin must list the same cells in the same order (createSharkGrid builds them that
    way, rrt_dubins.py:612-630)."""
    keys = list(sharkGrid.keys())
    if not keys:
        return np.zeros((0, 2)), np.zeros((0, 4)), np.zeros((0, 0))
    cell_keys = list(sharkGrid[keys[0]].keys())
    for k in keys[1:]:
        if list(sharkGrid[k].keys()) != cell_keys:
            raise NotImplementedError("shark grid bins with differing cell order are not supported")
    bins = np.array([(float(k[0]), float(k[1])) for k in keys], dtype=np.float64).reshape(-1, 2)
    cells = np.array(cell_keys, dtype=np.float64).reshape(-1, 4)
    prob = np.array([[float(sharkGrid[k][c]) for c in cell_keys] for k in keys], dtype=np.float64)
    return bins, cells, prob.reshape(len(keys), len(cell_keys))


def place_forecast(prob, n_bins, first_bin):
    """a forecast's prob [F, R+1, C] at the planner's absolute bins: [F, n_bins, C] whose bin t is forecast round
    min(max(t - first_bin, 0), R) (csrc/forecast_place.h: placed_round)"""
    prob = np.asarray(prob, dtype=np.float64)
    idx = np.clip(np.arange(int(n_bins)) - int(first_bin), 0, prob.shape[1] - 1)
    return np.ascontiguousarray(prob[:, idx, :])


class PlacedTables:
    """the host's view of a forecast placed on the device: table g is gathered from the forecast's host copy when somebody asks
    (the trajectory costs at the end of a replanning call), not on every round of a tracking loop"""

    def __init__(self, prob, n_bins, first_bin):
        self.prob, self.n_bins, self.first_bin = prob, int(n_bins), int(first_bin)
        self.shape = (prob.shape[0], self.n_bins, prob.shape[2])

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, g):
        return place_forecast(self.prob[g][None], self.n_bins, self.first_bin)[0]

    def __array__(self, dtype=None, copy=None):
        return place_forecast(self.prob, self.n_bins, self.first_bin)


def put_shark_tables(ctx, own_bins, own_cells, grids, first_bin=None):
    """set_shark_grids of RRT and astar_fixLenSOG.astar: the tables of `grids` onto ctx's probability sets (Context.set_prob_sets),
    checked against the planner's own bins [T,2] and cells [C,4].  `grids`: a list of sharkGrid dicts with the planner's bin keys
    and cell order, or a sharkForecast.Forecast -- its prob [F, R+1, C] goes device to device while it is still its context's
    latest forecast on ctx's device, from its host copy otherwise; None or an empty list clears the sets.  first_bin (a Forecast
    only): None -- R + 1 must be T and the tables are taken as they lie --, or b in 0 .. T-1: bin t reads forecast round
    min(max(t - b, 0), R), any R (place_forecast; on the device sf_place_kernel; b == 0 with R + 1 == T is the call without it).
    ValueError for tables that do not match.  Returns the host copy [G, T, C] (a PlacedTables, gathered on demand, for a forecast
    placed on the device), None when cleared."""
    if grids is None or (isinstance(grids, (list, tuple)) and len(grids) == 0):
        if first_bin not in (None, 0):
            raise ValueError("first_bin needs a Forecast")
        ctx.set_prob_sets()
        return None
    T, Cn = len(own_bins), len(own_cells)
    if hasattr(grids, "prob") and hasattr(grids, "cell_bounds"):  # a Forecast
        fc = grids
        if first_bin is not None:
            if isinstance(first_bin, (bool, np.bool_)) or not isinstance(first_bin, (int, np.integer)):
                raise ValueError("first_bin must be an integer, not %r" % (first_bin,))
            if not 0 <= int(first_bin) < T:
                raise ValueError("first_bin %d outside 0 .. %d" % (int(first_bin), T - 1))
        if fc.prob.ndim != 3 or (first_bin is None and fc.prob.shape[1] != T) or fc.prob.shape[1] < 1:
            raise ValueError("the forecast has %d time bins (rounds + 1), the planner %d" % (fc.prob.shape[1], T))
        cb = np.array(fc.cell_bounds, dtype=np.float64).reshape(-1, 4)
        if cb.shape != own_cells.shape or not np.array_equal(cb, own_cells):
            raise ValueError("the forecast's cell list is not the planner's")
        placed = first_bin is not None and not (int(first_bin) == 0 and fc.prob.shape[1] == T)
        src = getattr(fc, "ctx", None)
        if src is not None and src.device == ctx.device and getattr(src, "sf_serial", None) == getattr(fc, "serial", -1):
            ptr, F, Tf, Cf = src.sf_prob_dev()
            if (F, Tf, Cf) != fc.prob.shape:
                raise ValueError("the forecast's device copy is [%d, %d, %d], not %r" % (F, Tf, Cf, fc.prob.shape))
            if placed:
                ctx.set_prob_sets_placed(ptr, F, Tf, int(first_bin))
                return PlacedTables(fc.prob, T, first_bin)
            ctx.set_prob_sets(n_sets=F, prob_dev=ptr)
            return np.array(fc.prob, dtype=np.float64)
        # (a forecast of another device, or one its context has since replaced: from the host copy)
        host = place_forecast(fc.prob, T, first_bin) if placed else np.array(fc.prob, dtype=np.float64)
        ctx.set_prob_sets(host)
        return host
    if first_bin not in (None, 0):
        raise ValueError("first_bin needs a Forecast")
    tabs = []
    for g, grid in enumerate(grids):
        bins, cells, prob = pack_shark_grid(grid)
        if bins.shape != own_bins.shape or not np.array_equal(bins, own_bins):
            raise ValueError("shark grid %d: its time bins are not the constructor's" % g)
        if cells.shape != own_cells.shape or not np.array_equal(cells, own_cells):
            raise ValueError("shark grid %d: its cells are not the constructor's, in the constructor's order" % g)
        tabs.append(prob)
    if T == 0 or Cn == 0:
        raise ValueError("shark tables need a planner whose own grid has time bins and cells")
    host = np.stack(tabs)
    ctx.set_prob_sets(host)
    return host


def habitat_keep_bits(masks, n_habitats, n_episodes):
    """exploring_batch's habitat_masks -> [E] ints (bit h: habitats[h] is on the episode's list): None (all of them), [E] ints,
    or [E, H] booleans"""
    if masks is None:
        return [(1 << n_habitats) - 1] * n_episodes
    a = np.asarray(masks)
    if a.dtype == bool:
        a = a.reshape(n_episodes, n_habitats)
        return [sum(1 << h for h in range(n_habitats) if row[h]) for row in a]
    return [int(m) for m in masks]


def shark_set_indices(shark_of, n, n_sets, timebin=True):
    """shark_of -> [n] int32 indices into the planner's shark tables (RRT.set_shark_grids), checked without a device: ValueError
    for another mode than time-bin (the tables ride on the per-episode-limits route), without tables, for a wrong length, a
    value that is no integer, or an index outside [0, n_sets)."""
    if not timebin:
        raise ValueError("shark_of needs time-bin mode (plan_time=True, traj_time_stamp=True)")
    if n_sets < 1:
        raise ValueError("shark_of given, but the planner has no shark tables (set_shark_grids)")
    idx = list(shark_of)
    if len(idx) != n:
        raise ValueError("shark_of has %d entries, expected %d" % (len(idx), n))
    out = np.zeros(n, dtype=np.int32)
    for i, g in enumerate(idx):
        if isinstance(g, bool) or int(g) != g:
            raise ValueError("shark_of[%d] = %r is not an integer" % (i, g))
        if not 0 <= int(g) < n_sets:
            raise ValueError("shark_of[%d] = %d outside [0, %d)" % (i, int(g), n_sets))
        out[i] = int(g)
    return out


def _mt_state_of(rng_state):
    """random.getstate() -> (624 words, index)"""
    ver, internal, _ = rng_state
    if ver != 3 or len(internal) != 625:
        raise RuntimeError("unexpected random.getstate() layout")
    return np.array(internal[:624], dtype=np.uint32), int(internal[624])


class RRT:
    """Goal-less cost-optimising RRT with random-arc steering (reference class of the same name)."""

    iters_per_second = 1000  # the reference's measured loop rate: wall-clock -> budget

    def __init__(self, boundary, obstacles, sharkGrid, cell_list, exp_rate=1, dist_to_end=2, diff_max=0.5,
                 freq=30, device=0):
        self.boundary_poly = boundary
        self.obstacle_list = obstacles
        self.last_path = []
        self.exp_rate = exp_rate
        self.dist_to_end = dist_to_end
        self.diff_max = diff_max
        self.freq = freq
        self.cell_list = cell_list
        self.sharkGrid = sharkGrid
        self.t_start = 0.0
        self._ctx = _lib.Context(device)  # raises without the HIP library / a GPU
        self._bins, self._cells, self._prob = pack_shark_grid(sharkGrid)
        self._poly = _polygon_vertices(boundary)
        self._world_habitats = None
        self._ctx.set_world(_circles(obstacles), None, self._poly, self._bins, self._cells, self._prob)
        self._cost_ctx = None   # cost-only context of replanning() (created on first use)
        self._last = None       # (summary, initial, E index) of the last exploring call
        self._mps_cache = None
        self._set_prob = None   # host copy [G, T, C] of the shark tables of set_shark_grids (None: none)
        self._batch = None      # what rerank needs of the last exploring_batch: (initials, shark_interval, max_traj_time)
        self._session = None    # the open ReplanSession (replanning_session), None: none

    @property
    def n_shark_sets(self):
        return 0 if self._set_prob is None else len(self._set_prob)

    def set_shark_grids(self, grids, first_bin=None):
        """One shark-occupancy table per tracked shark, for shark_of: a list of sharkGrid dicts with the constructor's bin
        keys and cell order, or a sharkForecast.Forecast -- then its prob [F, R+1, C] goes from the forecast's context to
        the planner's without leaving HBM (the cell list must be the planner's).  first_bin=None: R + 1 must be the planner's
        bin count T and round j is bin j.  first_bin=b (0 .. T-1; a Forecast only): the forecast speaks from "now" and now is
        bin b -- set f's bin t reads forecast round min(max(t - b, 0), R), for any R; unless b == 0 and R + 1 == T (the call
        without first_bin) sf_place_kernel gathers the rows on the device.  ValueError otherwise.  None or an empty list
        clears the tables.  The constructor's own grid stays the table of every call without shark_of.  RuntimeError while a
        replanning session is open: its own set_shark_grids is the way then."""
        self._no_session("set_shark_grids")
        self._set_prob = put_shark_tables(self._ctx, self._bins, self._cells, grids, first_bin)

    def _no_session(self, what):
        session = getattr(self, "_session", None)
        if session is not None and not session.inside:
            raise RuntimeError("%s: a replanning session is open on this RRT (finish() it first)" % what)

    # ------------------------------------------------------------------ reference API
    def exploring(self, initial, habitats, plot_interval, bin_interval, v, shark_interval, traj_time_stamp=False,
                  max_plan_time=5, max_traj_time=200.0, plan_time=True, weights=[-1, -1, -1], max_iter=None,
                  seed=None):
        res = self.exploring_batch([initial], habitats, plot_interval, bin_interval, v, shark_interval,
                                   traj_time_stamp, max_plan_time, max_traj_time, plan_time, weights,
                                   max_iter=max_iter, seeds=None if seed is None else [seed])
        r = res[0]
        if r is None:
            # rrt_dubins.py:174: opt_path is None -> opt_path[1] raises
            raise TypeError("'NoneType' object is not subscriptable")
        return r

    def exploring_batch(self, initials, habitats, plot_interval, bin_interval, v, shark_interval,
                        traj_time_stamp=False, max_plan_time=5, max_traj_time=200.0, plan_time=True,
                        weights=[-1, -1, -1], max_iter=None, seeds=None, habitat_masks=None, shark_of=None):
        """E independent exploring() calls in one launch (one wavefront per episode).  Returns a list of
        result dicts (None where the reference would have raised for lack of a qualifying leaf).

        shark_of [E] (time-bin mode): episode e ranks its leaves against table shark_of[e] of set_shark_grids and equals
        exploring() of an RRT built with that table.  The tree does not depend on the table.

        Per-episode limits (time-bin mode): max_traj_time [E] gives every episode its own horizon, habitat_masks ([E] ints,
        bit h = habitats[h], or [E, H] booleans) its own habitat list -- the subsequence of `habitats` its mask selects.
        Episode e then equals exploring(initials[e], [its habitats], ..., max_traj_time=max_traj_time[e])."""
        self._no_session("exploring_batch")
        E = len(initials)
        sets = None if shark_of is None else shark_set_indices(shark_of, E, self.n_shark_sets, bool(plan_time and traj_time_stamp))
        if max_iter is None:
            max_iter = max(1, int(math.ceil(max_plan_time * self.iters_per_second)))
        use_global = seeds is None
        if use_global:
            if E != 1:
                raise ValueError("seeds are required for a batch (the global random stream is one stream)")
            words, idx = _mt_state_of(random.getstate())
            seed_arg = (words.reshape(1, 624), np.array([idx], dtype=np.int32))
        else:
            seed_arg = np.array([int(s) for s in seeds], dtype=np.uint64)
        summ = self._explore_summaries(initials, habitats, bin_interval, v, traj_time_stamp, max_traj_time, plan_time, weights,
                                       max_iter, seed_arg, habitat_masks, shark_set=sets)
        if use_global:
            n = int(summ[0]["n_draw32"])
            if n:
                random.getrandbits(32 * n)  # advance the global stream by what the device consumed
        self._batch = (list(initials), shark_interval, max_traj_time)
        return self._batch_results(summ)

    def rerank(self, shark_of):
        """The last exploring_batch's trees ranked again, every episode against table shark_of[e] (None: the constructor's
        grid): what exploring_batch would return with that shark_of, for the price of the leaf pass -- no tree is grown.  The
        batch must have gone the per-episode-limits route (shark_of, habitat_masks or max_traj_time [E]) for a table per
        episode; AuvpError (AUVP_ERR_STATE) otherwise, or without a batch."""
        self._no_session("rerank")
        if self._batch is None:
            raise _lib.AuvpError(-4, "no exploring_batch to rank again")
        sets = None if shark_of is None else shark_set_indices(shark_of, len(self._batch[0]), self.n_shark_sets)
        self._ctx.rrt_set_episode_grids(sets)
        return self._batch_results(self._ctx.rrt_rerank())

    def _batch_results(self, summ):
        """the result dicts of exploring_batch from the summaries of the batch self._batch describes"""
        initials, shark_interval, max_traj_time = self._batch
        E = len(initials)
        bad = summ["status"] < 0
        if bad.any():
            e = int(np.argmax(bad))
            raise _lib.AuvpError(int(summ[e]["status"]), "episode %d failed on the device (status %d)"
                                 % (e, int(summ[e]["status"])))
        paths = self._ctx.paths(summ)
        self._last = (summ, list(initials))
        self._mps_cache = None
        self.t_start = 0.0
        horizons = np.broadcast_to(np.asarray(max_traj_time, dtype=np.float64), (E,))
        out = []
        for e in range(E):
            s = summ[e]
            if s["status"] == _lib.NO_QUALIFYING_LEAF:
                out.append(None)
                continue
            course = self._materialise_course(paths[e], initials[e])
            mtt = max_traj_time if np.ndim(max_traj_time) == 0 else float(horizons[e])
            split = self.splitPath(course, shark_interval, [initials[e].traj_time_stamp, mtt])
            c = [float(x) for x in s["best_cost"]]
            out.append({"path length": float(s["best_length"]), "path": [course, split], "cost": [c[0], c[1:]]})
        return out

    def _explore_summaries(self, initials, habitats, bin_interval, v, traj_time_stamp, max_traj_time, plan_time, weights,
                           max_iter, seed_arg, habitat_masks=None, summaries=True, shark_set=None):
        """one prepare + run of exploring episodes on this object's context; the summaries (statuses unchecked), or None with
        summaries=False: they stay in HBM (best-of-K planning reads them there)"""
        mode = "timebin" if (plan_time and traj_time_stamp) else ("plantime" if plan_time else "nn")
        hab = _circles(habitats)
        self._ctx.set_habitats(hab)
        init = np.array([[float(m.x), float(m.y), float(m.theta), float(m.traj_time_stamp),
                          float(m.plan_time_stamp), float(m.length)] for m in initials], dtype=np.float64).reshape(-1, 6)
        keep = None
        self._batch = None  # (rerank follows an exploring_batch only)
        if habitat_masks is not None or np.ndim(max_traj_time) > 0:  # per-episode limits
            keep = np.array(habitat_keep_bits(habitat_masks, len(hab), len(init)), dtype=np.uint64)
        return self._ctx.rrt_explore_batch(init, seed_arg, int(max_iter), mode=mode, freq=self.freq,
                                           bin_interval=bin_interval, v=v, max_traj_time=max_traj_time,
                                           weights=weights, dist_to_end=self.dist_to_end, diff_max=self.diff_max,
                                           min_dist=0.5, max_plan_time=float(max_iter),  # virtual clock: 1 tick per iteration
                                           habitat_keep=keep, shark_set=shark_set, **({} if summaries else {"summaries": False}))

    def exploring_best_of(self, initials, habitats, plot_interval, bin_interval, v, shark_interval, traj_time_stamp=False,
                          max_plan_time=5, max_traj_time=200.0, plan_time=True, weights=[-1, -1, -1], max_iter=None,
                          seeds=None, habitat_masks=None, shark_of=None):
        """Best of K trees for each of N AUVs in one launch: seeds [N][K]; AUV i's members are the batch's episodes i*K ..
        i*K+K-1, each an ordinary exploring episode from initials[i] with seeds[i][m] (and max_traj_time[i], habitat_masks[i]
        where those are per AUV, as in exploring_batch).  The winner is exploring's own rule folded over the members in order
        (the lowest cost, the earliest member among equal costs), chosen on the device; only the winners' courses are copied to
        the host and turned into objects.  Returns N dicts shaped like exploring's plus "tree", the winning member's index;
        None where no member has a qualifying leaf.  A member that failed on the device raises AuvpError.
        shark_of [N]: AUV i's K trees are all ranked against table shark_of[i] of set_shark_grids."""
        self._no_session("exploring_best_of")
        N = len(initials)
        if seeds is None or len(seeds) != N or N == 0:
            raise ValueError("seeds [N][K] are required: one row of K seeds per AUV")
        K = len(seeds[0])
        if K < 1 or any(len(row) != K for row in seeds):
            raise ValueError("every AUV needs the same number (>= 1) of seeds")
        if max_iter is None:
            max_iter = max(1, int(math.ceil(max_plan_time * self.iters_per_second)))
        sets = None if shark_of is None else np.repeat(shark_set_indices(shark_of, N, self.n_shark_sets,
                                                                         bool(plan_time and traj_time_stamp)), K)
        seed_arg = np.array([int(s) for row in seeds for s in row], dtype=np.uint64)
        members = [initials[i] for i in range(N) for _ in range(K)]
        per_auv = habitat_masks is not None or np.ndim(max_traj_time) > 0
        horizons = np.broadcast_to(np.asarray(max_traj_time, dtype=np.float64), (N,))
        mtt = np.repeat(horizons, K) if per_auv else max_traj_time
        masks = np.repeat(np.array(habitat_keep_bits(habitat_masks, len(habitats), N), dtype=object), K).tolist() if per_auv else None
        self._explore_summaries(members, habitats, bin_interval, v, traj_time_stamp, mtt, plan_time, weights, max_iter,
                                seed_arg, masks, summaries=False, shark_set=sets)
        best = self._ctx.rrt_group_best(np.arange(N + 1, dtype=np.int64) * K)
        raise_bad_status(best["status"], range(N), fmt=TREE_FAILED)
        paths = self._ctx.group_paths(best)
        self._last = None  # (mps_list is the tree of a single exploring call)
        self._mps_cache = None
        self.t_start = 0.0
        out = []
        for i in range(N):
            b = best[i]
            if b["winner"] < 0:
                out.append(None)
                continue
            course = self._materialise_course(paths[i], initials[i])
            h = max_traj_time if np.ndim(max_traj_time) == 0 else float(horizons[i])
            split = self.splitPath(course, shark_interval, [initials[i].traj_time_stamp, h])
            c = [float(x) for x in b["cost"]]
            out.append({"path length": float(b["length"]), "path": [course, split], "cost": [c[0], c[1:]],
                        "tree": int(b["winner"]) - i * K})
        return out

    def replanning(self, start, habitats, plan_time_budget, traj_time_length, replan_time_interval, weight,
                   max_iter=None, seed=None):
        """Receding-horizon planning (rrt_dubins.py:51-90): plan a horizon with `exploring`, commit the first
        shark-interval bucket of the best course, drop the habitats that bucket visited, repeat until the
        shark grid's last bin ends.  Returns [committed trajectory, {round: [bucket, habitats at that round]},
        cost of the whole trajectory against the ORIGINAL habitat list].

        Like the reference (:67) the call leaves a `SharkUpdate` over the planner's boundary and cell list in
        `self.sharkEstimate` (sharkEstimate.py, host arithmetic; nothing here reads it, neither does the reference); the
        SharkOccupancyGrid of :68 is likewise never read and is not built (its constructor splits polygons with
        shapely).  The final cost runs on a cost-only device context of its own, so this object's obstacles and
        boundary stay on the device for later exploring() / check_collision() calls."""
        from .cost import habitat_shark_cost_func
        from .sharkEstimate import SharkUpdate
        self._no_session("replanning")
        self.sharkEstimate = SharkUpdate(self.boundary_poly, 10, self.cell_list)
        horizon_end = list(self.sharkGrid.keys())[-1][1]
        round_span = plan_time_budget + replan_time_interval  # also the shark_interval handed to exploring (:80)
        all_habitats = list(habitats)
        stream = random.Random(seed) if seed is not None else None
        committed, rounds = [start], {}
        while committed[-1].traj_time_stamp + round_span < horizon_end:
            t_now = committed[-1].traj_time_stamp
            if traj_time_length + t_now > horizon_end:  # stays clipped for the later rounds too (:76-77)
                traj_time_length = horizon_end - t_now
            plan = self.exploring(committed[-1], habitats, 0.5, 5, 2, round_span, traj_time_stamp=True,
                                  max_plan_time=plan_time_budget, max_traj_time=traj_time_length + t_now,
                                  plan_time=True, weights=weight, max_iter=max_iter,
                                  seed=stream.getrandbits(63) if stream is not None else None)
            buckets = plan["path"][1]
            first_bucket = buckets[next(iter(buckets))]
            committed += first_bucket
            rounds[len(rounds) + 1] = [first_bucket, list(habitats)]
            habitats = self.removeHabitat(habitats, first_bucket)
        if self._cost_ctx is None:
            self._cost_ctx = _lib.Context(self._ctx.device)
        total = habitat_shark_cost_func(committed[1:], committed[-1].traj_time_stamp, all_habitats, self.sharkGrid,
                                        weight=[-3, -3, -4], device_context=self._cost_ctx)
        return [committed[1:], rounds, total]

    def replanning_batch(self, starts, habitats, plan_time_budget, traj_time_length, replan_time_interval, weight,
                         max_iter=None, seeds=None, rngs=None, as_arrays=False, trees_per_auv=1, shark_of=None, commit="host",
                         teams=None, team_pick=None, team_separation=None, separation_tick=1.0, separation_ticks=None):
        """N replanning() loops -- independent ones unless `teams` is given --, one exploring launch per round over the AUVs still planning (per-episode
        limits: every AUV its own horizon and habitat list, rrt_explore_lim_kernel).  Entry e equals
        replanning(starts[e], list(habitats), ..., seed=seeds[e]); with rngs[e] (a random.Random, taking precedence over
        seeds[e]) it equals the call that continues the global stream in that generator's state, and the generator is
        advanced as exploring advances the global stream.  The caller's `habitats` list is not changed: every entry carries
        its own list of the habitats left.  An AUV whose call would raise TypeError (no qualifying leaf) gets None.

        Returns a list of [committed trajectory, {round: [bucket, habitats at that round]}, cost, habitats left]
        (Motion_plan_state objects and the caller's habitat objects; the first three as replanning returns them) or, with as_arrays=True, of dicts of numpy arrays: traj [n,7] (x, y, theta, v, traj_time_stamp,
        plan_time_stamp, length), round_len [R], round_keep [R] (habitat bit masks at each round), round_max_traj_time [R],
        round_cost [R,4], round_tree [R], keep (the habitats left), cost [4].  The SharkUpdate that replanning leaves in
        self.sharkEstimate is not built (nothing reads it).

        trees_per_auv = K > 1: every round grows K trees per AUV -- AUV e draws K seeds from its stream in member order, all K
        plan from its committed state with its horizon and habitat list -- and commits the first bucket of the best one (the
        rule of exploring_best_of, chosen on the device; only the winners' courses reach the host).  round_tree names the
        winning member of each round.  An AUV without a winner in some round gets None.  Seeds only: one generator cannot
        continue K streams, so rngs raises ValueError.

        shark_of [N]: AUV e plans every round against table shark_of[e] of set_shark_grids, and its whole trajectory's cost
        is taken against that table (one cost launch per table in use); entry e equals the call on an RRT built with it.

        commit="device": the step between two rounds runs on the device (rrt_commit_kernel behind the winners' selection) --
        the courses stay in HBM, one 128-byte record per AUV and round comes back, the host's part of a round is numpy over
        [N] arrays, and the committed trajectories are downloaded once at the end (a ReplanSession, run to its end:
        replanning_session gives the same loop one round at a time).  The results equal commit="host" (the default) in every field.  Seeds only (rngs raises ValueError).  On both routes the ValueError for a horizon that
        holds no whole bucket is raised before the round is launched.

        teams [N] integers: AUVs with the same label >= 0 form a team that shares one habitat list, a label < 0 is an AUV on
        its own, labels need not be dense, and a team of one member behaves as no team.  After every round, once all of the
        round's commits are done, every member's list becomes the intersection of the lists of ALL members of its team
        (team_fold) -- the members that are not planning any more included, whether they reached the end of their horizon or
        found no qualifying leaf.  A habitat one AUV has visited so comes off its teammates' lists.  Within a round every
        member plans against the list it had at the round's start; two teammates may visit the same habitat in one round.
        Round 1 of every AUV equals the run without teams; round_keep[r] and the rounds dict's habitat list are the team's list
        at the start of round r; keep / the habitats left of every member are the team's list at the end of the call; costs
        stay against the original list.  Without team_pick (below) the planner itself is not team-aware (leaf ranking and winner
        selection are each AUV's own).  Works with rngs (commit="host"), trees_per_auv and shark_of; with commit="device" the fold is
        replan_team_kernel behind rrt_commit_kernel, and the records that come back carry the team's list.  ValueError, before
        any launch, for a wrong length, a bool or a value that is no integer.

        team_pick="claims" (needs teams; None: the call as described so far) makes the winner selection team-aware, so that the K
        trees of trees_per_auv spread a team out instead of steering two members to one habitat.  Per round and team of two or
        more, claimed = 0 and the members that plan in this round are taken in ascending AUV index: each of the member's K
        trees offers its own best course (as the leaf pass ranked it under the member's list), every such course is scored
        again under list & ~claimed -- the cost exploring would have given it against the shorter list: only the habitat terms
        change, the shark term does not --, the winner is the usual fold over these scores, and the habitats its WHOLE course
        visits under that mask join claimed (team_pick_claims is the definition).  The first planning member of a team sees
        claimed == 0: its scores are the trees' own costs bit for bit and its winner is the one without team_pick; so are those of
        AUVs without a teammate.  The commit and the team fold run unchanged on the chosen winners (under the member's own list:
        a habitat visited is visited).  round_tree names the chosen tree; round_cost is the winner's score UNDER THE MASK IT WAS
        JUDGED BY, not its cost under the member's list; with as_arrays=True round_claimed [R] (uint64) is the claimed mask the
        member saw.  Not done: ranking a tree's leaves again under the reduced list (one leaf pass per member, one after the
        other) -- a tree's candidate is always its best leaf under the member's own list.  Works with trees_per_auv (any K),
        shark_of, seeds and both commit routes; with commit="host" every candidate's course is copied to the host, with
        commit="device" rrt_course_words_kernel and replan_team_pick_kernel run behind the leaf pass and nothing more than
        today's records crosses the bus.  Memory, paid only with team_pick on the device route: a scratch buffer of one 8-byte
        word per possible course point, (max_iter + 1 + the batch's path-point capacity) words for each of the N * K trees,
        reserved at the first round and kept by the context (4.3 GiB for 4 096 AUVs x 4 trees at max_iter=2000; about a sixth of
        what the trees' path points take); it grows with max_iter and with N * K, and where the device cannot provide it the
        round raises AuvpError (a HIP allocation error).  ValueError, before any launch, without teams or for another value.

        team_separation=d (metres, a finite float > 0; needs teams; None: the call as described so far) keeps the courses that
        teammates commit in one round apart.  It is a criterion of its own beside team_pick and works with None and "claims".
        A course is looked at on the ticks s * separation_tick (seconds, finite > 0) of a window of separation_ticks = W ticks
        from the AUV's committed state (an int in 1 .. 1024; None: ceil((plan_time_budget + replan_time_interval) /
        separation_tick), the part a round commits); between two points an AUV is taken to stay at the last point it reached
        (course_ticks is the definition).  Per round and team of two or more the members that plan are taken in ascending AUV
        index; n of a candidate is the number of its ticks at which it is closer than d to the winner some earlier member chose
        in this round (tick_conflicts: dx * dx + dy * dy < d * d); among the candidates whose score is < inf the winner is the
        smallest (n, score), the lowest tree among equals (team_pick_separated is the definition).  The score is the tree's own
        cost, or with team_pick="claims" the cost under list & ~claimed, and the claims accumulate as they do without the
        option.  Where no candidate has a conflict the choice is the one without the option; so are those of the first planning
        member of a team and of AUVs without a teammate.  Where every candidate conflicts the least conflicting one is
        committed and nothing is raised: with as_arrays=True round_conflicts [R] (int64) is the committed winner's n.  Works with
        any trees_per_auv, shark_of and both commit routes (commit="device": rrt_course_ticks_kernel and
        replan_team_pick_apart_kernel behind the leaf pass, N * K * W * 16 bytes of scratch, and the count rides in the round
        record); with rngs on commit="host" with one tree, where the one candidate is chosen and only the count is recorded.
        Limits: only the courses chosen in THIS round are compared -- not the committed log of earlier rounds, so teammates
        whose rounds start a few seconds apart are not compared over that gap --; positions are sampled, not swept: choose d with
        the margin that speed x separation_tick calls for.  ValueError, before any launch: without teams, for a d or tick that is
        not finite and > 0 or is a bool, W outside 1 .. 1024, a horizon whose end / separation_tick reaches 2**31, or a team of
        more than 1024 members."""
        self._no_session("replanning_batch")
        args = replan_args(self, starts, habitats, plan_time_budget, replan_time_interval, max_iter, trees_per_auv, shark_of, teams,
                           team_pick, team_separation, separation_tick, separation_ticks, seeds, rngs, commit)
        # one loop for both routes (replanning.py): a session, its rounds until nobody plans any more, its end
        return ReplanSession(self, starts, traj_time_length, weight, back_end=DeviceRounds if commit == "device" else HostRounds,
                             **args).run(as_arrays)

    def replanning_session(self, starts, habitats, plan_time_budget, traj_time_length, replan_time_interval, weight, max_iter=None,
                           seeds=None, trees_per_auv=1, shark_of=None, teams=None, team_pick=None, team_separation=None,
                           separation_tick=1.0, separation_ticks=None):
        """replanning_batch(commit="device") one round at a time: a ReplanSession whose round() is one iteration of that call's
        loop and whose finish() returns what the call returns; between two rounds set_shark_grids may swap the shark tables.
        The arguments are replanning_batch's (seeds only), with the same ValueErrors before any launch.  RuntimeError while
        another session is open on this RRT."""
        self._no_session("replanning_session")
        if getattr(self, "_session", None) is not None:
            raise RuntimeError("replanning_session: a replanning session is open on this RRT (finish() it first)")
        return ReplanSession(self, starts, traj_time_length, weight, **replan_args(
            self, starts, habitats, plan_time_budget, replan_time_interval, max_iter, trees_per_auv, shark_of, teams, team_pick,
            team_separation, separation_tick, separation_ticks, seeds))

    # ------------------------------------------------------------------ host-side helpers (reference names)
    def splitPath(self, path, shark_interval, traj_time):
        """Bucket a course by shark interval (rrt_dubins.py:590-602): floor(traj_time[1] / shark_interval)
        closed intervals starting at traj_time[0]; a point goes to the first interval that contains its
        traj_time_stamp (so a point on a shared end belongs to the earlier one) or to none."""
        t0 = traj_time[0]
        edges = [(t0 + k * shark_interval, t0 + (k + 1) * shark_interval)
                 for k in range(math.floor(traj_time[1] / shark_interval))]
        buckets = {e: [] for e in edges}
        for point in path:
            t = point.traj_time_stamp
            hit = next((e for e in edges if e[0] <= t <= e[1]), None)
            if hit is not None:
                buckets[hit].append(point)
        return buckets

    def removeHabitat(self, habitats, path):
        """rrt_dubins.py:604-610: every path point removes the first habitat (current list order) that contains
        it.  Mutates and returns the caller's list, like the reference."""
        for point in path:
            inside = next((h for h in habitats if math.sqrt((point.x - h.x) ** 2 + (point.y - h.y) ** 2) <= h.size), None)
            if inside is not None:
                habitats.remove(inside)
        return habitats

    def check_collision(self, mps, obstacleList=None):
        """rrt_dubins.py:530-549 for one node (its .path points), evaluated on the device against the
        obstacle list given at construction (the reference always passes self.obstacle_list)."""
        if mps is None:
            return False
        pts = [(float(p.x), float(p.y)) for p in mps.path]
        if not pts:
            return True
        return bool(self._ctx.check_collision([pts])[0])

    def _materialise_course(self, arr, initial):
        course = []
        for i in range(len(arr)):
            if i == 0:
                course.append(initial)  # the reference returns the caller's own start object
                continue
            r = arr[i]
            course.append(Motion_plan_state(float(r[0]), float(r[1]), theta=float(r[2]), v=float(r[3]),
                                            traj_time_stamp=float(r[4]), plan_time_stamp=float(r[5]),
                                            length=float(r[6])))
        return course

    @property
    def mps_list(self):
        """The tree of the last exploring() call as linked Motion_plan_state objects (built on first
        access: the tree stays in HBM until someone asks for Python objects)."""
        if self._mps_cache is None:
            if self._last is None:
                return []
            summ, initials = self._last
            t = self._ctx.tree(0, summ[0])
            nodes = [initials[0]]
            for i in range(1, len(t["nodes"])):
                n = t["nodes"][i]
                nodes.append(Motion_plan_state(float(n[0]), float(n[1]), theta=float(n[2]), traj_time_stamp=float(n[3]),
                                               plan_time_stamp=float(n[4]), length=float(n[5])))
            for i in range(1, len(nodes)):
                par = nodes[int(t["parent"][i])]
                nodes[i].parent = par
                path = [par]
                o, c = int(t["pt_off"][i]), int(t["pt_cnt"][i])
                for q in t["points"][o:o + c]:
                    path.append(Motion_plan_state(float(q[0]), float(q[1]), theta=float(q[2]), v=float(q[3]),
                                                  traj_time_stamp=float(q[4]), plan_time_stamp=float(q[5]),
                                                  length=float(q[6])))
                nodes[i].path = path
            self._mps_cache = nodes
        return self._mps_cache


def createSharkGrid(filepath, cell_list):
    """CSV -> {(t0,t1): {cell.bounds: prob}} (rrt_dubins.py:612-630): header `time bin,grid`, one row
    per bin: "(t0, t1)","[p0, p1, ...]"; value i belongs to cell_list[i]."""
    import csv
    out = {}
    with open(filepath, newline="") as f:
        for row in csv.DictReader(f):
            a, b = row["time bin"].split(", ")
            key = (int(a[1:]), int(b[:-1]))
            vals = row["grid"][1:-1].split(", ")
            out[key] = {cell_list[i].bounds: float(vals[i]) for i in range(len(vals))}
    return out

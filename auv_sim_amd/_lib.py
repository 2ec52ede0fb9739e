"""ctypes binding of libauvplan.so (include/auvplan.h).

There is no CPU fallback: importing this module without the built library, or creating a context
without a usable MI355X, raises.  Build with `python __graft_entry__.py build` (hipcc, gfx950).
"""
import ctypes as C
import os

import numpy as np

# the structs, constants and prototypes of the C-ABI live in _cabi; the names below stay importable from here
from ._cabi import (FLAG_ITER_LOG, FLAG_LEAF_LOG, FLAG_PHASE_CLOCKS, KFLAG_NN_EXACT, KFLAG_TIGHT_CULL, MODES,  # noqa: F401
                    NO_QUALIFYING_LEAF, OK, OPTION_NAMES, EPISODE_DTYPE, GROUP_BEST_DTYPE, REPLAN_RECORD_DTYPE, SUMMARY_DTYPE,
                    RRTGroupBest, RRTParams, RRTSummary, _PrrtLaunchChoice, _PrrtLaunchQuery, _RrtLaunchChoice, _RrtLaunchQuery,
                    _SfLaunchChoice, _SfLaunchQuery, bind)
from ._cabi import bp as _bp, dp as _dp, ip as _ip  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AUVPLAN_LIBRARY") or os.path.join(HERE, "libauvplan.so")  # override: kernel experiments
MEAS_MAX_TICKS = 64  # option MEAS_TICKS, the k of replan_measure's shark_xy [k,F,2] (csrc/replan_ticks.h: REPLAN_MEAS_MAX_TICKS)

# numpy element type -> pointer type (what _p picks for an array)
_PTR = {np.dtype(t): C.POINTER(c) for t, c in (("f8", C.c_double), ("i4", C.c_int32), ("i8", C.c_int64), ("u8", C.c_uint64),
                                               ("u4", C.c_uint32), ("u1", C.c_uint8), ("i1", C.c_int8))}


class AuvpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("auvplan error %d: %s" % (code, msg))
        self.code = code


_lib = None


def _share_hip_runtime_with_torch():
    """A process must hold ONE HIP/HSA runtime.  PyTorch-ROCm bundles its own libamdhip64.so.7 /
    libhsa-runtime64.so.1 (same SONAMEs as /opt/rocm's); whichever copy is loaded first serves both
    torch and libauvplan.so.  torch does not find its GPU on the system copy, so when torch is
    installed its copies are mapped first (without importing torch).  AUVP_SYSTEM_HIP=1 opts out."""
    import sys
    if os.environ.get("AUVP_SYSTEM_HIP") == "1" or "torch" in sys.modules:
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        libdir = os.path.join(os.path.dirname(spec.origin), "lib")
        for name in ("libhsa-runtime64.so", "libamdhip64.so"):
            p = os.path.join(libdir, name)
            if os.path.exists(p):
                C.CDLL(p, mode=C.RTLD_GLOBAL)
    except OSError:
        pass  # fall back to the system runtime; torch (if imported later) may then not see the GPU


def load():
    """Load libauvplan.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: build the HIP extension first "
                          "(python -c 'import __graft_entry__ as g; g.build()')" % LIB_PATH)
    _share_hip_runtime_with_torch()
    _lib = bind(C.CDLL(LIB_PATH))
    return _lib


def _arr(a, dtype, shape=None):
    """a as a C-contiguous array of dtype (no copy where it already is one), reshaped if a shape is given"""
    a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
    return a.reshape(shape) if shape is not None else a


def _f64(a, shape=None):
    return _arr(a, np.float64, shape)


def _p(a, t=None):
    """pointer to a's data: of type t, else of a's own element type (an array of records: a void pointer)"""
    return a.ctypes.data_as(t or _PTR.get(a.dtype, C.c_void_p))


def episode_limits(n_episodes, max_traj_time, habitat_keep, n_habitats, mode="timebin", iter_log=False, phase_clocks=False):
    """The per-episode limits of a batch (auvp_rrt_prepare_episodes): max_traj_time a number or [E], habitat_keep None (every
    habitat) or [E] bit masks over the world's habitat table.  Returns (cap = the largest horizon, [E] EPISODE_DTYPE records);
    raises ValueError on what the library refuses: another mode than time-bin, the iteration log or phase clocks, a horizon
    that is not > 0, a bit at or above n_habitats."""
    E = int(n_episodes)
    if mode != "timebin":
        raise ValueError("per-episode limits need time-bin mode, not %r" % (mode,))
    if iter_log or phase_clocks:
        raise ValueError("per-episode limits: no iteration log or phase clocks (the leaf log is allowed)")
    mtt = np.broadcast_to(np.asarray(max_traj_time, dtype=np.float64), (E,))
    if not np.all(mtt > 0) or not np.all(np.isfinite(mtt)):
        raise ValueError("every max_traj_time must be finite and > 0")
    allowed = (1 << int(n_habitats)) - 1 if n_habitats < 64 else (1 << 64) - 1
    if habitat_keep is None:
        keep = [allowed] * E
    elif isinstance(habitat_keep, np.ndarray) and habitat_keep.dtype == np.uint64 and habitat_keep.shape == (E,):
        # (a fleet's masks as an array: the same check without a Python loop over the episodes)
        bad = np.flatnonzero(habitat_keep & np.uint64(~allowed & ((1 << 64) - 1)))
        if len(bad):
            raise ValueError("episode %d: habitat_keep 0x%x names habitats outside the table of %d"
                             % (bad[0], int(habitat_keep[bad[0]]), n_habitats))
        rec = np.zeros(E, dtype=EPISODE_DTYPE)
        rec["max_traj_time"] = mtt
        rec["habitat_keep"] = habitat_keep
        return float(mtt.max()), rec
    else:
        keep = [int(k) for k in np.broadcast_to(np.asarray(habitat_keep, dtype=object), (E,))]
    for e, k in enumerate(keep):
        if k < 0 or k & ~allowed:
            raise ValueError("episode %d: habitat_keep 0x%x names habitats outside the table of %d" % (e, k, n_habitats))
    rec = np.zeros(E, dtype=EPISODE_DTYPE)
    rec["max_traj_time"] = mtt
    rec["habitat_keep"] = np.array(keep, dtype=np.uint64)
    return float(mtt.max()), rec


def rows_stream_shape(K, n_habitats, n_poly, n_bins, waves_wanted=12, force=-1):
    """the launch the host chooses for rrt_rows_stream_kernel (no GPU needed): (waves per workgroup, mirrored ring?, LDS bytes)
    for K time bins and a world with these table sizes; force: -1 the host's rule, 0 the masked ring, 1 the mirrored one"""
    w, m, l = C.c_int32(), C.c_int32(), C.c_int32()
    rc = load().auvp_rrt_rows_stream_shape(int(K), int(n_habitats), int(n_poly), int(n_bins), int(waves_wanted), int(force),
                                           C.byref(w), C.byref(m), C.byref(l))
    if rc != 0:
        raise AuvpError(rc, "auvp_rrt_rows_stream_shape: bad argument")
    return w.value, bool(m.value), l.value


RRT_KINDS = ("explore", "explore_lim", "duo", "trio", "rows", "rows_stream")
PRRT_KINDS = ("one", "pipe", "rows")


def _ask_launch(fn, query, choice, options, kinds):
    opts = sorted((options or {}).items())
    names = (C.c_char_p * max(len(opts), 1))(*[k.encode() for k, _ in opts])
    values = (C.c_int64 * max(len(opts), 1))(*[int(v) for _, v in opts])
    query.n_options, query.option_names, query.option_values = len(opts), names, values
    rc = getattr(load(), fn)(C.byref(query), C.byref(choice))
    if rc != 0:
        raise AuvpError(rc, fn + ": bad argument or unknown option")
    out = {n: getattr(choice, n) for n, _ in choice._fields_ if n != "_pad"}
    out["name"] = (choice.name or b"").decode()
    out["kind"] = kinds[choice.kind]
    return out


def rrt_choose_launch(E, n_cu=256, mode="timebin", max_iter=10000, K=100, flags=0, freq=30.0, dist_to_end=2.0, max_pts=None,
                      O=0, H=0, V=0, T=0, obst_area=0.0, lim=False, one_wave_only=False, no_stream=False, seen_most=0, seen_E=0,
                      options=None):
    """the expansion launch the host would choose for this RRT.exploring batch (auvp_rrt_choose_launch; no GPU needed): a dict
    of the plan -- kind (one of RRT_KINDS), name, J, quad, grid, block, lds, lds_max, kflags, stream_len, stream_waves, mirror,
    status (0, or -1 with lds_need: the LDS plan does not fit).  K: time bins (ceil(max_traj_time / bin_interval) in time-bin
    mode); O, H, V, T: the world's obstacles, habitats, boundary vertices, time bins; options: {name: value} of the options that
    are set; seen_most / seen_E: what earlier batches with the same parameters drew (0: nothing seen)"""
    import math
    q = _RrtLaunchQuery(n_episodes=int(E), n_cu=int(n_cu), mode=MODES.get(mode, mode), max_iter=int(max_iter),
                        n_time_bins=int(K), flags=int(flags), freq=float(freq), dist_to_end=float(dist_to_end),
                        max_pts=int(math.floor(freq)) + 2 if max_pts is None else int(max_pts), n_obstacles=int(O), n_habitats=int(H),
                        n_poly=int(V), n_bins=int(T), obst_area=float(obst_area), per_episode_limits=int(bool(lim)),
                        one_wave_only=int(bool(one_wave_only)), no_stream=int(bool(no_stream)), seen_E=int(seen_E), seen_most=int(seen_most))
    return _ask_launch("auvp_rrt_choose_launch", q, _RrtLaunchChoice(), options, RRT_KINDS)


def prrt_choose_launch(E, n_cu=256, O=0, freq=10.0, max_step=300, n_buckets=0, flags=0, max_pts=None, cap_nodes=None, step_mode=0,
                       waits=True, one_wave_only=False, rows=None, options=None):
    """the launch the host would choose for this Planner_RRT batch (auvp_prrt_choose_launch; no GPU needed): a dict of the plan --
    kind (one of PRRT_KINDS), name, lat, rows, pipe, draw_wave, next_lds, bk_lds, obst_lds, eps_wg, grid, block, lds, J, status.
    step_mode 0 / waits True: plan(); step_mode 1: step(); waits False: a step of the device-resident loop.  rows: None decides the
    four-episode choice as creating the batch does, True / False is the batch's frozen choice"""
    import math
    q = _PrrtLaunchQuery(n_episodes=int(E), n_cu=int(n_cu), n_obstacles=int(O),
                         max_pts=int(math.floor(freq)) + 3 if max_pts is None else int(max_pts),
                         cap_nodes=int(max_step) + 1 if cap_nodes is None else int(cap_nodes), n_buckets=int(n_buckets),
                         max_step=int(max_step), flags=int(flags), freq=float(freq), step_mode=int(step_mode), waits=int(bool(waits)),
                         one_wave_only=int(bool(one_wave_only)), rows=-1 if rows is None else int(bool(rows)))
    return _ask_launch("auvp_prrt_choose_launch", q, _PrrtLaunchChoice(), options, PRRT_KINDS)


SF_KINDS = ("one-wave", "wide")


def forecast_choose_launch(rows, cols, n_cells=0, widest_level=0, allow_large=False, options=None):
    """the launch the host would choose for a shark-occupancy forecast on a rows x cols grid (auvp_sf_choose_launch; no GPU
    needed): a dict -- kind (one of SF_KINDS), name, block (threads per workgroup; one workgroup per filter), lds (bytes), status
    (0; -2 AUVP_ERR_CAPACITY: more grid entries than the entry point takes; -1 AUVP_ERR_ARG: a shape < 1 or a bad SF_WIDE_BLOCK).
    allow_large: False = auvp_sf_forecast, True = auvp_sf_forecast_large (`SharkForecast.run(large_grids=True)`); n_cells /
    widest_level: of the list and its schedule (`forecast_plan`), 0 = not known; options: {name: value} of the options set"""
    q = _SfLaunchQuery(rows=int(rows), cols=int(cols), n_cells=int(n_cells), widest_level=int(widest_level),
                       allow_large=int(bool(allow_large)))
    return _ask_launch("auvp_sf_choose_launch", q, _SfLaunchChoice(), options, SF_KINDS)


def forecast_plan(rows, cols, cell_rc):
    """the level schedule the shark-occupancy forecast walks for prediction1 (auvp_sf_plan; no GPU needed).  cell_rc [C, 2]:
    (row, column) of every cell of cell_list, in list order.  Returns a dict: level [C] (0 where no 4-neighbour of the cell is
    earlier in the list, else 1 + the highest level among the earlier neighbours), order [C] (list positions sorted by (level,
    position)), level_off [n_levels + 1], n_levels.  AuvpError (AUVP_ERR_ARG): a cell outside the grid, a cell listed twice,
    an empty list."""
    rc = _arr(cell_rc, np.int32, (-1, 2))
    n = len(rc)
    level, order, off = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(n + 1, np.int32)
    nl = C.c_int32()
    code = load().auvp_sf_plan(int(rows), int(cols), _p(rc), n, _p(level), _p(order), _p(off), C.byref(nl))
    if code != 0:
        raise AuvpError(code, "auvp_sf_plan: a cell outside the %d x %d grid, a cell listed twice, or an empty list" % (rows, cols))
    return dict(level=level[:n], order=order[:n], level_off=off[:nl.value + 1], n_levels=nl.value)


class Context:
    """One planner context = one HIP device + stream + device-resident world and tree storage."""

    def __init__(self, device=0):
        self.L = load()
        self.h = C.c_void_p()
        rc = self.L.auvp_create(int(device), C.byref(self.h))
        if rc != 0:
            raise AuvpError(rc, "auvp_create(device=%d) failed: no usable HIP device (no CPU fallback)" % device)
        self.device = int(device)
        self.n_episodes = 0
        self.max_iter = 0
        self.world_sizes = {}
        self.n_prob_sets = 0
        self.n_replan_auvs = 0
        self._meas_steps = None  # k of the last replan_measure with shark_xy [k,F,2]; None: the [F,2] form
        self._world_stamp = 0  # counts set_world / set_habitats: a user that shares the context sees whether its world still stands
        self.session = None  # the open ReplanSession that owns this context's world, batch and fleet (rrt_dubins.py); None: none

    def _not_in_session(self, what):
        """RuntimeError while a ReplanSession owns the context and the call does not come from the session itself"""
        s = self.session
        if s is not None and not s.inside:
            raise RuntimeError("%s: a replanning session is open on this context (finish() it first)" % what)

    def close(self):
        if getattr(self, "h", None):
            self.L.auvp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise AuvpError(rc, self.L.auvp_last_error(self.h).decode())
        return rc

    # ---- options (include/auvplan.h: auvp_set_option) ----
    def set_option(self, name, value):
        """force a kernel choice / diagnostic switch of this context (`name` without the AUVP_ prefix); None: back to the default"""
        if value is None:
            self._chk(self.L.auvp_unset_option(self.h, name.encode()))
        else:
            self._chk(self.L.auvp_set_option(self.h, name.encode(), int(value)))

    def get_option(self, name):
        """the option's value, None when it is unset (the measured default applies)"""
        s, v = C.c_int32(0), C.c_int64(0)
        self._chk(self.L.auvp_get_option(self.h, name.encode(), C.byref(s), C.byref(v)))
        return int(v.value) if s.value else None

    def pipeline_fallbacks(self):
        """(episodes the last planning call redid on the one-wavefront kernel after AUVP_ERR_PIPELINE, total so far)"""
        a, b = C.c_int32(0), C.c_int64(0)
        self._chk(self.L.auvp_pipeline_fallbacks(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    # ---- world ----
    def set_world(self, obstacles=None, habitats=None, polygon=None, bins=None, cells=None, prob=None):
        ob = _f64(obstacles if obstacles is not None else [], (-1, 3))
        hb = _f64(habitats if habitats is not None else [], (-1, 3))
        pg = _f64(polygon if polygon is not None else [], (-1, 2))
        bn = _f64(bins if bins is not None else [], (-1, 2))
        ce = _f64(cells if cells is not None else [], (-1, 4))
        pr = _f64(prob if prob is not None else [])
        if pr.size != len(bn) * len(ce):
            raise ValueError("prob must be [n_bins, n_cells]")
        self._not_in_session("set_world")
        self._world_stamp += 1
        self._chk(self.L.auvp_world_set(self.h, _p(ob), len(ob), _p(hb), len(hb), _p(pg), len(pg), _p(bn), len(bn),
                                        _p(ce), len(ce), _p(pr)))
        self.world_sizes = dict(O=len(ob), H=len(hb), V=len(pg), T=len(bn), C=len(ce))
        self.n_prob_sets = 0  # (auvp_world_set drops the probability sets)

    def set_habitats(self, habitats):
        hb = _f64(habitats if habitats is not None else [], (-1, 3))
        self._not_in_session("set_habitats")
        self._world_stamp += 1
        self._chk(self.L.auvp_world_set_habitats(self.h, _p(hb), len(hb)))
        self.world_sizes["H"] = len(hb)

    # ---- probability sets: one shark-occupancy table per tracked shark, all over the world's bins and cells ----
    def set_prob_sets(self, prob=None, n_sets=None, prob_dev=None):
        """auvp_world_set_prob_sets: prob [G, T, C] on the host, or prob_dev = a device pointer to n_sets such tables (copied
        device to device); neither: the sets are cleared.  T and C are the world's."""
        T, Cn = self.world_sizes.get("T", 0), self.world_sizes.get("C", 0)
        self._not_in_session("set_prob_sets")
        if prob is None and prob_dev is None:
            self._chk(self.L.auvp_world_set_prob_sets(self.h, 0, None, None))
            self.n_prob_sets = 0
            return
        if prob is not None:
            pr = _f64(prob)
            if pr.ndim != 3 or pr.shape[1:] != (T, Cn):
                raise ValueError("prob must be [n_sets, %d, %d] (the world's bins and cells), not %r" % (T, Cn, pr.shape))
            n_sets = pr.shape[0] if n_sets is None else int(n_sets)
            self._chk(self.L.auvp_world_set_prob_sets(self.h, n_sets, _p(pr), None if prob_dev is None else C.c_void_p(prob_dev)))
        else:
            self._chk(self.L.auvp_world_set_prob_sets(self.h, int(n_sets), None, C.c_void_p(prob_dev)))
        self.n_prob_sets = int(n_sets)

    def set_prob_sets_placed(self, prob_dev, n_sets, n_rounds1, first_bin):
        """auvp_world_set_prob_sets_placed: the sets from a forecast's device copy [n_sets, n_rounds1, C], bin t = forecast round
        min(max(t - first_bin, 0), n_rounds1 - 1) (sf_place_kernel)"""
        self._not_in_session("set_prob_sets_placed")
        self._chk(self.L.auvp_world_set_prob_sets_placed(self.h, C.c_void_p(prob_dev), int(n_sets), int(n_rounds1),
                                                         int(self.world_sizes.get("C", 0)), int(first_bin)))
        self.n_prob_sets = int(n_sets)

    def prob_sets(self):
        """the handle's probability sets [G, T, C] copied back from HBM (auvp_world_prob_sets_read)"""
        out = np.zeros((self.n_prob_sets, self.world_sizes.get("T", 0), self.world_sizes.get("C", 0)))
        self._chk(self.L.auvp_world_prob_sets_read(self.h, None, _p(out)))
        return out

    def prob_set_stats(self, n_sets=None):
        """(absmax [G], one_sign [G]) of the handle's probability sets, as the device computed them"""
        n_sets = self.n_prob_sets if n_sets is None else int(n_sets)
        a, s = np.zeros(max(int(n_sets), 1)), np.zeros(max(int(n_sets), 1), np.int32)
        self._chk(self.L.auvp_world_prob_set_stats(self.h, _p(a), _p(s)))
        return a[:n_sets], s[:n_sets]

    def rrt_set_episode_grids(self, set_of):
        """episode e of the prepared batch ranks its leaves against set set_of[e]; None clears the assignment"""
        self._not_in_session("rrt_set_episode_grids")
        if set_of is None:
            self._chk(self.L.auvp_rrt_set_episode_grids(self.h, 0, None))
            return
        so = _arr(set_of, np.int32, (-1,))
        self._chk(self.L.auvp_rrt_set_episode_grids(self.h, len(so), _p(so)))

    def rrt_rerank(self, summaries=True):
        """the leaf ranking alone on the last run's trees, under the current assignment (auvp_rrt_rerank)"""
        self._chk(self.L.auvp_rrt_rerank(self.h))
        return self.summaries() if summaries else None

    def sf_prob_dev(self):
        """(device pointer, F, R + 1, C) of the last forecast's prob on this context (auvp_sf_prob_dev)"""
        p, f, t, c = C.c_void_p(), C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self.L.auvp_sf_prob_dev(self.h, C.byref(p), C.byref(f), C.byref(t), C.byref(c)))
        return p.value, f.value, t.value, c.value

    def sf_last_kernel(self):
        """name of the kernel the last forecast on this context ran (auvp_sf_last_kernel)"""
        return (self.L.auvp_sf_last_kernel(self.h) or b"").decode()

    # ---- RRT.exploring batch ----
    def rrt_explore_batch(self, init, seeds, n_iter, mode="timebin", freq=30, bin_interval=5, v=2,
                          max_traj_time=500.0, weights=(-3, -3, -4), dist_to_end=2, diff_max=0.5, min_dist=0.5,
                          max_plan_time=None, points_per_iter=0.0, iter_log=False, leaf_log=False, phase_clocks=False,
                          habitat_keep=None, summaries=True, shark_set=None):
        """prepare + run; the summaries, or None with summaries=False (they stay in HBM: rrt_group_best reads them there).
        shark_set [E]: every episode ranks its leaves against its own probability set (set_prob_sets); the batch then takes
        the per-episode-limits route, with every habitat kept and one horizon where the caller gave no limits."""
        self.rrt_prepare(init, seeds, n_iter, mode, freq, bin_interval, v, max_traj_time, weights, dist_to_end,
                         diff_max, min_dist, max_plan_time, points_per_iter, iter_log, leaf_log, phase_clocks, habitat_keep,
                         shark_set)
        self.rrt_run()
        return self.summaries() if summaries else None

    def rrt_run(self):
        """launch the kernel on the prepared batch (inputs already resident in HBM); repeatable"""
        self._chk(self.L.auvp_rrt_run(self.h))

    def rrt_prepare(self, init, seeds, n_iter, mode="timebin", freq=30, bin_interval=5, v=2,
                    max_traj_time=500.0, weights=(-3, -3, -4), dist_to_end=2, diff_max=0.5, min_dist=0.5,
                    max_plan_time=None, points_per_iter=0.0, iter_log=False, leaf_log=False, phase_clocks=False,
                    habitat_keep=None, shark_set=None):
        """max_traj_time [E] and / or habitat_keep [E] (bit masks over the world's habitat table): every episode plans with its
        own horizon and habitat list (auvp_rrt_prepare_episodes; the cap is the largest horizon).  Without both: one horizon.
        shark_set [E]: the episode's probability set (rrt_set_episode_grids, on the per-episode-limits route)."""
        self._not_in_session("rrt_prepare")
        init = _f64(init, (-1, 6))
        E = len(init)
        lim = None
        if habitat_keep is not None or np.ndim(max_traj_time) > 0 or shark_set is not None:
            max_traj_time, lim = episode_limits(E, max_traj_time, habitat_keep, self.world_sizes.get("H", 0), mode, iter_log,
                                                phase_clocks)
        states = None
        if isinstance(seeds, tuple):  # (mt [E,624] uint32, index [E]) as random.getstate() reports
            states = _arr(seeds[0], np.uint32, (E, 624))
            sidx = _arr(seeds[1], np.int32, (E,))
        else:
            seeds = _arr(seeds, np.uint64, (E,))
        p = RRTParams()
        p.dist_to_end, p.diff_max, p.freq, p.min_dist = float(dist_to_end), float(diff_max), float(freq), float(min_dist)
        p.bin_interval, p.v, p.max_traj_time = float(bin_interval), float(v), float(max_traj_time)
        p.max_plan_time = float(n_iter if max_plan_time is None else max_plan_time)
        for i in range(3):
            p.w[i] = float(weights[i])
        p.mode, p.max_iter, p.points_per_iter = MODES[mode], int(n_iter), float(points_per_iter)
        flags = (FLAG_ITER_LOG if iter_log else 0) | (FLAG_LEAF_LOG if leaf_log else 0) | (FLAG_PHASE_CLOCKS if phase_clocks else 0)
        if lim is not None:
            self._chk(self.L.auvp_rrt_prepare_episodes(
                self.h, E, _p(init), None if states is not None else _p(seeds), _p(states) if states is not None else None,
                _p(sidx) if states is not None else None, C.byref(p), _p(lim), flags))
        elif states is not None:
            self._chk(self.L.auvp_rrt_prepare_states(self.h, E, _p(init), _p(states), _p(sidx), C.byref(p), flags))
        else:
            self._chk(self.L.auvp_rrt_prepare(self.h, E, _p(init), _p(seeds), C.byref(p), flags))
        self.n_episodes, self.max_iter = E, int(n_iter)
        if shark_set is not None:
            self.rrt_set_episode_grids(shark_set)

    def summaries(self):
        out = np.zeros(self.n_episodes, dtype=SUMMARY_DTYPE)
        self._chk(self.L.auvp_rrt_summaries(self.h, _p(out)))
        return out

    def paths(self, summaries):
        """final course (root -> leaf) of every episode: list of [L,7] arrays"""
        lens = np.where(summaries["best_leaf"] >= 0, summaries["best_path_len"], 0).astype(np.int64)
        off = np.zeros(self.n_episodes + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        out = np.zeros((max(int(off[-1]), 1), 7))
        self._chk(self.L.auvp_rrt_paths(self.h, _p(off), _p(out)))
        return [out[off[e]:off[e + 1]] for e in range(self.n_episodes)]

    def paths_dev(self, offsets, out_dev_ptr):
        """final courses written to a caller-owned device buffer [offsets[E],7] f64 (e.g. a torch tensor's
        data_ptr()) -- stays in HBM for the multi-GPU gather"""
        off = _arr(offsets, np.int64)
        self._chk(self.L.auvp_rrt_paths_dev(self.h, _p(off), C.c_void_p(out_dev_ptr)))

    # ---- best-of-K: the winner of every group of episodes, chosen on the device ----
    def rrt_group_best(self, group_off):
        """winner of every group of the batch that just ran (auvp_rrt_group_best): group g = episodes group_off[g] ..
        group_off[g+1]-1, the groups partition the batch.  Returns [G] GROUP_BEST_DTYPE records: status (0, NO_QUALIFYING_LEAF,
        or the status < 0 of the lowest-indexed failed member), winner (episode index or -1), n_with_leaf, and the winner's
        path_len, cost [4], length."""
        off = _arr(group_off, np.int32, (-1,))
        G = len(off) - 1
        out = np.zeros(max(G, 1), dtype=GROUP_BEST_DTYPE)
        self._chk(self.L.auvp_rrt_group_best(self.h, G, _p(off), _p(out)))
        return out[:G]

    def group_best_dev(self):
        """device pointer of the last rrt_group_best call's records (None: none since the batch ran)"""
        return self.L.auvp_rrt_group_best_dev(self.h)

    @staticmethod
    def group_offsets(best):
        """[G+1] row offsets of the winners' courses: the exclusive prefix sum of path_len (0 without a winner)"""
        lens = np.where(best["winner"] >= 0, best["path_len"], 0).astype(np.int64)
        off = np.zeros(len(best) + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        return off

    def group_paths(self, best):
        """final course (root -> leaf) of every group's winner: list of [L,7] arrays, empty where there is none.  Only these
        rows are copied to the host."""
        off = self.group_offsets(best)
        out = np.zeros((max(int(off[-1]), 1), 7))
        self._chk(self.L.auvp_rrt_group_paths(self.h, _p(off), _p(out)))
        return [out[off[g]:off[g + 1]] for g in range(len(best))]

    def group_paths_dev(self, offsets, out_dev_ptr):
        """the winners' courses written to a caller-owned device buffer [offsets[G],7] f64"""
        off = _arr(offsets, np.int64)
        self._chk(self.L.auvp_rrt_group_paths_dev(self.h, _p(off), C.c_void_p(out_dev_ptr)))

    # ---- replanning a fleet with the commit step on the device (include/auvplan.h: auvp_replan_*) ----
    def replan_begin(self, start7, keep0):
        """a fleet's state on the handle: start7 [N,7] (x, y, theta, v, traj_time_stamp, plan_time_stamp, length), keep0 one
        habitat bit mask or [N]; an empty trajectory log"""
        self._not_in_session("replan_begin")
        s = _f64(start7, (-1, 7))
        k = _arr(keep0, np.uint64, (-1,))
        if len(k) not in (1, len(s)):
            raise ValueError("keep0 must be one mask or one per AUV")
        self._chk(self.L.auvp_replan_begin(self.h, len(s), _p(s), _p(k), 1 if len(k) == 1 and len(s) != 1 else 0))
        self.n_replan_auvs = len(s)

    def replan_set_teams(self, team_of):
        """the fleet's teams: team_of [N] int labels (equal labels >= 0: one team, < 0: on its own) or None to clear them.  From
        then on every replan_commit ends with replan_team_kernel: each member's keep, in the state and in the round's records,
        is the AND of its team's masks."""
        if team_of is None:
            self._chk(self.L.auvp_replan_set_teams(self.h, self.n_replan_auvs, None))
            return
        t = _arr(team_of, np.int32, (-1,))
        self._chk(self.L.auvp_replan_set_teams(self.h, len(t), _p(t)))

    def replan_team_fold(self, team_of, keep):
        """probe: replan_team_kernel on the caller's labels [n] and keep masks [n], one launch; returns the folded masks [n]
        (uint64).  Needs no world and no fleet, and touches neither."""
        t = _arr(team_of, np.int32, (-1,))
        kp = np.array(keep, dtype=np.uint64).reshape(-1)
        if len(kp) != len(t):
            raise ValueError("team_of has %d entries, keep %d" % (len(t), len(kp)))
        self._chk(self.L.auvp_replan_team_fold(self.h, len(t), _p(t), _p(kp)))
        return kp

    def replan_team_pick(self, auv_of, K):
        """the team-aware winner selection in place of rrt_group_best (auvp_replan_team_pick): group g of the batch that just
        ran = episodes g*K .. g*K+K-1 = AUV auv_of[g].  Returns [n_active] GROUP_BEST_DTYPE records: rrt_group_best's for AUVs
        without a teammate, the winner under the teammates' claims and its score for the members of teams."""
        a = _arr(auv_of, np.int32, (-1,))
        out = np.zeros(max(len(a), 1), dtype=GROUP_BEST_DTYPE)
        self._chk(self.L.auvp_replan_team_pick(self.h, len(a), _p(a), int(K), _p(out)))
        return out[:len(a)]

    def replan_team_pick_apart(self, auv_of, K, use_claims, d, tick, W):
        """the winner selection that keeps teammates' courses apart, in place of rrt_group_best / replan_team_pick
        (auvp_replan_team_pick_apart): d metres, tick seconds, W ticks per course; use_claims: the scores under the teammates'
        claims, as replan_team_pick's.  Returns [n_active] GROUP_BEST_DTYPE records; the conflict counts come back in the
        records of the replan_commit behind it."""
        a = _arr(auv_of, np.int32, (-1,))
        out = np.zeros(max(len(a), 1), dtype=GROUP_BEST_DTYPE)
        self._chk(self.L.auvp_replan_team_pick_apart(self.h, len(a), _p(a), int(K), 1 if use_claims else 0, float(d), float(tick), int(W),
                                                     _p(out)))
        return out[:len(a)]

    def replan_team_pick_apart_courses(self, team_of, keep, auv_of, K, courses_xyt, cost4, leaf_t, length, bin_lo, bin_hi, weights,
                                       use_claims, d, tick, W):
        """probe: replan_team_pick_courses with rrt_course_ticks_kernel and replan_team_pick_apart_kernel on the caller's
        candidates.  Returns (records [n_active], claimed [n_active], conflicts [n_active])."""
        return self.replan_team_pick_courses(team_of, keep, auv_of, K, courses_xyt, cost4, leaf_t, length, bin_lo, bin_hi, weights,
                                             apart=(1 if use_claims else 0, float(d), float(tick), int(W)))

    def replan_team_pick_courses(self, team_of, keep, auv_of, K, courses_xyt, cost4, leaf_t, length, bin_lo, bin_hi, weights, apart=None):
        """probe: rrt_group_best_kernel, rrt_course_words_kernel and replan_team_pick_kernel on the caller's candidates against
        the world's habitat table and time bins.  courses_xyt: n_active * K arrays [L,3] (L == 0: a tree without a leaf), in
        group order; cost4 [E,4], leaf_t [E], length [E], bin_lo / bin_hi [E].  Returns (records [n_active], claimed [n_active]).
        apart: replan_team_pick_apart_courses' arguments."""
        t = _arr(team_of, np.int32, (-1,))
        kp = np.array(keep, dtype=np.uint64).reshape(-1)
        a = _arr(auv_of, np.int32, (-1,))
        E = len(a) * int(K)
        if len(kp) != len(t) or len(courses_xyt) != E:
            raise ValueError("team_of / keep, or auv_of x K / courses, do not match")
        off = np.zeros(E + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(c) for c in courses_xyt])
        flat = _f64(np.concatenate([_f64(c, (-1, 3)) for c in courses_xyt]) if E else [], (-1, 3))
        if len(flat) == 0:
            flat = np.zeros((1, 3))
        c4, lt, ln = _f64(cost4, (E, 4)), _f64(leaf_t, (E,)), _f64(length, (E,))
        lo = _arr(bin_lo, np.int32, (E,))
        hi = _arr(bin_hi, np.int32, (E,))
        w = _f64(weights, (3,))
        out = np.zeros(max(len(a), 1), dtype=GROUP_BEST_DTYPE)
        claimed = np.zeros(max(len(a), 1), dtype=np.uint64)
        cand = (len(t), _p(t), _p(kp), len(a), _p(a), int(K), _p(off), _p(flat), _p(c4), _p(lt), _p(ln), _p(lo), _p(hi), _p(w))
        if apart is not None:
            conflicts = np.zeros(max(len(a), 1), dtype=np.int32)
            self._chk(self.L.auvp_replan_team_pick_apart_courses(self.h, *cand, *apart, _p(out), _p(claimed), _p(conflicts)))
            return out[:len(a)], claimed[:len(a)], conflicts[:len(a)]
        self._chk(self.L.auvp_replan_team_pick_courses(self.h, *cand, _p(out), _p(claimed)))
        return out[:len(a)], claimed[:len(a)]

    def replan_commit(self, auv_of, round_span, records=True):
        """one round behind rrt_group_best: group g is AUV auv_of[g]; the winners' first buckets go into the log, the states
        are updated in HBM.  Returns [n_active] REPLAN_RECORD_DTYPE records (None with records=False)."""
        a = _arr(auv_of, np.int32, (-1,))
        out = np.zeros(max(len(a), 1), dtype=REPLAN_RECORD_DTYPE) if records else None
        self._chk(self.L.auvp_replan_commit(self.h, len(a), _p(a), float(round_span), _p(out) if records else None))
        return out[:len(a)] if records else None

    def replan_measure(self, shark_of, n_per_shark, shark_xy):
        """auvp_replan_measure: the fleet's measurements [F, A, 5] of the sharks at shark_xy [F,2] from its committed states,
        left in HBM.  Returns the table's device pointer (valid until the next call or replan_begin).
        shark_xy [k,F,2], 1 <= k <= 64: k measurements per AUV along the bucket it committed last, [k, F, A, 5]
        (replan_measure_ticks_kernel; csrc/replan_ticks.h, tracking.fleet_measurements_ticks) -- option MEAS_TICKS = k for this
        call; it is back at what it was, set or unset, when the call returns or raises."""
        so = _arr(shark_of, np.int32, (-1,))
        if len(so) != self.n_replan_auvs:
            raise ValueError("shark_of has %d entries, the fleet %d AUVs" % (len(so), self.n_replan_auvs))
        A = int(n_per_shark)
        if A < 1 or len(so) % A:
            raise ValueError("%d AUVs are no multiple of %d AUVs per shark" % (len(so), A))
        F = len(so) // A
        if so.min() < 0 or so.max() >= F or np.any(np.bincount(so, minlength=F) != A):
            raise ValueError("every shark 0 .. %d must be tracked by exactly %d AUVs" % (F - 1, A))
        ptr = C.c_void_p()
        if np.ndim(shark_xy) == 3:
            k = np.shape(shark_xy)[0]
            if not 1 <= k <= MEAS_MAX_TICKS:
                raise ValueError("shark_xy [k,F,2] needs 1 <= k <= %d, not %d" % (MEAS_MAX_TICKS, k))
            if tuple(np.shape(shark_xy)[1:]) != (F, 2):
                raise ValueError("shark_xy must be [k,%d,2], not %r" % (F, tuple(np.shape(shark_xy))))
            xy = _f64(shark_xy, (k, F, 2))
            before = self.get_option("MEAS_TICKS")
            self.set_option("MEAS_TICKS", k)
            try:
                self._chk(self.L.auvp_replan_measure(self.h, _p(so), A, _p(xy), C.byref(ptr)))
            finally:
                self.set_option("MEAS_TICKS", before)
            self._meas_steps = k
            return ptr.value
        xy = _f64(shark_xy, (F, 2))
        k = self.get_option("MEAS_TICKS")  # (set by the caller: the library reads k x F positions)
        if k is not None:
            raise ValueError("option MEAS_TICKS = %d is set: pass shark_xy as [k,F,2]" % k)
        self._chk(self.L.auvp_replan_measure(self.h, _p(so), A, _p(xy), C.byref(ptr)))
        self._meas_steps = None
        return ptr.value

    def replan_meas(self):
        """the last replan_measure's table on the host (auvp_replan_meas): [F, A, 5], or [k, F, A, 5] where shark_xy was
        [k,F,2]"""
        f, a = C.c_int32(0), C.c_int32(0)
        self._chk(self.L.auvp_replan_meas(self.h, C.byref(f), C.byref(a), None))
        k = self._meas_steps
        out = np.zeros((f.value, a.value, 5) if k is None else (k, f.value, a.value, 5))
        self._chk(self.L.auvp_replan_meas(self.h, None, None, _p(out)))
        return out

    def replan_traj(self):
        """(row_off [N+1], rows [row_off[N],7]): every AUV's committed trajectory in round order -- the one bulk download"""
        off = np.zeros(self.n_replan_auvs + 1, dtype=np.int64)
        self._chk(self.L.auvp_replan_traj(self.h, _p(off), None))
        rows = np.zeros((int(off[-1]), 7))
        if len(rows):
            self._chk(self.L.auvp_replan_traj(self.h, _p(off), _p(rows)))
        return off, rows

    def replan_commit_courses(self, courses, last7, keep, round_span):
        """probe: rrt_commit_kernel's rule on the caller's courses (a list of [L,7] arrays, L == 0: a state without a winner)
        and states, against the world's habitat table, one launch.  Returns (records [n], committed rows per state, new
        last [n,7], new keep [n])."""
        n = len(courses)
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(c) for c in courses])
        flat = _f64(np.concatenate([_f64(c, (-1, 7)) for c in courses]) if n else [], (-1, 7))
        last = _f64(last7, (n, 7)).copy()
        kp = np.array(keep, dtype=np.uint64).reshape(n)
        out = np.zeros(max(n, 1), dtype=REPLAN_RECORD_DTYPE)
        rows = np.zeros((max(len(flat), 1), 7))
        self._chk(self.L.auvp_replan_commit_courses(self.h, n, _p(off), _p(flat), _p(last), _p(kp), float(round_span), _p(out),
                                                    _p(rows)))
        return out[:n], [rows[off[i]:off[i] + out[i]["n_committed"]] for i in range(n)], last, kp

    def replan_info(self):
        """counters since replan_begin: n_auvs, rounds, rows, bytes_to_host (what the replan entry points copied to the host),
        bytes_traj (replan_traj's part of it), commit_ms (rrt_commit_kernel's time, with teams replan_team_kernel's too, with replan_team_pick
        rrt_course_words_kernel's and replan_team_pick_kernel's, and with replan_team_pick_apart its kernels', summed)"""
        a, r = C.c_int32(0), C.c_int32(0)
        rows, b, bt, ms = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_double(0.0)
        self._chk(self.L.auvp_replan_info(self.h, C.byref(a), C.byref(r), C.byref(rows), C.byref(b), C.byref(bt), C.byref(ms)))
        return dict(n_auvs=a.value, rounds=r.value, rows=rows.value, bytes_to_host=b.value, bytes_traj=bt.value, commit_ms=ms.value)

    def tree(self, ep, summary):
        n, npnt = int(summary["n_nodes"]), int(summary["n_points"])
        nodes = np.zeros((n, 6))
        parent = np.zeros(n, np.int32)
        pt_off = np.zeros(n, np.int32)
        pt_cnt = np.zeros(n, np.int32)
        points = np.zeros((max(npnt, 1), 7))
        self._chk(self.L.auvp_rrt_tree(self.h, ep, _p(nodes), _p(parent), _p(pt_off), _p(pt_cnt), _p(points)))
        return dict(nodes=nodes, parent=parent, pt_off=pt_off, pt_cnt=pt_cnt, points=points[:npnt])

    def iter_log(self, ep):
        n = self.max_iter
        a, b, c = np.zeros(n, np.int32), np.zeros(n, np.int8), np.zeros(n, np.int32)
        self._chk(self.L.auvp_rrt_iter_log(self.h, ep, _p(a), _p(b), _p(c)))
        return dict(it_parent=a, it_accepted=b, it_npath=c)

    def leaf_log(self, ep, summary):
        n = int(summary["n_leaves"])
        lc, li = np.zeros((max(n, 1), 6)), np.zeros(max(n, 1), np.int32)
        self._chk(self.L.auvp_rrt_leaf_log(self.h, ep, _p(lc), _p(li)))
        return lc[:n], li[:n]

    def bin_sizes(self, ep):
        k = C.c_int32()
        self._chk(self.L.auvp_rrt_bin_sizes(self.h, ep, None, C.byref(k)))
        s = np.zeros(max(k.value, 1), np.int32)
        self._chk(self.L.auvp_rrt_bin_sizes(self.h, ep, _p(s), C.byref(k)))
        return s[:k.value]

    # ---- probes ----
    def check_collision(self, paths_xy):
        off = np.zeros(len(paths_xy) + 1, np.int32)
        off[1:] = np.cumsum([len(p) for p in paths_xy])
        pts = _f64(np.concatenate([_f64(p, (-1, 2)) for p in paths_xy]) if len(paths_xy) else [], (-1, 2))
        out = np.zeros(len(paths_xy), np.int8)
        self._chk(self.L.auvp_check_collision_batch(self.h, len(paths_xy), _p(off), _p(pts), _p(out)))
        return out.astype(bool)

    def cost_paths(self, paths_xyt, bin_lo, bin_hi, total, weights):
        n = len(paths_xyt)
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum([len(p) for p in paths_xyt])
        pts = _f64(np.concatenate([_f64(p, (-1, 3)) for p in paths_xyt]), (-1, 3))
        lo = _arr(bin_lo, np.int32)
        hi = _arr(bin_hi, np.int32)
        tt = _f64(total)
        w = _f64(weights, (n, 3))
        out = np.zeros((n, 4))
        self._chk(self.L.auvp_cost_paths(self.h, n, _p(off), _p(pts), _p(lo), _p(hi), _p(tt), _p(w), _p(out)))
        return out

    def nn_closest(self, xy, queries, force_exact=False):
        """get_closest_mps (rrt_dubins.py:505-513) of every query point against the node list xy -> (index, slow-path flag)"""
        xy, q = _f64(xy, (-1, 2)), _f64(queries, (-1, 2))
        idx, slow = np.zeros(len(q), np.int32), np.zeros(len(q), np.int32)
        self._chk(self.L.auvp_nn_closest_batch(self.h, len(xy), _p(xy), len(q), _p(q), 1 if force_exact else 0, _p(idx), _p(slow)))
        return idx, slow.astype(bool)

    def sincos(self, x):
        x = _f64(x).ravel()
        s, c = np.zeros_like(x), np.zeros_like(x)
        self._chk(self.L.auvp_sincos_dev(self.h, len(x), _p(x), _p(s), _p(c)))
        return s, c

    MATH_OPS = {"sincos": 0, "atan2": 1, "pow_e": 2, "div_plain": 3, "sqrt_plain": 4, "hypot": 5, "div": 6, "sqrt": 7,
                "sincos_sk": 8, "atan2_late": 9, "pow_e_lds": 10, "bearing": 11, "atan": 12}

    def math(self, op, a, b=None):
        """auvp_math_dev: one portable elementary function on the device (bit-exactness probe)"""
        a = _f64(a).ravel()
        b = np.zeros_like(a) if b is None else _f64(b).ravel()
        o0, o1 = np.zeros_like(a), np.zeros_like(a)
        self._chk(self.L.auvp_math_dev(self.h, self.MATH_OPS[op], len(a), _p(a), _p(b), _p(o0), _p(o1)))
        return (o0, o1) if op in ("sincos", "sincos_sk") else o0

    def theta_chain(self, theta0, phi):
        """auvp_theta_chain_dev: rows_theta_chain_dpp on its own.  theta0 [W, 4] (one per 16-lane row), phi [W, 64] (one per lane)
        -> [W, 64], lane rl of a row: (((theta0 + phi_0) + phi_1) + ... + phi_rl) of its row (lane 15: lane 14's sum)"""
        theta0, phi = _f64(theta0, (-1, 4)), _f64(phi, (-1, 64))
        assert len(theta0) == len(phi)
        out = np.zeros_like(phi)
        self._chk(self.L.auvp_theta_chain_dev(self.h, len(phi), _p(theta0), _p(phi), _p(out)))
        return out

    def row_ends(self, n, on, start, incs):
        """auvp_row_ends_dev: the end of a steer pass of the four-episode RRT kernels on its own.  n [W, 4] sub-arcs per row (1 .. 15),
        on [W, 4] (0 / 1), start [W, 4, 5] the rows' x, y, t, length, theta, incs [W, 5, 64] every lane's addends -> [W, 5, 64]: the
        row's x, y, t, length, theta after the pass, as each lane of the row holds them"""
        start, incs = _f64(start, (-1, 4, 5)), _f64(incs, (-1, 5, 64))
        head = np.concatenate([_f64(n, (-1, 4, 1)), _f64(on, (-1, 4, 1)), start], axis=2)
        assert len(head) == len(incs)
        head = np.ascontiguousarray(head)
        out = np.zeros_like(incs)
        self._chk(self.L.auvp_row_ends_dev(self.h, len(incs), _p(head), _p(incs), _p(out)))
        return out

    def random_stream(self, seed, n):
        out = np.zeros(n)
        self._chk(self.L.auvp_random_stream_dev(self.h, int(seed), n, _p(out)))
        return out

    def phase_clocks(self):
        out = np.zeros((self.n_episodes, 5), dtype=np.uint64)
        self._chk(self.L.auvp_rrt_phase_clocks(self.h, _p(out)))
        return out

    def prrt_last_kernel(self):
        """name of the kernel the last Planner_RRT launch ran (prrt_kernel: one episode per wavefront; prrt_rows_kernel: four)"""
        return (self.L.auvp_prrt_last_kernel(self.h) or b"").decode()

    def last_kernel_ms(self):
        return float(self.L.auvp_last_kernel_ms(self.h))

    def last_launch_parts(self):
        """(expansion ms, leaf-pass ms, episodes per wavefront) of the last rrt_run"""
        a, b, k = C.c_double(), C.c_double(), C.c_int32()
        self._chk(self.L.auvp_rrt_last_launch_parts(self.h, C.byref(a), C.byref(b), C.byref(k)))
        return a.value, b.value, k.value

    def last_stream_ms(self):
        """ms of the launch that generated the random numbers ahead of the last rrt_run's expansion kernel (0: it did not)"""
        return float(self.L.auvp_rrt_last_stream_ms(self.h))

    def last_stream_mirror(self):
        """the LDS ring of the last rrt_run's rrt_rows_stream_kernel: 1 its first entries mirrored behind it, 0 every read masked
        (-1: another expansion kernel ran)"""
        return int(self.L.auvp_rrt_last_stream_mirror(self.h))

    def last_stream_len(self):
        """random() numbers per episode that launch wrote (0: none)"""
        return int(self.L.auvp_rrt_last_stream_len(self.h))

    def last_rrt_kernel(self):
        """name of the expansion kernel the last rrt_run launched (rrt_rows_kernel / rrt_explore_kernel / rrt_duo_kernel /
        rrt_explore_lim_kernel)"""
        return (self.L.auvp_rrt_last_kernel(self.h) or b"").decode()

    def last_leaf_stats(self):
        """of the last rrt_run's leaf pass, summed over the batch: nodes visited, their path points, path elements re-summed
        in the reference's order, leaves re-summed"""
        out = (C.c_int64 * 4)()
        self._chk(self.L.auvp_rrt_last_leaf_stats(self.h, out))
        return dict(zip(("nodes_visited", "points_visited", "elements_resummed", "leaves_resummed"), (int(v) for v in out)))

    def hbm_probe(self, n_bytes=4 << 30, reps=3):
        """measured HBM streaming rates of this GPU in GB/s: (read, copy [read + written bytes])"""
        r, c = C.c_double(), C.c_double()
        self._chk(self.L.auvp_hbm_probe(self.h, int(n_bytes), int(reps), C.byref(r), C.byref(c)))
        return r.value, c.value

    def last_launch(self):
        g, b, l = C.c_int32(), C.c_int32(), C.c_int32()
        self.L.auvp_last_launch(self.h, C.byref(g), C.byref(b), C.byref(l))
        return g.value, b.value, l.value

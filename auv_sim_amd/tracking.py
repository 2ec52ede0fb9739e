"""Shark tracking with one path replan per particle hypothesis (BASELINE.json configs[4]).

The reference chains these by hand in robotSim.py:665-701: every tracking step the particle filter
(particleFilter.py:283-317) moves and re-weights its particles from the AUVs' range/bearing measurements, and a
planner is asked for a path towards the shark estimate.  Config 5 scales that out: EVERY particle (a hypothesis of
where the shark is) becomes the goal of its own Planner_RRT episode (gym_rrt/envs/rrt_dubins.py:162-248), F filters x
N particles per GPU.  Both stages stay on the device: the particle state the filter kernel leaves in HBM is what
the planner batch reads its goals from (auvp_prrt_replan_particles); nothing but the per-step measurements goes in
and nothing but the result records comes out.
"""
import math

import numpy as np

from . import _pf_lib
from ._prrt_lib import PlannerBatch


def range_bearing_measurements(tracks, auv_offsets, auv_theta=0.0):
    """Noise-free sensor model over recorded tracks: AUV a of filter f sits at tracks[f, 0] + auv_offsets[a]
    (x, y, theta fixed) and measures range and bearing to the shark at every sample.
    tracks [F, S, 2] -> meas [S, F, A, 5] = auv x, auv y, auv theta, range, bearing (the Z_shark the reference's
    update_weights reads, particleFilter.py:283-301) and shark_xy [S, F, 2]."""
    tracks = np.asarray(tracks, dtype=np.float64)
    F, S, _ = tracks.shape
    off = np.asarray(auv_offsets, dtype=np.float64).reshape(-1, 2)
    A = len(off)
    meas = np.zeros((S, F, A, 5))
    auv = tracks[:, 0, None, :] + off[None, :, :]          # [F, A, 2]
    d = tracks.transpose(1, 0, 2)[:, :, None, :] - auv[None]  # [S, F, A, 2]
    meas[..., 0:2] = auv[None]
    meas[..., 2] = auv_theta
    meas[..., 3] = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)
    meas[..., 4] = np.arctan2(d[..., 1], d[..., 0]) - auv_theta
    return meas, np.ascontiguousarray(tracks.transpose(1, 0, 2))


def goal_transforms(tracks, rect, margin=20.0):
    """per filter: map the bounding box of its track (grown by 10 %) into the planner rectangle inset by `margin`,
    same scale on both axes.  Returns xform [F, 4] = sx, ox, sy, oy and the clamp rectangle."""
    tracks = np.asarray(tracks, dtype=np.float64)
    lo, hi = tracks.min(axis=1), tracks.max(axis=1)
    span = np.maximum((hi - lo).max(axis=1) * 1.1, 1.0)
    room = min(rect[2] - rect[0], rect[3] - rect[1]) - 2.0 * margin
    s = room / span
    mid = 0.5 * (lo + hi)
    cx, cy = 0.5 * (rect[0] + rect[2]), 0.5 * (rect[1] + rect[3])
    xform = np.stack([s, cx - mid[:, 0] * s, s, cy - mid[:, 1] * s], axis=1)
    clamp = np.array([rect[0] + 5.0, rect[1] + 5.0, rect[2] - 5.0, rect[3] - 5.0])
    return np.ascontiguousarray(xform), clamp


class ParticleReplanner:
    """F filters x N particles on one GPU; step(s) = one tracking step (filter update from the measurements of sample
    s) followed by one Planner_RRT.planning(max_step) per particle towards that particle.

    ctx          auv_sim_amd._lib.Context whose world holds the obstacle list of the planning workspace
    tracks       [F, S, 2] recorded shark positions, one track per filter
    filter_seeds [F] np.random.seed values of the filters (numpy legacy stream, as particleFilter.py draws)
    episode_seed_base  episode e of tracking step s plans with random.seed(episode_seed_base + s * F * N + e)
    """

    def __init__(self, ctx, tracks, n_particles, rect, start, filter_seeds, auv_offsets=((60.0, -40.0), (-50.0, 70.0)),
                 max_step=200, freq=10, cell=5, subs=1, episode_seed_base=0, episode_offset=0, episodes_total=None):
        self.ctx = ctx
        self.tracks = np.asarray(tracks, dtype=np.float64)
        self.F, self.S_total = self.tracks.shape[0], self.tracks.shape[1]
        self.N = int(n_particles)
        self.E = self.F * self.N
        self.rect, self.start = tuple(float(v) for v in rect), tuple(float(v) for v in start)
        self.kw = dict(max_step=int(max_step), freq=freq, cell=cell, subs=subs)
        self.meas, self.shark = range_bearing_measurements(self.tracks, auv_offsets)
        self.xform, self.clamp = goal_transforms(self.tracks, self.rect)
        self.seed_base = int(episode_seed_base)
        self.episode_offset = int(episode_offset)                 # this rank's first global episode id
        self.episodes_total = int(episodes_total or self.E)       # over all ranks: seeds do not depend on the sharding
        mts = np.stack([_pf_lib.np_seed_state(int(s))[0] for s in filter_seeds])
        self.filters = _pf_lib.FilterBatch(ctx, self.F, self.N).create(self.tracks[:, 0, :], mts, 624)
        self.pf_ms = self.replan_ms = self.plan_ms = 0.0
        self.planner = None

    def episode_seed(self, s, e_local=0):
        return self.seed_base + s * self.episodes_total + self.episode_offset + e_local

    def step(self, s):
        """tracking step s: filter update -> goals from particles -> plan.  Returns the planner summaries [E]."""
        self.filters.run(meas=self.meas[s:s + 1], shark_xy=self.shark[s:s + 1])
        self.pf_ms = self.ctx.last_kernel_ms()
        self.planner = PlannerBatch.from_particles(self.ctx, self.E, list(self.start) + [0.0, 0.0], self.rect,
                                                   self.kw["max_step"], self.xform, self.clamp, self.episode_seed(s),
                                                   freq=self.kw["freq"], cell=self.kw["cell"], subs=self.kw["subs"])
        self.replan_ms = self.ctx.last_kernel_ms()
        summ = self.planner.plan()
        self.plan_ms = self.ctx.last_kernel_ms()
        return summ


# ---- closed-loop fleet tracking: measure -> filter -> forecast -> plan, every round, on the device -------------------------------

def shark_members(shark_of, n_sharks=None):
    """members [F, A]: row f lists the AUVs with shark_of == f in ascending AUV index.  Every shark 0 .. F-1 must be tracked by
    the same number A >= 1 of AUVs (F = n_sharks, or the largest label + 1); ValueError otherwise, for a label that is no
    integer or lies outside [0, F).  csrc/replan_measure.h: replan_measure_members."""
    so = list(shark_of)
    for i, g in enumerate(so):
        if isinstance(g, (bool, np.bool_)) or int(g) != g:
            raise ValueError("shark_of[%d] = %r is not an integer" % (i, g))
    so = [int(g) for g in so]
    if not so:
        raise ValueError("shark_of is empty")
    F = max(so) + 1 if n_sharks is None else int(n_sharks)
    if F < 1 or min(so) < 0 or max(so) >= F:
        raise ValueError("shark_of must lie in [0, %d)" % F)
    rows = [[] for _ in range(F)]
    for i, g in enumerate(so):  # (ascending AUV index within every shark)
        rows[g].append(i)
    A = len(rows[0])
    if A < 1 or any(len(r) != A for r in rows):
        raise ValueError("every shark must be tracked by the same number of AUVs, not %r" % ([len(r) for r in rows],))
    return np.array(rows, dtype=np.int32).reshape(F, A)


def fleet_measurements(last7, shark_of, shark_xy):
    """The range / bearing measurements of a fleet from its committed states -- the definition replan_measure_kernel is held
    to.  last7 [N,7] (x, y, theta, ...), shark_of [N], shark_xy [F,2] the sharks' true positions.  Returns meas [1, F, A, 5]
    (one step of `FilterBatch.run`): row (f, a) is the a-th AUV, in ascending index, of those tracking shark f --
    x, y, theta, range = math.sqrt(dx*dx + dy*dy), bearing = math.atan2(dy, dx) - theta with dx = shark_x - x, dy = shark_y - y.
    ValueError unless every shark is tracked by the same number of AUVs (shark_members)."""
    last = np.asarray(last7, dtype=np.float64).reshape(-1, 7)
    xy = np.asarray(shark_xy, dtype=np.float64).reshape(-1, 2)
    if len(list(shark_of)) != len(last):
        raise ValueError("shark_of has %d entries, last7 %d rows" % (len(list(shark_of)), len(last)))
    mem = shark_members(shark_of, len(xy))
    F, A = mem.shape
    meas = np.zeros((1, F, A, 5))
    for f in range(F):
        sx, sy = float(xy[f, 0]), float(xy[f, 1])
        for a in range(A):
            x, y, theta = (float(v) for v in last[mem[f, a], :3])
            dx, dy = sx - x, sy - y
            meas[0, f, a] = (x, y, theta, math.sqrt(dx * dx + dy * dy), math.atan2(dy, dx) - theta)
    return meas


MEAS_MAX_TICKS = 64  # filter steps (ticks) per round: csrc/replan_ticks.h, REPLAN_MEAS_MAX_TICKS


def tick_times(lo, round_span, k):
    """the k tick times of the bucket that starts at lo: lo + (j + 1) * (round_span / k) for j < k - 1, and lo + 1.0 * round_span
    -- the bucket's hi (first_bucket_commit) -- for the last, however k * (round_span / k) rounds.  Every operation rounded on
    its own, as csrc/replan_ticks.h has them."""
    lo, span = float(lo), float(round_span)
    step = span / float(k)
    return [lo + float(j + 1) * step for j in range(k - 1)] + [lo + 1.0 * span]


def tick_row(times, tau):
    """the greatest index i with times[i] <= tau (a NaN never qualifies), 0 where there is none: where an AUV that committed
    rows at `times` is when the clock shows tau -- at the last point it reached, nothing interpolated (replanning.course_ticks).
    A linear scan: the times need not ascend."""
    best = 0
    for i, t in enumerate(times):
        if float(t) <= tau:
            best = i
    return best


def fleet_measurements_ticks(segments, last7, shark_of, shark_xy_k, round_span):
    """k measurements per AUV along the bucket it committed last -- the definition replan_measure_ticks_kernel is held to
    (csrc/replan_ticks.h).  segments[i]: the [n,7] rows AUV i committed in the most recent round, row 0 the state it had before
    (so its time is the bucket's lo), or an empty array: every tick from last7[i] (an AUV that stopped planning or found no
    winner, a fleet before its first round).  last7 [N,7], shark_of [N], shark_xy_k [k,F,2] the sharks' true positions at the
    ticks, 1 <= k <= 64; round_span: of that round (read only where a segment has rows).  Tick j of AUV i: the row
    tick_row(segments[i][:, 4], tick_times(segments[i][0, 4], round_span, k)[j]).  Returns meas [k, F, A, 5], row (j, f, a) as
    fleet_measurements writes it from that row's x, y, theta against shark_xy_k[j, f].  With k = 1 and no segments it is
    fleet_measurements.  ValueError for a bad k, bad shapes, and unless every shark is tracked by the same number of AUVs."""
    last = np.asarray(last7, dtype=np.float64)
    xy = np.asarray(shark_xy_k, dtype=np.float64)
    if last.ndim != 2 or last.shape[1] != 7:
        raise ValueError("last7 must be [N,7]")
    if xy.ndim != 3 or xy.shape[2] != 2:
        raise ValueError("shark_xy_k must be [k,F,2]")
    k = xy.shape[0]
    if not 1 <= k <= MEAS_MAX_TICKS:
        raise ValueError("need 1 <= k <= %d ticks, not %d" % (MEAS_MAX_TICKS, k))
    N = len(last)
    if len(list(shark_of)) != N or len(segments) != N:
        raise ValueError("shark_of has %d entries, segments %d, last7 %d rows" % (len(list(shark_of)), len(segments), N))
    mem = shark_members(shark_of, xy.shape[1])
    F, A = mem.shape
    segs = []
    for i, s in enumerate(segments):
        s = np.zeros((0, 7)) if s is None else np.asarray(s, dtype=np.float64)
        if s.size and (s.ndim != 2 or s.shape[1] != 7):
            raise ValueError("segments[%d] must be [n,7]" % i)
        segs.append(s.reshape(-1, 7))
    meas = np.zeros((k, F, A, 5))
    for f in range(F):
        for a in range(A):
            i = int(mem[f, a])
            seg = segs[i]
            taus = tick_times(seg[0, 4], round_span, k) if len(seg) else None
            for j in range(k):
                row = seg[tick_row(seg[:, 4], taus[j])] if len(seg) else last[i]
                x, y, theta = (float(v) for v in row[:3])
                dx, dy = float(xy[j, f, 0]) - x, float(xy[j, f, 1]) - y
                meas[j, f, a] = (x, y, theta, math.sqrt(dx * dx + dy * dy), math.atan2(dy, dx) - theta)
    return meas


def first_bin_of_time(bins, t):
    """index of the first bin [t0, t1] of bins [T,2] with t0 <= t <= t1; T - 1 where there is none (past the end)"""
    b = np.asarray(bins, dtype=np.float64).reshape(-1, 2)
    hit = np.flatnonzero((b[:, 0] <= t) & (t <= b[:, 1]))
    return int(hit[0]) if len(hit) else len(b) - 1


class FleetTracker:
    """A fleet that tracks F sharks in a closed loop on the device.  Three contexts hold the state; what the loop itself moves
    across the bus in a round is the sharks' true positions (F x 2 doubles in) and the round records (128 bytes per AUV out).
    (`SharkForecast.run` still returns `prob` on the host as well -- the fallback of the hand-over and the final costs read it;
    DESIGN.md.)

        planner context (rrt)       the fleet's committed states, habitat lists and trajectory log (ReplanSession), the F shark
                                    tables the planner ranks against, the measurement table of the round
        filter context (filters)    the particles and their random streams (FilterBatch); the forecast's tables (SharkForecast
                                    on the same context)
        cost context (rrt's own)    the trajectories' final costs, at finish

    step() with r = session.round_index:
      1. meas [1, F, A, 5] from the AUVs' committed states against tracks[:, r] -- measure="device": replan_measure_kernel on
         the planner's context, handed to the filters' context as a device pointer (auvp_pf_run_dev_meas); measure="host":
         fleet_measurements on the host's mirror of the states and FilterBatch.run(meas=...) (the baseline, for tests);
      2. forecast.run(filters, prior, forecast_rounds, method, return_grids=False);
      3. session.set_shark_grids(fc, first_bin=b_r), b_r the first world bin that contains r * round_span (the last bin past
         the end): the forecast speaks from now on;
      4. session.round().
    filter_steps = k > 1: the filters hear the sharks k times per round, from where the AUVs were at k ticks of the bucket they
    just travelled (fleet_measurements_ticks; csrc/replan_ticks.h).  Round r consumes tracks[:, r*k : (r+1)*k] -- sample r*k + j
    is the shark at tick j, the round's last sample is "now" -- and the loop ends when fewer than k samples remain.  Step 1
    becomes meas [k, F, A, 5]: measure="device" is one replan_measure call (replan_measure_ticks_kernel) and one
    run_dev_meas(..., n_steps=k), k * F * 2 doubles in and nothing else across the bus; measure="host" downloads the
    trajectories (ReplanSession.last_segments) for fleet_measurements_ticks.  In round 0 nothing is committed yet: all k
    measurements are taken from the start states.  step() then returns estimates_all [k,F,2] beside estimates, the last step's.
    Limits: every shark is tracked by the same number of AUVs (ValueError); at most 64 filter steps per round, the sharks
    sampled at equal ticks of it; b_r comes from the NOMINAL time r * round_span, not from the AUVs' own clocks (their
    committed times drift apart by less than a round).
    tracks [F, S, 2]; shark_of [N]; the remaining keyword arguments are RRT.replanning_session's (shark_of is passed on)."""

    def __init__(self, rrt, forecast, filters, tracks, shark_of, prior, forecast_rounds, method=("ave", 1), measure="device",
                 large_grids=False, filter_steps=1, **session_args):
        if measure not in ("device", "host"):
            raise ValueError("measure must be 'device' or 'host', not %r" % (measure,))
        self.tracks = np.asarray(tracks, dtype=np.float64)
        if self.tracks.ndim != 3 or self.tracks.shape[2] != 2:
            raise ValueError("tracks must be [F, S, 2]")
        if isinstance(filter_steps, (bool, np.bool_)) or int(filter_steps) != filter_steps or not 1 <= int(filter_steps) <= MEAS_MAX_TICKS:
            raise ValueError("filter_steps must be an integer in 1 .. %d, not %r" % (MEAS_MAX_TICKS, filter_steps))
        self.filter_steps = int(filter_steps)
        if self.tracks.shape[1] < self.filter_steps:
            raise ValueError("tracks has %d samples, fewer than filter_steps = %d" % (self.tracks.shape[1], self.filter_steps))
        F = self.tracks.shape[0]
        if F != filters.F:
            raise ValueError("tracks has %d sharks, the filter batch %d" % (F, filters.F))
        self.members = shark_members(shark_of, F)  # (before anything is launched)
        self.shark_of = np.array([int(g) for g in shark_of], dtype=np.int32)
        self.A = self.members.shape[1]
        self.rrt, self.forecast, self.filters = rrt, forecast, filters
        self.prior, self.forecast_rounds, self.method, self.measure, self.large_grids = prior, int(forecast_rounds), method, measure, large_grids
        # the planner needs F tables before a session with shark_of can open: the forecast of the filters as they stand
        rrt.set_shark_grids(self._forecast(), first_bin=0)
        self.session = rrt.replanning_session(shark_of=[int(g) for g in shark_of], **session_args)

    def _forecast(self):
        return self.forecast.run(self.filters, self.prior, self.forecast_rounds, self.method, large_grids=self.large_grids,
                                 return_grids=False)

    def step(self):
        """one round of the loop; the round's dict (ReplanSession.round) plus estimates [F,2], the filters' means after the
        update (with filter_steps = k > 1: after the round's last step, and estimates_all [k,F,2], after each) -- or None once no
        AUV plans any more or the tracks have ended"""
        s = self.session
        r, k = s.round_index, self.filter_steps
        if (r + 1) * k > self.tracks.shape[1] or len(s.active()) == 0:
            return None
        if k == 1:
            shark = self.tracks[:, r, :]
            if self.measure == "device":
                ptr = self.rrt._ctx.replan_measure(self.shark_of, self.A, shark)
                self.filters.run_dev_meas(ptr, self.A, shark[None])
            else:
                self.filters.run(meas=fleet_measurements(s.last, self.shark_of, shark), shark_xy=shark[None])
        else:
            shark = np.ascontiguousarray(self.tracks[:, r * k:(r + 1) * k, :].transpose(1, 0, 2))  # [k,F,2]
            if self.measure == "device":
                ptr = self.rrt._ctx.replan_measure(self.shark_of, self.A, shark)
                self.filters.run_dev_meas(ptr, self.A, shark, n_steps=k)
            else:
                meas = fleet_measurements_ticks(s.last_segments(), s.last, self.shark_of, shark, s.round_span)
                self.filters.run(meas=meas, shark_xy=shark)
        fc = self._forecast()
        s.set_shark_grids(fc, first_bin=first_bin_of_time(self.rrt._bins, r * s.round_span))
        out = s.round()
        if out is not None:
            est = self.filters.estimates()[0]
            out["estimates"] = est[-1]
            if k > 1:
                out["estimates_all"] = est
        return out

    def run(self, as_arrays=False):
        """step() until the session is done or the tracks end; returns session.finish(as_arrays)"""
        while self.step() is not None:
            pass
        return self.session.finish(as_arrays)

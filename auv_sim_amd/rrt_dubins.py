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


def team_labels(teams, n):
    """replanning_batch's teams -> [n] int32 labels, checked without a device: AUVs with the same label >= 0 form a team, a
    label < 0 is an AUV on its own; labels need not be dense.  ValueError for a wrong length, a bool, a value that is no integer
    or one outside int32."""
    lab = list(teams)
    if len(lab) != n:
        raise ValueError("teams has %d entries, expected %d" % (len(lab), n))
    out = np.zeros(n, dtype=np.int32)
    for i, t in enumerate(lab):
        try:
            ok = not isinstance(t, (bool, np.bool_)) and int(t) == t
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("teams[%d] = %r is not an integer" % (i, t))
        if not -2 ** 31 <= int(t) < 2 ** 31:
            raise ValueError("teams[%d] = %d outside int32" % (i, int(t)))
        out[i] = int(t)
    return out


def team_csr(labels):
    """the teams of a label array as (team_off [T+1], members): team t's members are members[team_off[t]:team_off[t+1]],
    ascending; the teams in ascending order of their labels; a team of fewer than two members is left out (csrc/replan_teams.h
    builds the same tables for replan_team_kernel)."""
    groups = {}
    for i, t in enumerate(labels):
        if int(t) >= 0:
            groups.setdefault(int(t), []).append(i)
    team_off, members = [0], []
    for t in sorted(groups):
        if len(groups[t]) >= 2:
            members.extend(groups[t])
            team_off.append(len(members))
    return np.array(team_off, dtype=np.int32), np.array(members, dtype=np.int32)


def team_fold(keep, labels):
    """The step that lets a team share one habitat list: every member's mask becomes the bitwise AND of the masks of all members
    of its team -- a habitat one of them has visited leaves everybody's list.  keep [n] ints (bit h: habitat h is on the list),
    labels as team_labels returns them.  Returns the new masks, a list of n ints; AUVs without a teammate keep theirs."""
    out = [int(k) for k in keep]
    if len(out) != len(labels):
        raise ValueError("keep has %d entries, labels %d" % (len(out), len(labels)))
    team_off, members = team_csr(labels)
    for t in range(len(team_off) - 1):
        ms = [int(m) for m in members[team_off[t]:team_off[t + 1]]]
        k = out[ms[0]]
        for m in ms[1:]:
            k &= out[m]
        for m in ms:
            out[m] = k
    return out


def course_habitat_words(course_xy, course_t, bins, bin_lo, bin_hi, habitats_xys):
    """One Python int per course point: bit h is set iff habitat h of habitats_xys [H,3] contains the point
    (math.sqrt(dx * dx + dy * dy) <= size, first_bucket_commit's test), and 0 for a point whose time stamp lies in none of the
    shark bins bins[bin_lo:bin_hi] -- habitat_shark_cost_func (cost.py:171-179) skips such a point entirely.  The words do not
    depend on any habitat list: rescore judges them under a mask.  csrc/replan_pick.h: replan_pick_word."""
    xy = np.asarray(course_xy, dtype=np.float64).reshape(-1, 2)
    t = np.asarray(course_t, dtype=np.float64).reshape(-1)
    n = len(xy)
    b = np.asarray(bins, dtype=np.float64).reshape(-1, 2)[max(int(bin_lo), 0):max(int(bin_hi), 0)]
    hb = np.asarray(habitats_xys, dtype=np.float64).reshape(-1, 3)
    if n == 0 or len(b) == 0 or len(hb) == 0:
        return [0] * n
    counted = ((t[:, None] >= b[None, :, 0]) & (t[:, None] <= b[None, :, 1])).any(axis=1)
    dx, dy = xy[:, None, 0] - hb[None, :, 0], xy[:, None, 1] - hb[None, :, 1]
    with np.errstate(over="ignore", invalid="ignore"):
        inside = np.sqrt(dx * dx + dy * dy) <= hb[None, :, 2]
    bits = inside.astype(object) @ np.array([1 << h for h in range(len(hb))], dtype=object)
    return [int(w) if c else 0 for w, c in zip(bits, counted)]


def rescore(words, mask, c2, leaf_time, weights):
    """The cost exploring would have given a course against the habitat list `mask` (bit h: habitat h is on it), from the
    course's words (course_habitat_words), its shark term c2 as the summary reports it (already divided by the leaf time; it
    does not depend on the list) and its leaf's traj_time_stamp: habitat_shark_cost_func's habitat terms, float operation by
    float operation as the leaf pass computes them (csrc/rrt_leaf_body.h: total_of).  A counted point hits the lowest-numbered
    habitat of mask that contains it.  Returns ([total, c0, c1, c2], vis) with vis the set of habitats hit.
    csrc/replan_pick.h: replan_pick_hits + replan_pick_score."""
    mask = int(mask)
    hits, vis = 0, 0
    for w in words:
        m = int(w) & mask
        if m:
            hits += 1
            vis |= m & -m
    n_list = bin(mask).count("1")
    w1, w2, c2, leaf_time = float(weights[0]), float(weights[1]), float(c2), float(leaf_time)
    c0, c1 = 0.0, 0.0
    if w2 == w2 and abs(w2) < 1048576.0 and w2 == float(round(w2)):
        c1 = 0.0 + w2 * float(hits)  # (an integer weight: exactly `hits` rounded additions; 0.0 + ...: never -0.0)
    else:
        for _ in range(hits):
            c1 = c1 + w2
    if leaf_time > 0:
        c1 = c1 / leaf_time
    if n_list != 0:
        c0 = w1 * float(bin(vis).count("1")) / float(n_list)
    return [((0.0 + c0) + c1) + c2, c0, c1, c2], vis


def team_pick_claims(labels, keep, active, cands, weights):
    """The team-aware winner selection of replanning_batch(team_pick="claims") for one round -- the definition the device
    kernels (csrc/replan_pick.h, replan_kernels.hip) match bit for bit.  labels [n] as team_labels returns them, keep [n] the
    lists at the round's start, active: the AUVs that plan in this round (group g is AUV active[g]); cands[g]: that AUV's K
    candidates in tree order, each None (the tree has no leaf) or a dict(words=course_habitat_words of the tree's own best
    course, cost=its four costs as the leaf pass ranked it under keep, leaf_time=its leaf's time).

    Every team of two or more: claimed = 0; its members that are in `active`, in ascending AUV index: each candidate is scored
    by rescore under keep[m] & ~claimed (c2 = cost[3]); the winner is rrt_group_best's fold over the scores -- score < best so
    far, from inf: the lowest tree among equal scores, never a NaN, never a tree without a leaf --; claimed |= the winner's vis
    (its whole course).  A member without a winner claims nothing.  Everybody else gets the same fold over cost[0].
    Returns per group a dict(winner=tree or -1, cost=[4] the winner's score (inf without one), claimed=the mask the member
    saw (0 without teammates), n_with_leaf)."""
    active = [int(a) for a in active]
    slot_of = {a: g for g, a in enumerate(active)}
    inf = float("inf")
    out = []
    for g in range(len(active)):  # rrt_group_best_kernel's record
        best, win, cost = inf, -1, [inf] * 4
        for k, c in enumerate(cands[g]):
            if c is not None and float(c["cost"][0]) < best:
                best, win, cost = float(c["cost"][0]), k, [float(x) for x in c["cost"]]
        out.append(dict(winner=win, cost=cost, claimed=0, n_with_leaf=sum(c is not None for c in cands[g])))
    team_off, members = team_csr(labels)
    for t in range(len(team_off) - 1):
        claimed = 0
        for m in members[team_off[t]:team_off[t + 1]]:
            g = slot_of.get(int(m))
            if g is None:
                continue
            mask = int(keep[int(m)]) & ~claimed
            best, win, cost, vis_w = inf, -1, [inf] * 4, 0
            for k, c in enumerate(cands[g]):
                if c is None:
                    continue
                s, vis = rescore(c["words"], mask, c["cost"][3], c["leaf_time"], weights)
                if s[0] < best:
                    best, win, cost, vis_w = s[0], k, s, vis
            out[g].update(winner=win, cost=cost, claimed=claimed)
            claimed |= vis_w
    return out


MAX_SEPARATION_TICKS = 1024  # (csrc/replan_apart.h: REPLAN_APART_MAX_TICKS, the LDS tables of rrt_course_ticks_kernel)
MAX_SEPARATION_TEAM = 1024   # (REPLAN_APART_MAX_TEAM: the winner list of replan_team_pick_apart_kernel)


def course_ticks(course_t, course_xy, tick, W):
    """The tick table of a course, rows 0 .. L-1 root -> leaf (row 0: the AUV's committed state): where the AUV is at the
    instants s * tick, taking it to stay at the last point it reached -- no interpolation.  q_i = ceil(t_i / tick) (one IEEE
    division and a ceil, in double); s_lo = q_0, s_hi = s_lo + W - 1, s_last = min(s_hi, max of the non-NaN q_i); owner(s) is the
    LARGEST row index among the rows with q_i <= s (a q_i < s_lo counts as s_lo; a NaN q_i and a q_i > s_hi own nothing, but
    the latter -- an infinite time included -- extends the table to s_hi).  Returns (s_lo, xy [s_last - s_lo + 1, 2]), xy[j] the
    position of owner(s_lo + j).  A course without rows, or one whose q_0 is no number inside int32 (replanning_batch refuses
    a horizon that could give one), has the empty table (0, xy [0,2]): it conflicts with nothing.
    csrc/replan_apart.h: replan_tick_q / replan_tick_slot / replan_ticks_build."""
    t = np.asarray(course_t, dtype=np.float64).reshape(-1)
    xy = np.asarray(course_xy, dtype=np.float64).reshape(-1, 2)
    W = int(W)
    if len(t) == 0:
        return 0, np.zeros((0, 2))
    with np.errstate(all="ignore"):
        q = np.ceil(t / np.float64(tick))
    if not (q[0] == q[0] and -2.0 ** 31 < q[0] < 2.0 ** 31):
        return 0, np.zeros((0, 2))
    owner = [-1] * W  # per tick: the largest row that proposes it
    top = 0
    for i in range(len(t)):
        if q[i] != q[i]:
            continue
        r = q[i] - q[0]
        if r <= 0.0:
            slot = 0
        elif r > float(W - 1):
            top = W - 1
            continue
        else:
            slot = int(r)
        top = max(top, slot)
        owner[slot] = max(owner[slot], i)
    out = np.zeros((top + 1, 2))
    cur = -1
    for j in range(top + 1):
        cur = max(cur, owner[j])
        out[j] = xy[cur]
    return int(q[0]), out


def tick_conflicts(s_lo, xy, trail, d):
    """the ticks of the table (s_lo, xy) that are in conflict with the trail, a list of tables: some table of the trail covers
    the tick and dx * dx + dy * dy < d * d there (plain differences, no contraction; a NaN never conflicts).
    csrc/replan_apart.h: replan_apart_count."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    if len(xy) == 0 or not trail:
        return 0
    d2 = np.float64(d) * np.float64(d)
    hit = np.zeros(len(xy), dtype=bool)
    for w_lo, w_xy in trail:
        a, b = max(int(s_lo), int(w_lo)), min(int(s_lo) + len(xy), int(w_lo) + len(w_xy))
        if a >= b:
            continue
        with np.errstate(all="ignore"):
            dx = xy[a - s_lo:b - s_lo, 0] - w_xy[a - w_lo:b - w_lo, 0]
            dy = xy[a - s_lo:b - s_lo, 1] - w_xy[a - w_lo:b - w_lo, 1]
            hit[a - s_lo:b - s_lo] |= dx * dx + dy * dy < d2
    return int(hit.sum())


def team_pick_separated(labels, keep, active, cands, weights, d, claims):
    """The winner selection of replanning_batch(team_separation=d) for one round -- the definition the device kernels
    (csrc/replan_apart.h, replan_kernels.hip) match bit for bit.  Arguments as team_pick_claims takes them; every candidate
    also carries ticks=(s_lo, xy), its course_ticks table (and needs words / leaf_time only with claims).

    Every team of two or more: the trail is empty (and claimed = 0); its members that are in `active`, in ascending AUV index:
    a candidate's score is its own cost[0] (claims false) or rescore's under keep[m] & ~claimed (claims true: team_pick_claims'
    score); it is eligible if score < inf; n is tick_conflicts of its table against the trail; the winner is the smallest
    (n, score), the lowest tree among equals.  The winner's table joins the trail (and, with claims, its vis the claimed mask).
    Everybody else gets rrt_group_best's fold over cost[0].  Returns what team_pick_claims returns plus conflicts = the
    winner's n per group (0 without a winner or a teammate); claimed is 0 everywhere without claims."""
    active = [int(a) for a in active]
    slot_of = {a: g for g, a in enumerate(active)}
    inf = float("inf")
    out = []
    for g in range(len(active)):  # rrt_group_best_kernel's record
        best, win, cost = inf, -1, [inf] * 4
        for k, c in enumerate(cands[g]):
            if c is not None and float(c["cost"][0]) < best:
                best, win, cost = float(c["cost"][0]), k, [float(x) for x in c["cost"]]
        out.append(dict(winner=win, cost=cost, claimed=0, n_with_leaf=sum(c is not None for c in cands[g]), conflicts=0))
    team_off, members = team_csr(labels)
    for t in range(len(team_off) - 1):
        claimed, trail = 0, []
        for m in members[team_off[t]:team_off[t + 1]]:
            g = slot_of.get(int(m))
            if g is None:
                continue
            mask = int(keep[int(m)]) & ~claimed
            best, best_n, win, cost, vis_w = inf, 0, -1, [inf] * 4, 0
            for k, c in enumerate(cands[g]):
                if c is None:
                    continue
                if claims:
                    s, vis = rescore(c["words"], mask, c["cost"][3], c["leaf_time"], weights)
                else:
                    s, vis = [float(x) for x in c["cost"]], 0
                if not s[0] < inf:
                    continue
                n = tick_conflicts(c["ticks"][0], c["ticks"][1], trail, d)
                if win < 0 or n < best_n or (n == best_n and s[0] < best):
                    best, best_n, win, cost, vis_w = s[0], n, k, s, vis
            out[g].update(winner=win, cost=cost, claimed=claimed, conflicts=best_n if win >= 0 else 0)
            if win >= 0:
                trail.append(cands[g][win]["ticks"])
            claimed |= vis_w
    return out


def separation_args(team_separation, separation_tick, separation_ticks, labels, span):
    """replanning_batch's team_separation keywords checked without a device: (d, tick, W), or None with the option off.
    span: plan_time_budget + replan_time_interval, the part of a course a round commits (the default window).  The check of
    the horizon's end against the tick is replanning_batch's own."""
    if team_separation is None:
        return None

    def positive(x):
        return (isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_)) and math.isfinite(float(x))
                and float(x) > 0.0)

    if labels is None:
        raise ValueError("team_separation needs teams")
    if not positive(team_separation):
        raise ValueError("team_separation must be None or a finite distance > 0, not %r" % (team_separation,))
    if not positive(separation_tick):
        raise ValueError("separation_tick must be a finite time > 0, not %r" % (separation_tick,))
    d, tick = float(team_separation), float(separation_tick)
    if separation_ticks is None:
        W = span / tick
        W = int(math.ceil(W)) if math.isfinite(W) else 0
    else:
        try:
            ok = not isinstance(separation_ticks, (bool, np.bool_)) and int(separation_ticks) == separation_ticks
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError("separation_ticks must be None or an integer, not %r" % (separation_ticks,))
        W = int(separation_ticks)
    if not 1 <= W <= MAX_SEPARATION_TICKS:
        raise ValueError("separation_ticks = %d outside 1 .. %d" % (W, MAX_SEPARATION_TICKS))
    team_off = team_csr(labels)[0]
    if len(team_off) > 1 and int(np.diff(team_off).max()) > MAX_SEPARATION_TEAM:
        raise ValueError("team_separation: a team of %d members, more than %d" % (int(np.diff(team_off).max()), MAX_SEPARATION_TEAM))
    return d, tick, W


def first_bucket_commit(course_t, course_xy, t0, max_traj_time, round_span, keep, habitats_xys):
    """One round of replanning's host step (rrt_dubins.py:82-87) on arrays: the points of the course that splitPath
    (:590-602) puts into its first bucket, and removeHabitat (:604-610) applied to the episode's habitat list given as the
    bit mask `keep` over the table habitats_xys [H,3] (list order = table order).  Returns (boolean mask of the course's
    points in the first bucket, the new keep).  Raises ValueError where the reference's next(iter(buckets)) would raise:
    the horizon holds no whole bucket."""
    if math.floor(max_traj_time / round_span) < 1:
        raise ValueError("max_traj_time %r holds no shark-interval bucket of %r" % (max_traj_time, round_span))
    lo, hi = t0 + 0 * round_span, t0 + (0 + 1) * round_span  # splitPath's first edge, the same float operations
    t = np.asarray(course_t, dtype=np.float64)
    sel = (lo <= t) & (t <= hi)
    if keep and len(habitats_xys):
        hb = np.asarray(habitats_xys, dtype=np.float64).reshape(-1, 3)
        xy = np.asarray(course_xy, dtype=np.float64).reshape(-1, 2)[sel]
        # math.sqrt((x - hx) ** 2 + (y - hy) ** 2) <= size per (point, habitat): every habitat that contains each point
        dx, dy = xy[:, None, 0] - hb[None, :, 0], xy[:, None, 1] - hb[None, :, 1]
        inside = np.sqrt(dx * dx + dy * dy) <= hb[None, :, 2]
        bits = inside.astype(object) @ np.array([1 << h for h in range(len(hb))], dtype=object) if len(xy) else []
        for b in bits:  # point by point: the first habitat still on the list is removed
            m = int(b) & keep
            if m:
                keep &= ~(m & -m)
    return sel, keep


def _mt_state_of(rng_state):
    """random.getstate() -> (624 words, index)"""
    ver, internal, _ = rng_state
    if ver != 3 or len(internal) != 625:
        raise RuntimeError("unexpected random.getstate() layout")
    return np.array(internal[:624], dtype=np.uint32), int(internal[624])


class _Init:
    """a committed state as exploring reads it (x, y, theta, traj_time_stamp, plan_time_stamp, length)"""
    __slots__ = ("x", "y", "theta", "traj_time_stamp", "plan_time_stamp", "length")

    def __init__(self, row):
        self.x, self.y, self.theta, self.traj_time_stamp, self.plan_time_stamp, self.length = (
            row[0], row[1], row[2], row[4], row[5], row[6])


class ReplanSession:
    """RRT.replanning_batch(commit="device") as a resumable object (RRT.replanning_session).  The fleet's state -- last [N,7],
    keep [N], the trajectory log -- lives on the planner's context in HBM; the host keeps [N] mirrors from the round records.
    round() is one iteration of the loop; set_shark_grids() between two rounds swaps the F shark tables and touches nothing
    else; finish() downloads the trajectories once and closes the session.  While it is open the session owns the planner's
    context: every other call on the RRT that would prepare a batch, change the world or the tables, or open a second session
    raises RuntimeError and leaves the session as it was."""

    def __init__(self, rrt, starts, all_habitats, hab, horizon_end, round_span, traj_time_length, weight, max_iter, seeds, K, sets,
                 labels=None, team_pick=None, sep=None):
        N, H = len(starts), len(all_habitats)
        if seeds is None or len(seeds) != N or any(s is None for s in seeds):
            raise ValueError("AUV %d has neither a seed nor a generator"
                             % (0 if seeds is None or len(seeds) != N else [s is None for s in seeds].index(True)))
        if getattr(rrt, "_session", None) is not None:
            raise RuntimeError("replanning_session: a replanning session is open on this RRT (finish() it first)")
        self.rrt, self.inside, self.closed = rrt, False, False
        self._starts, self._all_habitats, self._hab = list(starts), all_habitats, hab
        self._horizon_end, self.round_span, self._weight, self._max_iter = horizon_end, round_span, weight, int(max_iter)
        self._K, self._sets, self._labels, self._team_pick, self._sep = K, sets, labels, team_pick, sep
        self._streams = [random.Random(s) for s in seeds]
        self._last = np.array([[float(m.x), float(m.y), float(m.theta), float(getattr(m, "v", 0.0) or 0.0), float(m.traj_time_stamp),
                                float(m.plan_time_stamp), float(m.length)] for m in starts], dtype=np.float64).reshape(N, 7)
        self._keep = np.full(N, (1 << H) - 1, dtype=np.uint64)
        self._ttl = np.full(N, float(traj_time_length))
        self._alive = np.ones(N, dtype=bool)
        ctx = rrt._ctx
        ctx.set_habitats(hab)  # (the whole list: every episode's own list is its keep mask over this table)
        ctx.replan_begin(self._last, self._keep)
        if labels is not None:
            ctx.replan_set_teams(labels)
        # (a fleet without a team of two or more: everybody gets rrt_group_best's record, which is what it runs)
        self._pick = (team_pick is not None or sep is not None) and len(team_csr(labels)[0]) > 1
        rrt._batch = None  # (rerank follows an exploring_batch only)
        self._log = []  # per round: (AUVs that committed, their records, keep and max_traj_time at that round, winning member)
        self.round_index = 0
        rrt._session = ctx.session = self

    # ---- views
    @staticmethod
    def _view(a):
        v = a.view()
        v.flags.writeable = False
        return v

    @property
    def last(self):
        """[N,7] the AUVs' committed states (read-only)"""
        return self._view(self._last)

    @property
    def keep(self):
        """[N] uint64 the AUVs' habitat lists (read-only); with teams the team's list of the member's last round"""
        return self._view(self._keep)

    def active(self):
        """indices of the AUVs that would plan in the next round"""
        return np.flatnonzero(self._alive & (self._last[:, 4] + self.round_span < self._horizon_end))

    def _open(self, what):
        if self.closed:
            raise RuntimeError("%s: the session is closed" % what)

    class _Own:
        def __init__(self, s):
            self.s = s

        def __enter__(self):
            self.s.inside = True

        def __exit__(self, *exc):
            self.s.inside = False

    def set_shark_grids(self, forecast, first_bin=0):
        """Swap the F shark tables between two rounds (RRT.set_shark_grids; a Forecast is placed at the planner's absolute
        bins from first_bin on).  The replan state -- last, keep, the log, the seeds' streams -- is not touched; the number of
        tables must still cover the session's shark_of (ValueError, and the old tables stay)."""
        self._open("set_shark_grids")
        rrt = self.rrt
        if self._sets is not None:
            n = 0 if forecast is None else (len(forecast.prob) if hasattr(forecast, "prob") else len(forecast))
            if n <= int(self._sets.max()):
                raise ValueError("%d tables do not cover the session's shark_of (up to %d)" % (n, int(self._sets.max())))
        with self._Own(self):
            rrt._set_prob = put_shark_tables(rrt._ctx, rrt._bins, rrt._cells, forecast, first_bin)

    def round(self):
        """One round: the active AUVs' round seeds, one exploring launch, the winners (or the team kernels), the commit on the
        device.  Returns a dict of [A] arrays -- auv (the active indices), last [A,7], keep, winner (the winning tree of the
        AUV's K, -1: no qualifying leaf; that AUV stops planning), cost [A,4] -- or None once no AUV is active."""
        self._open("round")
        act = self.active()
        if len(act) == 0:
            return None
        rrt, ctx, K, sets, sep = self.rrt, self.rrt._ctx, self._K, self._sets, self._sep
        last, keep, ttl = self._last, self._keep, self._ttl
        horizon_end, round_span = self._horizon_end, self.round_span
        with self._Own(self):
            t_now = last[act, 4]
            clip = ttl[act] + t_now > horizon_end  # stays clipped for the later rounds too (:76-77)
            ttl[act[clip]] = horizon_end - t_now[clip]
            mtt = ttl[act] + t_now
            short = np.floor(mtt / round_span) < 1  # (first_bucket_commit's ValueError, from the host's numbers, before the launch)
            if short.any():
                raise ValueError("max_traj_time %r holds no shark-interval bucket of %r" % (float(mtt[np.argmax(short)]), round_span))
            seed_arg = np.array([self._streams[e].getrandbits(63) for e in act for _ in range(K)], dtype=np.uint64)
            ctx.rrt_explore_batch(np.repeat(last[act][:, [0, 1, 2, 4, 5, 6]], K, axis=0), seed_arg, self._max_iter, mode="timebin",
                                  freq=rrt.freq, bin_interval=5, v=2, max_traj_time=np.repeat(mtt, K), weights=self._weight,
                                  dist_to_end=rrt.dist_to_end, diff_max=rrt.diff_max, min_dist=0.5, max_plan_time=float(self._max_iter),
                                  habitat_keep=np.repeat(keep[act], K), summaries=False,
                                  shark_set=None if sets is None else np.repeat(sets[act], K))
            pick = self._pick
            if pick and sep is not None:
                best = ctx.replan_team_pick_apart(act, K, self._team_pick is not None, *sep)
            else:
                best = ctx.replan_team_pick(act, K) if pick else ctx.rrt_group_best(np.arange(len(act) + 1, dtype=np.int64) * K)
            bad = best["status"] < 0
            if bad.any():
                i = int(np.argmax(bad))
                raise _lib.AuvpError(int(best[i]["status"]), ("a tree of AUV %d failed on the device (status %d)" if K > 1 else
                                                              "AUV %d failed on the device (status %d)") % (act[i], int(best[i]["status"])))
            rec = ctx.replan_commit(act, round_span)
            bad = rec["status"] < 0
            if bad.any():
                i = int(np.argmax(bad))
                raise _lib.AuvpError(int(rec[i]["status"]), "AUV %d: the commit step failed on the device (status %d)" % (act[i], int(rec[i]["status"])))
            won = rec["winner"] >= 0
            self._alive[act[~won]] = False  # no qualifying leaf: the sequential call would raise TypeError
            tree = rec["winner"] - np.arange(len(act)) * K
            self._log.append((act[won], rec[won], keep[act][won], mtt[won], tree[won],
                              rec["claimed"][won] if pick else np.zeros(int(won.sum()), dtype=np.uint64),
                              rec["conflicts"][won].astype(np.int64) if pick else np.zeros(int(won.sum()), dtype=np.int64)))
            last[act] = rec["last"]
            keep[act] = rec["keep"]
            self.round_index += 1
        return dict(auv=act, last=rec["last"].copy(), keep=rec["keep"].copy(), winner=np.where(won, tree, -1).astype(np.int64),
                    cost=rec["cost"].reshape(-1, 4).copy())

    def close(self):
        """give the planner's context back without results (finish() does it itself); harmless on a closed session"""
        if not self.closed:
            self.closed = True
            if self.rrt._session is self:
                self.rrt._session = None
            if self.rrt._ctx.session is self:
                self.rrt._ctx.session = None

    def finish(self, as_arrays=False):
        """What replanning_batch returns, from the rounds run so far; the session is closed afterwards.  Every trajectory's
        cost is taken against the shark tables SET LAST (set_shark_grids), not against the tables each round was planned
        under: with tables that change, the cost describes the trajectory under the latest forecast."""
        self._open("finish")
        try:
            with self._Own(self):
                return self._results(as_arrays)
        finally:
            self.close()

    def _results(self, as_arrays):
        rrt, ctx, starts, all_habitats, hab = self.rrt, self.rrt._ctx, self._starts, self._all_habitats, self._hab
        N, H = len(starts), len(all_habitats)
        labels, team_pick, sep, sets = self._labels, self._team_pick, self._sep, self._sets
        last, keep, alive, log = self._last, self._keep, self._alive, self._log
        if labels is not None:
            # a member that stopped planning holds the team's list of its last round: lists only shrink, so the AND over the
            # host's copies is the team's final one
            keep = np.array(team_fold(keep, labels), dtype=np.uint64)
        row_off, rows_all = ctx.replan_traj()
        done = [int(e) for e in np.flatnonzero(alive)]
        rows = {e: rows_all[row_off[e]:row_off[e + 1]] for e in done}
        costs = rrt._replan_costs(done, rows, last[:, 4], hab, sets)
        # the rounds of every AUV, in round order: one stable sort of all the rounds' records by AUV
        if log:
            auv = np.concatenate([x[0] for x in log])
            order = np.argsort(auv, kind="stable")
            r_rec = np.concatenate([x[1] for x in log])[order]
            r_keep = np.concatenate([x[2] for x in log])[order]
            r_mtt = np.concatenate([x[3] for x in log])[order]
            r_tree = np.concatenate([x[4] for x in log])[order].astype(np.int64)
            r_claimed = np.concatenate([x[5] for x in log])[order].astype(np.uint64)
            r_conflicts = np.concatenate([x[6] for x in log])[order]
            first = np.searchsorted(auv[order], np.arange(N + 1))
        else:
            r_rec, r_keep, r_mtt, r_tree = np.zeros(0, _lib.REPLAN_RECORD_DTYPE), np.zeros(0, np.uint64), np.zeros(0), np.zeros(0, np.int64)
            r_claimed, r_conflicts = np.zeros(0, np.uint64), np.zeros(0, np.int64)
            first = np.zeros(N + 1, dtype=np.int64)
        res = []
        for e in range(N):
            if not alive[e]:
                res.append(None)
                continue
            a, b = int(first[e]), int(first[e + 1])
            lens = r_rec["n_committed"][a:b].astype(np.int64)
            if as_arrays:
                res.append(dict(traj=rows[e], round_len=lens, round_keep=r_keep[a:b].copy(), round_max_traj_time=r_mtt[a:b].copy(),
                                round_cost=r_rec["cost"][a:b].reshape(-1, 4).copy(), round_tree=r_tree[a:b].copy(),
                                keep=int(keep[e]), cost=costs[e]))
                if team_pick is not None:
                    res[-1]["round_claimed"] = r_claimed[a:b].copy()
                if sep is not None:
                    res[-1]["round_conflicts"] = r_conflicts[a:b].copy()
                continue
            # objects: each round's first row is the previous round's last object (the start object in round 1), the rest are
            # new -- what _materialise_course makes of the course on the host route
            traj, rounds, prev, at = [], {}, starts[e], 0
            for k, n in enumerate(lens):
                objs = [prev] + [Motion_plan_state(float(r[0]), float(r[1]), theta=float(r[2]), v=float(r[3]), traj_time_stamp=float(r[4]),
                                                   plan_time_stamp=float(r[5]), length=float(r[6])) for r in rows[e][at + 1:at + n]]
                if n == 0:
                    objs = []
                at += int(n)
                traj.extend(objs)
                kb = int(r_keep[a + k])
                rounds[k + 1] = [objs, [all_habitats[h] for h in range(H) if (kb >> h) & 1]]
                if objs:
                    prev = objs[-1]
            c = costs[e]
            res.append([traj, rounds, [float(c[0]), [float(c[1]), float(c[2]), float(c[3])]],
                        [all_habitats[h] for h in range(H) if (int(keep[e]) >> h) & 1]])
        return res


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
        bad = best["status"] < 0
        if bad.any():
            i = int(np.argmax(bad))
            raise _lib.AuvpError(int(best[i]["status"]), "a tree of AUV %d failed on the device (status %d)" % (i, int(best[i]["status"])))
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
        replanning_session gives the same loop one round at a time).  The results equal commit="host" (the default) in every field.  Seeds only (rngs raises ValueError); the ValueError for a horizon that holds no whole bucket
        is raised before the round is launched.

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
        N, sets, labels, K, round_span, sep, horizon_end, all_habitats, hab, max_iter = self._replan_args(
            starts, habitats, plan_time_budget, replan_time_interval, max_iter, trees_per_auv, shark_of, teams, team_pick,
            team_separation, separation_tick, separation_ticks, rngs, commit)
        H = len(all_habitats)
        if commit == "device":
            # the one copy of the device loop: a session, its rounds until nobody plans any more, its end
            session = ReplanSession(self, starts, all_habitats, hab, horizon_end, round_span, traj_time_length, weight, max_iter, seeds,
                                    K, sets, labels, team_pick, sep)
            try:
                while session.round() is not None:
                    pass
                return session.finish(as_arrays)
            finally:
                session.close()
        gens = [None] * N     # rngs[e]: the global stream of a sequential call
        streams = [None] * N  # seeds[e]: replanning's private stream, one 63-bit seed per round
        for e in range(N):
            if rngs is not None and rngs[e] is not None:
                gens[e] = rngs[e]
            elif seeds is not None and seeds[e] is not None:
                streams[e] = random.Random(seeds[e])
            else:
                raise ValueError("AUV %d has neither a seed nor a generator" % e)
        keep = [(1 << H) - 1] * N
        ttl = [float(traj_time_length)] * N
        last = [[float(m.x), float(m.y), float(m.theta), float(getattr(m, "v", 0.0) or 0.0), float(m.traj_time_stamp),
                 float(m.plan_time_stamp), float(m.length)] for m in starts]
        last_obj = list(starts)
        traj = [[] for _ in range(N)]      # committed rows (arrays) or objects
        rounds = [[] for _ in range(N)]    # (bucket, keep at that round, max_traj_time, best_cost)
        alive = [True] * N
        while True:
            act = [e for e in range(N) if alive[e] and last[e][4] + round_span < horizon_end]
            if not act:
                break
            for e in act:
                if ttl[e] + last[e][4] > horizon_end:  # stays clipped for the later rounds too (:76-77)
                    ttl[e] = horizon_end - last[e][4]
            mtt = np.array([ttl[e] + last[e][4] for e in act], dtype=np.float64)
            claimed, conflicts = [0] * len(act), [0] * len(act)
            if sep is not None:
                status, best_cost, tree, paths, claimed, conflicts = self._replan_round_pick(
                    act, K, streams, gens, last, all_habitats, hab, mtt, keep, weight, max_iter, labels, None if sets is None else sets[act],
                    sep=sep, claims=team_pick is not None)
            elif team_pick is not None:
                status, best_cost, tree, paths, claimed = self._replan_round_pick(act, K, streams, gens, last, all_habitats, hab, mtt, keep,
                                                                                  weight, max_iter, labels, None if sets is None else sets[act])
            elif K > 1:
                status, best_cost, tree, paths = self._replan_round_best_of(act, K, streams, last, all_habitats, mtt, keep, weight,
                                                                            max_iter, None if sets is None else sets[act])
            else:
                status, best_cost, tree, paths = self._replan_round(act, streams, gens, last, all_habitats, mtt, keep, weight,
                                                                    max_iter, None if sets is None else sets[act])
            for i, e in enumerate(act):
                if status[i] == _lib.NO_QUALIFYING_LEAF:
                    alive[e] = False
                    traj[e] = None
                    continue
                p = paths[i].copy()
                p[0] = last[e]  # the course starts at the committed state itself (exploring returns the caller's object)
                sel, new_keep = first_bucket_commit(p[:, 4], p[:, :2], last[e][4], float(mtt[i]), round_span, keep[e], hab)
                bucket = p[sel]
                if as_arrays:
                    traj[e].append(bucket)
                    rounds[e].append((len(bucket), keep[e], float(mtt[i]), np.array(best_cost[i]), int(tree[i]), claimed[i], conflicts[i]))
                else:
                    course = self._materialise_course(paths[i], last_obj[e])
                    objs = [course[j] for j in np.flatnonzero(sel)]
                    traj[e].extend(objs)
                    rounds[e].append((objs, [all_habitats[h] for h in range(H) if (keep[e] >> h) & 1]))
                    if objs:
                        last_obj[e] = objs[-1]
                keep[e] = new_keep
                if len(bucket):
                    last[e] = [float(x) for x in bucket[-1]]
            if labels is not None:  # (once all of the round's commits are done)
                keep = team_fold(keep, labels)
        done = [e for e in range(N) if traj[e] is not None]
        rows = {e: (np.concatenate(traj[e]) if as_arrays and traj[e] else
                    np.array([[m.x, m.y, m.theta, m.v, m.traj_time_stamp, m.plan_time_stamp, m.length] for m in traj[e]],
                             dtype=np.float64).reshape(-1, 7)) for e in done}
        costs = self._replan_costs(done, rows, [s[4] for s in last], hab, sets)
        res = []
        for e in range(N):
            if traj[e] is None:
                res.append(None)
            elif as_arrays:
                r = rounds[e]
                res.append(dict(traj=rows[e], round_len=np.array([x[0] for x in r], dtype=np.int64),
                                round_keep=np.array([x[1] for x in r], dtype=np.uint64),
                                round_max_traj_time=np.array([x[2] for x in r]),
                                round_cost=np.array([x[3] for x in r]).reshape(-1, 4),
                                round_tree=np.array([x[4] for x in r], dtype=np.int64), keep=keep[e], cost=costs[e]))
                if team_pick is not None:
                    res[-1]["round_claimed"] = np.array([x[5] for x in r], dtype=np.uint64)
                if sep is not None:
                    res[-1]["round_conflicts"] = np.array([x[6] for x in r], dtype=np.int64)
            else:
                c = costs[e]
                res.append([traj[e], {k + 1: [b, hl] for k, (b, hl) in enumerate(rounds[e])},
                            [float(c[0]), [float(c[1]), float(c[2]), float(c[3])]],
                            [all_habitats[h] for h in range(H) if (keep[e] >> h) & 1]])
        return res

    def _replan_costs(self, done, rows, last_t, hab, sets):
        """{e: cost [4]} of the whole trajectories rows[e] of the AUVs `done` against the ORIGINAL habitat list (:192-195), every
        AUV in one launch on the cost-only context (with shark_of: the AUVs grouped by table, one launch per table in use, each
        against its own table); last_t[e]: the time of an AUV that committed nothing"""
        if self._cost_ctx is None:
            self._cost_ctx = _lib.Context(self._ctx.device)
        costs = {}
        if done:
            for g in ([None] if sets is None else sorted(set(int(sets[e]) for e in done))):
                grp = done if g is None else [e for e in done if int(sets[e]) == g]
                self._cost_ctx.set_world(None, hab, None, self._bins, self._cells, self._prob if g is None else self._set_prob[g])
                out = self._cost_ctx.cost_paths([rows[e][:, [0, 1, 4]] for e in grp], [0] * len(grp), [len(self._bins)] * len(grp),
                                                [float(rows[e][-1, 4]) if len(rows[e]) else float(last_t[e]) for e in grp],
                                                [[-3.0, -3.0, -4.0]] * len(grp))
                costs.update({e: out[i] for i, e in enumerate(grp)})
        return costs

    def _replan_args(self, starts, habitats, plan_time_budget, replan_time_interval, max_iter, trees_per_auv, shark_of, teams, team_pick,
                     team_separation, separation_tick, separation_ticks, rngs=None, commit="device"):
        """the argument checks replanning_batch and replanning_session share, in one order, before any launch"""
        N = len(starts)
        sets = None if shark_of is None else shark_set_indices(shark_of, N, self.n_shark_sets)
        labels = None if teams is None else team_labels(teams, N)
        if team_pick is not None:
            if team_pick != "claims":
                raise ValueError("team_pick must be None or 'claims', not %r" % (team_pick,))
            if labels is None:
                raise ValueError("team_pick='claims' needs teams")
        K = int(trees_per_auv)
        if K < 1:
            raise ValueError("trees_per_auv must be >= 1")
        if K > 1 and rngs is not None:
            raise ValueError("rngs cannot be combined with trees_per_auv > 1: one generator cannot continue K streams")
        if commit not in ("host", "device"):
            raise ValueError("commit must be 'host' or 'device', not %r" % (commit,))
        if commit == "device" and rngs is not None:
            raise ValueError("rngs cannot be combined with commit='device': continuing a generator takes every episode's draw "
                             "count and a state upload per AUV and round -- the host work this option removes; give seeds")
        round_span = plan_time_budget + replan_time_interval
        sep = separation_args(team_separation, separation_tick, separation_ticks, labels, round_span)
        horizon_end = list(self.sharkGrid.keys())[-1][1]
        if sep is not None and not float(horizon_end) / sep[1] < 2.0 ** 31:
            raise ValueError("separation_tick %r: the horizon's end %r is tick 2**31 or later" % (sep[1], horizon_end))
        all_habitats = list(habitats)
        hab = _circles(all_habitats)
        if max_iter is None:
            max_iter = max(1, int(math.ceil(plan_time_budget * self.iters_per_second)))
        return N, sets, labels, K, round_span, sep, horizon_end, all_habitats, hab, max_iter

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
        N, sets, labels, K, round_span, sep, horizon_end, all_habitats, hab, max_iter = self._replan_args(
            starts, habitats, plan_time_budget, replan_time_interval, max_iter, trees_per_auv, shark_of, teams, team_pick,
            team_separation, separation_tick, separation_ticks)
        return ReplanSession(self, starts, all_habitats, hab, horizon_end, round_span, traj_time_length, weight, max_iter, seeds, K,
                             sets, labels, team_pick, sep)

    def _replan_round_summaries(self, act, K, streams, gens, last, all_habitats, mtt, keep, weight, max_iter, sets=None):
        """K trees per active AUV, run with summaries: the batch's episodes i*K .. i*K+K-1 are AUV act[i]'s, each from its
        committed state with its horizon and list.  AUV e draws K round seeds from streams[e]; with K == 1 a generator gens[e]
        continues the global stream instead and is advanced as exploring advances it.  A tree that failed on the device raises
        AuvpError.  Returns (summaries [A*K], every tree's best course)."""
        if K == 1:
            round_seeds = {e: streams[e].getrandbits(63) for e in act if streams[e] is not None}
            if all(gens[e] is None for e in act):
                seed_arg = np.array([round_seeds[e] for e in act], dtype=np.uint64)
            else:
                st = [_mt_state_of(gens[e].getstate() if gens[e] is not None else random.Random(round_seeds[e]).getstate())
                      for e in act]
                seed_arg = (np.stack([w for w, _ in st]), np.array([i for _, i in st], dtype=np.int32))
        else:
            seed_arg = np.array([streams[e].getrandbits(63) for e in act for _ in range(K)], dtype=np.uint64)
        init_objs = [_Init(last[e]) for e in act for _ in range(K)]
        summ = self._explore_summaries(init_objs, all_habitats, 5, 2, True, np.repeat(mtt, K), True, weight, max_iter, seed_arg,
                                       [keep[e] for e in act for _ in range(K)], shark_set=None if sets is None else np.repeat(sets, K))
        if K == 1:
            for i, e in enumerate(act):
                n = int(summ[i]["n_draw32"])
                if gens[e] is not None and n:
                    gens[e].getrandbits(32 * n)  # what exploring does to the global stream
        bad = summ["status"] < 0
        if bad.any():
            i = int(np.argmax(bad))
            raise _lib.AuvpError(int(summ[i]["status"]), ("a tree of AUV %d failed on the device (status %d)" if K > 1 else
                                                          "AUV %d failed on the device (status %d)") % (act[i // K], int(summ[i]["status"])))
        return summ, self._ctx.paths(summ)

    def _replan_round(self, act, streams, gens, last, all_habitats, mtt, keep, weight, max_iter, sets=None):
        """one round of replanning_batch, one tree per active AUV: (status [A], best_cost [A,4], tree [A] = 0, courses)"""
        summ, paths = self._replan_round_summaries(act, 1, streams, gens, last, all_habitats, mtt, keep, weight, max_iter, sets)
        return summ["status"], summ["best_cost"], np.zeros(len(act), dtype=np.int64), paths

    def _replan_round_pick(self, act, K, streams, gens, last, all_habitats, hab, mtt, keep, weight, max_iter, labels, sets=None,
                           sep=None, claims=True):
        """one round with team_pick="claims" on the host: K trees per active AUV, the round runs with summaries, EVERY candidate's
        course is copied to the host and team_pick_claims chooses.  Returns as _replan_round, tree = the chosen member, the
        courses the chosen ones', plus the claimed mask every AUV saw.  With sep = (d, tick, W), team_separation's round:
        every candidate also gets its tick table, team_pick_separated chooses (under the claims or without them), and the
        winners' conflict counts are returned as well."""
        summ, paths = self._replan_round_summaries(act, K, streams, gens, last, all_habitats, mtt, keep, weight, max_iter, sets)
        cands = []
        for g, e in enumerate(act):
            row = []
            for k in range(K):
                s, p = summ[g * K + k], paths[g * K + k]
                if s["best_leaf"] < 0 or len(p) == 0:
                    row.append(None)
                    continue
                p = p.copy()
                p[0] = last[e]  # (row 0 is the committed state, as in the commit rule)
                row.append(dict(cost=[float(x) for x in s["best_cost"]], leaf_time=float(p[-1, 4])))
                if claims:
                    row[-1]["words"] = course_habitat_words(p[:, :2], p[:, 4], self._bins, 0, len(self._bins), hab)
                if sep is not None:
                    row[-1]["ticks"] = course_ticks(p[:, 4], p[:, :2], sep[1], sep[2])
            cands.append(row)
        picks = team_pick_claims(labels, keep, act, cands, weight) if sep is None else team_pick_separated(labels, keep, act, cands, weight,
                                                                                                           sep[0], claims)
        win = [r["winner"] for r in picks]
        status = np.array([_lib.OK if w >= 0 else _lib.NO_QUALIFYING_LEAF for w in win], dtype=np.int32)
        out = (status, np.array([r["cost"] for r in picks], dtype=np.float64).reshape(-1, 4), np.array(win, dtype=np.int64),
               [paths[g * K + w] if w >= 0 else np.zeros((0, 7)) for g, w in enumerate(win)], [r["claimed"] for r in picks])
        return out if sep is None else out + ([r["conflicts"] for r in picks],)

    def _replan_round_best_of(self, act, K, streams, last, all_habitats, mtt, keep, weight, max_iter, sets=None):
        """one round with K trees per active AUV: the batch's episodes i*K .. i*K+K-1 are AUV act[i]'s members; the winners are
        chosen on the device and only their courses are copied.  Returns as _replan_round, tree = the winning member."""
        seed_arg = np.array([streams[e].getrandbits(63) for e in act for _ in range(K)], dtype=np.uint64)
        init_objs = [_Init(last[e]) for e in act for _ in range(K)]
        self._explore_summaries(init_objs, all_habitats, 5, 2, True, np.repeat(mtt, K), True, weight, max_iter, seed_arg,
                                [keep[e] for e in act for _ in range(K)], summaries=False,
                                shark_set=None if sets is None else np.repeat(sets, K))
        best = self._ctx.rrt_group_best(np.arange(len(act) + 1, dtype=np.int64) * K)
        bad = best["status"] < 0
        if bad.any():
            i = int(np.argmax(bad))
            raise _lib.AuvpError(int(best[i]["status"]), "a tree of AUV %d failed on the device (status %d)" % (act[i], int(best[i]["status"])))
        tree = np.where(best["winner"] >= 0, best["winner"] - np.arange(len(act)) * K, -1)
        return best["status"], best["cost"], tree, self._ctx.group_paths(best)

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

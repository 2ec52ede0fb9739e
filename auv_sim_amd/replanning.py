"""Fleet replanning: RRT.replanning_batch and RRT.replanning_session (rrt_dubins.py keeps the two thin methods and their
docstrings, and re-exports every name defined here).

One loop -- ReplanSession.round: the active set, the horizon clip, max_traj_time, the round seeds, the status check, "no winner
stops planning", the log -- over one of two round back ends, one result builder (replan_results), and the pure definitions the
device kernels are tested against (team_fold, rescore, team_pick_claims, course_ticks, first_bucket_commit, ...).

A round back end is made from the session; round(act, mtt, seeds) explores from the session's state (act: the active AUVs,
mtt [A] their horizons, seeds [A * K] the round seeds in member order), chooses and commits, and returns one record per active
AUV in _lib.REPLAN_RECORD_DTYPE -- last, keep, winner (the winning episode g * K + tree of the round's batch, -1: none),
n_committed, cost, claimed, conflicts, status --; rows(done) gives {e: [n,7]}, the rows the AUVs `done` committed, in round order.
DeviceRounds commits on the device and keeps the rows in HBM; HostRounds commits with the definitions of this file."""
import math
import random

import numpy as np

from . import _lib
from .motion_plan_state import Motion_plan_state


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


def _team_pick(labels, keep, active, cands, weights, claims, d):
    """the one selection rule behind team_pick_claims (claims, d None: no tick tables, no conflicts key) and team_pick_separated
    (d the distance).  Every group gets rrt_group_best's fold over cost[0].  Every team of two or more: claimed = 0 and the
    trail is empty; its members that are in `active`, in ascending AUV index: a candidate's score is rescore's under
    keep[m] & ~claimed (claims) or its own cost; it is eligible iff score < inf; n is tick_conflicts of its table against the
    trail (0 without d); the smallest (n, score) wins, the lowest tree among equals."""
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
        if d is not None:
            out[-1]["conflicts"] = 0
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
                n = 0 if d is None else tick_conflicts(c["ticks"][0], c["ticks"][1], trail, d)
                if win < 0 or n < best_n or (n == best_n and s[0] < best):
                    best, best_n, win, cost, vis_w = s[0], n, k, s, vis
            out[g].update(winner=win, cost=cost, claimed=claimed)
            if d is not None:
                out[g]["conflicts"] = best_n if win >= 0 else 0
                if win >= 0:
                    trail.append(cands[g][win]["ticks"])
            claimed |= vis_w
    return out


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
    return _team_pick(labels, keep, active, cands, weights, True, None)


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
    return _team_pick(labels, keep, active, cands, weights, claims, d)


def separation_args(team_separation, separation_tick, separation_ticks, labels, span):
    """replanning_batch's team_separation keywords checked without a device: (d, tick, W), or None with the option off.
    span: plan_time_budget + replan_time_interval, the part of a course a round commits (the default window).  The check of
    the horizon's end against the tick is replan_args' own."""
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


def _no_bucket(max_traj_time, round_span):
    return ValueError("max_traj_time %r holds no shark-interval bucket of %r" % (max_traj_time, round_span))


def first_bucket_commit(course_t, course_xy, t0, max_traj_time, round_span, keep, habitats_xys):
    """One round of replanning's host step (rrt_dubins.py:82-87) on arrays: the points of the course that splitPath
    (:590-602) puts into its first bucket, and removeHabitat (:604-610) applied to the episode's habitat list given as the
    bit mask `keep` over the table habitats_xys [H,3] (list order = table order).  Returns (boolean mask of the course's
    points in the first bucket, the new keep).  Raises ValueError where the reference's next(iter(buckets)) would raise:
    the horizon holds no whole bucket."""
    if math.floor(max_traj_time / round_span) < 1:
        raise _no_bucket(max_traj_time, round_span)
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


TREE_FAILED, AUV_FAILED = "a tree of AUV %d failed on the device (status %d)", "AUV %d failed on the device (status %d)"


def raise_bad_status(status, auvs, K=1, fmt=None):
    """AuvpError for the first status < 0 of status [n], naming auvs[i]: "a tree of AUV ..." with K > 1 trees per AUV, the plain
    "AUV ..." with one (fmt: another wording)"""
    bad = status < 0
    if bad.any():
        i = int(np.argmax(bad))
        raise _lib.AuvpError(int(status[i]), (fmt or (TREE_FAILED if K > 1 else AUV_FAILED)) % (auvs[i], int(status[i])))


def replan_args(rrt, starts, habitats, plan_time_budget, replan_time_interval, max_iter, trees_per_auv, shark_of, teams, team_pick,
                team_separation, separation_tick, separation_ticks, seeds, rngs=None, commit="device"):
    """the argument checks replanning_batch and replanning_session share, in one order, before any launch"""
    from .rrt_dubins import _circles, shark_set_indices
    N = len(starts)
    sets = None if shark_of is None else shark_set_indices(shark_of, N, rrt.n_shark_sets)
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
    horizon_end = list(rrt.sharkGrid.keys())[-1][1]
    if sep is not None and not float(horizon_end) / sep[1] < 2.0 ** 31:
        raise ValueError("separation_tick %r: the horizon's end %r is tick 2**31 or later" % (sep[1], horizon_end))
    all_habitats = list(habitats)
    hab = _circles(all_habitats)
    if max_iter is None:
        max_iter = max(1, int(math.ceil(plan_time_budget * rrt.iters_per_second)))
    if commit == "device" and (seeds is None or len(seeds) != N):
        raise ValueError("AUV 0 has neither a seed nor a generator")
    return dict(all_habitats=all_habitats, hab=hab, horizon_end=horizon_end, round_span=round_span, max_iter=max_iter, seeds=seeds, K=K,
                sets=sets, labels=labels, team_pick=team_pick, sep=sep, rngs=rngs)


def replan_costs(rrt, done, rows, last_t, hab, sets):
    """{e: cost [4]} of the whole trajectories rows[e] of the AUVs `done` against the ORIGINAL habitat list (:192-195), every
    AUV in one launch on the cost-only context (with shark_of: the AUVs grouped by table, one launch per table in use, each
    against its own table); last_t[e]: the time of an AUV that committed nothing"""
    if rrt._cost_ctx is None:
        rrt._cost_ctx = _lib.Context(rrt._ctx.device)
    costs = {}
    if done:
        for g in ([None] if sets is None else sorted(set(int(sets[e]) for e in done))):
            grp = done if g is None else [e for e in done if int(sets[e]) == g]
            rrt._cost_ctx.set_world(None, hab, None, rrt._bins, rrt._cells, rrt._prob if g is None else rrt._set_prob[g])
            out = rrt._cost_ctx.cost_paths([rows[e][:, [0, 1, 4]] for e in grp], [0] * len(grp), [len(rrt._bins)] * len(grp),
                                           [float(rows[e][-1, 4]) if len(rows[e]) else float(last_t[e]) for e in grp],
                                           [[-3.0, -3.0, -4.0]] * len(grp))
            costs.update({e: out[i] for i, e in enumerate(grp)})
    return costs


def replan_results(starts, all_habitats, rows, log, keep, alive, costs, claims=False, separation=False, as_arrays=False):
    """What replanning_batch returns, from rows {e: [n,7]} (the committed rows of every AUV that is alive), the rounds' log
    (per round: the AUVs that committed, their records, keep and max_traj_time at the round's start, the winning tree), the
    final keep [N] and alive [N], and costs {e: [4]}.  Per AUV None (not alive), [trajectory, {round: [bucket, habitats at that
    round]}, cost, habitats left] or, with as_arrays, the dict of arrays; round_claimed only with `claims`, round_conflicts
    only with `separation`."""
    N, H = len(starts), len(all_habitats)
    # the rounds of every AUV, in round order: one stable sort of all the rounds' records by AUV
    auv = np.concatenate([x[0] for x in log] + [np.zeros(0, np.int64)])
    order = np.argsort(auv, kind="stable")
    r_rec = np.concatenate([x[1] for x in log] + [np.zeros(0, _lib.REPLAN_RECORD_DTYPE)])[order]
    r_keep = np.concatenate([x[2] for x in log] + [np.zeros(0, np.uint64)])[order]
    r_mtt = np.concatenate([x[3] for x in log] + [np.zeros(0)])[order]
    r_tree = np.concatenate([x[4] for x in log] + [np.zeros(0, np.int64)])[order].astype(np.int64)
    first = np.searchsorted(auv[order], np.arange(N + 1))

    def listed(mask):
        return [all_habitats[h] for h in range(H) if (int(mask) >> h) & 1]

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
            if claims:
                res[-1]["round_claimed"] = r_rec["claimed"][a:b].astype(np.uint64)
            if separation:
                res[-1]["round_conflicts"] = r_rec["conflicts"][a:b].astype(np.int64)
            continue
        # objects: each round's first row is the previous round's last object (the start object in round 1), the rest are new
        traj, rounds, prev, at = [], {}, starts[e], 0
        for k, n in enumerate(lens):
            objs = [prev] + [Motion_plan_state(float(r[0]), float(r[1]), theta=float(r[2]), v=float(r[3]), traj_time_stamp=float(r[4]),
                                               plan_time_stamp=float(r[5]), length=float(r[6])) for r in rows[e][at + 1:at + n]]
            if n == 0:
                objs = []
            at += int(n)
            traj.extend(objs)
            rounds[k + 1] = [objs, listed(r_keep[a + k])]
            if objs:
                prev = objs[-1]
        c = costs[e]
        res.append([traj, rounds, [float(c[0]), [float(c[1]), float(c[2]), float(c[3])]], listed(keep[e])])
    return res


class _Rounds:
    """what the round back ends share: the fleet's habitat table on the context and the round's exploring launch"""

    def __init__(self, s):
        self.s = s
        s.rrt._ctx.set_habitats(s._hab)  # (the whole list: every episode's own list is its keep mask over this table)

    def explore(self, act, mtt, seed_arg, summaries=False):
        """K trees per active AUV: the batch's episodes g*K .. g*K+K-1 are AUV act[g]'s, each from its committed state with its
        horizon, list and shark table.  The summaries (statuses unchecked), or None: they stay in HBM."""
        s, rrt, K = self.s, self.s.rrt, self.s._K
        return rrt._ctx.rrt_explore_batch(np.repeat(s._last[act][:, [0, 1, 2, 4, 5, 6]], K, axis=0), seed_arg, s._max_iter, mode="timebin",
                                          freq=rrt.freq, bin_interval=5, v=2, max_traj_time=np.repeat(mtt, K), weights=s._weight,
                                          dist_to_end=rrt.dist_to_end, diff_max=rrt.diff_max, min_dist=0.5,
                                          max_plan_time=float(s._max_iter),  # virtual clock: 1 tick per iteration
                                          habitat_keep=np.repeat(s._keep[act], K), summaries=summaries,
                                          shark_set=None if s._sets is None else np.repeat(s._sets[act], K))


class DeviceRounds(_Rounds):
    """commit="device": the winners are chosen (rrt_group_best, or the team kernels) and committed (rrt_commit_kernel, then
    replan_team_kernel) on the device; the fleet's state and the committed rows stay in HBM until rows()"""

    def __init__(self, s):
        _Rounds.__init__(self, s)
        ctx = s.rrt._ctx
        ctx.replan_begin(s._last, s._keep)
        if s._labels is not None:
            ctx.replan_set_teams(s._labels)
        # (a fleet without a team of two or more: everybody gets rrt_group_best's record, which is what it runs)
        self.pick = (s._team_pick is not None or s._sep is not None) and len(team_csr(s._labels)[0]) > 1

    def round(self, act, mtt, seeds):
        s, ctx, K = self.s, self.s.rrt._ctx, self.s._K
        self.explore(act, mtt, seeds)
        if self.pick and s._sep is not None:
            best = ctx.replan_team_pick_apart(act, K, s._team_pick is not None, *s._sep)
        else:
            best = ctx.replan_team_pick(act, K) if self.pick else ctx.rrt_group_best(np.arange(len(act) + 1, dtype=np.int64) * K)
        raise_bad_status(best["status"], act, K)
        rec = ctx.replan_commit(act, s.round_span)
        if not self.pick:  # (nobody wrote the two fields)
            rec["claimed"], rec["conflicts"] = 0, 0
        return rec

    def rows(self, done):
        row_off, rows_all = self.s.rrt._ctx.replan_traj()
        return {e: rows_all[row_off[e]:row_off[e + 1]] for e in done}

    def tails(self, n):
        row_off, rows_all = self.s.rrt._ctx.replan_traj()
        return [rows_all[row_off[e + 1] - n[e]:row_off[e + 1]].copy() for e in range(len(n))]


class HostRounds(_Rounds):
    """commit="host": the winners' courses come to the host -- every candidate's with team_pick or team_separation, where the
    definitions of this file choose --, first_bucket_commit and team_fold commit them, and the committed rows stay here.
    gens[e], a random.Random, stands for AUV e's seeds (one tree per AUV): every round continues it as exploring continues the
    global stream, and advances it by what the device drew."""

    def __init__(self, s):
        _Rounds.__init__(self, s)
        self.committed = [[] for _ in s._starts]

    def round(self, act, mtt, seeds):
        from .rrt_dubins import _mt_state_of
        s, ctx, K, sep = self.s, self.s.rrt._ctx, self.s._K, self.s._sep
        claims, pick = s._team_pick is not None, s._team_pick is not None or s._sep is not None
        gens = [s._gens[e] for e in act]
        continued = any(g is not None for g in gens)
        if continued:
            st = [_mt_state_of((g if g is not None else random.Random(int(x))).getstate()) for g, x in zip(gens, seeds)]
            seeds = (np.stack([w for w, _ in st]), np.array([i for _, i in st], dtype=np.int32))
        summ = self.explore(act, mtt, seeds, summaries=pick or continued)
        if continued:
            for g, n in zip(gens, summ["n_draw32"]):
                if g is not None and int(n):
                    g.getrandbits(32 * int(n))  # what exploring does to the global stream
        if summ is not None:
            raise_bad_status(summ["status"], np.repeat(act, K), K)
        rec = np.zeros(len(act), dtype=_lib.REPLAN_RECORD_DTYPE)
        if pick:
            paths = ctx.paths(summ)
            cands = []
            for g, e in enumerate(act):
                row = []
                for k in range(K):
                    c, p = summ[g * K + k], paths[g * K + k]
                    if c["best_leaf"] < 0 or len(p) == 0:
                        row.append(None)
                        continue
                    p = p.copy()
                    p[0] = s._last[e]  # (row 0 is the committed state, as in the commit rule)
                    row.append(dict(cost=[float(x) for x in c["best_cost"]], leaf_time=float(p[-1, 4])))
                    if claims:
                        row[-1]["words"] = course_habitat_words(p[:, :2], p[:, 4], s.rrt._bins, 0, len(s.rrt._bins), s._hab)
                    if sep is not None:
                        row[-1]["ticks"] = course_ticks(p[:, 4], p[:, :2], sep[1], sep[2])
                cands.append(row)
            picks = _team_pick(s._labels, s._keep, act, cands, s._weight, claims, None if sep is None else sep[0])
            for g, r in enumerate(picks):
                rec[g]["winner"] = g * K + r["winner"] if r["winner"] >= 0 else -1
                rec[g]["cost"], rec[g]["claimed"], rec[g]["conflicts"] = r["cost"], r["claimed"], r.get("conflicts", 0)
            courses = [paths[w] if w >= 0 else None for w in rec["winner"]]
        else:
            best = ctx.rrt_group_best(np.arange(len(act) + 1, dtype=np.int64) * K)
            raise_bad_status(best["status"], act, K)
            rec["winner"], rec["cost"] = best["winner"], best["cost"]
            courses = ctx.group_paths(best)
        rec["last"], rec["keep"] = s._last[act], s._keep[act]
        for g, e in enumerate(act):
            if rec[g]["winner"] < 0:
                rec[g]["status"] = _lib.NO_QUALIFYING_LEAF
                continue
            p = courses[g].copy()
            p[0] = s._last[e]  # the course starts at the committed state itself (exploring returns the caller's object)
            sel, rec[g]["keep"] = first_bucket_commit(p[:, 4], p[:, :2], s._last[e, 4], float(mtt[g]), s.round_span, int(s._keep[e]), s._hab)
            bucket = p[sel]
            self.committed[e].append(bucket)
            rec[g]["path_len"], rec[g]["n_committed"] = len(p), len(bucket)
            if len(bucket):
                rec[g]["last"] = bucket[-1]
        if s._labels is not None:  # (once all of the round's commits are done; a stopped member's list is the team's of its last round)
            keep = s._keep.copy()
            keep[act] = rec["keep"]
            rec["keep"] = np.array(team_fold(keep, s._labels), dtype=np.uint64)[act]
        return rec

    def rows(self, done):
        return {e: np.concatenate(self.committed[e] + [np.zeros((0, 7))]) for e in done}

    def tails(self, n):
        return [self.committed[e][-1].copy() if n[e] else np.zeros((0, 7)) for e in range(len(n))]


class ReplanSession:
    """RRT.replanning_batch as a resumable object (RRT.replanning_session gives the commit="device" one).  The host keeps [N]
    mirrors of the fleet's state -- last [N,7], keep [N] -- from the round records; with DeviceRounds the state itself and the
    trajectory log live on the planner's context in HBM.  round() is one iteration of the loop; set_shark_grids() between two
    rounds swaps the F shark tables and touches nothing else; finish() collects the trajectories once and closes the session.
    While it is open the session owns the planner's context: every other call on the RRT that would prepare a batch, change the
    world or the tables, or open a second session raises RuntimeError and leaves the session as it was."""

    def __init__(self, rrt, starts, traj_time_length, weight, all_habitats, hab, horizon_end, round_span, max_iter, seeds, K, sets,
                 labels=None, team_pick=None, sep=None, rngs=None, back_end=DeviceRounds):
        N, H = len(starts), len(all_habitats)
        self._gens = [None if rngs is None else rngs[e] for e in range(N)]  # rngs[e]: the global stream of a sequential call
        self._streams = []  # seeds[e]: replanning's private stream, one 63-bit seed per round and tree
        for e in range(N):
            if self._gens[e] is None and (seeds is None or seeds[e] is None):
                raise ValueError("AUV %d has neither a seed nor a generator" % e)
            # (an AUV with a generator: a stream whose seeds nobody reads, so that the round draws without looking)
            self._streams.append(random.Random(seeds[e] if self._gens[e] is None else 0))
        if getattr(rrt, "_session", None) is not None:
            raise RuntimeError("replanning_session: a replanning session is open on this RRT (finish() it first)")
        self.rrt, self.inside, self.closed = rrt, False, False
        self._starts, self._all_habitats, self._hab = list(starts), all_habitats, hab
        self._horizon_end, self.round_span, self._weight, self._max_iter = horizon_end, round_span, weight, int(max_iter)
        self._K, self._sets, self._labels, self._team_pick, self._sep = K, sets, labels, team_pick, sep
        self._last = np.array([[float(m.x), float(m.y), float(m.theta), float(getattr(m, "v", 0.0) or 0.0), float(m.traj_time_stamp),
                                float(m.plan_time_stamp), float(m.length)] for m in starts], dtype=np.float64).reshape(N, 7)
        self._keep = np.full(N, (1 << H) - 1, dtype=np.uint64)
        self._ttl = np.full(N, float(traj_time_length))
        self._alive = np.ones(N, dtype=bool)
        self._back = back_end(self)
        rrt._batch = None  # (rerank follows an exploring_batch only)
        self._log = []  # per round: (AUVs that committed, their records, keep and max_traj_time at that round, winning tree)
        self.round_index = 0
        rrt._session = rrt._ctx.session = self

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

    def last_segments(self):
        """[N] arrays [n,7]: the rows every AUV committed in the most recent round, row 0 the state it had before it -- empty for
        an AUV that did not plan in that round or found no winner, and for everybody before the first round.  With
        commit="device" this downloads the trajectories (replan_traj): for checks, not for a loop that is to stay on the device."""
        self._open("last_segments")
        n = np.zeros(len(self._starts), dtype=np.int64)
        if self._log:
            n[self._log[-1][0]] = self._log[-1][1]["n_committed"]
        with self._Own(self):
            return self._back.tails(n)

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
        if self._sets is not None:
            n = 0 if forecast is None else (len(forecast.prob) if hasattr(forecast, "prob") else len(forecast))
            if n <= int(self._sets.max()):
                raise ValueError("%d tables do not cover the session's shark_of (up to %d)" % (n, int(self._sets.max())))
        with self._Own(self):
            self.rrt.set_shark_grids(forecast, first_bin)

    def round(self):
        """One round: the active AUVs' round seeds, one exploring launch, the winners (or the team selection), the commit.
        Returns a dict of [A] arrays -- auv (the active indices), last [A,7], keep, winner (the winning tree of the
        AUV's K, -1: no qualifying leaf; that AUV stops planning), cost [A,4] -- or None once no AUV is active."""
        self._open("round")
        act = self.active()
        if len(act) == 0:
            return None
        last, keep, ttl, K = self._last, self._keep, self._ttl, self._K
        with self._Own(self):
            t_now = last[act, 4]
            clip = ttl[act] + t_now > self._horizon_end  # stays clipped for the later rounds too (:76-77)
            ttl[act[clip]] = self._horizon_end - t_now[clip]
            mtt = ttl[act] + t_now
            short = np.floor(mtt / self.round_span) < 1  # (first_bucket_commit's ValueError, before the launch)
            if short.any():
                raise _no_bucket(float(mtt[np.argmax(short)]), self.round_span)
            # every AUV's K round seeds from its own stream, in member order
            seeds = np.array([self._streams[e].getrandbits(63) for e in act for _ in range(K)], dtype=np.uint64)
            rec = self._back.round(act, mtt, seeds)
            raise_bad_status(rec["status"], act, fmt="AUV %d: the commit step failed on the device (status %d)")
            won = rec["winner"] >= 0
            self._alive[act[~won]] = False  # no qualifying leaf: the sequential call would raise TypeError
            tree = rec["winner"] - np.arange(len(act)) * K
            self._log.append((act[won], rec[won], keep[act][won], mtt[won], tree[won]))
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
                keep = self._keep
                if self._labels is not None:
                    # a member that stopped planning holds the team's list of its last round: lists only shrink, so the AND
                    # over the host's copies is the team's final one
                    keep = np.array(team_fold(keep, self._labels), dtype=np.uint64)
                done = [int(e) for e in np.flatnonzero(self._alive)]
                rows = self._back.rows(done)
                costs = replan_costs(self.rrt, done, rows, self._last[:, 4], self._hab, self._sets)
                return replan_results(self._starts, self._all_habitats, rows, self._log, keep, self._alive, costs,
                                      self._team_pick is not None, self._sep is not None, as_arrays)
        finally:
            self.close()

    def run(self, as_arrays=False):
        """the whole call: rounds until nobody plans any more, then finish()"""
        try:
            while self.round() is not None:
                pass
            return self.finish(as_arrays)
        finally:
            self.close()

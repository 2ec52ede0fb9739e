"""Probability sets: every episode of a batch ranks its leaves against its own shark-occupancy table (auvp_world_set_prob_sets,
auvp_rrt_set_episode_grids, rrt_leaf_grid_kernel), a finished batch is ranked again under another assignment (auvp_rrt_rerank),
and a forecast's tables go to a planner without leaving HBM (auvp_sf_prob_dev).  Checked bit for bit against the CPU checker on a
world holding the episode's table, against the plain per-episode-limits batch where all tables are equal, and -- the planner API
-- against planners built with the one table.  No tolerance appears in this file."""
import ctypes as C
import math
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
ARG, STATE = -1, -4
N_ITER, HORIZON = 350, 200.0
FIELDS = ("status", "n_nodes", "n_points", "n_leaves", "best_leaf", "best_path_len", "iters_run", "best_cost", "best_length",
          "rng_after", "leaf_elems", "n_draw32")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).tobytes()


def _world():
    from auv_sim_amd import synth
    return synth.make_world(seed=12, n_obstacles=64, n_habitats=9)


def _tables(P):
    """the world's own table, the same reversed along the cells, one of mixed signs, all zeros (every shark term 0: ties), and
    one whose absmax is 40 times the first's"""
    return np.stack([P, P[:, ::-1], (P - P.mean()) * 3, np.zeros_like(P), np.random.default_rng(5).uniform(0, .3, P.shape) * 40])


def _context(w, habitats=True, prob=None):
    from auv_sim_amd import _lib
    ctx = _lib.Context(0)
    ctx.set_world(w["obstacles"], w["habitats"] if habitats else None, w["polygon"], w["bins"], w["cells"],
                  w["prob"] if prob is None else prob)
    return ctx


def _same_summaries(a, b, fields=FIELDS):
    for e in range(len(a)):
        for f in fields:
            assert _bits(a[e][f]) == _bits(b[e][f]) if a[e][f].dtype.kind == "f" else np.array_equal(a[e][f], b[e][f]), (e, f)


def _same_paths(a, b):
    assert len(a) == len(b)
    for e in range(len(a)):
        assert a[e].shape == b[e].shape and _bits(a[e]) == _bits(b[e]), e


@pytest.fixture(scope="module")
def case(orc):
    """E = 9 episodes (two full leaf workgroups of four wavefronts and a partial one), five tables, set_of = e % 5; the checker's
    result of every episode under its own table and under table 0, computed once"""
    w = _world()
    tabs = _tables(w["prob"])
    E = 9
    init = np.zeros((E, 6))
    init[:, 0], init[:, 1] = w["start"]
    seeds = np.array([11 + 7 * e for e in range(E)], dtype=np.uint64)
    set_of = np.arange(E, dtype=np.int32) % 5

    def check(e, g, **kw):
        wa = orc.WorldArrays(w["obstacles"], kw.pop("habitats", w["habitats"]), w["polygon"], w["bins"], w["cells"], tabs[g])
        return orc.rrt_explore(wa, int(seeds[e]), N_ITER, init=init[e], max_traj_time=kw.pop("mtt", HORIZON), kind="portable")
    own = [check(e, int(set_of[e])) for e in range(E)]
    zero = [check(e, 0) for e in range(E)]
    return dict(w=w, tabs=tabs, E=E, init=init, seeds=seeds, set_of=set_of, own=own, zero=zero, check=check)


def _against_checker(summ, paths, refs, cost_bitwise=True):
    for e, r in enumerate(refs):
        s = summ[e]
        assert (int(s["status"]), int(s["n_nodes"]), int(s["n_points"]), int(s["n_leaves"])) == \
               (r["status"], r["n_nodes"], r["n_points"], r["n_leaves"]), e
        assert int(s["best_leaf"]) == r["best_leaf"], (e, int(s["best_leaf"]), r["best_leaf"])
        if cost_bitwise:
            assert _bits(s["best_cost"]) == _bits(r["best_cost"]), (e, s["best_cost"], r["best_cost"])
        else:
            assert np.array_equal(np.array(s["best_cost"]), r["best_cost"]), (e, s["best_cost"], r["best_cost"])
        assert int(s["n_draw32"]) == r["n_draw32"] and s["rng_after"] == r["rng_after"], e
        if r["best_leaf"] >= 0:
            assert paths[e].shape == r["path"].shape and _bits(paths[e]) == _bits(r["path"]), e


def test_each_episode_equals_checker_on_its_own_table(case):
    """every episode == the checker on a world holding its table: status, node / leaf counts, best leaf, best cost bit for bit
    and the path.  The tables were chosen so that the choice matters: at least three episodes have another best leaf under
    their own table than under table 0 (asserted from the checker alone); what grows the tree does not depend on the table."""
    c = case
    own, zero = c["own"], c["zero"]
    # the checker's facts first
    differ = [e for e in range(c["E"]) if own[e]["best_leaf"] != zero[e]["best_leaf"]]
    assert len(differ) >= 3, differ
    assert all(36 <= r["n_leaves"] <= 85 for r in own), [r["n_leaves"] for r in own]
    for a, b in zip(own, zero):
        assert (a["n_nodes"], a["n_leaves"], a["n_draw32"], a["rng_after"]) == (b["n_nodes"], b["n_leaves"], b["n_draw32"], b["rng_after"])
    ctx = _context(c["w"])
    ctx.set_prob_sets(c["tabs"])
    summ = ctx.rrt_explore_batch(c["init"], c["seeds"], N_ITER, max_traj_time=HORIZON, shark_set=c["set_of"])
    assert ctx.last_rrt_kernel() == "rrt_explore_lim_kernel"
    _against_checker(summ, ctx.paths(summ), own)
    # the same batch against the world's table alone: the trees are the same, the leaf differs where the checker's does
    base = ctx.rrt_explore_batch(c["init"], c["seeds"], N_ITER, max_traj_time=np.full(c["E"], HORIZON))
    _same_summaries(summ, base, ("n_nodes", "n_points", "n_leaves", "n_draw32", "rng_after", "iters_run"))
    assert [e for e in range(c["E"]) if int(summ[e]["best_leaf"]) != int(base[e]["best_leaf"])] == differ


def test_limits_survive_a_table_per_episode(case):
    """mixed horizons {150, 200} and keep masks with a table per episode: each episode == the checker on the sub-world of its
    kept habitats holding its table, with its own horizon -- compared as test_limits_kernel_equals_checker_per_episode compares
    (np.array_equal on the cost: a leaf without a habitat hit has cost[1] = w2 * 0 = -0.0 in every leaf kernel, the checker's
    empty sum is +0.0; that is the shared body's, not the table's)"""
    c = case
    w, E = c["w"], c["E"]
    H = len(w["habitats"])
    mtt = np.array([150.0 if e % 2 else 200.0 for e in range(E)])
    keep = [0, (1 << H) - 1, 1, 1 << (H - 1), 0b101010101, 0b010101010, 0b000111000, 0b111000111, 0b100000001]
    refs = [c["check"](e, int(c["set_of"][e]), mtt=float(mtt[e]),
                       habitats=w["habitats"][[h for h in range(H) if (keep[e] >> h) & 1]].reshape(-1, 3)) for e in range(E)]
    ctx = _context(w)
    ctx.set_prob_sets(c["tabs"])
    summ = ctx.rrt_explore_batch(c["init"], c["seeds"], N_ITER, max_traj_time=mtt, habitat_keep=np.array(keep, dtype=np.uint64),
                                 shark_set=c["set_of"])
    _against_checker(summ, ctx.paths(summ), refs, cost_bitwise=False)
    assert any(r["best_leaf"] >= 0 for r in refs)


def _np_stats(t):
    """auvp_world_set's rule for its one table"""
    a = np.abs(t)
    nan = bool(np.isnan(t).any())
    return (np.nan if nan else float(a.max())), int(not nan and not ((t > 0).any() and (t < 0).any()))


def test_set_statistics_equal_numpy(case):
    """absmax (bitwise) and one_sign of every set as the device computed them == numpy: the five tables, one holding a nan,
    one all negative, one of negative zeros, one whose largest entry is the very last"""
    P = case["w"]["prob"]
    nan_t = P.copy()
    nan_t[3, 17] = np.nan
    last = P.copy()
    last[-1, -1] = 7.5
    tabs = np.concatenate([case["tabs"], np.stack([nan_t, -P, np.full_like(P, -0.0), last])])
    ctx = _context(case["w"])
    ctx.set_prob_sets(tabs)
    absmax, one_sign = ctx.prob_set_stats()
    want = [_np_stats(t) for t in tabs]
    assert _bits(absmax) == _bits([a for a, _ in want]), (absmax, want)
    assert one_sign.tolist() == [s for _, s in want]
    assert one_sign.tolist() == [1, 1, 0, 1, 1, 0, 1, 1, 1] and np.isnan(absmax[5]) and absmax[8] == 7.5
    assert absmax[4] > 39 * absmax[0]


def test_equal_sets_equal_the_plain_limits_batch(case):
    """three copies of the world's table, uploaded from the host and through a device pointer, mixed set_of, mixed limits:
    summaries (leaf_elems included) and best paths bit-identical to the batch without an assignment"""
    import torch
    c = case
    w, E = c["w"], c["E"]
    H = len(w["habitats"])
    mtt = np.array([150.0 if e % 3 else 200.0 for e in range(E)])
    keep = np.array([(1 << H) - 1 if e % 2 else 0b101010101 for e in range(E)], dtype=np.uint64)
    ctx = _context(w)
    plain = ctx.rrt_explore_batch(c["init"], c["seeds"], N_ITER, max_traj_time=mtt, habitat_keep=keep)
    plain_paths = ctx.paths(plain)
    copies = np.stack([w["prob"]] * 3)
    set_of = np.array([2, 0, 1, 1, 2, 0, 0, 2, 1], dtype=np.int32)
    ctx.set_prob_sets(copies)
    got = ctx.rrt_explore_batch(c["init"], c["seeds"], N_ITER, max_traj_time=mtt, habitat_keep=keep, shark_set=set_of)
    _same_summaries(got, plain)
    _same_paths(ctx.paths(got), plain_paths)
    dev = torch.from_numpy(copies).to("cuda:0")
    torch.cuda.synchronize()
    ctx.set_prob_sets(n_sets=3, prob_dev=dev.data_ptr())
    del dev  # (copied: the handle owns its buffer)
    a, s = ctx.prob_set_stats()
    assert _bits(a) == _bits([np.abs(w["prob"]).max()] * 3) and s.tolist() == [1, 1, 1]
    got = ctx.rrt_explore_batch(c["init"], c["seeds"], N_ITER, max_traj_time=mtt, habitat_keep=keep, shark_set=set_of[::-1].copy())
    _same_summaries(got, plain)
    _same_paths(ctx.paths(got), plain_paths)


def test_rerank_equals_a_fresh_run(case):
    """grow with assignment A, rerank to B: best leaf, best cost, paths and the group winners over groups of 3 equal a fresh
    prepare + run with B; rerank back to A equals the first run; rerank without an assignment equals the world's table"""
    c = case
    E = c["E"]
    A = c["set_of"]
    B = np.array([(3 * e + 1) % 5 for e in range(E)], dtype=np.int32)
    off = np.arange(0, E + 1, 3, dtype=np.int32)
    fresh = _context(c["w"])
    fresh.set_prob_sets(c["tabs"])

    def run(ctx, sets):
        s = ctx.rrt_explore_batch(c["init"], c["seeds"], N_ITER, max_traj_time=HORIZON, shark_set=sets)
        return s, ctx.paths(s), ctx.rrt_group_best(off)
    want_b = run(fresh, B)
    ctx = _context(c["w"])
    ctx.set_prob_sets(c["tabs"])
    first = run(ctx, A)
    assert [int(x) for x in first[0]["best_leaf"]] != [int(x) for x in want_b[0]["best_leaf"]]  # (B ranks differently)

    def reranked(sets):
        ctx.rrt_set_episode_grids(sets)
        s = ctx.rrt_rerank()
        best = ctx.rrt_group_best(off)
        return s, ctx.paths(s), best, ctx.group_paths(best)
    got = reranked(B)
    _same_summaries(got[0], want_b[0])
    _same_paths(got[1], want_b[1])
    assert got[2].tobytes() == want_b[2].tobytes()
    _same_paths(got[3], fresh.group_paths(want_b[2]))
    back = reranked(A)
    _same_summaries(back[0], first[0])
    _same_paths(back[1], first[1])
    assert back[2].tobytes() == first[2].tobytes()
    world = reranked(None)
    _same_summaries(world[0], fresh.rrt_explore_batch(c["init"], c["seeds"], N_ITER, max_traj_time=np.full(E, HORIZON)))


# ---- the planner API on the g13 world ----
class _Cell:
    def __init__(self, b):
        self.bounds = tuple(float(v) for v in b)


class _Poly:
    class _Ext:
        def __init__(self, pts):
            self.coords = list(pts) + [pts[0]]

    def __init__(self, pts):
        self.exterior = _Poly._Ext([tuple(p) for p in pts])


def _free_starts(rng, g, n):
    poly, obst = g["polygon"], g["obstacles"]
    x0, y0, x1, y1 = poly[:, 0].min(), poly[:, 1].min(), poly[:, 0].max(), poly[:, 1].max()
    out = []
    while len(out) < n:
        x, y = rng.uniform(x0 + 10, x1 - 10), rng.uniform(y0 + 10, y1 - 10)
        if all(math.hypot(x - o[0], y - o[1]) > o[2] + 3.0 for o in obst):
            out.append((x, y))
    return out


def _rows(objs):
    return np.array([[p.x, p.y, p.theta, p.v, p.traj_time_stamp, p.plan_time_stamp, p.length] for p in objs]).reshape(-1, 7)


def _same_result(have, want, tag):
    if want is None:
        assert have is None, tag
        return
    assert _bits(_rows(have["path"][0])) == _bits(_rows(want["path"][0])), tag
    assert list(have["path"][1].keys()) == list(want["path"][1].keys()), tag
    for k in want["path"][1]:
        assert _bits(_rows(have["path"][1][k])) == _bits(_rows(want["path"][1][k])), (tag, k)
    assert have["cost"] == want["cost"] and have["path length"] == want["path length"], tag
    assert have.get("tree") == want.get("tree"), tag


@pytest.fixture(scope="module")
def g13():
    """the golden's world with two tables, its own and the cell-reversed copy: a planner holding both as sets, and one planner
    built with each"""
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    from auv_sim_amd.rrt_dubins import RRT
    g = np.load(os.path.join(GOLDEN, "g13_replan_a.npz"))
    obstacles = [MPS(o[0], o[1], size=o[2]) for o in g["obstacles"].tolist()]
    habitats = [MPS(h[0], h[1], size=h[2]) for h in g["habitats"].tolist()]
    cell_list = [_Cell(c) for c in g["cells"].tolist()]
    poly = _Poly(g["polygon"].tolist())

    def grid(prob):
        return {(int(b[0]), int(b[1])): {cell_list[i].bounds: p for i, p in enumerate(prob[t].tolist())}
                for t, b in enumerate(g["bins"].tolist())}
    grids = [grid(g["prob"]), grid(g["prob"][:, ::-1])]
    fleet = RRT(poly, obstacles, grids[0], cell_list)
    fleet.set_shark_grids(grids)
    single = [RRT(poly, obstacles, gr, cell_list) for gr in grids]
    return g, fleet, single, habitats, (poly, obstacles, cell_list, grids)


def test_exploring_best_of_with_a_table_per_auv(g13):
    """3 AUVs x 3 trees, shark_of over 2 tables: every entry == exploring_best_of of a planner built with that one table; so is
    exploring_batch with shark_of, and rerank under the swapped assignment"""
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    g, fleet, single, habitats, _ = g13
    N, K, n_iter = 3, 3, 400
    initials = [MPS(x, y) for x, y in _free_starts(random.Random(7), g, N)]
    seeds = [[100 * i + m + 1 for m in range(K)] for i in range(N)]
    args = (habitats, 0.5, 5, 2, 100.0, True, 2.0, 150.0, True, [-3, -3, -4])
    shark_of = [1, 0, 1]
    got = fleet.exploring_best_of(initials, *args, max_iter=n_iter, seeds=seeds, shark_of=shark_of)
    some = 0
    for i in range(N):
        want = single[shark_of[i]].exploring_best_of([initials[i]], *args, max_iter=n_iter, seeds=[seeds[i]])[0]
        _same_result(got[i], want, i)
        some += want is not None
    assert some > 0
    flat = [s[0] for s in seeds]
    got = fleet.exploring_batch(initials, *args, max_iter=n_iter, seeds=flat, shark_of=shark_of)
    swapped = fleet.rerank([1 - s for s in shark_of])
    for i in range(N):
        _same_result(got[i], single[shark_of[i]].exploring_batch([initials[i]], *args, max_iter=n_iter, seeds=[flat[i]])[0], i)
        _same_result(swapped[i], single[1 - shark_of[i]].exploring_batch([initials[i]], *args, max_iter=n_iter, seeds=[flat[i]])[0], i)
    with pytest.raises(ValueError):
        fleet.exploring_batch(initials, *args[:5], False, *args[6:], max_iter=n_iter, seeds=flat, shark_of=shark_of)  # not time-bin


def test_replanning_batch_with_a_table_per_auv(g13):
    """5 AUVs, 2 tables, seeds only: entry e == the one-AUV replanning_batch of a planner built with its table -- trajectory,
    rounds, final cost (taken against its own table) and the habitats left"""
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    g, fleet, single, habitats, _ = g13
    N, budget, length, interval, n_iter = 5, 2.0, 150.0, 98.0, 400
    starts = [MPS(x, y) for x, y in _free_starts(random.Random(5), g, N)]
    seeds = [31 * e + 3 for e in range(N)]
    shark_of = [0, 1, 1, 0, 1]
    batch = fleet.replanning_batch(starts, habitats, budget, length, interval, [-3, -3, -4], max_iter=n_iter, seeds=seeds,
                                   shark_of=shark_of)
    done, costs = 0, set()
    for e in range(N):
        want = single[shark_of[e]].replanning_batch([starts[e]], habitats, budget, length, interval, [-3, -3, -4], max_iter=n_iter,
                                                    seeds=[seeds[e]])[0]
        b = batch[e]
        if want is None:
            assert b is None, e
            continue
        done += 1
        assert _bits(_rows(want[0])) == _bits(_rows(b[0])), e
        assert list(want[1].keys()) == list(b[1].keys()), e
        for k in want[1]:
            assert _bits(_rows(want[1][k][0])) == _bits(_rows(b[1][k][0])), (e, k)
            assert want[1][k][1] == b[1][k][1], (e, k)
        assert want[2] == b[2], (e, want[2], b[2])
        assert want[3] == b[3], e
        costs.add(shark_of[e])
    assert done > 0 and costs == {0, 1}


# ---- the forecast hand-off ----
class _B:
    def __init__(self, *b):
        self.bounds = tuple(float(v) for v in b)


def test_forecast_tables_reach_the_planner_without_leaving_hbm():
    """F = 3 filters from a host [3, 200, 2] array over a 200 m box of 10 m cells (400 listed cells, 21 x 21 grid entries), R = 9;
    a planner whose world has those 400 cells and 10 bins: set_shark_grids(forecast) + exploring_batch(shark_of) == one planner
    per filter built from forecast.shark_grid(f); the sets' statistics == numpy on forecast.prob; a forecast with another R or
    another cell list is refused"""
    from auv_sim_amd import _lib
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    from auv_sim_amd.rrt_dubins import RRT
    from auv_sim_amd.sharkForecast import SharkForecast
    F, R = 3, 9
    boundary = _B(0, 0, 200, 200)
    cells = [_B(10 * c, 10 * r, 10 * c + 10, 10 * r + 10) for r in range(20) for c in range(20)]
    rng = np.random.default_rng(8)
    xy = np.stack([rng.normal(loc=m, scale=30.0, size=(200, 2)) for m in ((60.0, 70.0), (140.0, 120.0), (100.0, 40.0))])
    sf = SharkForecast(boundary, 10, cells, device_context=_lib.Context(0))
    assert (sf.n_row, sf.n_col, len(cells)) == (21, 21, 400)
    fc = sf.run(xy, np.ones((21, 21)), R)
    assert not fc.status.any() and fc.prob.shape == (F, R + 1, 400)
    grids = [fc.shark_grid(f, (0, 20), 20) for f in range(F)]
    poly = _Poly([(0.0, 0.0), (200.0, 0.0), (200.0, 200.0), (0.0, 200.0)])
    orng = random.Random(2)
    obstacles = [MPS(orng.uniform(10, 190), orng.uniform(10, 190), size=orng.uniform(2, 6)) for _ in range(12)]
    obstacles = [o for o in obstacles if math.hypot(o.x - 100, o.y - 100) > 15]
    habitats = [MPS(orng.uniform(20, 180), orng.uniform(20, 180), size=orng.uniform(8, 15)) for _ in range(5)]
    fleet = RRT(poly, obstacles, grids[0], cells)
    calls, upload = [], fleet._ctx.set_prob_sets
    fleet._ctx.set_prob_sets = lambda *a, **k: (calls.append((a, k)), upload(*a, **k))[1]
    fleet.set_shark_grids(fc)
    assert len(calls) == 1 and not calls[0][0] and calls[0][1]["prob_dev"] == sf._ctx.sf_prob_dev()[0]  # device to device
    assert fleet.n_shark_sets == F
    absmax, one_sign = fleet._ctx.prob_set_stats()
    assert _bits(absmax) == _bits([np.abs(fc.prob[f]).max() for f in range(F)]) and one_sign.tolist() == [1] * F
    E = 6
    shark_of = [0, 1, 2, 2, 0, 1]
    initials = [MPS(100.0, 100.0) for _ in range(E)]
    seeds = [50 + 3 * e for e in range(E)]
    args = (habitats, 0.5, 20, 2, 50.0, True, 2.0, 90.0, True, [-3, -3, -4])
    got = fleet.exploring_batch(initials, *args, max_iter=350, seeds=seeds, shark_of=shark_of)
    some = 0
    for f in range(F):
        ids = [e for e in range(E) if shark_of[e] == f]
        want = RRT(poly, obstacles, grids[f], cells).exploring_batch([initials[e] for e in ids], *args, max_iter=350,
                                                                     seeds=[seeds[e] for e in ids])
        for j, e in enumerate(ids):
            _same_result(got[e], want[j], e)
            some += want[j] is not None
    assert some >= 3
    # another R, another cell list
    with pytest.raises(ValueError):
        fleet.set_shark_grids(sf.run(xy, np.ones((21, 21)), R - 1))
    other = cells[:-2] + [cells[-1], cells[-2]]
    with pytest.raises(ValueError):
        fleet.set_shark_grids(SharkForecast(boundary, 10, other, device_context=sf._ctx).run(xy, np.ones((21, 21)), R))
    with pytest.raises(ValueError):
        fleet.set_shark_grids([grids[0], {k: v for k, v in list(grids[1].items())[:-1]}])  # a dict with a bin less
    assert fleet.n_shark_sets == F  # refused calls change nothing


def test_statuses(case):
    """every status the header names for the new entry points; no refused call launches or changes anything"""
    from auv_sim_amd import _lib
    c = case
    w, E = c["w"], c["E"]
    L = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    tabs = np.ascontiguousarray(c["tabs"])

    def sets(ctx, n, host=True, dev=None):
        return L.auvp_world_set_prob_sets(ctx.h, n, tabs.ctypes.data_as(dp) if host else None, dev)

    def assign(ctx, n, idx):
        a = np.ascontiguousarray(idx, dtype=np.int32)
        return L.auvp_rrt_set_episode_grids(ctx.h, n, a.ctypes.data_as(ip))
    bare = _lib.Context(0)
    assert sets(bare, 5) == STATE  # no world
    bare.set_world(w["obstacles"], w["habitats"], w["polygon"])
    assert sets(bare, 5) == STATE  # a world without bins and cells
    assert L.auvp_world_prob_set_stats(bare.h, None, None) == STATE
    assert L.auvp_sf_prob_dev(bare.h, None, None, None, None) == STATE
    assert L.auvp_rrt_rerank(bare.h) == STATE
    ctx = _context(w)
    assert sets(ctx, 0) == ARG and sets(ctx, -1) == ARG
    assert sets(ctx, 5, host=False) == ARG                      # neither pointer
    assert sets(ctx, 5, dev=C.c_void_p(tabs.ctypes.data)) == ARG  # both
    assert L.auvp_world_prob_set_stats(ctx.h, None, None) == STATE
    ctx.rrt_prepare(c["init"], c["seeds"], N_ITER, max_traj_time=np.full(E, HORIZON))
    assert assign(ctx, E, c["set_of"]) == STATE                 # no sets on the handle
    assert sets(ctx, 5) == 0
    assert assign(ctx, E, c["set_of"]) == 0
    assert assign(ctx, E - 1, c["set_of"][:E - 1]) == ARG and assign(ctx, E + 1, list(c["set_of"]) + [0]) == ARG
    bad = c["set_of"].copy()
    bad[E - 1] = 5
    assert assign(ctx, E, bad) == ARG
    bad[E - 1] = -1
    assert assign(ctx, E, bad) == ARG
    assert L.auvp_rrt_rerank(ctx.h) == STATE                    # prepared, nothing has run
    ctx.rrt_run()
    first = ctx.summaries()
    _against_checker(first, ctx.paths(first), c["own"])          # the refused calls left the good assignment in place
    assert L.auvp_rrt_rerank(ctx.h) == 0
    _same_summaries(ctx.summaries(), first)
    assert L.auvp_rrt_set_episode_grids(ctx.h, 0, None) == 0    # NULL clears
    ctx.rrt_run()
    _against_checker(ctx.summaries(), ctx.paths(ctx.summaries()), c["zero"])
    # a plain prepare is no prepare_episodes; any new prepare clears the assignment
    ctx.rrt_prepare(c["init"], c["seeds"], N_ITER, max_traj_time=HORIZON)
    assert assign(ctx, E, c["set_of"]) == STATE
    assert L.auvp_rrt_rerank(ctx.h) == STATE                    # no run since this prepare
    ctx.rrt_prepare(c["init"], c["seeds"], N_ITER, max_traj_time=np.full(E, HORIZON))
    assert assign(ctx, E, c["set_of"]) == 0
    ctx.rrt_prepare(c["init"], c["seeds"], N_ITER, max_traj_time=np.full(E, HORIZON))
    ctx.rrt_run()
    _against_checker(ctx.summaries(), ctx.paths(ctx.summaries()), c["zero"])
    # habitats keep the sets, the world drops them; clearing the sets clears the assignment
    ctx.set_habitats(w["habitats"])
    assert L.auvp_world_prob_set_stats(ctx.h, None, None) == 0
    ctx.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"])
    assert L.auvp_world_prob_set_stats(ctx.h, None, None) == STATE
    ctx.rrt_prepare(c["init"], c["seeds"], N_ITER, max_traj_time=np.full(E, HORIZON))
    assert assign(ctx, E, c["set_of"]) == STATE
    assert sets(ctx, 5) == 0 and assign(ctx, E, c["set_of"]) == 0
    assert L.auvp_world_set_prob_sets(ctx.h, 0, None, None) == 0
    assert L.auvp_world_prob_set_stats(ctx.h, None, None) == STATE
    ctx.rrt_run()
    _against_checker(ctx.summaries(), ctx.paths(ctx.summaries()), c["zero"])
    # the binding
    with pytest.raises(ValueError):
        ctx.set_prob_sets(tabs[:, :-1])
    with pytest.raises(ValueError):
        ctx.rrt_prepare(c["init"], c["seeds"], N_ITER, mode="nn", shark_set=c["set_of"])
    with pytest.raises(_lib.AuvpError) as e:
        ctx.rrt_set_episode_grids(c["set_of"])
    assert e.value.code == STATE

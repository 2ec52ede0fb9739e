"""astar_fixLenSOG against a shark-occupancy table per search instance: auvp_astar_batch_sets / auvp_astar_sets_topn
(csrc/astar_sets_kernels.hip, astar_host.h) and astar_fixLenSOG.astar.set_shark_grids / astar_batch(shark_of=).  Every
comparison is exact: the top-n tables against get_top_n_prob's own loop on Python floats (astar_fixLenSOG.py:516-531), the
searches against the portable CPU checker run on the instance's own table."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests", "experiments"))

ERR_ARG, ERR_STATE = -1, -4
WEIGHTS = (0, 10, 10, 100)
WORLD_KEYS = ("obstacles", "habitats", "polygon", "bins", "cells", "prob")
SCALARS = ("status", "found", "n_nodes", "n_children", "visited_count")
ARRAYS = ("expansions", "path", "cost_list", "node_path", "smooth_path", "hab_left")


def python_topn(prob):
    """[..., C] -> [..., C + 1]: sorted(row, reverse=True) and a running `total += v` from 0, on Python floats"""
    flat = prob.reshape(-1, prob.shape[-1])
    out = np.zeros((len(flat), prob.shape[-1] + 1))
    for t, row in enumerate(flat):
        total = 0
        for i, v in enumerate(sorted(row.tolist(), reverse=True)):
            total += v
            out[t, i + 1] = total
    return out.reshape(prob.shape[:-1] + (prob.shape[-1] + 1,))


def five_tables(P):
    return [P, P[:, ::-1], (P - P.mean()) * 3, np.zeros_like(P), np.random.default_rng(5).uniform(0, .3, P.shape) * 40]


def world12():
    from auv_sim_amd import synth
    return synth.make_world(seed=12, n_obstacles=32, obst_radius=(2.0, 6.0), n_habitats=8, hab_radius=(10.0, 25.0))


def nine_starts():
    rng = np.random.default_rng(17)
    return np.array([(-290 + 10 * rng.integers(0, 6), -90 + 10 * rng.integers(0, 6)) for _ in range(9)], dtype=np.float64)


def check(w, start, prob, cells=None):
    from oracle import orc_astar as oa
    kw = {k: w[k] for k in WORLD_KEYS}
    kw["prob"] = prob
    if cells is not None:
        kw["cells"] = cells
    return oa.run("astar_fixLenSOG", start, kind="portable", cap_nodes=20000, limit=150.0, weights=WEIGHTS, velocity=1.0, **kw)


def assert_same(r, o, what):
    for f in SCALARS:
        assert r[f] == o[f], (what, f, r[f], o[f])
    for f in ARRAYS:
        assert np.array_equal(r[f], o[f]), (what, f)


@pytest.fixture(scope="module")
def case(orc):
    """the issue's world, tables, starts and the checker's answers (computed once, never changed): ref[e] on table e % 5,
    ref0[e] on table 0, ref_perm[e] on table e % 5 with the cells shuffled"""
    w = world12()
    P = np.array(w["prob"], dtype=np.float64)
    assert P.shape == (10, 400)
    tabs = five_tables(P)
    starts = nine_starts()
    set_of = [e % 5 for e in range(9)]
    ref = [check(w, starts[e], tabs[set_of[e]]) for e in range(9)]
    ref0 = [check(w, starts[e], tabs[0]) for e in range(9)]
    perm = np.random.default_rng(29).permutation(400)
    cells_p = np.array(w["cells"], dtype=np.float64)[perm]
    ref_perm = [check(w, starts[e], tabs[set_of[e]][:, perm], cells=cells_p) for e in range(9)]
    return dict(w=w, tabs=tabs, starts=starts, set_of=set_of, ref=ref, ref0=ref0, perm=perm, cells_p=cells_p, ref_perm=ref_perm)


def sets_batch(ctx, starts, set_of, **kw):
    from auv_sim_amd import _astar_lib as al
    return al.run_batch(ctx, "astar_fixLenSOG", starts, limits=np.full(len(starts), 150.0), velocity=1.0, weights=WEIGHTS, cap_nodes=20000,
                        exp_log=True, set_of=set_of, **kw)


# ---- 1. the top-n tables ----
def awkward_tables(G, T, C, seed):
    """[G, T, C]: ties, zeros of both signs, mixed signs and a +inf; every bin differs from the others"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.5, 1.0, (G, T, C))
    p[0, 0] = np.round(p[0, 0], 1)          # ties
    p[0, 1, ::3] = 0.0
    p[0, 1, 1::3] = -0.0
    p[1, 2, rng.integers(0, C)] = np.inf
    p[2, 0] = -np.abs(p[2, 0])
    p[2, 1] = np.round(p[2, 1] * 4) / 4     # few distinct values, both signs, zeros
    return p


@pytest.mark.parametrize("C", [1, 63, 64, 65, 987, 4096, 16384, 16385])
def test_topn_tables_equal_the_reference_loop(C):
    """the bitonic sort's padding on either side of a power of two, the Catalina cell count, the forecast's cap, the LDS bound and
    the first C that takes the host route"""
    from auv_sim_amd import _astar_lib as al, _lib
    G = T = 3
    p = awkward_tables(G, T, C, seed=C)
    assert C == 1 or len({p[g, t].tobytes() for g in range(G) for t in range(T)}) == G * T   # (a wrong row stride would show)
    ctx = _lib.Context(0)
    try:
        bins = np.array([(20.0 * t, 20.0 * t + 20.0) for t in range(T)])
        cells = np.array([(float(c), 0.0, float(c) + 1.0, 1.0) for c in range(C)])
        ctx.set_world(bins=bins, cells=cells, prob=np.zeros((T, C)))
        ctx.set_prob_sets(p)
        got = al.sets_topn(ctx)
    finally:
        ctx.close()
    want = python_topn(p)
    assert got.shape == want.shape == (G, T, C + 1)
    assert got.tobytes() == want.tobytes(), [(g, t) for g in range(G) for t in range(T) if got[g, t].tobytes() != want[g, t].tobytes()]


# ---- 2. every instance against the checker on its own table ----
def test_the_checker_alone_tells_the_tables_apart(case):
    assert all(o["found"] and o["status"] == 0 for o in case["ref"])
    differ = [e for e in range(9) if not np.array_equal(case["ref"][e]["node_path"], case["ref0"][e]["node_path"])]
    print("node_path differs from table 0's for instances", differ, "nodes", [o["n_nodes"] for o in case["ref"]])
    assert len(differ) >= 5
    ts = max(o["node_path"][:, 7].max() for o in case["ref"])
    assert (np.asarray(case["w"]["bins"])[:, 1] < ts).sum() >= 2   # (time stamps past bin 1: three rows of a table are read)


@pytest.mark.parametrize("cells_as", ["product_grid", "shuffled_list"])
@pytest.mark.parametrize("pair", [0, 1], ids=["one_wavefront", "two_wavefronts"])
def test_every_instance_equals_the_checker_on_its_own_table(case, pair, cells_as):
    from auv_sim_amd import _lib
    test_the_checker_alone_tells_the_tables_apart(case)
    w, tabs = case["w"], np.stack(case["tabs"])
    ctx = _lib.Context(0)
    try:
        ctx.set_option("ASTAR_PAIR", pair)
        if cells_as == "shuffled_list":   # (no product grid: the sweep lookup, and never the paired form)
            ctx.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], case["cells_p"], tabs[0][:, case["perm"]])
            ctx.set_prob_sets(tabs[:, :, case["perm"]])
            ref = case["ref_perm"]
        else:
            ctx.set_world(*[w[k] for k in WORLD_KEYS])
            ctx.set_prob_sets(tabs)
            ref = case["ref"]
        res = sets_batch(ctx, case["starts"], case["set_of"])
        block = ctx.last_launch()[1]
    finally:
        ctx.close()
    assert block == (512 if pair and cells_as == "product_grid" else 256)
    for e in range(9):
        assert_same(res[e], ref[e], (pair, cells_as, e))


# ---- 3. equal tables change nothing ----
@pytest.mark.parametrize("pair", [0, 1], ids=["one_wavefront", "two_wavefronts"])
def test_sets_equal_to_the_worlds_table_change_nothing(case, pair):
    from auv_sim_amd import _astar_lib as al, _lib
    w = case["w"]
    ctx = _lib.Context(0)
    try:
        ctx.set_option("ASTAR_PAIR", pair)
        ctx.set_world(*[w[k] for k in WORLD_KEYS])
        ctx.set_prob_sets(np.stack([w["prob"], w["prob"]]))
        kw = dict(limits=np.full(9, 150.0), velocity=1.0, weights=WEIGHTS, cap_nodes=20000, exp_log=True, return_visited=True)
        plain = al.run_batch(ctx, "astar_fixLenSOG", case["starts"], **kw)
        assert ctx.n_prob_sets == 2
        sets = al.run_batch(ctx, "astar_fixLenSOG", case["starts"], set_of=[e % 2 for e in range(9)], **kw)
        assert ctx.last_launch()[1] == (512 if pair else 256)
    finally:
        ctx.close()
    for e in range(9):
        assert_same(sets[e], plain[e], (pair, e))
        assert_same(plain[e], case["ref0"][e], (pair, e))
        assert np.array_equal(sets[e]["visited"], plain[e]["visited"]) and plain[e]["visited"].sum() == plain[e]["visited_count"] > 0


# ---- 4. the redo keeps the tables ----
REDO_CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, %r)
import test_gpu_astar_shark_sets as t
from auv_sim_amd import _lib
from oracle import orc
orc.build()
w = t.world12()
tabs = t.five_tables(np.array(w["prob"], dtype=np.float64))
starts, set_of = t.nine_starts(), [e %% 5 for e in range(9)]
ref = [t.check(w, starts[e], tabs[set_of[e]]) for e in range(9)]
ctx = _lib.Context(0)
ctx.set_world(*[w[k] for k in t.WORLD_KEYS])
ctx.set_prob_sets(np.stack(tabs))
ctx.set_option("ASTAR_PAIR", 1)
res = t.sets_batch(ctx, starts, set_of)
fb, block = ctx.pipeline_fallbacks(), ctx.last_launch()[1]
bad = []
for e in range(9):
    try:
        t.assert_same(res[e], ref[e], e)
    except AssertionError as x:
        bad.append(str(x))
print(json.dumps(dict(redone=fb[0], block=block, bad=bad, ref_status=[o["status"] for o in ref])))
'''


def test_the_redo_after_a_wait_that_ran_out_keeps_the_tables():
    """the diagnostic build, the partners delayed by up to 64 units against waits of six polls (tests/test_gpu_astar_pair.py's
    setting): instances of the paired sets launch end with AUVP_ERR_PIPELINE and the batch is searched again by the one-wavefront
    sets form -- every instance still on its own table"""
    import test_gpu_astar_pair as tp
    out = tp._child(["-c", REDO_CHILD % os.path.join(REPO, "tests")], jitter="%s,64,3" % tp.PARTNERS, spin=6)
    f = json.loads(out.strip().splitlines()[-1])
    print("instances redone by the one-wavefront sets kernel:", f["redone"])
    assert f["ref_status"] == [0] * 9
    assert f["redone"] > 0 and f["block"] == 256
    assert f["bad"] == []


# ---- 5. the forecast hand-over ----
class _B:
    def __init__(self, *b):
        self.bounds = tuple(float(v) for v in b)


def _same_plan(a, b, what):
    assert (a is None) == (b is None), what
    if a is None:
        return
    assert a["cost list"] == b["cost list"] and a["cost"] == b["cost"] and a["path length"] == b["path length"], what
    assert [(p.x, p.y, p.traj_time_stamp) for p in a["path"]] == [(p.x, p.y, p.traj_time_stamp) for p in b["path"]], what
    fields = lambda n: (n.position, n.g, n.h, n.f, n.cost, n.pathLen, n.time_stamp)  # noqa: E731
    assert [fields(n) for n in a["node"]] == [fields(n) for n in b["node"]], what


@pytest.mark.parametrize("hand_over", ["forecast", "dicts"])
def test_forecast_tables_reach_the_astar_planner(hand_over):
    """F = 3 filters over a 200 m box of 10 m cells, R + 1 = 10 bins: set_shark_grids(forecast) on the forecast's context (device
    to device) or the same tables as dicts, then astar_batch(shark_of=[0, 1, 2, 1]) == four planners built from
    forecast.shark_grid(f)"""
    import math
    import random
    from auv_sim_amd import _lib
    from auv_sim_amd.astar_fixLenSOG import astar
    from auv_sim_amd.motion_plan_state import Motion_plan_state as MPS
    from auv_sim_amd.sharkForecast import SharkForecast
    F, R = 3, 9
    X0, Y0 = -300, -100   # (the reference's visited array is indexed [x + 500][y + 200] of 600 x 600: the box lies inside it)
    boundary = _B(X0, Y0, X0 + 200, Y0 + 200)
    cells = [_B(X0 + 10 * c, Y0 + 10 * r, X0 + 10 * c + 10, Y0 + 10 * r + 10) for r in range(20) for c in range(20)]
    rng = np.random.default_rng(8)
    xy = np.stack([rng.normal(loc=(X0 + m[0], Y0 + m[1]), scale=30.0, size=(200, 2)) for m in ((60.0, 70.0), (140.0, 120.0), (100.0, 40.0))])
    sf = SharkForecast(boundary, 10, cells, device_context=_lib.Context(0))
    fc = sf.run(xy, np.ones((21, 21)), R)
    assert not fc.status.any() and fc.prob.shape == (F, R + 1, 400)
    grids = [fc.shark_grid(f, (0, 20), 20) for f in range(F)]
    corners = [MPS(X0 + 0.0, Y0 + 0.0), MPS(X0 + 200.0, Y0 + 0.0), MPS(X0 + 200.0, Y0 + 200.0), MPS(X0 + 0.0, Y0 + 200.0)]
    orng = random.Random(2)
    obstacles = [MPS(X0 + orng.uniform(10, 190), Y0 + orng.uniform(10, 190), size=orng.uniform(2, 6)) for _ in range(12)]
    obstacles = [o for o in obstacles if min(math.hypot(o.x - X0 - sx, o.y - Y0 - sy) for sx, sy in ((100, 100), (60, 120), (140, 80))) > 15]
    habitats = [MPS(X0 + orng.uniform(20, 180), Y0 + orng.uniform(20, 180), size=orng.uniform(8, 15)) for _ in range(5)]
    starts = [(X0 + 100, Y0 + 100), (X0 + 100, Y0 + 100), (X0 + 60, Y0 + 120), (X0 + 140, Y0 + 80)]
    shark_of, limit = [0, 1, 2, 1], 100.0
    args = (obstacles, corners, habitats)
    fleet = astar(starts[0], *args, grids[0], {}, 1.0, cap_nodes=20000, device_context=sf._ctx)
    with pytest.raises(ValueError):
        fleet.astar_batch(starts, [limit] * 4, WEIGHTS, shark_of=shark_of)   # no tables yet
    calls, upload = [], fleet._ctx.set_prob_sets
    fleet._ctx.set_prob_sets = lambda *a, **k: (calls.append((a, k)), upload(*a, **k))[1]
    fleet.set_shark_grids(fc if hand_over == "forecast" else grids)
    assert len(calls) == 1 and fleet.n_shark_sets == F
    if hand_over == "forecast":
        assert not calls[0][0] and calls[0][1]["prob_dev"] == sf._ctx.sf_prob_dev()[0]   # device to device
    got = fleet.astar_batch(starts, [limit] * 4, WEIGHTS, shark_of=shark_of)
    assert len(calls) == 1   # (astar_batch found its world in place and left the tables alone)
    for i in range(4):
        want = astar(starts[i], *args, grids[shark_of[i]], {}, 1.0, cap_nodes=20000).astar_batch([starts[i]], [limit], WEIGHTS)[0]
        assert want is not None
        _same_plan(got[i], want, i)
    assert got[0]["cost list"] != got[1]["cost list"]   # one start, two sharks
    with pytest.raises(ValueError):
        fleet.astar_batch(starts, [limit] * 4, WEIGHTS, shark_of=[0, 1, 3, 1])
    # without shark_of nothing changes: the constructor's grid
    plain = fleet.astar_batch(starts[:1], [limit], WEIGHTS)[0]
    _same_plan(plain, got[0], "plain")
    fleet.set_shark_grids(None)
    assert fleet.n_shark_sets == 0 and fleet._ctx.n_prob_sets == 0


# ---- 6. errors ----
def test_statuses(case):
    from auv_sim_amd import _astar_lib as al, _lib
    w, tabs, starts = case["w"], np.stack(case["tabs"]), case["starts"]
    ctx = _lib.Context(0)

    def refused(code, names=None, **kw):
        args = dict(variant="astar_fixLenSOG", set_of=case["set_of"])
        args.update(kw)
        variant = args.pop("variant")
        with pytest.raises(_lib.AuvpError) as x:
            al.run_batch(ctx, variant, starts, limits=np.full(9, 150.0), velocity=1.0, weights=WEIGHTS, cap_nodes=20000, exp_log=True, **args)
        assert x.value.code == code, x.value
        if names:
            assert names in str(x.value), x.value
        # a plain batch still runs on the same handle
        res = al.run_batch(ctx, "astar_fixLenSOG", starts[:2], limits=np.full(2, 150.0), velocity=1.0, weights=WEIGHTS, cap_nodes=20000,
                           exp_log=True)
        for e in range(2):
            assert_same(res[e], case["ref0"][e], ("plain after", code, e))

    try:
        ctx.set_world(*[w[k] for k in WORLD_KEYS])
        refused(ERR_STATE)                                                   # no tables
        with pytest.raises(_lib.AuvpError) as x:
            al.sets_topn(ctx)
        assert x.value.code == ERR_STATE
        ctx.set_prob_sets(tabs)
        refused(ERR_ARG, "instance 4", set_of=[0, 1, 2, 3, 5, 0, 1, 2, 3])   # an index equal to n_sets
        refused(ERR_ARG, "instance 0", set_of=[-1] + case["set_of"][1:])
        with pytest.raises(ValueError):                                      # a set_of of another length than E
            al.run_batch(ctx, "astar_fixLenSOG", starts, limits=np.full(9, 150.0), weights=WEIGHTS, set_of=case["set_of"][:8])
        refused(ERR_ARG, "variant", variant="astar_fixLen")                  # a variant other than 3
        nan = tabs.copy()
        nan[3, 2, 17] = np.nan
        ctx.set_prob_sets(nan)
        refused(ERR_ARG, "set 3")                                            # a table with one nan: the message names the set
        res = sets_batch(ctx, starts[:3], [0, 1, 2])                         # (the other sets stay usable)
        for e in range(3):
            assert_same(res[e], case["ref"][e], ("beside the nan", e))
        ctx.set_prob_sets(tabs)
        res = sets_batch(ctx, starts, case["set_of"])
        for e in range(9):
            assert_same(res[e], case["ref"][e], ("replaced", e))
        ctx.set_world(*[w[k] for k in WORLD_KEYS])                           # a new world drops the tables
        refused(ERR_STATE)
    finally:
        ctx.close()

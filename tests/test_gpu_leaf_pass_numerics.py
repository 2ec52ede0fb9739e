"""The leaf pass's error bound at the ends of the number format.  rrt_leaf_body.h ranks leaves by an unordered running sum with an
error bound and re-sums the survivors in the reference's order; this file drives the parts of the bound that weights near
(-3, -3, -4) and tables from uniform(0, pmax) never reach: a shark term absorbed into cost[0], a huge cost[0], zero weights and
the signs of zero (the e2 == 0 shortcut), tables of mixed sign (prob_one_sign == 0), infinities, subnormal and overflowing terms,
and the switch of the habitat weight between one multiplication and repeated addition at 2^20.

Every row (tables x weight triples over the same trees) goes through rrt_leaf_kernel (set_world per table, pruned and with the
leaf log) and through rrt_leaf_grid_kernel (all tables of the row in one set_prob_sets batch, episodes = seeds x tables), and is
compared with the CPU checker run with the same table and weights.  What a row is there for is asserted on the checker's
output before the device is looked at, so that a row cannot become vacuous.  Every comparison is exact
(leaf_pass_cases.same); no tolerance appears in this file."""
import numpy as np
import pytest

import leaf_pass_cases as lp

pytestmark = pytest.mark.gpu
INF, NAN = float("inf"), float("nan")
DEFAULT_W = (-3.0, -3.0, -4.0)


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


# ---- tables: functions of the world's own table P [T, C] --------------------------------------------------------------------
def _cancelling(P):
    t = P.copy()
    t[0, :], t[1, :] = 2.0 ** 40, -2.0 ** 40
    return t


def _random_signs(P):
    return P * np.where(np.random.default_rng(17).random(P.shape) < 0.5, -1.0, 1.0)


def _some_inf(P):
    t = P.copy()
    t[np.random.default_rng(13).random(P.shape) < 0.02] = INF
    return t


def _both_inf(P):
    t = P.copy()
    u = np.random.default_rng(19).random(P.shape)
    t[u < 0.01], t[u > 0.99] = INF, -INF
    return t


# ---- what each row is there for, from the checker's output of the base tree's first seed -----------------------------------
def _leaf_nodes(r):
    return lp.structure(r, lp.HORIZON_DEFAULT if "_mtt" not in r else r["_mtt"])["leaves"]


def _ties(r):
    """(indexes of the leaves that tie at the best total, in creation order)"""
    return np.flatnonzero(r["leaf_cost"][:, 0] == r["best_cost"][0])


def _first_of_ties_wins(r, at_least, distinct_c2=False):
    t = _ties(r)
    assert len(t) >= at_least, len(t)
    if distinct_c2:
        assert len(set(r["leaf_cost"][t, 3].tolist())) >= at_least
    assert r["best_leaf"] == _leaf_nodes(r)[t[0]]


def _fact_absorbed(r, orc, wa, weights):
    _first_of_ties_wins(r, 10, distinct_c2=True)


def _fact_runner_up(r, orc, wa, weights):
    tot = r["leaf_cost"][:, 0]
    k = int(np.flatnonzero(_leaf_nodes(r) == r["best_leaf"])[0])
    runner = np.delete(tot, k).min()
    assert abs(runner / tot[k] - 1.0) < 1e-12, (runner, tot[k])


def _fact_negative_zero(r, orc, wa, weights):
    assert len(_ties(r)) == r["n_leaves"] >= 10 and r["best_leaf"] == _leaf_nodes(r)[0]
    assert lp.same(r["best_cost"], [0.0, -0.0, 0.0, 0.0]), r["best_cost"]


def _fact_order_matters(r, orc, wa, weights):
    """summing a leaf's elements in the reverse of the reference's order changes the total of at least half the leaves; in the
    reference's order orc.cost reproduces the log"""
    leaves = _leaf_nodes(r)
    changed = 0
    for k, leaf in enumerate(leaves):
        el = lp.leaf_elements(r, leaf)
        ctt = r["nodes"][leaf, 3]
        fwd = orc.cost(wa, 0, len(wa.bins), el, ctt, weights, kind="portable")
        assert lp.same(fwd[0], r["leaf_cost"][k, 0]), (k, fwd, r["leaf_cost"][k])
        changed += orc.cost(wa, 0, len(wa.bins), el[::-1].copy(), ctt, weights, kind="portable")[0] != fwd[0]
    assert 2 * changed >= len(leaves) > 0, (changed, len(leaves))
    assert (wa.prob > 0).any() and (wa.prob < 0).any()  # prob_one_sign == 0


def _fact_minus_inf_wins(r, orc, wa, weights):
    assert r["best_cost"][0] == -INF and (r["leaf_cost"][:, 0] == -INF).any()


def _fact_plus_inf_loses(r, orc, wa, weights):
    assert (r["leaf_cost"][:, 0] == INF).any() and np.isfinite(r["best_cost"][0]) and r["status"] == 0


def _fact_nan_loses(r, orc, wa, weights):
    assert np.isnan(r["leaf_cost"][:, 0]).any() and np.isfinite(r["best_cost"][0]) and r["status"] == 0


def _fact_no_best(r, orc, wa, weights):
    assert (r["status"], r["best_leaf"]) == (1, -1) and r["n_leaves"] >= 10


def _fact_subnormal(r, orc, wa, weights):
    assert 0.0 < abs(r["best_cost"][3]) < np.finfo(np.float64).tiny, r["best_cost"]


def _fact_all_minus_inf(r, orc, wa, weights):
    assert (r["leaf_cost"][:, 0] == -INF).all()
    _first_of_ties_wins(r, r["n_leaves"])


def _fact_two_hits(r, orc, wa, weights):
    leaves = _leaf_nodes(r)
    hits = np.rint(r["leaf_cost"][:, 2] * r["nodes"][leaves, 3] / weights[1])
    assert hits.max() >= 2, hits.max()


# a row: tables (functions of P), weight triples, facts {(table index, weight index): assertion on seed 0's checker result}
ROWS = {
    "absorbed_c2": dict(tables=[lambda P: P], weights=[(-3.0, 0.0, -1e-17)], facts={(0, 0): _fact_absorbed}),
    "huge_c0": dict(tables=[lambda P: P], weights=[(-2.0 ** 52, -3.0, -4.0), (-2.0 ** 40, -3.0, -4.0)],
                    facts={(0, 0): _fact_runner_up, (0, 1): _fact_runner_up}),
    "zero_weights": dict(tables=[lambda P: P], weights=[(0.0, 0.0, -4.0), (-3.0, -3.0, 0.0), (-0.0, -0.0, -0.0)],
                         facts={(0, 2): _fact_negative_zero}),
    "cancelling": dict(tables=[_cancelling], weights=[(0.0, 0.0, -4.0)], facts={(0, 0): _fact_order_matters}),
    "random_signs": dict(tables=[_random_signs], weights=[(0.0, 0.0, -4.0), (-2.0 ** 45, 0.5, -4.0)], facts={}),
    "infinities": dict(tables=[_some_inf, _both_inf, lambda P: np.full_like(P, INF)],
                       weights=[DEFAULT_W, (-3.0, -3.0, 4.0), (-3.0, -3.0, 0.0)],
                       facts={(0, 0): _fact_minus_inf_wins, (0, 1): _fact_plus_inf_loses, (0, 2): _fact_nan_loses,
                              (2, 1): _fact_no_best}),
    "range": dict(tables=[lambda P: P * 1e-310, lambda P: P, lambda P: P * 1e300], weights=[DEFAULT_W, (-3.0, -3.0, -1e300)],
                  facts={(0, 0): _fact_subnormal, (2, 1): _fact_all_minus_inf}),
    "w2_switch": dict(tables=[lambda P: P],
                      weights=[(-3.0, w2, -4.0) for w2 in (-1048575.0, -1048576.0, -2097152.0, -1048576.5, -0.1)],
                      facts={(0, k): _fact_two_hits for k in (1, 2, 3, 4)}),
}
DEEP_ROWS = ("absorbed_c2", "cancelling", "infinities")  # rows 1, 4 and 6 on the deep tree
PARAMS = [("control", n) for n in ROWS] + [("bin_deep_a", n) for n in DEEP_ROWS]


def _check(ctx, summ, refs, log, tag):
    paths = ctx.paths(summ)
    for e, r in enumerate(refs):
        lp.assert_summary(summ[e], r, tag + (e,))
        lp.assert_path(paths[e], r, tag + (e,))
        if log:
            lp.assert_leaf_log(ctx.leaf_log(e, summ[e]), r, tag + (e,))


@pytest.mark.parametrize("case,row", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_row_equals_the_checker(ctx, orc, case, row, monkeypatch):
    """control: the base tree (world 51 / 64 obstacles, 900 iterations, seeds 4000-4003, default parameters); bin_deep_a: a
    time-bin tree whose best chain is longer than 64 nodes (two seeds), with the rows that decide ties, order and infinities"""
    c = lp.CASES[case]
    w = lp.world(case)
    S = 4 if case == "control" else 2
    init, seeds = lp.inits(case, S), lp.seeds(case, S)
    spec = ROWS[row]
    tabs = np.stack([f(w["prob"]) for f in spec["tables"]])
    G = len(tabs)
    was = [lp.world_arrays(orc, w, prob=t) for t in tabs]
    mtt = lp.horizon(case)
    ref = {}
    for g in range(G):
        for k, wt in enumerate(spec["weights"]):
            for s in range(S):
                r = orc.rrt_explore(was[g], int(seeds[s]), c["n_iter"], init=init[s], weights=wt, kind="portable", **c["kw"])
                r["_mtt"] = mtt
                ref[(g, k, s)] = r
    # what the row is there for: the checker's facts on the first seed, before the device is looked at
    if case == "control":
        for (g, k), fact in spec["facts"].items():
            fact(ref[(g, k, 0)], orc, was[g], spec["weights"][k])
    else:
        assert lp.structure(ref[(0, 0, 0)], mtt)["max_chain"] >= lp.CHAIN_CHUNK + 1
    monkeypatch.delenv("AUVP_LEAF_SWEEP_ALL", raising=False)
    # (a) rrt_leaf_kernel: the table is the world's
    for g in range(G):
        lp.set_world(ctx, w, prob=tabs[g])
        for k, wt in enumerate(spec["weights"]):
            for log in (False, True):
                summ = ctx.rrt_explore_batch(init, seeds, c["n_iter"], mode=c["mode"], weights=wt, leaf_log=log, **c["kw"]).copy()
                _check(ctx, summ, [ref[(g, k, s)] for s in range(S)], log, (case, row, "world", g, k, log))
    # (b) rrt_leaf_grid_kernel: every table of the row as a probability set, episodes = seeds x tables
    lp.set_world(ctx, w)
    ctx.set_prob_sets(tabs)
    absmax, one_sign = ctx.prob_set_stats()
    for g in range(G):
        nan = bool(np.isnan(tabs[g]).any())
        assert lp.same(absmax[g], NAN if nan else np.abs(tabs[g]).max()), g
        assert int(one_sign[g]) == int(not nan and not ((tabs[g] > 0).any() and (tabs[g] < 0).any())), g
    set_of = np.tile(np.arange(G, dtype=np.int32), S)
    init_b, seeds_b = init.repeat(G, axis=0), seeds.repeat(G)
    for k, wt in enumerate(spec["weights"]):
        for log in (False, True):
            summ = ctx.rrt_explore_batch(init_b, seeds_b, c["n_iter"], weights=wt, leaf_log=log, shark_set=set_of, **c["kw"]).copy()
            _check(ctx, summ, [ref[(int(set_of[e]), k, e // G)] for e in range(S * G)], log, (case, row, "sets", k, log))
    ctx.set_prob_sets()

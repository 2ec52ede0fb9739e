"""The leaf pass (csrc/rrt_leaf_body.h: rrt_leaf_kernel, rrt_leaf_lim_kernel, rrt_leaf_grid_kernel) and the course kernels behind
it on trees whose shape takes the branches that steer parameters near the reference's defaults never reach: chains of more than
64 nodes (the second descriptor chunk of the ordered re-summation), leaves of more than 256 elements (its second window), passes
of more than 2 048 point slots (the owner search) and passes whose 64 nodes hang on each other in series (the in-pass loops).
The cases and what the CPU checker says about their shape are in tests/leaf_pass_cases.py, asserted without a GPU by
tests/test_leaf_pass_cases.py.  Every comparison is exact (leaf_pass_cases.same); no tolerance appears in this file."""
import numpy as np
import pytest

import leaf_pass_cases as lp
import replan_cases as rc

pytestmark = pytest.mark.gpu
E = 5  # one full workgroup of four wavefronts and a partial one


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _run(ctx, name, E, leaf_log, **extra):
    c = lp.CASES[name]
    kw = dict(c["kw"], **extra)
    summ = ctx.rrt_explore_batch(lp.inits(name, E), lp.seeds(name, E), c["n_iter"], mode=c["mode"], leaf_log=leaf_log, **kw).copy()
    trees = [ctx.tree(e, summ[e]) for e in range(E)]
    logs = [ctx.leaf_log(e, summ[e]) for e in range(E)] if leaf_log else None
    return summ, trees, ctx.paths(summ), logs


# the control first, then by the size of the tree
ORDER = ["control", "wide_a", "wide_b", "bin_deep_a", "bin_deep_c", "plan_long", "plan_deep_b", "plan_deep_a", "bin_deep_b", "nn_deep"]
assert sorted(ORDER) == sorted(lp.CASES)


@pytest.mark.parametrize("name", ORDER)
def test_every_route_equals_the_checker(ctx, orc, name, monkeypatch):
    """E episodes of a case (seed + e, a heading of their own), run four ways -- pruning or the leaf log (every qualifying leaf
    re-summed), the marked nodes or (LEAF_SWEEP_ALL) every node swept: each run equals the checker episode by episode in the
    summary, the tree and the best course, the leaf log equals the checker's leaf_cost and leaf_iter, and the four runs agree
    with each other in every field"""
    lp.set_world(ctx, lp.world(name))
    refs = [lp.reference(name, e) for e in range(E)]
    runs = {}
    for sweep in ("0", "1"):
        monkeypatch.setenv("AUVP_LEAF_SWEEP_ALL", sweep)
        for log in (False, True):
            run = runs[(sweep, log)] = _run(ctx, name, E, log)
            for e, r in enumerate(refs):
                tag = (name, "sweep" + sweep, "log" if log else "prune", e)
                lp.assert_summary(run[0][e], r, tag)
                lp.assert_tree(run[1][e], r, tag)
                lp.assert_path(run[2][e], r, tag)
                if log:
                    lp.assert_leaf_log(run[3][e], r, tag)
    first = runs[("0", False)]
    for k, run in runs.items():
        lp.assert_same_runs(first, run, (name, k))
    lp.assert_same_runs(runs[("0", True)], runs[("1", True)], (name, "logs"))


def _lim_inputs(name):
    """six episodes of a deep time-bin case: the case's own tree under every habitat, no habitat and a subset; another seed;
    two shorter horizons (another K, another tree, another leaf threshold) with single habitats"""
    c = lp.CASES[name]
    H = len(lp.world(name)["habitats"])
    full = (1 << H) - 1
    mtt0 = lp.horizon(name)
    seeds = np.array([c["seed"], c["seed"], c["seed"], c["seed"] + 1, c["seed"], c["seed"] + 2], dtype=np.uint64)
    mtt = np.array([mtt0, mtt0, mtt0, mtt0, mtt0 - 5.0, mtt0 - 12.0])
    keep = [full, 0, 0b1010101010 & full, full, 1, 1 << (H - 1)]
    init = lp.inits(name, 1).repeat(6, axis=0)
    init[3:, 2] = [0.5, 0.0, -0.5]
    return seeds, mtt, keep, init


@pytest.mark.parametrize("name", lp.DEEP_TIMEBIN)
def test_lim_kernel_on_deep_trees(ctx, orc, name, monkeypatch):
    """rrt_leaf_lim_kernel: per-episode horizons and habitat subsets (none and all among them) on the deep time-bin trees; each
    episode equals the checker on a world holding its kept habitats with its own horizon, pruned and with the leaf log.  From
    the checker alone: at least one episode keeps a best chain of >= 65 nodes, at the horizon it ran with."""
    c = lp.CASES[name]
    w = lp.world(name)
    H = len(w["habitats"])
    seeds, mtt, keep, init = _lim_inputs(name)
    kw = {k: v for k, v in c["kw"].items() if k != "max_traj_time"}
    refs = []
    for e in range(len(seeds)):
        sub = w["habitats"][[h for h in range(H) if (keep[e] >> h) & 1]].reshape(-1, 3)
        refs.append(orc.rrt_explore(lp.world_arrays(orc, w, habitats=sub), int(seeds[e]), c["n_iter"], init=init[e],
                                    max_traj_time=float(mtt[e]), kind="portable", **kw))
    shapes = [lp.structure(r, float(mtt[e])) for e, r in enumerate(refs)]
    assert sum(s["best_chain"] >= lp.CHAIN_CHUNK + 1 for s in shapes) >= 1, [s["best_chain"] for s in shapes]
    assert all(s["max_chain"] >= lp.CHAIN_CHUNK + 1 for s in shapes[:3])
    assert any(r["n_nodes"] != refs[0]["n_nodes"] for r in refs[4:])  # a shorter horizon grows another tree
    lp.set_world(ctx, w)
    monkeypatch.delenv("AUVP_LEAF_SWEEP_ALL", raising=False)
    for log in (False, True):
        summ = ctx.rrt_explore_batch(init, seeds, c["n_iter"], max_traj_time=mtt, habitat_keep=np.array(keep, dtype=np.uint64),
                                     leaf_log=log, **kw).copy()
        assert ctx.last_rrt_kernel() == "rrt_explore_lim_kernel"
        paths = ctx.paths(summ)
        for e, r in enumerate(refs):
            tag = (name, "log" if log else "prune", e)
            lp.assert_summary(summ[e], r, tag)
            lp.assert_tree(ctx.tree(e, summ[e]), r, tag)
            lp.assert_path(paths[e], r, tag)
            if log:
                lp.assert_leaf_log(ctx.leaf_log(e, summ[e]), r, tag)


def _tables(P):
    """the world's table, the same reversed along the cells, one of mixed signs (one_sign == 0), all zeros (ties)"""
    return np.stack([P, P[:, ::-1], (P - P.mean()) * 3, np.zeros_like(P)])


@pytest.mark.parametrize("name", lp.DEEP_TIMEBIN[:2])
def test_grid_kernel_on_deep_trees(ctx, orc, name, monkeypatch):
    """rrt_leaf_grid_kernel: four probability tables over the same seeds (episodes = 2 seeds x 4 tables), each episode against
    the checker run on a world holding its table; then another assignment with rrt_set_episode_grids + rrt_rerank equals a
    fresh run under that assignment, and the checker"""
    c = lp.CASES[name]
    w = lp.world(name)
    tabs = _tables(w["prob"])
    G, S = len(tabs), 2
    n = G * S
    init = lp.inits(name, S).repeat(G, axis=0)
    seeds = lp.seeds(name, S).repeat(G)
    A = np.arange(n, dtype=np.int32) % G
    B = (A + 1 + np.arange(n, dtype=np.int32) // G) % G
    ref = {}
    for e in range(n):
        for g in {int(A[e]), int(B[e])}:
            ref[(e, g)] = orc.rrt_explore(lp.world_arrays(orc, w, prob=tabs[g]), int(seeds[e]), c["n_iter"], init=init[e],
                                          kind="portable", **c["kw"])
    assert any(lp.structure(ref[(e, int(A[e]))], lp.horizon(name))["best_chain"] >= lp.CHAIN_CHUNK + 1 for e in range(n))
    assert len({ref[(e, int(A[e]))]["best_leaf"] for e in range(G)}) > 1  # the table matters to the ranking
    lp.set_world(ctx, w)
    ctx.set_prob_sets(tabs)
    monkeypatch.delenv("AUVP_LEAF_SWEEP_ALL", raising=False)

    def check(summ, sets, tag):
        paths = ctx.paths(summ)
        for e in range(n):
            r = ref[(e, int(sets[e]))]
            lp.assert_summary(summ[e], r, (name, tag, e))
            lp.assert_path(paths[e], r, (name, tag, e))
        return paths
    first = ctx.rrt_explore_batch(init, seeds, c["n_iter"], shark_set=A, **c["kw"]).copy()
    check(first, A, "A")
    lp.assert_tree(ctx.tree(0, first[0]), ref[(0, int(A[0]))], (name, "A", 0))
    ctx.rrt_set_episode_grids(B)
    again = ctx.rrt_rerank().copy()
    again_paths = check(again, B, "rerank B")
    fresh = ctx.rrt_explore_batch(init, seeds, c["n_iter"], shark_set=B, **c["kw"]).copy()
    fresh_paths = check(fresh, B, "fresh B")
    for e in range(n):
        for f in lp.SUMMARY_FIELDS:
            assert np.asarray(again[e][f]).tobytes() == np.asarray(fresh[e][f]).tobytes(), (name, e, f)
        assert again_paths[e].tobytes() == fresh_paths[e].tobytes(), (name, e)
    logged = ctx.rrt_explore_batch(init, seeds, c["n_iter"], shark_set=A, leaf_log=True, **c["kw"]).copy()
    check(logged, A, "A, log")
    for e in range(n):
        lp.assert_leaf_log(ctx.leaf_log(e, logged[e]), ref[(e, int(A[e]))], (name, "A, log", e))
    ctx.set_prob_sets()


def _fold(refs):
    """exploring's rule over the members in order: the first strictly smallest best_cost[0] among those with a leaf, or -1"""
    best, win = np.inf, -1
    for m, r in enumerate(refs):
        if r["best_leaf"] >= 0 and r["best_cost"][0] < best:
            best, win = r["best_cost"][0], m
    return win


def test_fleet_courses_on_a_deep_tree(ctx, orc, monkeypatch):
    """the courses the fleet routes use, on chains of more than 64 nodes: rrt_group_best with K = 2 + group_paths
    (rrt_group_course_kernel) equal the checker's members folded on the host and the winner's path; one replan_begin /
    replan_commit round (the PRODUCE path of rrt_commit_kernel) equals replan_cases.expected on the checker's path, with a
    round_span that selects more than 64 and fewer than all rows of a course"""
    name = "bin_deep_a"
    c = lp.CASES[name]
    w = lp.world(name)
    H = len(w["habitats"])
    G, K = 2, 2
    n = G * K
    # group 0: the case's own episode and the next seed; group 1: the two after it
    init, seeds = lp.inits(name, n), lp.seeds(name, n)
    kw = {k: v for k, v in c["kw"].items() if k != "max_traj_time"}
    mtt, keep0 = lp.horizon(name), (1 << H) - 1
    refs = [orc.rrt_explore(lp.world_arrays(orc, w), int(seeds[e]), c["n_iter"], init=init[e], max_traj_time=mtt, kind="portable", **kw)
            for e in range(n)]
    wins = [_fold(refs[g * K:(g + 1) * K]) for g in range(G)]
    assert all(x >= 0 for x in wins)
    winners = [refs[g * K + wins[g]] for g in range(G)]
    chains = [lp.structure(r, mtt)["best_chain"] for r in winners]
    assert max(chains) >= lp.CHAIN_CHUNK + 1, chains
    # the span: 60 % of the way along the deepest winner's course, so that part of every course stays behind
    deep = winners[int(np.argmax(chains))]["path"]
    span = float(deep[int(0.6 * len(deep)), 4])
    start7 = np.zeros((G, 7))
    start7[:, 0], start7[:, 1] = w["start"]
    want = [rc.expected(rc.case(r["path"], start7[g], keep0, span, w["habitats"])) for g, r in enumerate(winners)]
    n_sel = [int(x[0].sum()) for x in want]
    assert any(64 < s < len(r["path"]) for s, r in zip(n_sel, winners)), (n_sel, [len(r["path"]) for r in winners])
    lp.set_world(ctx, w)
    monkeypatch.delenv("AUVP_LEAF_SWEEP_ALL", raising=False)
    ctx.replan_begin(start7, keep0)
    ctx.rrt_explore_batch(init, seeds, c["n_iter"], max_traj_time=np.full(n, mtt), habitat_keep=np.full(n, keep0, np.uint64),
                          summaries=False, **kw)
    best = ctx.rrt_group_best(np.arange(G + 1) * K)
    gp = ctx.group_paths(best)
    for g, r in enumerate(winners):
        b = best[g]
        assert (int(b["status"]), int(b["winner"]), int(b["path_len"])) == (0, g * K + wins[g], len(r["path"])), (g, b)
        assert int(b["n_with_leaf"]) == sum(x["best_leaf"] >= 0 for x in refs[g * K:(g + 1) * K])
        assert lp.same(b["cost"], r["best_cost"]) and lp.same(b["length"], r["best_length"]), (g, b["cost"], r["best_cost"])
        assert lp.same(gp[g], r["path"]), g
    auv_of = [1, 0]
    rec = ctx.replan_commit(auv_of, span)
    off, rows = ctx.replan_traj()
    for g, a in enumerate(auv_of):
        sel, e_rows, e_keep, e_last = want[g]
        assert int(rec["status"][g]) == 0 and int(rec["n_committed"][g]) == len(e_rows) == n_sel[g], (g, rec[g])
        assert rc.same(rows[off[a]:off[a + 1]], e_rows) and lp.same(rows[off[a]:off[a + 1]], e_rows), g
        assert int(rec["keep"][g]) == e_keep and lp.same(rec["last"][g], e_last), g
        assert int(rec["path_len"][g]) == len(winners[g]["path"]) and lp.same(rec["cost"][g], winners[g]["best_cost"]), g


def test_leaf_stats_progress(ctx, orc, monkeypatch):
    """last_leaf_stats() of one deep episode: under pruning every strict prefix minimum of the checker's leaf totals (creation
    order) became the best leaf at some point, so it was re-summed, and no more leaves than qualify; with the leaf log every
    qualifying leaf is re-summed, element for element"""
    name = "plan_deep_a"
    c = lp.CASES[name]
    r = lp.reference(name)
    s = lp.structure(r, lp.horizon(name))
    minima = lp.strict_prefix_minima(r["leaf_cost"][:, 0])
    assert 1 <= minima <= r["n_leaves"]
    lp.set_world(ctx, lp.world(name))
    for sweep in ("0", "1"):
        monkeypatch.setenv("AUVP_LEAF_SWEEP_ALL", sweep)
        summ = ctx.rrt_explore_batch(lp.inits(name, 1), lp.seeds(name, 1), c["n_iter"], mode=c["mode"], **c["kw"])
        st = ctx.last_leaf_stats()
        assert int(summ[0]["n_leaves"]) == r["n_leaves"]
        assert minima <= st["leaves_resummed"] <= r["n_leaves"], (sweep, st, minima)
        assert st["nodes_visited"] == (r["n_nodes"] if sweep == "1" else len(s["marked"])), (sweep, st)
        assert st["points_visited"] == int(s["swept" if sweep == "1" else "pruned"]["slots"].sum()), (sweep, st)
        ctx.rrt_explore_batch(lp.inits(name, 1), lp.seeds(name, 1), c["n_iter"], mode=c["mode"], leaf_log=True, **c["kw"])
        st = ctx.last_leaf_stats()
        assert st["leaves_resummed"] == r["n_leaves"] and st["elements_resummed"] == int(r["leaf_cost"][:, 4].sum()), (sweep, st)

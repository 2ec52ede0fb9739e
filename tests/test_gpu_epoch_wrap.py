"""The 8-bit epoch tags of the tables that are NOT cleared per batch, across their wrap.

Planner_RRT's bucket table (planner_rrt_host.h: prrt_plant) and the A* visited words (astar_host.h: auvp_astar_batch,
auvp_astar_set_visited) count a word only if its top byte equals the batch's epoch; a new batch takes the next epoch, and the
table is zeroed when the tag has reached 255 (or the table outgrew what was last cleared).  Were that clear missing or too
short, a bucket would report members it does not have, a lattice cell would count as visited -- and the plan would still come
back with status 0.  Tags from 128 on also set the sign bit of (epoch << 24) | count.

Each test runs 260 batches on a FRESH handle, so the tag of every batch follows from the host's rule, which `TagModel`
restates (the constant beside `>= 255` in the two host files, which name this test): batch k carries tag k, batch 256 clears.  Every batch must equal the
first of its kind, and the batches around tag 1, the sign bit and the wrap are compared with the checker as well.

A stale word does harm only if it still carries the tag of the batch that reads it.  Batches that repeat the same few inputs
re-tag their own words every few batches, so nothing stale would survive until the wrap: the first batches therefore have
more episodes than the others, and so have the batches after the wrap, with other inputs -- the words of the extra episodes
keep their early tags until those tags come round again.  The model, fed with the words the checker says every episode
touches, asserts that this is so: no batch ever meets a stale word under the host's rule, and some do under the same rule
without its clears.  (A schedule of 260 batches that repeat two input sets stays green with the clear taken out.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_BATCHES = 260
WRAP_AT = 255  # a table is cleared by the batch that finds this tag taken: the constant of prrt_plant / auvp_astar_batch


def _fields_equal(a, b):
    return all(np.array_equal(a[n], b[n]) for n in a.dtype.names)


class TagModel:
    """The host's rule for a table of tagged words, restated: a batch takes the next tag; the table is cleared -- as far as the
    batch needs it (`clear_all`: all of it) -- when the tag has reached WRAP_AT or the batch needs more than was last cleared.
    batch(need, touched) -- sizes in words -- returns (tag, words the batch touches that still carry its tag from an earlier batch).
    wrap_clears / growth_clears = False: the same rule without one of its clears, i.e. what this test must be able to see."""

    def __init__(self, clear_all=False, wrap_clears=True, growth_clears=True):
        self.clear_all, self.wrap_clears, self.growth_clears = clear_all, wrap_clears, growth_clears
        self.cap = self.cleared = self.epoch = 0
        self.words = {}

    def batch(self, need, touched, wipe=0):
        fresh = need > self.cap  # a new allocation
        if fresh:
            self.cap, self.cleared, self.words = need, 0, {}
        wrap, growth = self.epoch >= WRAP_AT, need > self.cleared
        if fresh or wrap or (growth and self.growth_clears):
            upto = self.cap if self.clear_all else need
            if fresh or not wrap or self.wrap_clears:
                self.words = {w: t for w, t in self.words.items() if w >= upto}
            self.cleared, self.epoch = upto, 0
        self.epoch += 1
        if wipe:  # (a visited array the caller brings is written over the batch's part of the table, zeros included)
            self.words = {w: t for w, t in self.words.items() if w >= wipe}
        stale = [w for w in touched if self.words.get(w) == self.epoch]
        self.words.update((w, self.epoch) for w in touched)
        return self.epoch, stale


def _model_says(schedule, clear_all):
    """[(need, touched words[, wiped up to])] per batch -> the tags under the host's rule; asserts that no batch meets a stale word under it and
    that some batch would without the wrap's clear (and, where the schedule has growth after the wrap, without that clear)"""
    right = TagModel(clear_all)
    tags = []
    for b in schedule:
        tag, stale = right.batch(*b)
        assert not stale
        tags.append(tag)
    seen = {}
    for name, kw in (("wrap", dict(wrap_clears=False)), ("growth", dict(growth_clears=False))):
        m = TagModel(clear_all, **kw)
        seen[name] = [i for i, b in enumerate(schedule) if m.batch(*b)[1]]
    return tags, seen


# ---- Planner_RRT: the bucket table ----

PRRT_KERNELS = (
    ("prrt_kernel", dict(PRRT_ROWS=0, PRRT_PIPE=0)),
    ("prrt_rows_kernel", dict(PRRT_ROWS=1, PRRT_LAT=0, PRRT_ROWS_GRID=1)),
    ("prrt_pipe_kernel", dict(PRRT_ROWS=0, PRRT_PIPE=1)),
)
PRRT_KW = dict(freq=10, cell=5, subs=2)  # a 40 m side: 8 x 8 cells x 2 = 128 buckets, so that batches share buckets
PRRT_BUCKETS = 128
PRRT_MAX_STEP = 40
# against the checker, every episode: tags 1 and 2, the sign bit, the wrap -- and every batch that is not one of six episodes
PRRT_CHECKED = (1, 2, 3, 4, 5, 6, 7, 127, 128, 129, 130, 254, 255, 256, 257, 258, 259, 260, 261, 262)


def _prrt_inputs(w, which, E):
    """input set `which` on the one world: goals and seeds differ between sets, start headings between sets of another last digit
    (sets 11 and 21 start alike: the start node of a tree goes into the same bucket, whatever else the trees do)"""
    starts = np.tile(np.array([w["start"][0], w["start"][1], 0.0, 0.0]), (E, 1))
    starts[:, 2] = np.random.default_rng(40 + which % 10).uniform(-3.0, 3.0, E)
    rng = np.random.default_rng(140 + which)
    goals = np.column_stack([rng.uniform(w["rect"][0] + 4, w["rect"][2] - 4, E), rng.uniform(w["rect"][1] + 4, w["rect"][3] - 4, E)])
    seeds = np.arange(E, dtype=np.uint64) + 11 + 1000 * which
    return starts, goals, seeds


def _prrt_batch(ctx, w, inputs, kernel):
    """one batch on the handle: (records, trees, (occupied list, bucket counts), paths) of every episode"""
    from auv_sim_amd._prrt_lib import PlannerBatch
    name, opts = PRRT_KERNELS[kernel]
    for k in ("PRRT_ROWS", "PRRT_PIPE", "PRRT_LAT", "PRRT_ROWS_GRID"):
        ctx.set_option(k, opts.get(k))
    starts, goals, seeds = inputs
    pb = PlannerBatch(ctx, starts, goals, w["rect"], PRRT_MAX_STEP, seeds=seeds, **PRRT_KW)
    s = pb.plan().copy()
    # (an episode the speculative pipeline gave up on is redone by prrt_kernel, which is then the last kernel)
    assert ctx.prrt_last_kernel() == name or (name == "prrt_pipe_kernel" and ctx.pipeline_fallbacks()[0] > 0)
    if name == "prrt_rows_kernel" and len(starts) > 16:
        assert ctx.last_launch()[0] == 1  # 16 rows: they refill
    E = len(starts)
    return s, [pb.tree(e, s[e]) for e in range(E)], [pb.grid(e) for e in range(E)], [p.copy() for p in pb.paths(s)]


def _prrt_same(x, y):
    sx, tx, gx, px = x
    sy, ty, gy, py = y
    bad = [] if _fields_equal(sx, sy) else ["records"]
    for e in range(len(sx)):
        bad += [(e, k) for k in tx[e] if not np.array_equal(tx[e][k], ty[e][k])]
        if not (np.array_equal(gx[e][0], gy[e][0]) and np.array_equal(gx[e][1], gy[e][1])):
            bad.append((e, "occupied list / bucket counts"))
        if not np.array_equal(px[e], py[e]):
            bad.append((e, "path"))
    return bad


def _prrt_equals_checker(got, chk):
    s, trees, grids, paths = got
    bad = []
    for e, r in enumerate(chk):
        t = trees[e]
        if (s[e]["status"], s[e]["steps"], bool(s[e]["done"]), s[e]["n_nodes"], s[e]["n_points"], s[e]["rng_after"]) != \
                (r["status"], r["steps"], r["done"], r["n_nodes"], r["n_points"], r["rng_after"]):
            bad.append((e, "record"))
        if not (np.array_equal(t["parent"], r["parent"]) and np.array_equal(t["nodes"], r["nodes"][:, :4])
                and np.array_equal(t["node_bucket"], r["node_bucket"]) and np.array_equal(t["points"], r["points"])):
            bad.append((e, "tree"))
        if not (np.array_equal(grids[e][0], r["occupied"]) and np.array_equal(grids[e][1], r["bucket_counts"])):
            bad.append((e, "occupied list / bucket counts"))
        if r["done"] and not np.array_equal(paths[e], r["path"]):
            bad.append((e, "path"))
    return bad


def test_planner_bucket_table_across_the_tag_wrap(orc):
    """260 batches on one handle (and two more), the kernel cycling prrt_kernel / prrt_rows_kernel / prrt_pipe_kernel with the
    batch number; batch k carries tag k, batch 256 finds tag 255 taken, clears and carries tag 1 again.  Most batches have 6
    episodes, their input set alternating with the batch's parity.  Batches 2 .. 5 have 16, 15, 14, 13 episodes of inputs of their
    own: the words of episode 17 - k are touched by batches up to k only and keep tag k.  Batch 256 has 16 episodes and batches
    257 .. 260, tags 2 .. 5, again 16 .. 13, of other inputs: episode 15, 14 .. of theirs reads words that batch 2, 3 .. left
    under its tag.

    Batch 1 has 64 episodes (a table that outgrows the allocation is cleared and restarts the tags, so such a batch anywhere
    but in front would move the wrap past batch 260).  It makes the allocation:
    from then on every table is a part of it, and the wrap's clear covers only the 16 episodes batch 256 needs.  Batch 7, 64
    episodes again, leaves tag 7 in the words of episodes 16 .. 63, and batch 262, 64 episodes where tag 7 would be next, needs
    more than the wrap cleared and must get a clear of its own."""
    from auv_sim_amd import _lib, synth
    from oracle import orc_planner as op
    w = synth.make_rect_world(seed=3, n_obstacles=12, size=40.0, start=(8.0, 8.0), goal=(32.0, 33.0), obst_radius=(1.0, 2.5))
    sets = {0: _prrt_inputs(w, 0, 6), 1: _prrt_inputs(w, 1, 6), 20: _prrt_inputs(w, 20, 16)}
    for t in range(1, 5):
        sets[10 + t], sets[20 + t] = _prrt_inputs(w, 10 + t, 17 - t), _prrt_inputs(w, 20 + t, 17 - t)
    for i in (30, 31, 32):
        sets[i] = _prrt_inputs(w, i, 64)
    special = {1: 30, 7: 31, 262: 32, 256: 20}
    special.update({1 + t: 10 + t for t in range(1, 5)})
    special.update({256 + t: 20 + t for t in range(1, 5)})
    # (batch number, input set, kernel)
    plan = [(k, special.get(k, k % 2), k % 3) for k in range(1, N_BATCHES + 3)]
    assert all(k in PRRT_CHECKED for k in special)

    chk = {i: [op.planning(w["obstacles"], w["rect"], s[0][e], s[1][e], int(s[2][e]), PRRT_MAX_STEP, kind="portable", **PRRT_KW)
               for e in range(len(s[0]))] for i, s in sets.items()}
    assert all(r["status"] == 0 for c in chk.values() for r in c)
    assert all(sum(r["n_nodes"] for r in c) > 10 * len(c) for c in chk.values())  # trees that fill buckets
    # the words every batch touches, the tags the host gives it, and that stale words would be met without the clears
    touched = {i: [e * PRRT_BUCKETS + int(b) for e, r in enumerate(c) for b in np.flatnonzero(r["bucket_counts"])] for i, c in chk.items()}
    tags, seen = _model_says([(len(sets[i][0]) * PRRT_BUCKETS, touched[i]) for _, i, _ in plan], clear_all=False)
    assert tags == list(range(1, 256)) + list(range(1, 7)) + [1]
    assert {plan[i][0] for i in seen["wrap"]} >= {257, 258, 259, 260}, seen  # the batches whose tags batches 2 .. 5 had
    assert [plan[i][0] for i in seen["growth"]] == [262], seen

    ctx = _lib.Context(0)
    try:
        ctx.set_world(obstacles=w["obstacles"])
        first, bad, n_checked = {}, [], 0
        for k, i, kernel in plan:
            got = _prrt_batch(ctx, w, sets[i], kernel)
            ref = first.setdefault((i, kernel), got)
            bad += [(k, "first of its kind", x) for x in (_prrt_same(got, ref) if ref is not got else [])]
            if k in PRRT_CHECKED:
                n_checked += 1
                bad += [(k, "checker", x) for x in _prrt_equals_checker(got, chk[i])]
        assert n_checked == len(PRRT_CHECKED) and len(first) == 6 + 4 + 5 + 3
        print("bucket table: %d batches, %d against the checker, %d mismatches" % (len(plan), n_checked, len(bad)))
        assert not bad, bad[:10]
    finally:
        ctx.close()


# ---- A*: the visited words ----

ASTAR_VARIANTS = ("astar_fixLen", "astar_fixLenSOG")  # even / odd TAGS (the first batch has the larger table: 600 x 600)
ASTAR_STARTS = (np.array([(-280.0, -80.0), (-250.0, -60.0)]), np.array([(-270.0, -80.0), (-240.0, -60.0)]))  # a lattice step apart
# further searches of batches 1 .. 4 (4, 3, 2, 1 of them); the last search of batches 256 .. 259 starts a lattice step beside the
# last of batches 1 .. 4, the searches between stay out of reach (the world is 200 m wide, a search goes 80 m at most)
ASTAR_EXTRA = np.array([(-260.0, -40.0), (-230.0, -70.0), (-270.0, -60.0), (-240.0, -30.0)])
ASTAR_FAR = np.array([(-130.0, 70.0)])
ASTAR_LIMIT = 80.0       # some 60 to 130 expansions per search
ASTAR_VISITED = (250, 260)  # these batches (one of either variant) carry a visited array in (auvp_astar_set_visited + KEEP_VISITED): one on each side
ASTAR_CHECKED = (1, 2, 3, 4, 127, 128, 129, 130, 254, 255, 256, 257, 258, 259)  # against the checker, every search


def _bitmap(variant, E):
    """a visited_nodes array that is not empty where the searches go: every third diagonal of the 10 m lattice"""
    vx = 550 if variant == "astar_fixLen" else 600
    x, y = np.meshgrid(np.arange(vx), np.arange(600), indexing="ij")
    one = ((x % 10 == 0) & (y % 10 == 0) & ((x // 10 + y // 10) % 3 == 0)).astype(np.uint8)
    return np.stack([np.roll(one, 10 * e, axis=0) for e in range(E)])


def test_astar_visited_words_across_the_tag_wrap(orc):
    """260 batches of two searches on one handle, world set once.  Every batch takes one tag (a batch with a visited array takes
    its tag in auvp_astar_set_visited) and the first allocates the largest table, so batch k carries tag k, batch 256 clears
    and carries tag 1 again.  The variant alternates with the TAG (the two tables differ in width, and a word means a cell only
    to the variant that wrote it), the pair of starts every two batches.  Batches 1 .. 4 search from 4, 3, 2, 1 further starts:
    the words of search 6 - t are touched by batches 1 .. t only and keep tag t; the last search of batches 256 .. 259, tags
    1 .. 4, goes over the same cells from a lattice step beside."""
    from auv_sim_amd import _astar_lib as al, _lib, synth
    from oracle import orc_astar as oa
    w = synth.make_world(seed=12, n_obstacles=32, obst_radius=(2.0, 6.0), n_habitats=8, hab_radius=(10.0, 25.0))
    world = dict(obstacles=w["obstacles"], habitats=w["habitats"], polygon=w["polygon"], bins=w["bins"], cells=w["cells"], prob=w["prob"])
    kw = dict(weights=(0, 10, 10, 100), velocity=1.0, cap_nodes=4000)
    chk = {}

    def batch_of(k):
        tag = k if k <= WRAP_AT else k - WRAP_AT
        variant, starts = ASTAR_VARIANTS[tag % 2], ASTAR_STARTS[(k // 2) % 2]
        if k <= 4:
            starts = np.concatenate([starts, ASTAR_EXTRA[:5 - tag]])
        elif 256 <= k <= 259:
            starts = np.concatenate([starts] + [ASTAR_FAR] * (4 - tag) + [ASTAR_EXTRA[4 - tag:5 - tag] + np.array([10.0, 0.0])])
        return variant, starts, (_bitmap(variant, len(starts)) if k in ASTAR_VISITED else None)

    def checker(k):
        variant, starts, vis = batch_of(k)
        key = (variant, starts.tobytes(), vis is not None)
        if key not in chk:
            zeros = np.zeros((550 if variant == "astar_fixLen" else 600, 600), np.uint8)
            chk[key] = [oa.run(variant, starts[e], kind="portable", limit=ASTAR_LIMIT, visited=zeros if vis is None else vis[e],
                               **world, **kw) for e in range(len(starts))]
        return key, chk[key]

    def equals_checker(res, ref, with_bitmap):
        bad = []
        for e, (r, o) in enumerate(zip(res, ref)):
            if (r["status"], r["found"], r["n_nodes"], r["n_expansions"], r["n_children"], r["visited_count"]) != \
                    (o["status"], o["found"], o["n_nodes"], o["n_expansions"], o["n_children"], o["visited_count"]):
                bad.append((e, "record"))
            if not (np.array_equal(r["path"], o["path"]) and np.array_equal(r["cost_list"], o["cost_list"])
                    and np.array_equal(r["node_path"], o["node_path"])):
                bad.append((e, "path"))
            if with_bitmap and not np.array_equal(r["visited"], o["visited"]):
                bad.append((e, "visited array"))
        return bad

    # the words every batch touches (the cells it marks, and those of an array it brings), the tags, the stale words
    schedule = []
    for k in range(1, N_BATCHES + 1):
        variant, starts, vis = batch_of(k)
        one = (550 if variant == "astar_fixLen" else 600) * 600
        schedule.append((len(starts) * one, [e * one + int(c) for e, o in enumerate(checker(k)[1]) for c in np.flatnonzero(o["visited"])],
                         0 if vis is None else len(starts) * one))
    assert schedule[0][0] == max(b[0] for b in schedule)
    tags, seen = _model_says(schedule, clear_all=True)
    assert tags == list(range(1, 256)) + list(range(1, 6))
    assert {i + 1 for i in seen["wrap"]} >= {256, 257, 258, 259}, seen

    ctx = _lib.Context(0)
    try:
        ctx.set_world(**world)
        first, bad, n_checked, n_found = {}, [], 0, 0
        for k in range(1, N_BATCHES + 1):
            variant, starts, vis = batch_of(k)
            E = len(starts)
            limits = np.full(E, ASTAR_LIMIT)
            key, ref = checker(k)
            assert all(o["status"] == 0 and o["visited_count"] > 0 for o in ref)
            if vis is not None:
                res = al.run_batch(ctx, variant, starts, limits=limits, visited=vis, **kw)
                # (the array changes the search: otherwise this batch would say nothing of the words it uploaded)
                same = next(j for j in range(5, k) if batch_of(j)[0] == variant and np.array_equal(batch_of(j)[1], starts))
                assert [o["n_nodes"] for o in ref] != [o["n_nodes"] for o in checker(same)[1]]
                bad += [(k, "checker, visited array in", x) for x in equals_checker(res, ref, True)]
                continue
            got = al.run_batch_arrays(ctx, variant, starts, limits=limits, **kw)
            was = first.setdefault(key, got)
            if was is not got:
                if not _fields_equal(got["summ"], was["summ"]):
                    bad.append((k, "first of its kind", "records"))
                if not all(np.array_equal(got[n], was[n]) for n in ("off", "path", "cost_list", "node_path")):
                    bad.append((k, "first of its kind", "paths / cost lists"))
            if k in ASTAR_CHECKED:
                n_checked += 1
                s, off = got["summ"], got["off"]
                res = [dict(status=int(s[e]["status"]), found=bool(s[e]["found"]), n_nodes=int(s[e]["n_nodes"]),
                            n_expansions=int(s[e]["n_expansions"]), n_children=int(s[e]["n_children"]),
                            visited_count=int(s[e]["visited_count"]), path=got["path"][off[e]:off[e + 1]],
                            cost_list=got["cost_list"][off[e]:off[e + 1]], node_path=got["node_path"][off[e]:off[e + 1]])
                       for e in range(E)]
                n_found += sum(o["found"] for o in ref)
                bad += [(k, "checker", x) for x in equals_checker(res, ref, False)]
        assert len(first) == 4 + 8 and n_checked == len(ASTAR_CHECKED) and n_found > 0
        print("visited words: %d batches, %d against the checker, %d mismatches" % (N_BATCHES, n_checked, len(bad)))
        assert not bad, bad[:10]
    finally:
        ctx.close()

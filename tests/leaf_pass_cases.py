"""Cases of tests/test_gpu_leaf_pass_shapes.py and tests/test_gpu_leaf_pass_numerics.py (the leaf pass, csrc/rrt_leaf_body.h, on
deep trees, wide passes and extreme costs) and of tests/test_leaf_pass_cases.py (the properties those cases must have, asserted
with the CPU checker alone).  Not a test module.

The leaf pass branches on four quantities of a tree's shape, each against a constant of rrt_leaf_body.h:

  chain     nodes from a re-summed leaf to the root     64    the descriptor chunk of the ordered re-summation, step (A)
  elements  path elements of a re-summed leaf           256   RS_CAP, the re-summation window, steps (B) and (C)
  slots     path points of the 64 nodes of one pass     2048  the owner table; above it the owner comes from a binary search
  depth     longest parent-child chain inside one pass  -     rounds of the `pending` loop and of the marking sweep (<= 63)

A case is a dict: world (synth.make_world's arguments), mode, n_iter, seed (the first episode's; episode e runs seed + e), kw
(arguments of rrt_explore_batch / orc.rrt_explore other than the defaults).  `structure(r, max_traj_time)` computes the four
quantities from a checker result; `reference(name, e)` is the checker's result of episode e of a case, computed once and
read-only.

Measured with the checker (kind="portable"), episode 0 of every case; best = the best leaf, max = over the qualifying leaves;
slots and depth as (pruned passes, swept passes):

  case            leaves  best chain/elements  max chain/elements  slots          depth
  control            50       12 /   121           12 /  178         688 /  768    11 /  8
  plan_deep_a        91      113 /   318          147 /  417         125 /  130    63 / 31
  plan_deep_b        18      125 /   346          125 /  346         121 /  149    45 / 25
  plan_long          17      106 /   466          137 /  583         227 /  245    63 / 31
  bin_deep_a        129       91 /   243           91 /  243         176 /  288    58 / 25
  bin_deep_b        381       80 /   190           81 /  190         239 /  257    34 / 23
  bin_deep_c         57       66 /   111           66 /  111          45 /  278    63 / 10
  nn_deep          1173       52 /   178           85 /  320         167 /  164    26 / 16
  wide_a            113        5 /   268            9 /  418        5581 / 4673     5 /  6
  wide_b            159        6 /   247            8 /  270        3522 / 3043     5 /  5

(tests/test_leaf_pass_cases.py prints this table with `pytest -s`.)  The largest values over all cases: a chain of 147 nodes
(three descriptor chunks), 583 elements (three windows), 5 581 slots in a pass, and 63 dependent nodes in a pass -- a whole pass
in series.
"""
import functools

import numpy as np

CHAIN_CHUNK, RS_CAP, OWNER_TABLE, PASS = 64, 256, 2048, 64

_DEEP_PLAN = dict(world=dict(seed=55, n_obstacles=16), mode="plantime", n_iter=1500,
                  kw=dict(freq=6, v=10, max_traj_time=100.0))
_DEEP_BIN = dict(world=dict(seed=60, n_obstacles=32), mode="timebin", n_iter=1500,
                 kw=dict(freq=10, v=50, min_dist=0.2, max_traj_time=50.0, bin_interval=20.0))

CASES = {
    # the default-parameter case of tests/test_gpu_rows_kernel.py (o64_default): on the near side of every threshold
    "control": dict(world=dict(seed=51, n_obstacles=64), mode="timebin", n_iter=900, seed=4000, kw={}),
    "plan_deep_a": dict(_DEEP_PLAN, seed=4000),
    "plan_deep_b": dict(_DEEP_PLAN, seed=4003),
    "plan_long": dict(world=dict(seed=55, n_obstacles=16), mode="plantime", n_iter=1500, seed=4001,
                      kw=dict(freq=10, max_traj_time=2000.0)),
    # 50 / 20: the key past max_traj_time holds one member and is reset at each insertion -- the tree grows as a chain
    "bin_deep_a": dict(_DEEP_BIN, seed=4002),
    "bin_deep_b": dict(_DEEP_BIN, seed=4000),
    "bin_deep_c": dict(_DEEP_BIN, seed=4004),
    "nn_deep": dict(world=dict(seed=55, n_obstacles=16), mode="nn", n_iter=2000, seed=4000,
                    kw=dict(freq=6, v=20, min_dist=0.2, max_traj_time=40.0)),
    "wide_a": dict(world=dict(seed=51, n_obstacles=4), mode="timebin", n_iter=500, seed=4000,
                   kw=dict(freq=200, min_dist=0.1, max_traj_time=400.0)),
    "wide_b": dict(world=dict(seed=51, n_obstacles=16), mode="timebin", n_iter=600, seed=4000,
                   kw=dict(freq=150, max_traj_time=300.0)),
}
DEEP = ("plan_deep_a", "plan_deep_b", "plan_long", "bin_deep_a", "bin_deep_b", "bin_deep_c", "nn_deep")
DEEP_TIMEBIN = ("bin_deep_a", "bin_deep_b", "bin_deep_c")
WIDE = ("wide_a", "wide_b")
HORIZON_DEFAULT = 500.0


def horizon(name):
    return float(CASES[name]["kw"].get("max_traj_time", HORIZON_DEFAULT))


@functools.lru_cache(maxsize=None)
def world(name):
    from auv_sim_amd import synth
    return synth.make_world(**CASES[name]["world"])


def world_arrays(orc, w, prob=None, habitats=True):
    return orc.WorldArrays(w["obstacles"], w["habitats"] if habitats is True else habitats, w["polygon"], w["bins"], w["cells"],
                           w["prob"] if prob is None else prob)


def set_world(ctx, w, prob=None):
    ctx.set_world(w["obstacles"], w["habitats"], w["polygon"], w["bins"], w["cells"], w["prob"] if prob is None else prob)


def inits(name, E):
    """E start states at the world's start; the headings differ where the mode allows (nn mode steers from the nearest node
    whatever the heading; a heading changes every tree, so episode 0 keeps heading 0: the one the table above was measured at)"""
    w = world(name)
    init = np.zeros((E, 6))
    init[:, 0], init[:, 1] = w["start"]
    init[:, 2] = 0.37 * np.arange(E)
    return init


def seeds(name, E):
    return np.arange(CASES[name]["seed"], CASES[name]["seed"] + E, dtype=np.uint64)


def freeze(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def reference(name, e=0):
    """the CPU checker's result of episode e of a case (computed once; read-only)"""
    from oracle import orc
    c = CASES[name]
    w = world(name)
    r = orc.rrt_explore(world_arrays(orc, w), int(c["seed"]) + e, c["n_iter"], mode=c["mode"], init=inits(name, e + 1)[e],
                        kind="portable", **c["kw"])
    return freeze(r)


def structure(r, max_traj_time):
    """The shape quantities of a checker result r (nodes, parent, pt_cnt) at a horizon.  Returns a dict:
    leaves [n] qualifying leaves in creation order (node >= 1 with traj_t >= max_traj_time - 30); chain [n] / elems [n]: nodes
    on the leaf's chain to the root, and 1 per node plus pt_cnt of every non-root node; best_chain / best_elems / max_chain /
    max_elems; marked: the qualifying leaves and their ancestors; and for pruned (the marked ids, ascending, 64 per pass) and
    swept (every id): slots [passes] = the sum of pt_cnt over a pass, depth [passes] = the longest chain of nodes whose
    parent is in the same pass (0: no node's parent is)."""
    parent, pt_cnt = np.asarray(r["parent"]), np.asarray(r["pt_cnt"])
    n = len(parent)
    traj_t = np.asarray(r["nodes"])[:, 3]
    depth_of, elems_of = np.zeros(n, np.int64), np.zeros(n, np.int64)
    depth_of[0], elems_of[0] = 1, 1
    for m in range(1, n):  # (a parent precedes its children)
        depth_of[m] = depth_of[parent[m]] + 1
        elems_of[m] = elems_of[parent[m]] + 1 + pt_cnt[m]
    leaves = np.array([m for m in range(1, n) if traj_t[m] >= max_traj_time - 30], dtype=np.int64)
    marked = np.zeros(n, bool)
    for m in leaves:
        while m >= 0 and not marked[m]:
            marked[m] = True
            m = parent[m]

    def passes(ids):
        slots, depth = [], []
        for i in range(0, len(ids), PASS):
            p = ids[i:i + PASS]
            lo = p[0]
            d = {}
            for m in p:  # ascending
                d[m] = d[parent[m]] + 1 if parent[m] >= lo and parent[m] in d else 0
            slots.append(int(pt_cnt[p].sum()))
            depth.append(max(d.values()))
        return dict(slots=np.array(slots, dtype=np.int64), depth=np.array(depth, dtype=np.int64))
    out = dict(leaves=leaves, chain=depth_of[leaves], elems=elems_of[leaves], marked=np.flatnonzero(marked),
               pruned=passes(np.flatnonzero(marked)) if len(leaves) else dict(slots=np.zeros(0, np.int64), depth=np.zeros(0, np.int64)),
               swept=passes(np.arange(n)))
    best = int(r["best_leaf"])
    out["best_chain"] = int(depth_of[best]) if best >= 0 else 0
    out["best_elems"] = int(elems_of[best]) if best >= 0 else 0
    out["max_chain"] = int(out["chain"].max()) if len(leaves) else 0
    out["max_elems"] = int(out["elems"].max()) if len(leaves) else 0
    return out


def leaf_elements(r, leaf):
    """the (x, y, t) elements of a leaf in the reference's order: the leaf, its points last to first, its parent, ... the root"""
    nodes, parent, pt_off, pt_cnt, points = r["nodes"], r["parent"], r["pt_off"], r["pt_cnt"], r["points"]
    out = []
    m = int(leaf)
    while m >= 0:
        out.append((nodes[m, 0], nodes[m, 1], nodes[m, 3]))
        if parent[m] >= 0:
            for k in range(int(pt_cnt[m]) - 1, -1, -1):
                p = points[int(pt_off[m]) + k]
                out.append((p[0], p[1], p[4]))
        m = int(parent[m])
    return np.array(out, dtype=np.float64).reshape(-1, 3)


def strict_prefix_minima(totals):
    """how many entries are smaller than every entry before them (NaN: never): each becomes the best leaf at some point"""
    best, n = np.inf, 0
    for t in totals:
        if t < best:
            best, n = t, n + 1
    return n


# ---- exact comparison: no tolerance anywhere ------------------------------------------------------------------------------
def same(a, b):
    """equal shapes and values with a NaN equal to a NaN, and equal sign bits wherever the value is a number (so that -0.0 is
    not +0.0; a NaN's sign says how the hardware made it, not what the cost is)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(a, b, equal_nan=True):
        return False
    num = ~np.isnan(a)
    return bool(np.array_equal(np.signbit(a[num]), np.signbit(b[num])))


SUMMARY_FIELDS = ("status", "n_nodes", "n_points", "n_leaves", "leaf_elems", "best_leaf", "best_path_len", "best_cost",
                  "best_length", "rng_after", "n_draw32")


def expected_summary(r):
    """the checker's value of every field of SUMMARY_FIELDS (best_cost and best_length only with a best leaf: the device
    leaves them as they were without one)"""
    out = dict(status=r["status"], n_nodes=r["n_nodes"], n_points=r["n_points"], n_leaves=r["n_leaves"],
               leaf_elems=int(r["leaf_cost"][:, 4].sum()), best_leaf=r["best_leaf"],
               best_path_len=len(r["path"]) if r["best_leaf"] >= 0 else 0, rng_after=r["rng_after"], n_draw32=int(r["n_draw32"]))
    if r["best_leaf"] >= 0:
        out["best_cost"], out["best_length"] = r["best_cost"], r["best_length"]
    return out


def assert_summary(s, r, tag=None):
    for f, want in expected_summary(r).items():
        if f in ("best_cost", "best_length", "rng_after"):
            assert same(s[f], want), (tag, f, s[f], want)
        else:
            assert int(s[f]) == int(want), (tag, f, int(s[f]), int(want))


def assert_tree(t, r, tag=None):
    for k in ("parent", "pt_off", "pt_cnt"):
        assert np.array_equal(t[k], r[k]), (tag, k)
    for k in ("nodes", "points"):
        assert same(t[k], r[k]), (tag, k)


def assert_path(p, r, tag=None):
    if r["best_leaf"] >= 0:
        assert same(p, r["path"]), (tag, "path")
    else:
        assert len(p) == 0, (tag, "path")


def assert_leaf_log(log, r, tag=None):
    """ctx.leaf_log == the checker's leaf_cost (all six columns) and leaf_iter"""
    cost, it = log
    assert cost.shape == r["leaf_cost"].shape, (tag, cost.shape, r["leaf_cost"].shape)
    for k in range(len(cost)):
        assert same(cost[k], r["leaf_cost"][k]), (tag, "leaf", k, cost[k], r["leaf_cost"][k])
    assert np.array_equal(it, r["leaf_iter"]), (tag, "leaf_iter")


def assert_same_runs(a, b, tag=None):
    """two device runs (summaries, trees, paths[, leaf logs]) agree in every field"""
    sa, ta, pa = a[:3]
    sb, tb, pb = b[:3]
    for e in range(len(sa)):
        for f in SUMMARY_FIELDS + ("iters_run",):
            x, y = sa[e][f], sb[e][f]
            assert same(x, y) if np.asarray(x).dtype.kind == "f" else np.array_equal(x, y), (tag, e, f, x, y)
        for k in ta[e]:
            assert ta[e][k].tobytes() == tb[e][k].tobytes(), (tag, e, k)
        assert same(pa[e], pb[e]), (tag, e, "path")
    if len(a) > 3 and len(b) > 3 and a[3] is not None and b[3] is not None:
        for e in range(len(sa)):
            assert same(a[3][e][0], b[3][e][0]) and np.array_equal(a[3][e][1], b[3][e][1]), (tag, e, "leaf log")


def table_row(name, e=0):
    s = structure(reference(name, e), horizon(name))
    mx = lambda a: int(a.max()) if len(a) else 0  # noqa: E731
    return "%-14s %6d   %6d / %5d       %6d / %5d       %5d / %4d   %3d / %2d" % (
        name, len(s["leaves"]), s["best_chain"], s["best_elems"], s["max_chain"], s["max_elems"], mx(s["pruned"]["slots"]),
        mx(s["swept"]["slots"]), mx(s["pruned"]["depth"]), mx(s["swept"]["depth"]))

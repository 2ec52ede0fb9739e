"""ctypes binding of the A* entry points of libauvplan.so (auvp_astar_*, include/auvplan.h)."""
import ctypes as C

import numpy as np

from . import _lib
from ._cabi import ASTAR_SUMMARY_DTYPE, AstarParams  # noqa: F401

VARIANTS = {"astar": 0, "astar_real": 1, "astar_fixLen": 2, "astar_fixLenSOG": 3}


def _bind():
    return _lib.load()


def sets_topn(ctx):
    """[G, T, C + 1]: the top-n tables of ctx's probability sets as the searches read them (auvp_astar_sets_topn)"""
    L = _bind()
    out = np.zeros((max(ctx.n_prob_sets, 1), ctx.world_sizes.get("T", 0), ctx.world_sizes.get("C", 0) + 1))
    ctx._chk(L.auvp_astar_sets_topn(ctx.h, _lib._p(out)))
    return out[:ctx.n_prob_sets]


def _launch(L, ctx, E, starts, g, lim, p, flags, set_of):
    """auvp_astar_batch, or auvp_astar_batch_sets with set_of [E]: instance e against probability set set_of[e]"""
    if set_of is None:
        return ctx._chk(L.auvp_astar_batch(ctx.h, E, _lib._p(starts), _lib._p(g) if g is not None else None,
                                           _lib._p(lim) if lim is not None else None, C.byref(p), flags))
    so = _lib._arr(set_of, np.int32, (-1,))
    if len(so) != E:
        raise ValueError("set_of has %d entries, expected %d" % (len(so), E))
    if g is not None:
        raise ValueError("set_of is astar_fixLenSOG's: no goals")
    return ctx._chk(L.auvp_astar_batch_sets(ctx.h, E, _lib._p(starts), _lib._p(lim) if lim is not None else None, C.byref(p), flags,
                                            _lib._p(so)))


def run_batch_arrays(ctx, variant, starts, goals=None, limits=None, box=(0, 0, 0, 0), velocity=1.0, weights=(0, 0, 0, 0),
                     cap_nodes=20000, set_of=None):
    """E searches in one launch + one path-extraction launch; results as arrays (no per-instance Python work):
    summaries [E], offsets [E+1] and the concatenated path / cost_list / node_path / smooth_path rows."""
    L = _bind()
    starts = _lib._f64(starts, (-1, 2))
    E = len(starts)
    p = AstarParams()
    p.variant, p.cap_nodes, p.velocity = VARIANTS[variant], int(cap_nodes), float(velocity)
    wts = list(weights) + [0.0] * (4 - len(weights))
    for i in range(4):
        p.box[i] = float(box[i])
        p.w[i] = float(wts[i])
    g = _lib._f64(goals, (-1, 2)) if goals is not None else None
    lim = _lib._f64(limits).reshape(E) if limits is not None else None
    _launch(L, ctx, E, starts, g, lim, p, 0, set_of)
    batch_ms = ctx.last_kernel_ms()
    summ = np.zeros(E, dtype=ASTAR_SUMMARY_DTYPE)
    ctx._chk(L.auvp_astar_summaries(ctx.h, _lib._p(summ)))
    lens = np.where(summ["found"] != 0, summ["path_len"], 0).astype(np.int64)
    off = np.zeros(E + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    n = max(int(off[-1]), 1)
    path, cost, npath, smooth = np.zeros((n, 3)), np.zeros(n), np.zeros((n, 8)), np.zeros((n, 3))
    ctx._chk(L.auvp_astar_paths(ctx.h, _lib._p(off), _lib._p(path), _lib._p(cost), _lib._p(npath),
                                _lib._p(smooth)))
    return dict(summ=summ, off=off, path=path, cost_list=cost, node_path=npath, smooth_path=smooth, batch_ms=batch_ms)


def run_batch(ctx, variant, starts, goals=None, limits=None, box=(0, 0, 0, 0), velocity=1.0, weights=(0, 0, 0, 0),
              cap_nodes=20000, exp_log=False, visited=None, set_of=None, return_visited=False):
    """E searches over ctx's world in one launch.  Returns a list of per-instance dicts.  set_of [E] (astar_fixLenSOG): instance e
    reads the shark-occupancy table and its top-n table of ctx's probability set set_of[e] (Context.set_prob_sets).
    return_visited: "visited" (the fixLen variants' bitmap after the search) also without a bitmap carried in."""
    L = _bind()
    starts = _lib._f64(starts, (-1, 2))
    E = len(starts)
    p = AstarParams()
    p.variant, p.cap_nodes, p.velocity = VARIANTS[variant], int(cap_nodes), float(velocity)
    wts = list(weights) + [0.0] * (4 - len(weights))
    for i in range(4):
        p.box[i] = float(box[i])
        p.w[i] = float(wts[i])
    g = _lib._f64(goals, (-1, 2)) if goals is not None else None
    lim = _lib._f64(limits).reshape(E) if limits is not None else None
    flags = 1 if exp_log else 0
    if visited is not None:  # [E, vx, 600] uint8: the solver's visited_nodes carried over from earlier calls
        vis = _lib._arr(visited, np.uint8)
        ctx._chk(L.auvp_astar_set_visited(ctx.h, E, p.variant, _lib._p(vis)))
        flags |= 8
    _launch(L, ctx, E, starts, g, lim, p, flags, set_of)
    summ = np.zeros(E, dtype=ASTAR_SUMMARY_DTYPE)
    ctx._chk(L.auvp_astar_summaries(ctx.h, _lib._p(summ)))
    lens = np.where(summ["found"] != 0, summ["path_len"], 0).astype(np.int64)
    off = np.zeros(E + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    n = max(int(off[-1]), 1)
    path, cost, npath, smooth = np.zeros((n, 3)), np.zeros(n), np.zeros((n, 8)), np.zeros((n, 3))
    ctx._chk(L.auvp_astar_paths(ctx.h, _lib._p(off), _lib._p(path), _lib._p(cost), _lib._p(npath),
                                _lib._p(smooth)))
    ctx._chk(L.auvp_astar_summaries(ctx.h, _lib._p(summ)))  # smooth_len is filled by the path pass
    H = ctx.world_sizes.get("H", 0)
    out = []
    for e in range(E):
        s = summ[e]
        a, b = int(off[e]), int(off[e + 1])
        r = {"status": int(s["status"]), "found": bool(s["found"]), "n_nodes": int(s["n_nodes"]),
             "n_expansions": int(s["n_expansions"]), "n_children": int(s["n_children"]),
             "visited_count": int(s["visited_count"]), "path": path[a:b].copy(), "cost_list": cost[a:b].copy(),
             "node_path": npath[a:b].copy(), "smooth_path": smooth[a:a + int(s["smooth_len"])].copy()}
        hl = np.zeros(max(H, 1), np.int32)
        if H:
            ctx._chk(L.auvp_astar_hab_left(ctx.h, e, _lib._p(hl)))
        r["hab_left"] = hl[:int(s["n_hab_left"])]
        if p.variant >= 2 and (visited is not None or return_visited):
            vb = np.zeros((550 if p.variant == 2 else 600, 600), dtype=np.uint8)
            ctx._chk(L.auvp_astar_get_visited(ctx.h, e, _lib._p(vb)))
            r["visited"] = vb
        if exp_log:
            ex = np.zeros((max(int(s["n_expansions"]), 1), 8))
            ctx._chk(L.auvp_astar_exp_log(ctx.h, e, _lib._p(ex)))
            r["expansions"] = ex[:int(s["n_expansions"])]
        out.append(r)
    return out

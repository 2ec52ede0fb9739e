"""Seeded inputs of tests/test_gpu_sog_tiles.py (SharkOccupancyGrid.convert on the device) and tests/test_sog_tile_inputs.py
(the properties those inputs must have, asserted with numpy and the CPU checker alone).  Not a test module.

A case is a dict of convert_arrays' arguments without the detection range: cells [C,4], box, cell_size, bin_interval,
traj_len [S], pts [sum(traj_len),3].  `reference(name, count)` runs the checker once per (case, window radius) and keeps the
result; callers must not write to it.

The host-side facts the cases are built around are restated here from csrc/sog_kernels.h: the LDS tile's pitch and size
(sog_tile_q / sog_tile_bytes, the launch rule of auvp_sog_convert) and the sizing of the (x, y) bucket index of
sog_count_kernel (NBX, NBY, the table and item budgets, the halving loop)."""
import functools
import math

import numpy as np

TILE_ROWS, TILE_COLS = 16, 64  # SOG_TH, SOG_TW
LDS_RULE_BYTES = 150 * 1024    # auvp_sog_convert: the tiled kernels run while sog_tile_bytes(count) <= 150 KiB
BOX = (-7.0, 3.0, 123.0, 37.0)  # 35 rows x 131 columns of 1 m cells: tiles of 64 + 64 + 3 columns, 16 + 16 + 3 rows
CS, BI = 1.0, 10.0
ROWS, COLS = 35, 131


def tile_q(count):
    """sog_tile_q: doubles per quarter row of the LDS tile"""
    return (((TILE_COLS + 2 * count + 1 + 3) // 4 + 7) // 8) * 8 + 4


def tile_bytes(count):
    """sog_tile_bytes: two buffers of (16 + 2 count) rows of 4 Q doubles"""
    return 2 * (TILE_ROWS + 2 * count) * 4 * tile_q(count) * 8


def lds_boundary(limit=LDS_RULE_BYTES):
    """(the last radius that runs from LDS tiles, the first that falls back to the per-cell sweep)"""
    last = max(c for c in range(1, 256) if tile_bytes(c) <= limit)
    assert all(tile_bytes(c) <= limit for c in range(1, last + 1)) and tile_bytes(last + 1) > limit
    return last, last + 1


def detect_range(count, cs=CS):
    """a detection range whose window radius ceil(detect_range / cell_size) is `count` cells"""
    return (count - 0.5) * cs


def grid_shape(box, cs):
    return int(math.ceil(box[3] - box[1]) / cs) + 1, int(math.ceil(box[2] - box[0]) / cs) + 1


def cell_index(cells, box, cs, rows, cols):
    """cellToIndex with Python's negative-index wrap: (row, col) per listed cell"""
    col = np.trunc((cells[:, 0] - box[0]) / cs).astype(int)
    row = np.trunc((cells[:, 1] - box[1]) / cs).astype(int)
    return np.where(row < 0, row + rows, row), np.where(col < 0, col + cols, col)


def multiplicity(case):
    rows, cols = grid_shape(case["box"], case["cell_size"])
    m = np.zeros((rows, cols), dtype=int)
    if len(case["cells"]):
        r, c = cell_index(case["cells"], case["box"], case["cell_size"], rows, cols)
        np.add.at(m, (r, c), 1)
    return m


def bucket_plan(cells):
    """The sizing of the bucket index in auvp_sog_convert, restated: NBX / NBY from the smallest positive cell width / height
    (clamped to 1024), the table budget max(4096, 8 C), the item budget 16 C + 4096, and the halving loop.  Returns the first
    and the final (NBX, NBY), the item count at the first size and whether the first size is over either budget."""
    cells = np.asarray(cells, dtype=np.float64)
    C = len(cells)
    lo, hi, ylo, yhi = cells[:, 0].min(), cells[:, 2].max(), cells[:, 1].min(), cells[:, 3].max()
    w, h = cells[:, 2] - cells[:, 0], cells[:, 3] - cells[:, 1]
    wmin = w[w > 0].min() if (w > 0).any() else math.inf
    hmin = h[h > 0].min() if (h > 0).any() else math.inf
    span, yspan = hi - lo, yhi - ylo
    nbx = int(min(1024.0, max(1.0, math.ceil(span / wmin)))) if span > 0 and math.isfinite(wmin) else 1
    nby = int(min(1024.0, max(1.0, math.ceil(yspan / hmin)))) if yspan > 0 and math.isfinite(hmin) else 1

    def bucket(v, v0, inv, nb):
        return np.clip(np.floor((v - v0) * inv), 0, nb - 1).astype(np.int64)

    def items(nx, ny):
        inv_w, inv_h = (nx / span if span > 0 else 0.0), (ny / yspan if yspan > 0 else 0.0)
        return int(((bucket(cells[:, 2], lo, inv_w, nx) - bucket(cells[:, 0], lo, inv_w, nx) + 1)
                    * (bucket(cells[:, 3], ylo, inv_h, ny) - bucket(cells[:, 1], ylo, inv_h, ny) + 1)).sum())
    table_budget, item_budget = max(4096, 8 * C), 16 * C + 4096
    first = (nbx, nby)
    first_items = items(nbx, nby)
    over = nbx * nby > table_budget or first_items > item_budget
    halvings = 0
    while not (nbx == 1 and nby == 1) and (nbx * nby > table_budget or items(nbx, nby) > item_budget):
        nbx, nby = max(1, nbx // 2), max(1, nby // 2)
        halvings += 1
    return {"first": first, "final": (nbx, nby), "first_items": first_items, "table_budget": table_budget,
            "item_budget": item_budget, "over_budget": over, "halvings": halvings}


def point_keys(case):
    """per point: bin * S + shark, or -1 for a point in no bin (first bin whose closed interval holds the time stamp; the
    number of bins from the LAST point of the longest-running trajectory, as createBinList has it)"""
    tl, pts, bi = np.asarray(case["traj_len"]), case["pts"], case["bin_interval"]
    ends = np.cumsum(tl)
    longest = 0.0
    for s, n in enumerate(tl):
        if n > 0 and pts[ends[s] - 1, 2] > longest:
            longest = pts[ends[s] - 1, 2]
    T = int(math.floor(longest / bi))
    b = np.full(len(pts), -1)
    for q in reversed(range(T)):
        b[(pts[:, 2] >= q * bi) & (pts[:, 2] <= (q + 1) * bi)] = q
    shark = np.repeat(np.arange(len(tl)), tl)
    return np.where(b >= 0, b * len(tl) + shark, -1), T


# ---------------------------------------------------------------------------------------------------------------------------
def _raster(box, cs, r0=0, r1=None, c0=0, c1=None):
    nrow, ncol = int(math.ceil((box[3] - box[1]) / cs)), int(math.ceil((box[2] - box[0]) / cs))
    r, c = np.meshgrid(np.arange(r0, nrow if r1 is None else r1), np.arange(c0, ncol if c1 is None else c1), indexing="ij")
    return r.ravel(), c.ravel()


def _cells_at(box, cs, r, c, dx=0.0, dy=0.0):
    r, c = np.asarray(r, dtype=np.float64), np.asarray(c, dtype=np.float64)
    return np.stack([box[0] + (c + dx) * cs, box[1] + (r + dy) * cs, box[0] + (c + dx + 1) * cs, box[1] + (r + dy + 1) * cs], axis=1)


def _traj(rng, n, box, cs, bi, tmax, margin=5.0):
    """n points over the box plus a margin, a fifth of the coordinates snapped onto cell edges, a tenth of the time stamps
    exactly on a bin edge; sorted by time"""
    x = rng.uniform(box[0] - margin, box[2] + margin, size=n)
    y = rng.uniform(box[1] - margin, box[3] + margin, size=n)
    snap = rng.random(n) < 0.2
    x[snap] = box[0] + cs * np.round((x[snap] - box[0]) / cs)
    snap = rng.random(n) < 0.2
    y[snap] = box[1] + cs * np.round((y[snap] - box[1]) / cs)
    t = rng.uniform(0.0, tmax, size=n)
    edge = rng.random(n) < 0.1
    t[edge] = bi * rng.integers(0, 3, size=int(edge.sum()))
    return np.stack([x, y, np.sort(t)], axis=1)


def _case(cells, traj, box=BOX, cs=CS, bi=BI):
    return {"cells": np.ascontiguousarray(cells, dtype=np.float64).reshape(-1, 4), "box": box, "cell_size": cs, "bin_interval": bi,
            "traj_len": np.array([len(t) for t in traj], dtype=np.int32),
            "pts": np.concatenate([np.asarray(t, dtype=np.float64).reshape(-1, 3) for t in traj])}


FORCED_DUPLICATES = [(5, 60), (12, 129), (3, 128), (33, 70), (20, 66), (14, 10)]  # (row, col): beside the column and row seams


def _seam_cells(rng):
    """the raster of unit cells thinned to 85 %; the tile rows 0-15 x columns 64-127 listed exactly once (the `plain` path),
    the tile rows 16-31 x columns 0-63 unlisted; 40 cells outside the plain tile listed twice, 10 of them three times;
    shuffled"""
    keep = rng.random((ROWS - 1, COLS - 1)) < 0.85
    keep[0:16, 64:128] = True
    keep[16:32, 0:64] = False
    for r, c in FORCED_DUPLICATES:
        keep[r, c] = True
    in_plain = np.zeros_like(keep)
    in_plain[0:16, 64:128] = True
    cand = np.argwhere(keep & ~in_plain)
    forced = np.array(FORCED_DUPLICATES)
    rest = np.array([rc for rc in cand.tolist() if tuple(rc) not in set(FORCED_DUPLICATES)])
    dup = np.concatenate([forced, rest[rng.choice(len(rest), 40 - len(forced), replace=False)]])
    once = np.argwhere(keep)
    rc = np.concatenate([once, dup, dup[:10]])
    rc = rc[rng.permutation(len(rc))]
    return _cells_at(BOX, CS, rc[:, 0], rc[:, 1])


def _seam_traj(rng):
    a, b, c = _traj(rng, 300, BOX, CS, BI, 24.0), np.array([[40.25, 9.5, 10.0]]), _traj(rng, 170, BOX, CS, BI, 19.0)
    a[-1, 2] = 24.5  # the longest last time stamp: two bins; the points of (20, 24.5] are in no bin
    return [a, b, c]


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


def _seams():
    """part 1: three column tiles (64, 64, 3 wide), three row tiles, plain / empty / mixed tiles side by side"""
    rng = np.random.default_rng(20240611)
    return _case(_seam_cells(rng), _seam_traj(rng))


def _narrow(box, seed, dup=3):
    def build():
        rng = np.random.default_rng(seed)
        r, c = _raster(box, CS, r1=max(1, int(math.ceil(box[3] - box[1]))))
        cells = _cells_at(box, CS, r, c)
        cells = cells[rng.random(len(cells)) < 0.9]
        cells = np.concatenate([cells, cells[:dup]])
        cells = cells[rng.permutation(len(cells))]
        tb = (box[0], box[1], box[2], max(box[3], box[1] + 1.0))  # (a zero-height box: its one row of cells is 1 m high)
        traj = [_traj(rng, n, tb, CS, BI, 24.0, margin=1.5) for n in (90, 1, 45)]
        traj[0][-1, 2] = 24.5
        return _case(cells, traj, box=box)
    return build


def _with_extremes(cells, traj, rng):
    """appends to trajectory 0 points exactly on the smallest / largest x and y over all cells and one ulp outside each of
    them (clamped buckets; the latter contained by nothing), at the mid-height / mid-width of the cell that sets the extreme"""
    k0, k1, k2, k3 = cells[:, 0].argmin(), cells[:, 2].argmax(), cells[:, 1].argmin(), cells[:, 3].argmax()
    lo, hi, ylo, yhi = cells[k0, 0], cells[k1, 2], cells[k2, 1], cells[k3, 3]
    ym0, ym1 = 0.5 * (cells[k0, 1] + cells[k0, 3]), 0.5 * (cells[k1, 1] + cells[k1, 3])
    xm2, xm3 = 0.5 * (cells[k2, 0] + cells[k2, 2]), 0.5 * (cells[k3, 0] + cells[k3, 2])
    inf = math.inf
    xy = [(lo, ym0), (np.nextafter(lo, -inf), ym0), (hi, ym1), (np.nextafter(hi, inf), ym1),
          (xm2, ylo), (xm2, np.nextafter(ylo, -inf)), (xm3, yhi), (xm3, np.nextafter(yhi, inf)),
          (lo, ylo), (hi, yhi), (np.nextafter(lo, -inf), np.nextafter(ylo, -inf)), (np.nextafter(hi, inf), np.nextafter(yhi, inf))]
    return _append_points(traj, xy, rng)


def _append_points(traj, xy, rng):
    extra = np.array([[x, y, t] for (x, y), t in zip(xy, rng.uniform(0.5, 19.5, size=len(xy)))])
    t0 = np.concatenate([traj[0], extra])
    t0 = t0[np.argsort(t0[:, 2], kind="stable")]
    return [t0] + list(traj[1:])


def _big_cell(first):
    def build():
        rng = np.random.default_rng(31)
        r, c = _raster(BOX, CS)
        small = _cells_at(BOX, CS, r, c)
        small = small[rng.random(len(small)) < 0.85]
        small = small[rng.permutation(len(small))]
        big = np.array([[BOX[0], BOX[1], BOX[2], BOX[3]]])
        cells = np.concatenate([big, small] if first else [small, big])
        return _case(cells, _with_extremes(cells, _seam_traj(rng), rng))
    return build


SLIVER = 1e-3


def _slivers():
    rng = np.random.default_rng(32)
    r, c = _raster(BOX, CS)
    pick = rng.choice(len(r), 200, replace=False)
    normal = _cells_at(BOX, CS, r[pick], c[pick])
    corners = _cells_at(BOX, CS, [0, 33], [0, 129])  # (so that the extremes of x and y belong to ordinary cells)
    sx = _cells_at(BOX, CS, rng.integers(0, 34, 20), rng.integers(0, 130, 20), dx=0.37)
    sx[:, 2] = sx[:, 0] + SLIVER                      # 1e-3 wide, 1 high
    sy = _cells_at(BOX, CS, rng.integers(0, 34, 20), rng.integers(0, 130, 20), dy=0.61)
    sy[:, 3] = sy[:, 1] + SLIVER                      # 1 wide, 1e-3 high
    zero = _cells_at(BOX, CS, [17], [66], dx=0.25)
    zero[:, 2] = zero[:, 0]                           # zero width: a vertical line 1 high
    cells = np.concatenate([normal, corners, sx, sy, zero])
    order = rng.permutation(len(cells))
    cells = cells[order]
    traj = _seam_traj(rng)
    xy = []
    for s in sx[:6]:   # exactly on a sliver: its two edges and inside it
        xy += [(s[0], s[1] + 0.5), (s[2], s[1] + 0.25), (s[0] + 0.5 * SLIVER, s[1] + 0.75)]
    for s in sy[:6]:
        xy += [(s[0] + 0.5, s[1]), (s[0] + 0.25, s[3]), (s[0] + 0.75, s[1] + 0.5 * SLIVER)]
    z = zero[0]
    xy += [(z[0], z[1]), (z[0], z[1] + 0.5), (z[0], z[3]), (np.nextafter(z[0], math.inf), z[1] + 0.5)]
    traj = _append_points(traj, xy, rng)
    return _case(cells, _with_extremes(cells, traj, rng))


def _overlap():
    """unit cells at whole and half offsets over rows 10-21 x columns 58-70 (both seams inside): a point lies in up to four"""
    rng = np.random.default_rng(33)
    r, c = _raster(BOX, CS, 10, 22, 58, 71)
    cells = np.concatenate([_cells_at(BOX, CS, r, c, dx, dy) for dx in (0.0, 0.5) for dy in (0.0, 0.5)])
    cells = cells[rng.random(len(cells)) < 0.8]
    cells = cells[rng.permutation(len(cells))]
    region = (BOX[0] + 58, BOX[1] + 10, BOX[0] + 71.5, BOX[1] + 22.5)
    traj = [_traj(rng, n, region, 0.5, BI, 24.0, margin=2.0) for n in (300, 1, 170)]
    traj[0][-1, 2] = 24.5
    return _case(cells, _with_extremes(cells, traj, rng))


def _wrapped():
    """cells one and two cell widths left of / below the box: cellToIndex gives -1 / -2, which index from the far end"""
    rng = np.random.default_rng(34)
    r, c = _raster(BOX, CS)
    pick = rng.choice(len(r), 700, replace=False)  # (8 C above the 132 x 36 buckets: the index keeps its first size)
    normal = _cells_at(BOX, CS, r[pick], c[pick])
    left = _cells_at(BOX, CS, [2, 9, 20, 33, 15, 16], [-1, -2, -1, -2, -1, -2])
    below = _cells_at(BOX, CS, [-1, -2, -1, -2, -1, -2], [5, 63, 64, 100, 128, 129])
    corner = _cells_at(BOX, CS, [-1, -2], [-1, -2])
    cells = np.concatenate([normal, left, below, corner])
    cells = cells[rng.permutation(len(cells))]
    traj = _seam_traj(rng)
    xy = [(0.5 * (w[0] + w[2]), 0.5 * (w[1] + w[3])) for w in np.concatenate([left, below, corner])]
    return _case(cells, _append_points(traj, xy, rng))


def _empty_list():
    rng = np.random.default_rng(35)
    return _case(np.zeros((0, 4)), _seam_traj(rng))


def _nan_points():
    """the seam case with NaN x, NaN y, NaN x and y (no cell, but counted in the bin's normaliser) and one NaN time stamp (no
    bin); none of them is a trajectory's last point"""
    base = case("seams")
    pts = base["pts"].copy()
    pts[[3, 70, 131], 0] = np.nan
    pts[[40, 131, 250], 1] = np.nan
    pts[310, 0] = np.nan
    pts[200, 2] = np.nan
    out = dict(base)
    out["pts"] = pts
    return out


def _many_short():
    """70 sharks of 1..3 points: a wavefront of 64 points holds dozens of (bin, shark) keys; the time stamps past 20 are in no
    bin; the number of points is no multiple of 64"""
    rng = np.random.default_rng(41)
    lens = rng.integers(1, 4, size=70)
    lens[-1] += (1 if lens.sum() % 64 == 0 else 0)
    traj = [_traj(rng, int(n), BOX, CS, BI, 29.0) for n in lens]
    traj[7][-1, 2] = 29.5  # the longest: two bins
    return _case(_seam_cells(rng), traj)


def _empty_traj():
    rng = np.random.default_rng(42)
    traj = [_traj(rng, n, BOX, CS, BI, 24.0) for n in (40, 0, 30, 1, 25)]
    traj[0][-1, 2] = 24.5
    return _case(_seam_cells(rng), traj)


def _no_bin():
    """valid, late (past the last bin) and negative time stamps interleaved point by point: lanes leave before the ballot in
    the middle of a wavefront"""
    rng = np.random.default_rng(43)
    traj = []
    for n in (200, 61, 90):
        p = _traj(rng, n, BOX, CS, BI, 20.0)
        i = np.arange(n)
        p[:, 2] = np.where(i % 3 == 0, rng.uniform(0.0, 20.0, n), np.where(i % 3 == 1, rng.uniform(20.01, 24.9, n), -rng.uniform(0.1, 5.0, n)))
        traj.append(p)
    traj[0][-1, 2] = 24.9
    return _case(_seam_cells(rng), traj)


def _unsorted():
    """trajectory 0 is not sorted by time and runs to 58 s, but its LAST point (21.0) defines the number of bins: two"""
    rng = np.random.default_rng(44)
    traj = [_traj(rng, 150, BOX, CS, BI, 58.0), _traj(rng, 80, BOX, CS, BI, 19.0)]
    traj[0] = traj[0][rng.permutation(150)]
    traj[0][-1, 2] = 21.0
    return _case(_seam_cells(rng), traj)


_BUILDERS = {
    "seams": _seams,
    "cols3": _narrow((2.0, -1.0, 4.0, 9.0), 21),         # 11 rows x 3 columns: narrower than a thread's four cells
    "rows1": _narrow((0.0, 5.0, 70.0, 5.0), 22),         # 1 row x 71 columns on a zero-height box
    "interior_64x16": _narrow((-3.0, 1.0, 61.0, 17.0), 23),  # 17 x 65: the +1 row and column open a second tile each
    "big_last": _big_cell(False), "big_first": _big_cell(True), "slivers": _slivers, "overlap": _overlap,
    "wrapped": _wrapped, "empty_list": _empty_list, "nan_points": _nan_points,
    "many_short": _many_short, "empty_traj": _empty_traj, "no_bin": _no_bin, "unsorted": _unsorted,
}
NARROW = ("cols3", "rows1", "interior_64x16")
BUCKETS = ("big_last", "big_first", "slivers", "overlap", "wrapped", "empty_list", "nan_points")
ATOMICS = ("many_short", "empty_traj", "no_bin", "unsorted")
SEAM_COUNTS = tuple(range(1, 10)) + lds_boundary()
# every (case, radius) the device tests run; the CPU-only module asserts the checker's status 0 on each
ALL_RUNS = ([("seams", c) for c in SEAM_COUNTS] + [(n, c) for n in NARROW for c in (1, 4, 9)] + [(n, 2) for n in BUCKETS]
            + [(n, 1) for n in ATOMICS])


@functools.lru_cache(maxsize=None)
def reference(name, count):
    """the CPU checker's result for a case at a window radius (computed once; read-only)"""
    from oracle import orc_sog
    c = case(name)
    ref = orc_sog.convert(c["cells"], c["box"], c["cell_size"], c["bin_interval"], detect_range(count, c["cell_size"]),
                          c["traj_len"], c["pts"], kind="portable")
    for k in ("bins", "grids", "occ", "auv"):
        ref[k].setflags(write=False)
    return ref

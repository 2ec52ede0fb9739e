"""The world's device tables, built without a GPU: csrc/world_tables.h (the pure host functions auvp_world_set uploads the
results of) compiled into tests/host/world_tables_dump.cpp with g++ and the address / undefined-behaviour sanitizers, run on
worlds written from numpy, and every table checked against the rule the kernels read it by -- restated here from the comments
of csrc/auvp_types.h, not shared with the device code.

The ground truth of the three cell indexes is the plain scan of cost.py:181-184: the first cell in list order with
minx <= x <= min(maxx, maxy) (sic: x against maxy too) and miny <= y."""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from auv_sim_amd import synth  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

DTYPES = {0: np.float64, 1: np.int32, 2: np.float32, 3: np.uint64}
SCALARS = {"n_xbuckets", "xb_x0", "xb_inv_w", "rg_enabled", "n_rg_bp", "sg_enabled", "sg_ncol", "sg_nrow", "sg_x1_0", "sg_y1_0",
           "sg_inv_dx", "sg_inv_dy", "obst_area", "hg_n", "hg_x0", "hg_y0", "hg_inv_w", "hg_inv_h", "prob_absmax", "prob_one_sign",
           "bins_sorted", "bins_t1_0", "bins_inv_len", "has_safe_box"}
HABITAT_FIELDS = ("hab_t", "hg_mask", "hg_n", "hg_x0", "hg_y0", "hg_inv_w", "hg_inv_h")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """tables(world arrays, options) -> {name: array or scalar}, through the sanitized program"""
    d = tmp_path_factory.mktemp("world_tables")
    exe = str(d / "world_tables_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "auv_sim_amd", "csrc"), "-o", exe,
                    os.path.join(REPO, "tests", "host", "world_tables_dump.cpp")], check=True)
    count = [0]

    def tables(obstacles=None, habitats=None, polygon=None, bins=None, cells=None, prob=None, rg_max_entries=32 << 20,
               grid_index=True, habitat_grid=True):
        arr = [np.ascontiguousarray(a if a is not None else [], dtype=np.float64).reshape(-1, k)
               for a, k in ((obstacles, 3), (habitats, 3), (polygon, 2), (bins, 2), (cells, 4))]
        pr = np.ascontiguousarray(prob if prob is not None else [], dtype=np.float64).ravel()
        assert pr.size == len(arr[3]) * len(arr[4])
        count[0] += 1
        src, dst = str(d / ("in%d.bin" % count[0])), str(d / ("out%d.bin" % count[0]))
        with open(src, "wb") as f:
            f.write(np.array([len(a) for a in arr] + [int(grid_index), int(habitat_grid), 0], dtype=np.int32).tobytes())
            f.write(np.array([rg_max_entries], dtype=np.int64).tobytes())
            for a in arr + [pr]:
                f.write(a.tobytes())
        r = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]   # the sanitizers report on stderr
        raw = open(dst, "rb").read()
        out, pos = {}, 0
        while pos < len(raw):
            name = raw[pos:pos + 16].rstrip(b"\0").decode()
            kind, n = np.frombuffer(raw, np.int32, 2, pos + 16)
            v = np.frombuffer(raw, DTYPES[int(kind)], int(n), pos + 24)
            pos += 24 + int(n) * v.itemsize
            out[name] = v[0].item() if name.replace("alone_", "") in SCALARS else v
        for k in HABITAT_FIELDS:   # the habitats' part built alone (auvp_world_set_habitats) is the whole build's
            assert np.array_equal(out[k], out["alone_" + k], equal_nan=True), k
        return out

    return tables


# ---- the reading rules, restated ---------------------------------------------------------------------------------------------

def plain_scan(cells, x, y):
    """first cell in list order with minx <= x <= min(maxx, maxy) and miny <= y; -1: none"""
    if len(cells) == 0:
        return np.full(len(x), -1)
    hit = ((cells[:, 0] <= x[:, None]) & (x[:, None] <= np.minimum(cells[:, 2], cells[:, 3])) & (cells[:, 1] <= y[:, None]))
    return np.where(hit.any(axis=1), hit.argmax(axis=1), -1)


def bucket_of(t, x):
    fb = math.floor((x - t["xb_x0"]) * t["xb_inv_w"])
    return 0 if fb < 0 else (t["n_xbuckets"] - 1 if fb >= t["n_xbuckets"] else int(fb))


def bucket_scan(t, x, y):
    """xb_*: the bucket of x lists its candidates in list order; column 3 = the least miny from here on ends the scan"""
    b = bucket_of(t, x)
    data = t["xb_data"].reshape(-1, 4)
    for k in range(t["xb_off"][b], t["xb_off"][b + 1]):
        d = data[k]
        if y < d[3]:
            return -1
        if d[0] <= x <= d[1] and y >= d[2]:
            return int(t["xb_items"][k])
    return -1


def region_lookup(t, x, y):
    """rg_*: the breakpoints before bucket b are < x and those from bucket b + 1 on are > x; region 2i is the open interval
    below breakpoint i, 2i + 1 the breakpoint itself; first candidate whose running min of miny is <= y"""
    b = bucket_of(t, x)
    bp, pm = t["rg_bp"], t["rg_pm"]
    lo, hi = int(t["rg_first"][b]), int(t["rg_first"][b + 1])
    while lo < hi:
        mid = (lo + hi) >> 1
        if bp[mid] < x:
            lo = mid + 1
        else:
            hi = mid
    r = 2 * lo + (1 if lo < t["n_rg_bp"] and bp[lo] == x else 0)
    s, e = int(t["rg_off"][r]), int(t["rg_off"][r + 1])
    if s == e or not pm[e - 1] <= y:
        return -1
    return int(t["rg_id"][s + int(np.argmax(pm[s:e] <= y))])


def lower_bound_from(a, v, i):
    """first i with a[i] >= v, stepping from a guess"""
    n = len(a)
    i = min(max(i, 0), n - 1)
    while i > 0 and a[i - 1] >= v:
        i -= 1
    while i < n and a[i] < v:
        i += 1
    return i


def grid_lookup(t, x, y, stepping):
    """sg_*: column = lower bound of x in X1, row = lower bound of x (sic) in Y1; then X0[c] <= x and Y0[r] <= y.
    The guess is checked against one interleaved entry {a1[i-1], a1[i], a0[i], 0}; `stepping`: from the far end instead.
    -> (cell, whether the guess was right)"""
    nc, nr = t["sg_ncol"], t["sg_nrow"]
    gc = min(max(math.floor((x - t["sg_x1_0"]) * t["sg_inv_dx"]) + 1, 0), nc - 1)
    gr = min(max(math.floor((x - t["sg_y1_0"]) * t["sg_inv_dy"]) + 1, 0), nr - 1)
    cc, rr = t["sg_col"].reshape(-1, 4)[gc], t["sg_row"].reshape(-1, 4)[gr]
    guessed = bool(cc[0] < x <= cc[1] and rr[0] < x <= rr[1])
    if guessed and not stepping:
        return (gr * nc + gc if cc[2] <= x and rr[2] <= y else -1), True
    c = lower_bound_from(t["sg_x1"], x, nc - 1 - gc if stepping else gc)
    r = lower_bound_from(t["sg_y1"], x, nr - 1 - gr if stepping else gr)
    if c >= nc or r >= nr or not t["sg_x0"][c] <= x or not t["sg_y0"][r] <= y:
        return -1, guessed
    return r * nc + c, guessed


# ---- cells that are no grid ----------------------------------------------------------------------------------------------------

def scattered_cells(seed, n_points=4000):
    """the 300 cells of test_gpu_edge_cases.py::test_cell_lookup_index_is_exact_for_arbitrary_cell_lists and points on and off
    their edges"""
    rng = np.random.default_rng(seed)
    C = 300
    x0 = np.round(rng.uniform(-60, 60, C), 1)
    y0 = np.round(rng.uniform(-60, 60, C), 1)
    cells = np.stack([x0, y0, x0 + np.round(rng.uniform(0, 40, C), 1), y0 + np.round(rng.uniform(0, 40, C), 1)], axis=1)
    cells[::17, 2] = cells[::17, 0]            # zero-width cells
    cells[5::29, 3] = cells[5::29, 0] - 1.0    # maxy < minx: can never match (x <= maxy fails)
    edges = np.concatenate([cells[:, 0], cells[:, 2], cells[:, 3]])
    x = rng.uniform(-70, 110, n_points)
    on = rng.random(n_points) < 0.4
    x[on] = rng.choice(edges, on.sum())
    y = rng.uniform(-70, 110, n_points)
    yon = rng.random(n_points) < 0.2
    y[yon] = rng.choice(cells[:, 1], yon.sum())
    return cells, x, y


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_region_index_and_bucket_scan_of_scattered_cells(dump, seed):
    cells, x, y = scattered_cells(seed)
    t = dump(cells=cells)
    assert t["sg_enabled"] == 0 and t["sg_ncol"] == 0 and t["sg_nrow"] == 0 and len(t["sg_col"]) == 0 and len(t["sg_x1"]) == 0
    assert t["rg_enabled"] == 1 and t["n_rg_bp"] == len(t["rg_bp"]) > 0
    NB = t["n_xbuckets"]
    assert NB == {0: 686, 1: 1352, 2: 1274}[seed]
    want = plain_scan(cells, x, y)
    assert [region_lookup(t, a, b) for a, b in zip(x, y)] == want.tolist()
    assert [bucket_scan(t, a, b) for a, b in zip(x, y)] == want.tolist()
    print("seed %d: NB %d, %d of %d points in a cell" % (seed, NB, (want >= 0).sum(), len(x)))
    assert 3 * (want >= 0).sum() >= len(x)   # of every seed, so of the 12 000 together
    # structure
    xoff, roff, data = t["xb_off"], t["rg_off"], t["xb_data"].reshape(-1, 4)
    assert len(xoff) == NB + 1 and xoff[0] == 0 and np.all(np.diff(xoff) >= 0) and xoff[-1] == len(t["xb_items"]) == len(data)
    assert len(roff) == 2 * t["n_rg_bp"] + 2 and roff[0] == 0 and np.all(np.diff(roff) >= 0)
    assert roff[-1] == len(t["rg_id"]) == len(t["rg_pm"])
    assert len(t["rg_first"]) == NB + 1 and np.all(np.diff(t["rg_first"]) >= 0) and t["rg_first"][-1] == t["n_rg_bp"]
    assert np.all(np.diff(t["rg_bp"]) > 0)
    for r in range(len(roff) - 1):
        assert np.all(np.diff(t["rg_pm"][roff[r]:roff[r + 1]]) <= 0), r
    for b in range(NB):
        d = data[xoff[b]:xoff[b + 1]]
        assert np.array_equal(d[:, 3], np.minimum.accumulate(d[::-1, 2])[::-1]), b
    own = cells[t["xb_items"]]
    assert np.array_equal(data[:, :3], np.stack([own[:, 0], np.minimum(own[:, 2], own[:, 3]), own[:, 1]], axis=1))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_no_entry_budget_leaves_the_bucket_scan(dump, seed):
    cells, x, y = scattered_cells(seed)
    t = dump(cells=cells, rg_max_entries=0)
    assert t["rg_enabled"] == 0 and t["n_rg_bp"] == 0 and len(t["rg_bp"]) == 0
    assert len(t["rg_first"]) == t["n_xbuckets"] + 1 and not t["rg_first"].any()
    assert [bucket_scan(t, a, b) for a, b in zip(x, y)] == plain_scan(cells, x, y).tolist()


# ---- a grid --------------------------------------------------------------------------------------------------------------------

def test_separable_grid_of_the_synthetic_world(dump):
    w = synth.make_world(seed=1, n_obstacles=64)
    cells = w["cells"]
    nrow, ncol = w["grid_shape"]
    t = dump(w["obstacles"], w["habitats"], w["polygon"], w["bins"], cells, w["prob"])
    assert t["sg_enabled"] == 1 and (t["sg_nrow"], t["sg_ncol"]) == (nrow, ncol) and ncol * nrow == len(cells)
    for a0, a1, tab in ((cells[:ncol, 0], cells[:ncol, 2], "sg_col"), (cells[::ncol, 1], cells[::ncol, 3], "sg_row")):
        want = np.stack([np.concatenate([[-np.inf], a1[:-1]]), a1, a0, np.zeros(len(a0))], axis=1)
        assert np.array_equal(t[tab].reshape(-1, 4), want)
    assert np.array_equal(t["sg_x0"], cells[:ncol, 0]) and np.array_equal(t["sg_x1"], cells[:ncol, 2])
    assert np.array_equal(t["sg_y0"], cells[::ncol, 1]) and np.array_equal(t["sg_y1"], cells[::ncol, 3])
    # points inside, on cell edges (x on X0 / X1 / Y1 values, y on Y0 values) and outside the grid.  x is looked up among the
    # rows' Y1 too (sic), so x runs over both extents
    rng = np.random.default_rng(5)
    n = 3000
    x = np.where(rng.random(n) < 0.5, rng.uniform(-330.0, -70.0, n), rng.uniform(-130.0, 130.0, n))
    on = rng.random(n) < 0.4
    x[on] = rng.choice(np.concatenate([cells[:, 0], cells[:, 2], cells[:, 3]]), on.sum())
    y = rng.uniform(-130.0, 130.0, n)
    yon = rng.random(n) < 0.2
    y[yon] = rng.choice(cells[:, 1], yon.sum())
    want = plain_scan(cells, x, y).tolist()
    assert sum(c >= 0 for c in want) > n // 5 and sum(c < 0 for c in want) > n // 5
    got = [grid_lookup(t, a, b, False) for a, b in zip(x, y)]
    assert [g[0] for g in got] == want
    n_guessed = sum(g[1] for g in got)
    assert n // 4 < n_guessed < n   # both the checked guess and the search behind a wrong one were walked
    assert [grid_lookup(t, a, b, True)[0] for a, b in zip(x, y)] == want
    # the index switched off: the region index answers the same
    t = dump(w["obstacles"], w["habitats"], w["polygon"], w["bins"], cells, w["prob"], grid_index=False)
    assert t["sg_enabled"] == 0 and t["sg_ncol"] == 0 and t["sg_nrow"] == 0 and len(t["sg_col"]) == 0 and len(t["sg_row"]) == 0
    assert (t["sg_x1_0"], t["sg_y1_0"], t["sg_inv_dx"], t["sg_inv_dy"]) == (0.0, 0.0, 0.0, 0.0)
    assert t["rg_enabled"] == 1
    assert [region_lookup(t, a, b) for a, b in zip(x, y)] == want


# ---- the empty world -----------------------------------------------------------------------------------------------------------

def assert_slots_are_padding(t):
    assert np.array_equal(t["os_t"], np.full(256, -1.0)) and np.array_equal(t["os_r"], np.full(256, -np.inf, np.float32))
    box = t["os_box"].reshape(16, 4)
    assert np.all(box[:, 0] > box[:, 2]) and np.all(box[:, 1] > box[:, 3])


def test_empty_world(dump):
    t = dump()
    assert t["n_xbuckets"] == 0 and t["xb_off"].tolist() == [0, 0] and len(t["xb_items"]) == 0
    assert len(t["ox"]) == 0 and t["obst_area"] == 0.0
    assert_slots_are_padding(t)
    assert t["bins_sorted"] == 0 and t["has_safe_box"] == 0 and t["hg_n"] == 0 and len(t["hg_mask"]) == 0
    assert t["sg_enabled"] == 0 and t["rg_enabled"] == 0 and t["prob_one_sign"] == 1 and t["prob_absmax"] == 0.0


# ---- obstacles -----------------------------------------------------------------------------------------------------------------

def some_obstacles(O):
    rng = np.random.default_rng(11)
    ob = np.stack([rng.uniform(-200, 200, O), rng.uniform(-80, 120, O), rng.uniform(0.0, 6.0, O)], axis=1)
    ob[10:40:3, 2] = ob[10, 2]       # repeated radii
    ob[200:, 2] = 0.75
    ob[O - 1, 2] = -2.0              # `d <= size` can never hold: behind it no radius is left
    return ob


def test_obstacle_thresholds_and_slots(dump):
    ob = some_obstacles(256)
    t = dump(obstacles=ob)
    assert np.array_equal(t["ox"], ob[:, 0]) and np.array_equal(t["oy"], ob[:, 1])
    R = np.maximum.accumulate(ob[::-1, 2])[::-1]    # the largest radius from obstacle i on
    ot = t["ot"]
    assert R[-1] < 0 and ot[-1] == -1.0 and np.all(R[:-1] >= 0)
    assert np.all(np.sqrt(ot[:-1]) <= R[:-1]) and np.all(R[:-1] < np.sqrt(np.nextafter(ot[:-1], np.inf)))
    rows = lambda a: sorted(map(tuple, np.stack(a, axis=1).tolist()))  # noqa: E731
    assert rows([t["os_x"], t["os_y"], t["os_t"]]) == rows([ob[:, 0], ob[:, 1], ot])
    r = t["os_r"].astype(np.float64)
    live = t["os_t"] >= 0
    assert live.sum() == 255 and np.all(r[live] >= np.sqrt(t["os_t"][live])) and np.all(r[~live] == -np.inf)
    box = t["os_box"].reshape(16, 4)[np.arange(256) // 16]
    assert np.all(box[live, 0] <= t["os_x"][live] - r[live]) and np.all(box[live, 1] <= t["os_y"][live] - r[live])
    assert np.all(box[live, 2] >= t["os_x"][live] + r[live]) and np.all(box[live, 3] >= t["os_y"][live] + r[live])
    area = (ob[:, 0].max() - ob[:, 0].min()) * (ob[:, 1].max() - ob[:, 1].min())
    assert t["obst_area"] == area > 0


def test_more_obstacles_than_slots(dump):
    ob = some_obstacles(257)
    t = dump(obstacles=ob)
    assert len(t["ot"]) == 257
    assert_slots_are_padding(t)
    assert not t["os_x"].any() and not t["os_y"].any()
    assert t["obst_area"] == (ob[:, 0].max() - ob[:, 0].min()) * (ob[:, 1].max() - ob[:, 1].min()) > 0


# ---- habitats ------------------------------------------------------------------------------------------------------------------

def habitat_points(hab, n=2000):
    rng = np.random.default_rng(3)
    hx, hy, hr = hab[:, 0], hab[:, 1], np.abs(hab[:, 2])
    x = np.concatenate([rng.uniform(hx.min() - 40, hx.max() + 40, n), hx - hr, hx + hr, hx, hx])
    y = np.concatenate([rng.uniform(hy.min() - 40, hy.max() + 40, n), hy, hy, hy - hr, hy + hr])
    return x, y


def mask_of_points(t, x, y):
    """hg_*: the cell of a point, 0 outside the box -> (bit set of the cell, inside the box)"""
    n = t["hg_n"]
    fx, fy = np.floor((x - t["hg_x0"]) * t["hg_inv_w"]), np.floor((y - t["hg_y0"]) * t["hg_inv_h"])
    inside = (fx >= 0) & (fy >= 0) & (fx < n) & (fy < n)
    idx = np.where(inside, fy * n + fx, 0).astype(np.int64)
    return np.where(inside, t["hg_mask"][idx], np.uint64(0)), inside


def test_habitat_thresholds_and_mask_grid(dump):
    hab = synth.make_world(seed=1, n_obstacles=64)["habitats"].copy()
    assert len(hab) == 10
    hab[4, 2] = -3.0    # can never contain a point
    t = dump(habitats=hab)
    assert t["hg_n"] == 32 and len(t["hg_mask"]) == 32 * 32
    ht = t["hab_t"]
    assert ht[4] == -1.0
    pos = np.arange(10) != 4
    assert np.all(np.sqrt(ht[pos]) <= hab[pos, 2]) and np.all(hab[pos, 2] < np.sqrt(np.nextafter(ht[pos], np.inf)))
    x, y = habitat_points(hab)
    mask, inside = mask_of_points(t, x, y)
    n_in = 0
    for i in range(10):
        ddx, ddy = hab[i, 0] - x, hab[i, 1] - y
        contains = ddx * ddx + ddy * ddy <= ht[i]
        bit = (mask >> np.uint64(i)) & np.uint64(1) == 1
        assert np.all(bit[contains]), i        # (a point outside the box has no bit: then no habitat may contain it)
        n_in += int(contains.sum())
    assert n_in > 100 and (~inside).sum() > 100
    assert not ((t["hg_mask"] >> np.uint64(4)) & np.uint64(1)).any()
    assert not (t["hg_mask"] >> np.uint64(10)).any()


def test_habitat_grid_is_left_out(dump):
    hab = synth.make_world(seed=1, n_obstacles=64)["habitats"]
    many = np.tile(hab, (7, 1))[:65]
    nan = hab.copy()
    nan[3, 0] = np.nan
    for t in (dump(habitats=many), dump(habitats=nan), dump(habitats=hab, habitat_grid=False)):
        assert t["hg_n"] == 0 and len(t["hg_mask"]) == 0
        assert (t["hg_x0"], t["hg_y0"], t["hg_inv_w"], t["hg_inv_h"]) == (0.0, 0.0, 0.0, 0.0)
    assert len(dump(habitats=many)["hab_t"]) == 65


# ---- polygon -------------------------------------------------------------------------------------------------------------------

def test_polygon_bounds_and_safe_box(dump):
    rect = np.array([[-30.0, 5.0], [40.0, 5.0], [40.0, 25.0], [-30.0, 25.0]])
    for winding in (rect, rect[::-1]):
        for k in range(4):
            t = dump(polygon=np.roll(winding, k, axis=0))
            assert t["has_safe_box"] == 1 and t["bb"].tolist() == [-30.0, 5.0, 40.0, 25.0] == t["safe_box"].tolist()
    c, s = math.cos(0.3), math.sin(0.3)
    rotated = rect @ np.array([[c, s], [-s, c]])
    diagonal = np.array([[0.0, 0.0], [10.0, 0.0], [10.0, 10.0], [1.0, 10.0]])
    hexagon = np.array([[0.0, 0.0], [10.0, 0.0], [10.0, 5.0], [10.0, 10.0], [0.0, 10.0], [0.0, 5.0]])
    for poly in (rotated, diagonal, hexagon):
        t = dump(polygon=poly)
        assert t["has_safe_box"] == 0
        assert t["bb"].tolist() == [poly[:, 0].min(), poly[:, 1].min(), poly[:, 0].max(), poly[:, 1].max()]


# ---- time bins -----------------------------------------------------------------------------------------------------------------

def test_bin_guess_constants(dump):
    bins = synth.make_world(seed=1, n_obstacles=64)["bins"]
    T = len(bins)
    t = dump(bins=bins)
    assert t["bins_sorted"] == 1 and t["bins_t1_0"] == bins[0, 1] and t["bins_inv_len"] == (T - 1) / (bins[T - 1, 1] - bins[0, 1])
    unordered = np.array([[100.0, 150.0], [0.0, 50.0], [30.0, 120.0], [250.0, 300.0], [50.0, 100.0], [150.0, 250.0]])
    t = dump(bins=unordered)   # (tests/test_gpu_edge_cases.py::test_exploring_with_unordered_overlapping_bins)
    assert t["bins_sorted"] == 0 and t["bins_inv_len"] == 0.0
    t = dump(bins=bins[:1])
    assert t["bins_sorted"] == 1 and t["bins_inv_len"] == 0.0
    bad = bins.copy()
    bad[T - 1, 1] = np.nan
    assert dump(bins=bad)["bins_sorted"] == 0


# ---- probabilities -------------------------------------------------------------------------------------------------------------

def test_probability_statistics(dump):
    w = synth.make_world(seed=1, n_obstacles=64)
    bins, cells, prob = w["bins"][:3], w["cells"][:50], w["prob"][:3, :50].copy()
    t = dump(bins=bins, cells=cells, prob=prob)
    assert t["prob_one_sign"] == 1 and t["prob_absmax"] == prob.max()
    prob[1, 7] = -0.9
    t = dump(bins=bins, cells=cells, prob=prob)
    assert t["prob_one_sign"] == 0 and t["prob_absmax"] == 0.9
    prob[1, 7] = np.nan
    t = dump(bins=bins, cells=cells, prob=prob)
    assert t["prob_one_sign"] == 0 and math.isnan(t["prob_absmax"])

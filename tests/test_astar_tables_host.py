"""The top-n table of astar_fixLenSOG's heuristic, built without a GPU: csrc/astar_tables.h (the pure host function behind the
world's own table and behind the host route of the probability sets' tables) compiled into tests/host/astar_tables_dump.cpp with
g++, once plain and once with the address / undefined-behaviour sanitizers, and its rows compared byte for byte with what
get_top_n_prob computes (astar_fixLenSOG.py:516-531): sorted(row, reverse=True) and a running `total += v` from 0."""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def python_topn(prob):
    """[T, C] -> [T, C + 1], the reference's own operations on Python floats"""
    out = np.zeros((prob.shape[0], prob.shape[1] + 1))
    for t, row in enumerate(prob):
        total = 0
        for i, v in enumerate(sorted(row.tolist(), reverse=True)):
            total += v
            out[t, i + 1] = total
    return out


def awkward_rows(C, seed):
    """[4, C]: ties, zeros of both signs, negative values, one +inf; the rows differ from each other"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.5, 1.0, (4, C))
    if C >= 2:
        p[0, :] = np.round(p[0, :], 1)                # ties
        p[1, ::3] = 0.0
        p[1, 1::3] = -0.0
        p[2, rng.integers(0, C)] = np.inf
        p[3, :] = -np.abs(p[3, :])
        p[3, C // 2] = 0.25
    return p


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("astar_tables")
    out = []
    for name, extra in (("plain", ["-O2"]), ("san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / ("astar_tables_dump_" + name))
        subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + extra + ["-I", os.path.join(REPO, "auv_sim_amd", "csrc"), "-o", exe,
                        os.path.join(REPO, "tests", "host", "astar_tables_dump.cpp")], check=True)
        out.append(exe)
    count = [0]

    def run(exe, prob):
        count[0] += 1
        src, dst = str(d / ("in%d.bin" % count[0])), str(d / ("out%d.bin" % count[0]))
        with open(src, "wb") as f:
            f.write(np.array(prob.shape, dtype=np.int64).tobytes())
            f.write(np.ascontiguousarray(prob, dtype=np.float64).tobytes())
        r = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])   # the sanitizers report on stderr
        return np.fromfile(dst, dtype=np.float64).reshape(prob.shape[0], prob.shape[1] + 1)

    return out, run


@pytest.mark.parametrize("C", [0, 1, 2, 987])
def test_topn_rows_equal_the_reference_loop_byte_for_byte(programs, C):
    (plain, san), run = programs
    prob = awkward_rows(C, seed=C + 1)
    want = python_topn(prob)
    assert np.all(want[:, 0] == 0.0) and not np.signbit(want[:, 0]).any()
    if C == 987:
        assert np.isinf(want[2, 1:]).all() and len(np.unique(prob[0])) < C // 2 and (want[3, 2:] < want[3, 1:-1]).all()
    for exe in (plain, san):
        got = run(exe, prob)
        assert got.tobytes() == want.tobytes(), (C, exe)


def test_no_rows(programs):
    (plain, san), run = programs
    for exe in (plain, san):
        assert run(exe, np.zeros((0, 5))).size == 0


# ---- build_astar_world_tables: everything astar_build_world uploads, against its rules restated in numpy -------------------------

@pytest.fixture(scope="module")
def world_tables(programs, tmp_path_factory):
    """tables(obstacles, habitats, polygon, cells, prob [T, C], no_grid) -> dict, the same from the plain and the sanitized program"""
    (plain, san), _ = programs
    d = tmp_path_factory.mktemp("astar_world")
    count = [0]

    def one(exe, arrays, T, no_grid):
        count[0] += 1
        src, dst = str(d / ("in%d.bin" % count[0])), str(d / ("out%d.bin" % count[0]))
        with open(src, "wb") as f:
            f.write(np.array([len(arrays[0]), len(arrays[1]), len(arrays[2]), T, len(arrays[3]), int(no_grid)], dtype=np.int32).tobytes())
            for a in arrays:
                f.write(a.tobytes())
        r = subprocess.run([exe, "world", src, dst], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
        return open(dst, "rb").read()

    def tables(obstacles=None, habitats=None, polygon=None, cells=None, prob=None, no_grid=False):
        arr = [np.ascontiguousarray(a if a is not None else [], dtype=np.float64).reshape(-1, k)
               for a, k in ((obstacles, 3), (habitats, 3), (polygon, 2), (cells, 4))]
        pr = np.ascontiguousarray(prob if prob is not None else np.zeros((0, len(arr[3]))), dtype=np.float64)
        assert pr.ndim == 2 and pr.shape[1] == len(arr[3])
        raw = one(plain, arr + [pr], pr.shape[0], no_grid)
        assert raw == one(san, arr + [pr], pr.shape[0], no_grid)
        out = dict(zip(("g_ncol", "g_nrow"), np.frombuffer(raw, np.int32, 2, 0).tolist()))
        out.update(zip(("g_x1_0", "g_y1_0", "g_inv_dx", "g_inv_dy", "cx", "cy"), np.frombuffer(raw, np.float64, 6, 8).tolist()))
        sizes, pos = np.frombuffer(raw, np.int64, 7, 56), 112
        for name, n in zip(("ox", "oy", "ot", "hab", "rc", "topn", "gtab"), sizes.tolist()):
            out[name] = np.frombuffer(raw, np.float64, n, pos)
            pos += 8 * n
        assert pos == len(raw)
        return out

    return tables


def is_sq_threshold(t, size):
    """t = the largest double whose square root does not exceed size (`d <= size` as a test on d squared); -1 where none does"""
    if not size >= 0:
        return t == -1.0
    return np.sqrt(t) <= size < np.sqrt(np.nextafter(t, np.inf))


def numpy_centroid(poly):
    """the shoelace sums in list order, then sx / (3 a2): IEEE division (0 / 0 for a polygon of no area)"""
    a2 = sx = sy = np.float64(0.0)
    V = len(poly)
    for i in range(V):
        (x0, y0), (x1, y1) = poly[i], poly[(i + 1) % V]
        cr = x0 * y1 - x1 * y0
        a2, sx, sy = a2 + cr, sx + (x0 + x1) * cr, sy + (y0 + y1) * cr
    with np.errstate(all="ignore"):
        return (float(sx / (3.0 * a2)), float(sy / (3.0 * a2))) if V else (0.0, 0.0)


def numpy_grid(rc, no_grid=False):
    """the product-grid rule -> (ncol, nrow, X0, X1, Y0, Y1) or None: the first run of cells with the first cell's y interval is a
    row; every cell's x interval is its column's and its y interval its row's; edges finite, each interval at least 1e-6 of the
    largest magnitude (at least 1) wide, the next one starting no lower than this one ends"""
    C = len(rc)
    if C == 0 or no_grid:
        return None
    same = (rc[:, 1] == rc[0, 1]) & (rc[:, 3] == rc[0, 3])
    nc = C if same.all() else int(np.argmin(same))
    if C % nc:
        return None
    g = rc.reshape(C // nc, nc, 4)
    X0, X1, Y0, Y1 = g[0, :, 0], g[0, :, 2], g[:, 0, 1], g[:, 0, 3]
    if not ((g[:, :, 0] == X0).all() and (g[:, :, 2] == X1).all() and (g[:, :, 1] == Y0[:, None]).all() and (g[:, :, 3] == Y1[:, None]).all()):
        return None
    for lo, hi in ((X0, X1), (Y0, Y1)):
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            return None
        scale = max(1.0, np.abs(lo).max(), np.abs(hi).max())
        if not ((hi - lo >= 1e-6 * scale).all() and (lo[1:] >= hi[:-1]).all()):
            return None
    return nc, C // nc, X0, X1, Y0, Y1


def check_world_tables(t, obstacles, habitats, polygon, cells, prob, no_grid=False):
    ob, hb, cl = (np.asarray(a, dtype=np.float64).reshape(-1, k) for a, k in ((obstacles, 3), (habitats, 3), (cells, 4)))
    assert np.array_equal(t["ox"], ob[:, 0]) and np.array_equal(t["oy"], ob[:, 1]) and len(t["ot"]) == len(ob)
    assert all(is_sq_threshold(a, b) for a, b in zip(t["ot"], ob[:, 2]))
    hab = t["hab"].reshape(-1, 4)
    assert np.array_equal(hab[:, :3], hb) and all(is_sq_threshold(a, b) for a, b in zip(hab[:, 3], hb[:, 2]))
    rc = np.array([round(v, 2) for v in cl.ravel().tolist()]).reshape(-1, 4)
    assert np.array_equal(t["rc"].reshape(-1, 4), rc, equal_nan=True)
    assert t["topn"].tobytes() == python_topn(np.asarray(prob, dtype=np.float64)).tobytes()   # (prob is [T, C])
    assert np.array_equal([t["cx"], t["cy"]], numpy_centroid(np.asarray(polygon, dtype=np.float64).reshape(-1, 2).tolist()), equal_nan=True)
    g = numpy_grid(rc, no_grid)
    if g is None:
        assert (t["g_ncol"], t["g_nrow"], len(t["gtab"])) == (0, 0, 0)
        assert (t["g_x1_0"], t["g_y1_0"], t["g_inv_dx"], t["g_inv_dy"]) == (0.0, 0.0, 0.0, 0.0)
    else:
        nc, nr, X0, X1, Y0, Y1 = g
        assert (t["g_ncol"], t["g_nrow"]) == (nc, nr) and np.array_equal(t["gtab"], np.concatenate([X0, X1, Y0, Y1]))
        assert (t["g_x1_0"], t["g_y1_0"]) == (X1[0], Y1[0])
        assert t["g_inv_dx"] == ((nc - 1) / (X1[-1] - X1[0]) if nc > 1 else 0.0)
        assert t["g_inv_dy"] == ((nr - 1) / (Y1[-1] - Y1[0]) if nr > 1 else 0.0)
    return g is not None


def grid_cells(xs, ys):
    """row-major cells of the product of the x intervals [(x0, x1)] and the y intervals"""
    return np.array([[x0, y0, x1, y1] for (y0, y1) in ys for (x0, x1) in xs])


WORLD = dict(obstacles=[[1.0, 2.0, 3.0], [-4.5, 0.25, 0.1], [7.0, 7.0, 0.0], [0.0, 0.0, -1.0], [2.0, 2.0, 1e-300]],
             habitats=[[10.0, -3.0, 4.0], [0.5, 0.5, 2.675]],
             polygon=[[-30.0, 5.0], [40.0, 5.0], [55.0, 25.0], [-30.0, 31.0]])


def world_check(world_tables, cells, seed=0, **kw):
    args = dict(WORLD, cells=cells, prob=np.random.default_rng(seed).uniform(0.0, 1.0, (3, len(cells))))
    args.update(kw)
    no_grid = args.pop("no_grid", False)
    t = world_tables(no_grid=no_grid, **args)
    return t, check_world_tables(t, args["obstacles"], args["habitats"], args["polygon"], args["cells"], args["prob"], no_grid)


def test_world_tables_of_a_product_grid(world_tables):
    # (edges that round(v, 2) moves: the grid is detected on the rounded cells)
    xs = [(-10.004, -5.0), (-5.0, 0.125), (0.125, 6.0), (7.0, 9.999)]
    ys = [(0.0, 2.5), (2.5, 5.0), (6.0, 8.0)]
    t, is_grid = world_check(world_tables, grid_cells(xs, ys))
    assert is_grid and (t["g_ncol"], t["g_nrow"]) == (4, 3)
    assert t["gtab"].tolist() == [-10.0, -5.0, 0.12, 7.0, -5.0, 0.12, 6.0, 10.0, 0.0, 2.5, 6.0, 2.5, 5.0, 8.0]
    assert (t["g_x1_0"], t["g_y1_0"], t["g_inv_dx"], t["g_inv_dy"]) == (-5.0, 2.5, 3 / 15.0, 2 / 5.5)
    # one row, one column, one cell
    for cells, shape in ((grid_cells(xs, ys[:1]), (4, 1)), (grid_cells(xs[:1], ys), (1, 3)), (grid_cells(xs[:1], ys[:1]), (1, 1))):
        t, is_grid = world_check(world_tables, cells)
        assert is_grid and (t["g_ncol"], t["g_nrow"]) == shape
    assert (t["g_inv_dx"], t["g_inv_dy"]) == (0.0, 0.0)
    t, is_grid = world_check(world_tables, grid_cells(xs, ys), no_grid=True)
    assert not is_grid and len(t["rc"]) == 48


def test_world_tables_of_cells_that_are_no_product_grid(world_tables):
    xs, ys = [(0.0, 1.0), (1.0, 2.0), (2.0, 3.0)], [(0.0, 1.0), (1.0, 2.0), (2.0, 3.0)]
    good = grid_cells(xs, ys)
    assert world_check(world_tables, good)[1]
    shifted = good.copy()
    shifted[4, [0, 2]] += 0.01                       # one cell of the middle row shifted
    touching = grid_cells([(0.0, 1.0), (1.0, 1.5), (1.5, 3.0)], ys)
    overlapping = grid_cells([(0.0, 1.0), (0.99, 2.0), (2.0, 3.0)], ys)
    descending = grid_cells(xs, ys[::-1])
    thin = grid_cells([(0.0, 1.0), (1.0, 1.0), (2.0, 3.0)], ys)         # a degenerate width
    thin_for_its_size = grid_cells([(0.0, 1.0), (1.0, 1.01), (2.0, 20000.0)], ys)   # 0.01 < 1e-6 x 20 000
    infinite = grid_cells([(0.0, 1.0), (1.0, 2.0), (2.0, np.inf)], ys)
    nan_edge = grid_cells(xs, [(0.0, 1.0), (1.0, 2.0), (2.0, np.nan)])
    ragged = np.concatenate([good[:3], good[3:5], good[6:8]])           # 7 cells, rows of 3: C % nc != 0
    for name, cells, want in (("shifted", shifted, False), ("touching", touching, True), ("overlapping", overlapping, False),
                              ("descending", descending, False), ("thin", thin, False), ("thin_for_its_size", thin_for_its_size, False),
                              ("infinite", infinite, False), ("nan_edge", nan_edge, False), ("ragged", ragged, False)):
        assert world_check(world_tables, cells)[1] == want, name


def test_world_tables_without_cells_polygon_or_area(world_tables):
    t, is_grid = world_check(world_tables, np.zeros((0, 4)), obstacles=[], habitats=[], polygon=[])
    assert not is_grid and (t["cx"], t["cy"]) == (0.0, 0.0) and len(t["topn"]) == 3 and not t["topn"].any()   # V = 0; C = 0: topn [T][1]
    t, _ = world_check(world_tables, grid_cells([(0.0, 1.0)], [(0.0, 1.0)]), polygon=[[0.0, 0.0], [4.0, 0.0], [4.0, 2.0], [0.0, 2.0]])
    assert (t["cx"], t["cy"]) == (2.0, 1.0)
    # no area: three points on a line, a point three times -- 0 / 0
    for poly in ([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]], [[3.0, 4.0]] * 3):
        t, _ = world_check(world_tables, np.zeros((0, 4)), polygon=poly)
        assert np.isnan(t["cx"]) and np.isnan(t["cy"])


def test_round2_is_pythons_round(programs, tmp_path):
    (plain, san), _ = programs
    rng = np.random.default_rng(42)
    v = np.concatenate([rng.uniform(-1000.0, 1000.0, 5000), rng.integers(-100000, 100000, 3000) / 1000.0, rng.normal(0.0, 1e-3, 1000),
                        10.0 ** rng.uniform(-12, 15, 1000) * rng.choice([-1.0, 1.0], 1000),
                        # halves of the second decimal (what they round to depends on the binary value: 2.675 is below the half)
                        [2.675, 0.125, 0.375, 1.005, -2.675, -0.125, 0.005, 0.015, 0.025, 1e15 + 0.5, 0.0, -0.0, 1e300, -1e308, 5e-324, np.inf,
                         -np.inf, np.nan]])
    assert len(v) >= 10000
    src = str(tmp_path / "in.bin")
    v.tofile(src)
    want = np.array([round(x, 2) for x in v.tolist()])
    assert want[10000:10004].tolist() == [2.67, 0.12, 0.38, 1.0]
    for exe in (plain, san):
        dst = str(tmp_path / "out.bin")
        r = subprocess.run([exe, "round2", src, dst], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
        got = np.fromfile(dst, dtype=np.float64)
        number = ~np.isnan(want)
        assert np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got[number]), np.signbit(want[number]))

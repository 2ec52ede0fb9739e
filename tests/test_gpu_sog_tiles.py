"""SharkOccupancyGrid.convert on the device (csrc/sog_kernels.h through auvp_sog_convert) against the CPU checker, bit for bit,
where tests/test_gpu_sog.py does not reach: more than one column and row tile in a launch (the halo that reaches into the
neighbour tile, a last tile narrower than 64 columns, cols % 4 != 0), plain / empty / masked tiles side by side, every radius
of the templated kernel, the last radius that runs from LDS and the first that does not, grids narrower than a thread's four
cells, the bucket index of sog_count_kernel on lists of mixed cell sizes, and the per-wavefront aggregation of its npts atomics
with dozens of keys and departed lanes in a wavefront.  The inputs and what they guarantee: tests/sog_tile_inputs.py,
asserted without a GPU in tests/test_sog_tile_inputs.py.  The checker (oracle/orc_sog.c) scans the cells linearly in list order
and sums the reference's 4 count x 4 count window literally."""
import numpy as np
import pytest

import sog_tile_inputs as si

pytestmark = pytest.mark.gpu
MODES = (None, "0", "2")  # AUVP_SOG_TILE: unset = LDS tiles, radius a template parameter up to 8; 0 = per-cell sweep; 2 = LDS tiles, radius at run time


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    return _lib.Context(0)


def _run(ctx, monkeypatch, name, count, tile):
    from auv_sim_amd.sharkOccupancyGrid import convert_arrays
    if tile is None:
        monkeypatch.delenv("AUVP_SOG_TILE", raising=False)
    else:
        monkeypatch.setenv("AUVP_SOG_TILE", tile)
    c = si.case(name)
    return convert_arrays(ctx, c["cells"], c["box"], c["cell_size"], c["bin_interval"], si.detect_range(count, c["cell_size"]),
                          c["traj_len"], c["pts"])


def _check(ctx, monkeypatch, name, count, tile):
    ref = si.reference(name, count)
    assert ref["status"] == 0
    bins, grids = _run(ctx, monkeypatch, name, count, tile)
    assert np.array_equal(bins, ref["bins"])
    assert grids.shape == ref["grids"].shape
    bad = np.argwhere(grids != ref["grids"])
    assert len(bad) == 0, "%d of %d entries differ, the first at (bin, row, col) %s" % (len(bad), grids.size, bad[0].tolist())
    assert np.array_equal(grids, ref["grids"])  # (NaN included: there is none)
    return grids


def test_lds_boundary_restated():
    """sog_tile_q / sog_tile_bytes restated (tests/sog_tile_inputs.py): under the launch rule's 150 KiB the last radius of the
    LDS tiles is 25 (148.5 KiB of dynamic LDS) and 26 is the first of the per-cell sweep.  A change of the tile shape or of the
    rule has to revisit the radii of test_seams_every_radius."""
    assert si.lds_boundary() == (25, 26) and si.tile_bytes(25) == 152064 and si.tile_bytes(26) == 156672
    assert si.SEAM_COUNTS[-2:] == (25, 26)


@pytest.mark.parametrize("tile", MODES, ids=["default", "percell", "runtime"])
@pytest.mark.parametrize("count", si.SEAM_COUNTS)
def test_seams_every_radius(ctx, orc, monkeypatch, count, tile):
    """35 x 131 grid of 1 m cells with a non-zero origin: column tiles of 64, 64 and 3 columns (cols % 4 == 3), row tiles of 16,
    16 and 3 rows; one tile listed exactly once (the plain path) beside masked ones, one tile unlisted, 30 cells listed twice and
    10 three times, some of them beside the seams.  Radii 1..8 (sog_grid_tile_c_kernel<C>, 6 and 7 included), 9 (the first of
    sog_grid_tile_kernel), 25 (the last that fits the LDS rule) and 26 (sog_grid_kernel by itself), each through all three
    kernel choices: every one equals the checker, hence they equal each other."""
    grids = _check(ctx, monkeypatch, "seams", count, tile)
    assert grids.max() > 0
    assert (grids[:, si.ROWS - 1, :] == 0).all() and (grids[:, :, si.COLS - 1] == 0).all()  # the +1 row / column: no listed cell


@pytest.mark.parametrize("tile", ["1", "2"])
@pytest.mark.parametrize("count", [1, 4, 9])
@pytest.mark.parametrize("name", si.NARROW)
def test_narrow_grids_through_the_tiles(ctx, orc, monkeypatch, name, count, tile):
    """cols3: 11 x 3, narrower than the four cells of a thread; rows1: 1 x 71 on a zero-height box (ceil(0) / cs + 1 = 1 row), two
    column tiles; interior_64x16: 17 x 65, whose +1 row and column open a second tile each that holds only unlisted cells"""
    grids = _check(ctx, monkeypatch, name, count, tile)
    assert grids.max() > 0
    assert (grids[:, :, -1] == 0).all()
    if grids.shape[1] > 1:
        assert (grids[:, -1, :] == 0).all()


@pytest.mark.parametrize("name", ["big_last", "big_first"])
def test_bucket_index_big_cell_beside_small_ones(ctx, orc, monkeypatch, name):
    """One cell that spans the whole box beside the unit cells.  Branch: the bucket size comes from the SMALLEST cell (NBX x NBY =
    130 x 34 = 4 420 <= max(4 096, 8 C), items <= 16 C + 4 096: the index keeps its first size, no halving) and the big cell is
    entered into every bucket.  Listed last, a bucket's item list ends with it: the small cells win their points and it takes
    the rest; listed first, it heads every bucket and takes every point of the box (first match in list order)."""
    _check(ctx, monkeypatch, name, 2, None)
    c, ref = si.case(name), si.reference(name, 2)
    keys, _ = si.point_keys(c)
    in_box = ((c["pts"][:, 0] >= si.BOX[0]) & (c["pts"][:, 0] <= si.BOX[2]) & (c["pts"][:, 1] >= si.BOX[1]) & (c["pts"][:, 1] <= si.BOX[3]))
    n00 = int((in_box & (keys == 0)).sum())  # bin 0 / shark 0's points inside the box
    nor = int((keys == 0).sum()) + 0.01 * len(c["cells"])
    if name == "big_first":
        v = 0.01
        for _ in range(n00):
            v = v + 1
        assert ref["occ"][0, 0] == v / nor  # the big cell maps to grid cell (0, 0): every point of the box
    else:
        assert 0 < ref["occ"][0, 0] * nor < n00 / 2


def test_bucket_index_halving_loop(ctx, orc, monkeypatch):
    """Slivers 1e-3 wide, slivers 1e-3 high and one zero-width cell among 200 unit cells.  Branch: the smallest positive width and
    height put NBX and NBY at the 1 024 clamp; 1 048 576 buckets > max(4 096, 8 C), so the halving loop runs (to 64 x 64) and
    the device looks points up in a coarser index than the cells' own size.  Points exactly on the slivers' edges and inside
    them, on the zero-width cell's line, on the smallest / largest x and y over all cells, and one ulp outside each of those
    (clamped buckets, contained by nothing)."""
    _check(ctx, monkeypatch, "slivers", 2, None)


def test_bucket_index_overlapping_cells(ctx, orc, monkeypatch):
    """Unit cells at whole and half offsets: a point lies in up to four of them and the first in list order takes it; up to four
    listed cells map to one grid cell.  Branch: NBX x NBY = 14 x 13 from the 1 m cells, within both budgets: no halving; a bucket
    lists the cells of all four offsets that touch it, in list order."""
    _check(ctx, monkeypatch, "overlap", 2, None)


def test_bucket_index_wrapped_cells(ctx, orc, monkeypatch):
    """Cells one and two cell widths left of / below the box: cellToIndex gives -1 / -2, which index from the far end as Python's
    negative index does (the +1 row and column are listed here).  Branch: the cells outside the box widen the index to
    132 x 36 buckets <= 8 C: first size, no halving; points in the margin fall into the wrapped cells."""
    grids = _check(ctx, monkeypatch, "wrapped", 2, None)
    assert (grids[:, si.ROWS - 1, :] != 0).any() and (grids[:, :, si.COLS - 1] != 0).any()


def test_bucket_index_empty_list(ctx, orc, monkeypatch):
    """C = 0.  Branch: no index is built (one empty bucket) and sog_count_kernel leaves after the npts count.  The checker's
    result: every bin's grid is zero (no listed cell takes a window); the 0 / 0 occupancies of a (bin, shark) without points
    never enter a sum."""
    grids = _check(ctx, monkeypatch, "empty_list", 2, None)
    assert grids.shape == (2, si.ROWS, si.COLS) and (grids == 0).all()


def test_bucket_index_nan_points(ctx, orc, monkeypatch):
    """Points with NaN x or y: every comparison of the reference is false, so no cell takes them, but they count in their bin's
    normaliser; a NaN time stamp is in no bin.  Branch: floor((NaN - x0) * inv) is NaN, which the bucket clamp sends to bucket 0
    before any conversion to int; the containment test then rejects every item."""
    grids = _check(ctx, monkeypatch, "nan_points", 2, None)
    assert not np.array_equal(grids, si.reference("seams", 2)["grids"])  # (the lost counts and the kept normaliser show)


@pytest.mark.parametrize("name", si.ATOMICS)
def test_npts_aggregation(ctx, orc, monkeypatch, name):
    """sog_count_kernel adds len(traj) per (bin, shark) with one atomic per key and wavefront.  many_short: 70 sharks of 1..3
    points, dozens of keys in a wavefront, a last wavefront that is not full; empty_traj: one shark of five without points;
    no_bin: late and negative time stamps between valid ones, so lanes have left before the ballot; unsorted: a trajectory
    that is not sorted by time, whose last point still sets the number of bins.  The normaliser npts + 0.01 C enters every
    occupancy: a lost or doubled count changes every entry of that shark's bin."""
    grids = _check(ctx, monkeypatch, name, 1, None)
    assert grids.max() > 0

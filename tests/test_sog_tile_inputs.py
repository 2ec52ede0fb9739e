"""The inputs of tests/test_gpu_sog_tiles.py (tests/sog_tile_inputs.py) have the properties those tests rely on -- asserted with
numpy and the CPU checker alone, so that they are checked where there is no GPU."""
import numpy as np
import pytest

import sog_tile_inputs as si


def _tiles(a):
    """the 16 x 64 blocks of the grid's interior that are whole tiles"""
    return [a[r:r + si.TILE_ROWS, c:c + si.TILE_COLS] for r in range(0, a.shape[0] - si.TILE_ROWS + 1, si.TILE_ROWS)
            for c in range(0, a.shape[1] - si.TILE_COLS + 1, si.TILE_COLS)]


def test_lds_boundary_is_25_26():
    """the last radius whose two tile buffers fit the launch rule's 150 KiB, and the first that does not"""
    assert si.tile_q(25) == 36 and si.tile_bytes(25) == 152064 and si.tile_bytes(26) == 156672
    assert si.lds_boundary() == (25, 26)
    assert si.SEAM_COUNTS == (1, 2, 3, 4, 5, 6, 7, 8, 9, 25, 26)


def test_seam_grid_shape_and_multiplicity():
    c = si.case("seams")
    assert si.grid_shape(c["box"], c["cell_size"]) == (35, 131) == (si.ROWS, si.COLS)
    assert si.COLS % 4 == 3 and c["box"][0] != 0.0 and c["box"][1] != 0.0
    m = si.multiplicity(c)
    assert m.shape == (35, 131) and set(np.unique(m).tolist()) == {0, 1, 2, 3}
    assert (m == 2).sum() == 30 and (m == 3).sum() == 10
    assert (m[34, :] == 0).all() and (m[:, 130] == 0).all()  # the +1 row and column hold no listed cell
    tiles = _tiles(m)
    assert len(tiles) == 4
    assert any((t == 1).all() for t in tiles) and any((t == 0).all() for t in tiles)
    assert any(len(np.unique(t)) > 1 for t in tiles)
    assert (m[0:16, 64:128] == 1).all() and (m[16:32, 0:64] == 0).all()
    rr, cc = np.nonzero(m >= 2)
    assert any(abs(col - seam) <= 8 for col in cc for seam in (64, 128))
    assert any(abs(row - seam) <= 8 for row in rr for seam in (16, 32))
    # also ON both sides of a seam's first halo cell: a multiply listed cell whose window crosses the seam at radius 1
    assert ((np.abs(cc - 64) <= 4) | (np.abs(cc - 128) <= 4)).any()


def test_seam_trajectories():
    c = si.case("seams")
    assert c["traj_len"].tolist() == [300, 1, 170]
    keys, T = si.point_keys(c)
    assert T >= 2 and (keys < 0).any()
    t = c["pts"][:, 2]
    assert ((t == 10.0) | (t == 20.0)).sum() >= 5  # exactly on a bin edge
    x, y = c["pts"][:, 0] - c["box"][0], c["pts"][:, 1] - c["box"][1]
    assert (x == np.round(x)).sum() >= 40 and (y == np.round(y)).sum() >= 40  # on cell edges
    assert (x < 0).any() and (x > 130).any() and (y < 0).any() and (y > 34).any()  # the margin: in no cell


def test_seam_occupancy_not_constant_across_the_seams(orc):
    occ = si.reference("seams", 1)["occ"]
    assert (occ[:, 63] != occ[:, 64]).any() and (occ[15, :] != occ[16, :]).any()
    # nor within the seam's neighbourhood on either side, so that a shifted or a missing halo column changes a sum
    assert len(np.unique(occ[0:16, 56:64])) > 1 and len(np.unique(occ[0:16, 64:72])) > 1
    assert len(np.unique(occ[8:16, :])) > 1 and len(np.unique(occ[32:34, :])) > 1


@pytest.mark.parametrize("name,shape", [("cols3", (11, 3)), ("rows1", (1, 71)), ("interior_64x16", (17, 65))])
def test_narrow_grids(name, shape):
    c = si.case(name)
    assert si.grid_shape(c["box"], c["cell_size"]) == shape
    m = si.multiplicity(c)
    assert m.max() >= 2 and (m == 0).any() and (m == 1).any()
    if shape[0] > 1:
        assert (m[-1, :] == 0).all()
    assert (m[:, -1] == 0).all()
    assert si.point_keys(c)[1] >= 2


@pytest.mark.parametrize("name", [n for n in si.BUCKETS if n != "empty_list"])
def test_bucket_index_branch(name):
    """the sliver list is over the bucket index's budgets at its first size, so the halving loop runs, from the 1024 clamp in
    both directions; every other list fits at its first size"""
    c = si.case(name)
    plan = si.bucket_plan(c["cells"])
    if name == "slivers":
        assert plan["first"] == (1024, 1024) and plan["first"][0] * plan["first"][1] > plan["table_budget"]
        assert plan["over_budget"] and plan["halvings"] >= 1 and plan["final"] != plan["first"]
        w, h = c["cells"][:, 2] - c["cells"][:, 0], c["cells"][:, 3] - c["cells"][:, 1]
        assert (w == 0).sum() == 1 and ((w > 0) & (w < 2e-3)).sum() == 20 and ((h > 0) & (h < 2e-3)).sum() == 20
    else:
        assert not plan["over_budget"] and plan["halvings"] == 0 and plan["final"] == plan["first"]
        assert plan["first"][0] > 1 and plan["first"][1] > 1
        assert plan["first"][0] * plan["first"][1] <= plan["table_budget"] and plan["first_items"] <= plan["item_budget"]


def test_bucket_case_contents():
    big_last, big_first = si.case("big_last"), si.case("big_first")
    assert tuple(big_last["cells"][-1]) == si.BOX and tuple(big_first["cells"][0]) == si.BOX
    assert np.array_equal(np.sort(big_last["cells"], axis=0), np.sort(big_first["cells"], axis=0))
    ov = si.case("overlap")
    p, cl = ov["pts"], ov["cells"]
    inside = ((p[:, None, 0] >= cl[None, :, 0]) & (p[:, None, 0] <= cl[None, :, 2])
              & (p[:, None, 1] >= cl[None, :, 1]) & (p[:, None, 1] <= cl[None, :, 3])).sum(axis=1)
    assert inside.max() >= 4 and (inside == 0).any()
    wr = si.case("wrapped")
    col = np.trunc((wr["cells"][:, 0] - si.BOX[0]) / si.CS)
    row = np.trunc((wr["cells"][:, 1] - si.BOX[1]) / si.CS)
    assert {-1, -2} <= set(col.tolist()) and {-1, -2} <= set(row.tolist())
    m = si.multiplicity(wr)
    assert m[:, 130].any() and m[34, :].any() and m[34, 130] == 1 and m[33, 129] >= 1
    assert len(si.case("empty_list")["cells"]) == 0
    nn = si.case("nan_points")["pts"]
    assert np.isnan(nn[:, 0]).sum() == 4 and np.isnan(nn[:, 1]).sum() == 3 and np.isnan(nn[:, 2]).sum() == 1
    ends = np.cumsum(si.case("nan_points")["traj_len"]) - 1
    assert not np.isnan(nn[ends]).any()


@pytest.mark.parametrize("name", ["big_last", "slivers", "overlap"])
def test_extreme_points_present(name):
    """points exactly on the smallest and largest x and y over all cells, and one ulp outside each"""
    c = si.case(name)
    cl, p = c["cells"], c["pts"]
    for v, col, out in ((cl[:, 0].min(), 0, -np.inf), (cl[:, 2].max(), 0, np.inf), (cl[:, 1].min(), 1, -np.inf), (cl[:, 3].max(), 1, np.inf)):
        assert (p[:, col] == v).any() and (p[:, col] == np.nextafter(v, out)).any()


def test_sliver_points_present():
    c = si.case("slivers")
    cl, p = c["cells"], c["pts"]
    w, h = cl[:, 2] - cl[:, 0], cl[:, 3] - cl[:, 1]
    on = lambda k: ((p[:, 0] >= cl[k, 0]) & (p[:, 0] <= cl[k, 2]) & (p[:, 1] >= cl[k, 1]) & (p[:, 1] <= cl[k, 3])).sum()  # noqa: E731
    assert sum(on(k) > 0 for k in np.nonzero((w > 0) & (w < 2e-3))[0]) >= 6
    assert sum(on(k) > 0 for k in np.nonzero((h > 0) & (h < 2e-3))[0]) >= 6
    assert on(int(np.nonzero(w == 0)[0][0])) >= 3


def test_atomics_cases():
    c = si.case("many_short")
    assert len(c["traj_len"]) == 70 and c["traj_len"].min() == 1 and c["traj_len"].max() == 3 and len(c["pts"]) % 64 != 0
    keys, T = si.point_keys(c)
    assert T == 2
    groups = [keys[i:i + 64] for i in range(0, len(keys), 64)]
    assert any(len(g) == 64 and len(set(g[g >= 0].tolist())) >= 20 and (g < 0).any() for g in groups)
    assert si.case("empty_traj")["traj_len"].tolist() == [40, 0, 30, 1, 25]
    c = si.case("no_bin")
    keys, T = si.point_keys(c)
    t = c["pts"][:, 2]
    assert T == 2 and (t < 0).any() and (t > T * c["bin_interval"]).any()
    first = keys[:64]
    assert (first[0::3] >= 0).all() and (first[1::3] < 0).all() and (first[2::3] < 0).all()
    c = si.case("unsorted")
    n0 = int(c["traj_len"][0])
    t0 = c["pts"][:n0, 2]
    assert (np.diff(t0) < 0).any() and t0.max() > 50.0 and t0[-1] == 21.0 and si.point_keys(c)[1] == 2


@pytest.mark.parametrize("name,count", si.ALL_RUNS, ids=["%s-%d" % rc for rc in si.ALL_RUNS])
def test_oracle_status_and_shape(orc, name, count):
    c = si.case(name)
    ref = si.reference(name, count)
    assert ref["status"] == 0
    assert ref["grids"].shape == (si.point_keys(c)[1],) + si.grid_shape(c["box"], c["cell_size"])
    assert len(ref["bins"]) >= 2
    if name != "empty_list":
        assert ref["grids"].max() > 0 and np.isfinite(ref["grids"]).all()

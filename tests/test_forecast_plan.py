"""The level schedule of the shark-occupancy forecast, asked of the library without a GPU (auvp_sf_plan: the pure host function
sf_plan of csrc/forecast_plan.h that auvp_sf_forecast's launch goes through), and the forecast kernel's register budget as the
compiler reports it.

SharkUpdate.prediction1 walks cell_list in order and a cell only sees neighbours filled in before it, so cell i depends on its
4-neighbours that are EARLIER in the list: level 0 without one, else 1 + the highest level among them.  The kernel fills a
level's cells side by side, so what must hold is: every earlier neighbour is strictly lower, and the levels are tight."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from auv_sim_amd import _lib  # noqa: E402

ERR_ARG = -1


def raster(rows, cols):
    return [(r, c) for r in range(rows) for c in range(cols)]


def snake(rows, cols):
    return [(r, c) for r in range(rows) for c in (range(cols) if r % 2 == 0 else range(cols - 1, -1, -1))]


def check_schedule(rows, cols, cells, plan):
    """the two properties of the levels + the sorted order is a permutation by (level, position) with matching offsets"""
    n = len(cells)
    pos = {rc: i for i, rc in enumerate(cells)}
    level = plan["level"]
    for i, (r, c) in enumerate(cells):
        earlier = [pos[q] for q in ((r - 1, c), (r, c - 1), (r + 1, c), (r, c + 1)) if q in pos and pos[q] < i]
        assert all(level[j] < level[i] for j in earlier), (i, cells)
        if level[i] > 0:
            assert any(level[j] == level[i] - 1 for j in earlier), (i, cells)
        else:
            assert not earlier
    order = plan["order"]
    assert sorted(order.tolist()) == list(range(n))
    assert order.tolist() == sorted(range(n), key=lambda i: (level[i], i))
    off = plan["level_off"]
    assert plan["n_levels"] == int(level.max()) + 1 == len(off) - 1 and off[0] == 0 and off[-1] == n
    for l in range(plan["n_levels"]):
        assert off[l] < off[l + 1] and all(level[i] == l for i in order[off[l]:off[l + 1]])


def test_raster_3x3_levels_are_the_anti_diagonals():
    plan = _lib.forecast_plan(3, 3, raster(3, 3))
    assert plan["level"].tolist() == [0, 1, 2, 1, 2, 3, 2, 3, 4]
    assert plan["n_levels"] == 5 and plan["level_off"].tolist() == [0, 1, 3, 6, 8, 9]
    assert plan["order"].tolist() == [0, 1, 3, 2, 4, 6, 5, 7, 8]
    check_schedule(3, 3, raster(3, 3), plan)


def test_reversed_raster_gives_the_mirrored_levels():
    cells = raster(3, 3)[::-1]
    plan = _lib.forecast_plan(3, 3, cells)
    assert plan["level"].tolist() == [0, 1, 2, 1, 2, 3, 2, 3, 4]   # by list position; by grid entry that is the mirror image:
    by_entry = np.zeros((3, 3), dtype=int)
    for i, (r, c) in enumerate(cells):
        by_entry[r, c] = plan["level"][i]
    assert by_entry.tolist() == [[4, 3, 2], [3, 2, 1], [2, 1, 0]]
    check_schedule(3, 3, cells, plan)


def test_raster_has_rows_plus_cols_minus_one_levels():
    for rows, cols in ((3, 2), (7, 5), (1, 9), (9, 1), (64, 64)):
        assert _lib.forecast_plan(rows, cols, raster(rows, cols))["n_levels"] == rows + cols - 1


def test_200_shuffled_lists_with_holes():
    rng = random.Random(14)
    for _ in range(200):
        cells = [rc for rc in raster(5, 4) if rng.random() < 0.75] or [(0, 0)]
        rng.shuffle(cells)
        check_schedule(5, 4, cells, _lib.forecast_plan(5, 4, cells))


def test_snake_list_is_one_cell_per_level():
    for rows, cols in ((7, 5), (2, 2), (4, 1)):
        cells = snake(rows, cols)
        plan = _lib.forecast_plan(rows, cols, cells)
        assert plan["n_levels"] == len(cells) and plan["level"].tolist() == list(range(len(cells)))
        check_schedule(rows, cols, cells, plan)


@pytest.mark.parametrize("cells", [
    [(0, 0), (0, 1), (0, 0)],       # a cell listed twice
    [(0, 0), (-1, 1)],              # a negative index (the reference wraps it silently)
    [(0, 0), (0, -1)],
    [(0, 0), (3, 0)],               # past the grid (the reference: IndexError)
    [(0, 0), (0, 2)],
    [],                             # no cell
], ids=["duplicate", "negative-row", "negative-col", "row-outside", "col-outside", "empty"])
def test_bad_lists_are_err_arg(cells):
    with pytest.raises(_lib.AuvpError) as e:
        _lib.forecast_plan(3, 2, cells)
    assert e.value.code == ERR_ARG


def test_bad_grid_shape_is_err_arg():
    for rows, cols in ((0, 3), (3, 0), (-1, 2)):
        with pytest.raises(_lib.AuvpError) as e:
            _lib.forecast_plan(rows, cols, [(0, 0)])
        assert e.value.code == ERR_ARG


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_forecast_kernel_uses_no_scratch(tmp_path):
    """sf_forecast_kernel: one wavefront per filter, every grid in LDS -- no private segment (the neighbour sum is written out
    per direction: an array under a computed index would become scratch), and registers for the eight wavefronts per SIMD
    that 300+ filters on a CU-count of workgroups can use"""
    import __graft_entry__ as ge
    src = tmp_path / "sf_unit.hip"
    src.write_text('#include "forecast_kernel.h"\n')
    cmd = [ge.HIPCC] + ge.HIP_FLAGS + dict(ge.UNITS)["auvplan.hip"] + ["-I", ge.CSRC, "-Rpass-analysis=kernel-resource-usage", "-c",
                                                                      "-o", os.devnull, str(src)]
    err = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO).stderr
    blk = [b for b in re.split(r"(?=[^\n]*remark: [^\n]*Function Name: )", err) if "sf_forecast_kernel" in b]
    assert len(blk) == 1, err[-2000:]
    g = lambda k: int(re.search(k + r": (\d+)", blk[0]).group(1))  # noqa: E731
    assert g(r"ScratchSize \[bytes/lane\]") == 0, blk[0]
    assert g("VGPRs") <= 64 and g(r"Occupancy \[waves/SIMD\]") == 8, blk[0]

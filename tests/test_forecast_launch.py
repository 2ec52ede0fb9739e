"""Which kernel a shark-occupancy forecast gets, and at what shape, asked of the library without a GPU (auvp_sf_choose_launch:
the pure host function sf_choose_launch of csrc/forecast_launch.h that auvp_sf_forecast / auvp_sf_forecast_large go through),
and sf_wide_kernel's resources as the compiler reports them.

The rules: without allow_large (auvp_sf_forecast) a grid of at most 4 096 entries takes the one-wavefront kernel and a larger
one is AUVP_ERR_CAPACITY, as ever; with it (auvp_sf_forecast_large) 4 097 .. 2**22 entries take sf_wide_kernel and more is
AUVP_ERR_CAPACITY.  Option SF_WIDE_MIN moves the lower edge (tests), SF_WIDE_BLOCK forces the threads per workgroup."""
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from auv_sim_amd import _lib  # noqa: E402

OK, ERR_ARG, ERR_CAPACITY = 0, -1, -2
ONE, WIDE = "sf_forecast_kernel", "sf_wide_kernel"
WIDE_MAX = 1 << 22


def choose(rows, cols, **kw):
    return _lib.forecast_choose_launch(rows, cols, **kw)


def test_without_allow_large_the_rule_is_todays():
    p = choose(64, 64)                          # 4 096 entries
    assert (p["status"], p["kind"], p["name"], p["block"]) == (OK, "one-wave", ONE, 64)
    assert p["lds"] == 4096 * 20                # two fp64 grids + the int32 counts
    assert choose(17, 241)["status"] == ERR_CAPACITY     # 4 097
    assert choose(201, 201)["status"] == ERR_CAPACITY
    # the options of the wide kernel do not reach the entry point that never launches it
    for opts in (dict(SF_WIDE_MIN=1), dict(SF_WIDE_BLOCK=512), dict(SF_WIDE_BLOCK=100), dict(SF_WIDE_MIN=1, SF_WIDE_BLOCK=0)):
        assert choose(64, 64, options=opts) == p
        assert choose(3, 2, options=opts)["name"] == ONE
        assert choose(17, 241, options=opts)["status"] == ERR_CAPACITY


def test_allow_large_changes_kernels_at_4097_entries():
    small = choose(64, 64, allow_large=True)
    assert small == choose(64, 64)              # up to the cap: the launch the default entry point makes
    p = choose(17, 241, allow_large=True)
    assert (p["status"], p["kind"], p["name"]) == (OK, "wide", WIDE)
    for rows, cols in ((65, 64), (201, 201), (1, 4097), (4097, 1)):
        q = choose(rows, cols, allow_large=True)
        assert (q["status"], q["name"], q["block"], q["lds"]) == (OK, WIDE, p["block"], p["lds"])
    assert choose(1, 4096, allow_large=True)["name"] == ONE


def test_the_wide_kernels_limit_is_2_to_the_22():
    assert WIDE_MAX == 2048 * 2048
    p = choose(2048, 2048, allow_large=True)
    assert (p["status"], p["name"]) == (OK, WIDE)
    assert choose(1, WIDE_MAX, allow_large=True)["status"] == OK
    assert choose(1, WIDE_MAX + 1, allow_large=True)["status"] == ERR_CAPACITY
    assert choose(2049, 2048, allow_large=True)["status"] == ERR_CAPACITY
    assert choose(65536, 65536, allow_large=True)["status"] == ERR_CAPACITY      # (the product is taken in 64 bits)
    assert choose(1, WIDE_MAX)["status"] == ERR_CAPACITY


def test_the_default_block_is_a_multiple_of_64_in_range():
    for rows, cols in ((17, 241), (201, 201), (2048, 2048)):
        b = choose(rows, cols, allow_large=True)["block"]
        assert 64 <= b <= 1024 and b % 64 == 0


def test_sf_wide_min_sends_small_grids_to_the_wide_kernel():
    for rows, cols in ((1, 1), (3, 2), (7, 5), (64, 64)):
        p = choose(rows, cols, allow_large=True, options=dict(SF_WIDE_MIN=1))
        assert (p["status"], p["name"]) == (OK, WIDE)
    assert choose(7, 5, allow_large=True, options=dict(SF_WIDE_MIN=35))["name"] == WIDE
    assert choose(7, 5, allow_large=True, options=dict(SF_WIDE_MIN=36))["name"] == ONE
    # a value above the default cannot keep a grid on a kernel whose LDS it does not fit
    assert choose(17, 241, allow_large=True, options=dict(SF_WIDE_MIN=100000))["name"] == WIDE
    assert choose(64, 64, allow_large=True, options=dict(SF_WIDE_MIN=100000))["name"] == ONE


def test_sf_wide_block_forces_the_block_and_refuses_bad_values():
    for b in (64, 128, 256, 512, 960, 1024):
        p = choose(201, 201, allow_large=True, options=dict(SF_WIDE_BLOCK=b))
        assert (p["status"], p["name"], p["block"]) == (OK, WIDE, b)
        p = choose(3, 2, allow_large=True, options=dict(SF_WIDE_MIN=1, SF_WIDE_BLOCK=b))
        assert (p["status"], p["name"], p["block"]) == (OK, WIDE, b)
    for b in (0, -64, 1, 63, 65, 100, 32, 1025, 1088, 2048):
        assert choose(201, 201, allow_large=True, options=dict(SF_WIDE_BLOCK=b))["status"] == ERR_ARG, b
    # where the one-wavefront kernel runs the option is not read
    assert choose(64, 64, allow_large=True, options=dict(SF_WIDE_BLOCK=100))["name"] == ONE


def test_bad_shapes_and_unknown_options():
    for rows, cols in ((0, 3), (3, 0), (-1, 2)):
        for large in (False, True):
            assert choose(rows, cols, allow_large=large)["status"] == ERR_ARG
    with pytest.raises(_lib.AuvpError) as e:
        choose(3, 2, options=dict(SF_WIDE=1))
    assert e.value.code == ERR_ARG
    for name in ("SF_WIDE_MIN", "SF_WIDE_BLOCK"):
        assert name in _lib.OPTION_NAMES


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_wide_kernel_resources(tmp_path):
    """sf_wide_kernel, compiled from a unit that holds its header alone: no private segment (at up to 16 wavefronts per
    workgroup a spill would cost every level of every round), and static + dynamic LDS within what sf_choose_launch reports --
    the figure a caller sizes occupancy by"""
    import __graft_entry__ as ge
    src = tmp_path / "sf_wide_unit.hip"
    src.write_text('#include "forecast_wide_kernel.h"\n')
    cmd = [ge.HIPCC] + ge.HIP_FLAGS + dict(ge.UNITS)["auvplan.hip"] + ["-I", ge.CSRC, "-Rpass-analysis=kernel-resource-usage", "-c",
                                                                      "-o", os.devnull, str(src)]
    err = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO).stderr
    blk = [b for b in re.split(r"(?=[^\n]*remark: [^\n]*Function Name: )", err) if "sf_wide_kernel" in b]
    assert len(blk) == 1, err[-2000:]
    g = lambda k: int(re.search(k + r": (\d+)", blk[0]).group(1))  # noqa: E731
    assert g(r"ScratchSize \[bytes/lane\]") == 0, blk[0]
    plan = choose(201, 201, allow_large=True)
    static_lds = g(r"LDS Size \[bytes/block\]")
    dynamic_lds = 0          # (forecast_host.h launches it with none)
    assert 0 < static_lds + dynamic_lds <= plan["lds"], blk[0]

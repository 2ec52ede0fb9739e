"""The steer's theta chain of the four-episode RRT expansion kernels runs on 64-bit DPP row broadcasts (rows_theta_chain_dpp,
auv_sim_amd/csrc/rrt_rows_kernel.h) -- checked without a GPU on the machine code cross-compiled for gfx950, the way
tests/test_rows_trip_lgkm.py does:
  * rrt_rows_stream_kernel<12> holds exactly 30 v_fmac_f64_dpp: fifteen steps in each of the two instances of a steer pass;
  * it holds no more LDS instructions than the 235 the change left (267 before: a pass's write of the phis and its fifteen
    broadcast reads are gone, twice)."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM = "_ZN4auvpL22rrt_rows_stream_kernelILi12EEE"
DPP_STEPS = 30
LDS_INSTRUCTIONS = 235


@pytest.fixture(scope="module")
def stream_body(tmp_path_factory):
    import __graft_entry__ as ge
    out = str(tmp_path_factory.mktemp("rows_theta_asm") / "rows_kernels.s")
    cmd = [ge.HIPCC] + ge.HIP_FLAGS + dict(ge.UNITS)["rows_kernels.hip"] + ["-I" + os.path.join(REPO, "include"), "--cuda-device-only", "-S",
                                                                           os.path.join(ge.CSRC, "rows_kernels.hip"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, cwd=REPO)
    lines = open(out).read().split("\n")
    s = [i for i, l in enumerate(lines) if re.match(re.escape(STREAM) + r"\w*:", l)]
    assert len(s) == 1, s
    e = next(i for i in range(s[0], len(lines)) if lines[i].startswith(".Lfunc_end"))
    return [l.strip() for l in lines[s[0]:e]]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_theta_chain_is_thirty_dpp_fmacs(stream_body):
    steps = [l for l in stream_body if l.startswith("v_fmac_f64_dpp")]
    assert len(steps) == DPP_STEPS, len(steps)
    # every step is a row broadcast over all rows and banks; lanes 0 .. 14 of the row, in order, once per instance
    lanes = [int(re.search(r"row_newbcast:(\d+) row_mask:0xf bank_mask:0xf", l).group(1)) for l in steps]
    assert lanes == list(range(15)) * 2, lanes


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_more_lds_instructions_than_the_change_left(stream_body):
    ds = [l for l in stream_body if l.startswith("ds_")]
    print("ds_*:", len(ds))
    assert len(ds) <= LDS_INSTRUCTIONS, len(ds)

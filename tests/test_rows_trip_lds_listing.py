"""A trip of rrt_rows_stream_kernel<12> takes no LDS round trip for numbers its lanes already hold in registers
(profiles/rows_trip_lds.md) -- checked without a GPU on the machine code cross-compiled for gfx950, the way
tests/test_rows_theta_listing.py does:
  * a steer pass's end state comes from the chain ends: five v_mov_b64_dpp row broadcasts (lanes 0, 1, 2, 3: the four sums; lane
    14: the angle) in each of the two instances of a pass, ten in all (rows_pass_ends_dpp, auv_sim_amd/csrc/rrt_rows_kernel.h);
  * no more LDS instructions than the 223 these changes left (235 before: per instance of a pass the two 16-byte reads of the end
    state, the two ds_bpermute of the last angle and the two writes that zeroed entry 15 of the rows are gone)."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM = "_ZN4auvpL22rrt_rows_stream_kernelILi12EEE"
LDS_INSTRUCTIONS = 223
END_LANES = [0, 1, 2, 3, 14]


@pytest.fixture(scope="module")
def stream_body(tmp_path_factory):
    import __graft_entry__ as ge
    out = str(tmp_path_factory.mktemp("rows_trip_lds_asm") / "rows_kernels.s")
    cmd = [ge.HIPCC] + ge.HIP_FLAGS + dict(ge.UNITS)["rows_kernels.hip"] + ["-I" + os.path.join(REPO, "include"), "--cuda-device-only", "-S",
                                                                           os.path.join(ge.CSRC, "rows_kernels.hip"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, cwd=REPO)
    lines = open(out).read().split("\n")
    s = [i for i, l in enumerate(lines) if re.match(re.escape(STREAM) + r"\w*:", l)]
    assert len(s) == 1, s
    e = next(i for i in range(s[0], len(lines)) if lines[i].startswith(".Lfunc_end"))
    return [l.strip() for l in lines[s[0]:e]]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_a_pass_ends_with_five_dpp_moves(stream_body):
    movs = [l for l in stream_body if l.startswith("v_mov_b64_dpp")]
    assert len(movs) == 2 * len(END_LANES), len(movs)
    lanes = [int(re.search(r"row_newbcast:(\d+) row_mask:0xf bank_mask:0xf", l).group(1)) for l in movs]
    assert lanes == END_LANES * 2, lanes
    # the four sums are moves of ONE register pair (the chains' `acc`), the angle of another
    src = [re.match(r"v_mov_b64_dpp v\[\d+:\d+\], (v\[\d+:\d+\])", l).group(1) for l in movs]
    for k in (0, 5):
        assert len(set(src[k:k + 4])) == 1 and src[k + 4] != src[k], src


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_more_lds_instructions_than_the_changes_left(stream_body):
    ds = [l for l in stream_body if l.startswith("ds_")]
    print("ds_*:", len(ds))
    assert len(ds) <= LDS_INSTRUCTIONS, len(ds)

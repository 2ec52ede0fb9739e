"""The four-episode RRT kernels keep the obstacles' collision thresholds off the vector-memory counter (profiles/rows_trip_waits.md):
`vmcnt` is one in-order counter for loads and stores, so a wait for a threshold load also waited for the trip's point stores.
Checked on the machine code, cross-compiled for gfx950 (no GPU needed), without tying anything to label or register numbers:
  * no global load of the kernel has a scalar-register base and a vector offset -- the form `W.os_t[oi]` compiled to, the only
    table the loop indexed per lane straight from memory (the obstacle tile is in LDS, the per-episode arrays have vector bases);
  * each kernel has the eight scalar 8-byte loads at a computed address that replace it (four rows x the two cull forms);
  * no scalar register is spilled and there is no scratch: the four row masks of the naive form cost 4-8 spills, reloaded in the loop.
What the listing cannot show without label numbers -- that no wait lies between a pass's point stores and the next trip's
bin-member read on the path without candidates -- is recorded in the profile note."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("_ZN4auvpL15rrt_rows_kernelE", "_ZN4auvpL22rrt_rows_stream_kernelILi12EEE", "_ZN4auvpL29rrt_rows_stream_masked_kernelILi12EEE")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    import __graft_entry__ as ge
    out = str(tmp_path_factory.mktemp("rows_asm") / "rows_kernels.s")
    cmd = [ge.HIPCC] + ge.HIP_FLAGS + dict(ge.UNITS)["rows_kernels.hip"] + ["-I" + os.path.join(REPO, "include"), "--cuda-device-only", "-S",
                                                                           os.path.join(ge.CSRC, "rows_kernels.hip"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, cwd=REPO)
    return open(out).read().split("\n")


def _function(lines, prefix):
    s = [i for i, l in enumerate(lines) if re.match(re.escape(prefix) + r"\w*:", l)]
    assert len(s) == 1, (prefix, s)
    e = next(i for i in range(s[0], len(lines)) if lines[i].startswith(".Lfunc_end"))
    return [l.strip() for l in lines[s[0]:e]]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
@pytest.mark.parametrize("kernel", KERNELS)
def test_thresholds_are_read_through_the_scalar_path_without_spills(listing, kernel):
    body = _function(listing, kernel)
    per_lane_table_loads = [l for l in body if re.match(r"global_load_\w+ v(\[\d+:\d+\]|\d+), v\d+, s\[\d+:\d+\]", l) and "dwordx4" not in l]
    assert per_lane_table_loads == [], per_lane_table_loads   # (dwordx4: the slot boxes, loaded once before the loop)
    computed = [l for l in body if re.match(r"s_load_dwordx2 s\[\d+:\d+\], s\[\d+:\d+\], 0x0$", l) and ", s[0:1], " not in l]  # (s[0:1]: the kernel's arguments)
    assert len(computed) == 8, computed
    meta = "\n".join(listing)
    m = re.search(r"\.name:\s+" + re.escape(kernel) + r"\w*\n(.*?)\.wavefront_size", meta, re.S)
    assert m, kernel
    g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", m.group(1)).group(1))
    assert g("sgpr_spill_count") == 0 and g("vgpr_spill_count") == 0 and g("private_segment_fixed_size") == 0

"""What profiles/rows_trip_lgkm.md states about the waits of the four-episode RRT expansion kernels, as far as it can be checked
without a GPU and without label numbers, on the machine code cross-compiled for gfx950 as in profiles/rows_trip_waits.md:
  * rrt_rows_stream_kernel<12> has no more `s_waitcnt vmcnt` than the 31 the census counted (the accept path's own append
    helper -- step 1 of the note -- was measured inside the box's spread and is NOT in the product, so nothing is subtracted);
  * no scratch, no spilled register, at most 168 vector registers in the three kernels built from the body.
(Step 2 of the note -- the thresholds in the LDS tile -- was not kept either, so the eight scalar loads of the candidate loop
stay what tests/test_rows_trip_waits.py asserts.)
And the probe's source patch (tools/instrument/rows_wait_stamps_patch.py) still finds every anchor in today's body and leaves the
unstamped text as it was: with the stamped blocks taken out again the file is the committed one."""
import os
import re
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM = "_ZN4auvpL22rrt_rows_stream_kernelILi12EEE"
KERNELS = ("_ZN4auvpL15rrt_rows_kernelE", STREAM, "_ZN4auvpL29rrt_rows_stream_masked_kernelILi12EEE")
PARENT_VMCNT_WAITS = 31


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    import __graft_entry__ as ge
    out = str(tmp_path_factory.mktemp("rows_lgkm_asm") / "rows_kernels.s")
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
def test_no_vector_memory_wait_more_than_the_census_counted(listing):
    body = _function(listing, STREAM)
    waits = [l for l in body if re.match(r"s_waitcnt\b.*\bvmcnt\(\d+\)", l)]
    print("s_waitcnt vmcnt:", len(waits), "of them vmcnt(0):", sum("vmcnt(0)" in l for l in waits))
    assert len(waits) <= PARENT_VMCNT_WAITS, len(waits)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
@pytest.mark.parametrize("kernel", KERNELS)
def test_resources(listing, kernel):
    meta = "\n".join(listing)
    m = re.search(r"\.name:\s+" + re.escape(kernel) + r"\w*\n(.*?)\.wavefront_size", meta, re.S)
    assert m, kernel
    g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", m.group(1)).group(1))
    assert g("vgpr_count") <= 168
    assert g("sgpr_spill_count") == 0 and g("vgpr_spill_count") == 0 and g("private_segment_fixed_size") == 0


def test_the_stamp_patch_fits_todays_body(tmp_path):
    src = os.path.join(REPO, "auv_sim_amd", "csrc", "rrt_rows_body.h")
    work = str(tmp_path / "rrt_rows_body.h")
    shutil.copy(src, work)
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "instrument", "rows_wait_stamps_patch.py"), work], check=True)
    patched = open(work).read()
    assert patched.count("#ifdef AUVP_ROWS_WAIT_STAMPS") >= 14
    for c in range(1, 8):   # every class is stamped somewhere
        assert re.search(r"ROWS_WS_IN\(%d\)" % c, patched) and re.search(r"ROWS_WS_OUT\(%d\)" % c, patched), c
    # (every block the patch adds starts on a line of its own -- after a newline it adds itself -- and ends with #endif)
    stripped = re.sub(r"\n?#ifdef AUVP_ROWS_WAIT_STAMPS\n.*?#endif\n?", "", patched, flags=re.S)
    orig = open(src).read()
    assert "".join(stripped.split()) == "".join(orig.split())

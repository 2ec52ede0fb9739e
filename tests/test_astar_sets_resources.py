"""astar_fixLenSOG with a table per instance lives in a translation unit of its own (csrc/astar_sets_kernels.hip) so that the
plain kernels keep their code.  The compiler's own report (cross-compiled for gfx950, no GPU needed): astar_kernel<3> and
astar_kernel<3, true> of auvplan.hip have the registers, scratch and occupancy they had before the sets forms existed, and the
sets forms are not below their plain twins in occupancy (their registers and scratch are recorded in
profiles/astar_shark_sets.md, not gated)."""
import os

import pytest

from test_kernel_resources import _resources

# -Rpass-analysis=kernel-resource-usage on auvplan.hip at commit f3646e3 (the parent of the commit that added the sets forms)
PARENT = {"auvp::astar_kernel<3, false>": dict(vgprs=120, scratch=0, waves=3),
          "auvp::astar_kernel<3, true>": dict(vgprs=105, scratch=0, waves=4)}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_plain_kernels_keep_their_resources_and_the_sets_forms_their_occupancy():
    plain = _resources("auvplan.hip")
    for name, want in PARENT.items():
        assert plain[name] == want, (name, plain[name], want)
    sets = _resources("astar_sets_kernels.hip")
    for name in PARENT:
        twin = name.replace("astar_kernel", "astar_sets_kernel")
        print(twin, sets[twin])
        assert sets[twin]["waves"] >= plain[name]["waves"], (twin, sets[twin], plain[name])
    assert not any("astar_kernel<" in k or "astar_path_kernel" in k for k in sets), sorted(sets)

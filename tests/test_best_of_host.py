"""Best-of-K planning, the parts that need no GPU: the four entry points are declared in include/auvplan.h and exported by the
built library, the record's numpy dtype and ctypes struct agree with the C struct, and the header stays valid C although the
record and the entry point share their name (a struct tag beside a function)."""
import ctypes
import os
import re
import subprocess

from conftest import REPO

NAMES = ("auvp_rrt_group_best", "auvp_rrt_group_best_dev", "auvp_rrt_group_paths", "auvp_rrt_group_paths_dev")
HEADER = os.path.join(REPO, "include", "auvplan.h")


def test_group_entry_points_declared_and_exported():
    import __graft_entry__ as ge
    ge.build()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(auvp_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(os.path.join(REPO, "auv_sim_amd", "libauvplan.so"))
    for n in NAMES:
        assert n in declared, "not declared: " + n
        assert hasattr(lib, n), "missing export: " + n


def test_group_record_layout():
    from auv_sim_amd import _lib
    assert _lib.GROUP_BEST_DTYPE.itemsize == ctypes.sizeof(_lib.RRTGroupBest) == 56
    for name, _ in _lib.RRTGroupBest._fields_:
        assert _lib.GROUP_BEST_DTYPE.fields[name][1] == getattr(_lib.RRTGroupBest, name).offset, name
    assert _lib.GROUP_BEST_DTYPE.names == tuple(n for n, _ in _lib.RRTGroupBest._fields_)


def test_header_is_valid_c_with_the_shared_name(tmp_path):
    """a C caller sees struct auvp_rrt_group_best (tag) and auvp_rrt_group_best() (function) side by side, 56 bytes"""
    src = tmp_path / "use.c"
    src.write_text('#include <stddef.h>\n#include "auvplan.h"\n'
                   "_Static_assert(sizeof(struct auvp_rrt_group_best) == 56, \"record size\");\n"
                   "int use(auvp_handle* h, const int32_t* off, struct auvp_rrt_group_best* out) {\n"
                   "  return auvp_rrt_group_best(h, 1, off, out);\n}\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)])

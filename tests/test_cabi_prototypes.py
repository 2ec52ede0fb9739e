"""auv_sim_amd/_cabi.py against include/auvplan.h, without a GPU: the prototype table against the header's declarations, the
ctypes Structures and the record dtypes against the C and the C++ compiler's layout of the header's structs, the header on its
own, every prototype bound by `_lib.load()` alone, and no prototype assigned anywhere else.

The rule the table must follow (the module's docstring): a scalar is the ctypes scalar of exactly that type; `const char*` is
c_char_p; `auvp_handle*` and `void*` are c_void_p; any other `T*` is POINTER(ctype of T) -- for a public struct its registered
Structure -- or c_void_p (a device address, an array of records); `X**` is POINTER(c_void_p); c_void_p stands for pointers only."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

from auv_sim_amd import _cabi

HEADER = os.path.join(REPO, "include", "auvplan.h")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double,
           "size_t": C.c_size_t}
POINTEES = dict(SCALARS, int8_t=C.c_int8, uint8_t=C.c_uint8, uint32_t=C.c_uint32)
needs_gcc = pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="no gcc / g++")


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def split_type(t):
    """'const struct auvp_x* ' -> ('auvp_x', 1)"""
    return " ".join(w for w in t.replace("*", " ").split() if w not in ("const", "struct")), t.count("*")


def declarations(text):
    """{name: ((base, stars) of the return type, [(base, stars) per parameter])} of every auvp_* function the header text declares"""
    text = re.sub(r"^\s*#.*$", "", strip_comments(text), flags=re.M)
    out = {}
    for statement in re.split(r"[;{}]", text):
        m = re.match(r"^\s*([\w\s\*]+?)\b(auvp_\w+)\s*\((.*)\)\s*$", statement, flags=re.S)
        if not m:
            continue
        params = []
        for p in m.group(3).split(","):
            p = " ".join(p.split())
            if p != "void":
                params.append(split_type(re.match(r"^(.*[\s\*])\w+$", p).group(1)))
        assert m.group(2) not in out, "declared twice: " + m.group(2)
        out[m.group(2)] = (split_type(m.group(1)), params)
    return out


def param_ok(ctype, base, stars):
    if stars == 0:
        return ctype is SCALARS.get(base)
    if base == "char":
        return stars == 1 and ctype is C.c_char_p
    if ctype is C.c_void_p:
        return True
    if stars == 2:
        return ctype is C.POINTER(C.c_void_p)
    if base in ("auvp_handle", "void"):
        return False
    pointee = POINTEES.get(base) or _cabi.STRUCTS.get(base)
    return pointee is not None and ctype is C.POINTER(pointee)


def return_ok(ctype, base, stars):
    if stars == 0:
        return ctype is (None if base == "void" else SCALARS.get(base))
    return stars == 1 and ctype is {"char": C.c_char_p, "void": C.c_void_p}.get(base)


def mismatches(decl, table):
    """every way the table departs from the declarations, as a list of messages"""
    bad = ["only in the header: " + n for n in sorted(set(decl) - set(table))]
    bad += ["only in the table: " + n for n in sorted(set(table) - set(decl))]
    for name in sorted(set(decl) & set(table)):
        (ret, params), (restype, argtypes) = decl[name], table[name]
        if not return_ok(restype, *ret):
            bad.append("%s: returns %r, the table has %r" % (name, ret, restype))
        if len(params) != len(argtypes):
            bad.append("%s: %d parameters, the table has %d" % (name, len(params), len(argtypes)))
            continue
        bad += ["%s: parameter %d is %r, the table has %r" % (name, k, p, t)
                for k, (p, t) in enumerate(zip(params, argtypes)) if not param_ok(t, *p)]
    return bad


@pytest.fixture(scope="module")
def header_text():
    return open(HEADER).read()


def test_table_matches_the_header(header_text):
    decl = declarations(header_text)
    assert len(decl) == 134 and len(_cabi.PROTOTYPES) == 134
    assert mismatches(decl, _cabi.PROTOTYPES) == []


def test_a_wrong_table_or_header_is_caught(header_text):
    decl = declarations(header_text)
    # a scalar of the wrong width
    restype, argtypes = _cabi.PROTOTYPES["auvp_set_option"]
    assert argtypes[2] is C.c_int64
    swapped = dict(_cabi.PROTOTYPES, auvp_set_option=(restype, argtypes[:2] + (C.c_int32,)))
    assert mismatches(decl, swapped) == ["auvp_set_option: parameter 2 is ('int64_t', 0), the table has %r" % (C.c_int32,)]
    restype, argtypes = _cabi.PROTOTYPES["auvp_rrt_last_stream_len"]
    assert len(mismatches(decl, dict(_cabi.PROTOTYPES, auvp_rrt_last_stream_len=(C.c_int32, argtypes)))) == 1
    # a parameter dropped
    restype, argtypes = _cabi.PROTOTYPES["auvp_rrt_tree"]
    assert mismatches(decl, dict(_cabi.PROTOTYPES, auvp_rrt_tree=(restype, argtypes[:-1]))) == \
        ["auvp_rrt_tree: 7 parameters, the table has 6"]
    # c_void_p for a scalar, a pointer of the wrong element type, a struct pointer of the wrong struct
    for name, k, wrong in (("auvp_rrt_tree", 1, C.c_void_p), ("auvp_rrt_tree", 3, C.POINTER(C.c_double)),
                           ("auvp_rrt_prepare", 4, C.POINTER(_cabi.PrrtParams)), ("auvp_create", 1, C.POINTER(C.c_double))):
        restype, argtypes = _cabi.PROTOTYPES[name]
        assert len(mismatches(decl, {**_cabi.PROTOTYPES, name: (restype, argtypes[:k] + (wrong,) + argtypes[k + 1:])})) == 1, name
    # the header with one function more, with one function less
    more = header_text.replace("int auvp_rrt_run(auvp_handle* h);", "int auvp_rrt_run(auvp_handle* h);\nint auvp_rrt_walk(auvp_handle* h, double* out);")
    assert mismatches(declarations(more), _cabi.PROTOTYPES) == ["only in the header: auvp_rrt_walk"]
    less = header_text.replace("int auvp_rrt_run(auvp_handle* h);", "")
    assert mismatches(declarations(less), _cabi.PROTOTYPES) == ["only in the table: auvp_rrt_run"]


def struct_fields(text):
    """{struct name: [field names]} of the header's struct definitions, in order"""
    text = re.sub(r"^\s*#.*$", "", strip_comments(text), flags=re.M)
    out = {}
    for m in re.finditer(r"(?:typedef\s+struct|struct\s+(\w+))\s*\{([^{}]*)\}\s*(\w*)\s*;", text):
        names = []
        for member in m.group(2).split(";"):
            if member.strip():
                names += [re.search(r"(\w+)\s*(?:\[\d+\])?\s*$", d).group(1) for d in member.split(",")]
        out[m.group(1) or m.group(3)] = names
    return out


def test_structures_name_every_field_of_the_header(header_text):
    fields = struct_fields(header_text)
    assert sorted(fields) == sorted(_cabi.STRUCTS)
    for name, cls in _cabi.STRUCTS.items():
        assert [f[0] for f in cls._fields_] == fields[name], name


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """{struct: sizeof}, {(struct, field): (offset, size)} as the C compiler lays the header's structs out; the C++ compiler agrees"""
    d = tmp_path_factory.mktemp("cabi_layout")
    src, inc = os.path.join(REPO, "tests", "host", "cabi_layout_dump.c"), ["-I", os.path.join(REPO, "include")]
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror"] + inc + ["-o", str(d / "dump_c"), src], check=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-x", "c++"] + inc + ["-o", str(d / "dump_cxx"), src], check=True)
    text = subprocess.run([str(d / "dump_c")], capture_output=True, text=True, check=True).stdout
    assert text == subprocess.run([str(d / "dump_cxx")], capture_output=True, text=True, check=True).stdout
    sizes, fields = {}, {}
    for line in text.splitlines():
        name, a, b = line.split()
        if a == "sizeof":
            sizes[name] = int(b)
        else:
            fields[tuple(name.split("."))] = (int(a), int(b))
    return sizes, fields


@needs_gcc
def test_structures_have_the_compilers_layout(layout):
    sizes, fields = layout
    assert sorted(sizes) == sorted(_cabi.STRUCTS)
    assert sorted(fields) == sorted((name, f[0]) for name, cls in _cabi.STRUCTS.items() for f in cls._fields_)
    for name, cls in _cabi.STRUCTS.items():
        assert C.sizeof(cls) == sizes[name], name
        for f in cls._fields_:
            d = getattr(cls, f[0])
            assert (d.offset, d.size) == fields[name, f[0]], (name, f[0])
    assert sizes["auvp_replan_record"] == 128  # (the header's comment)


@needs_gcc
def test_record_dtypes_have_the_compilers_layout(layout):
    sizes, fields = layout
    records = {"auvp_rrt_summary": _cabi.SUMMARY_DTYPE, "auvp_rrt_episode": _cabi.EPISODE_DTYPE,
               "auvp_rrt_group_best": _cabi.GROUP_BEST_DTYPE, "auvp_replan_record": _cabi.REPLAN_RECORD_DTYPE,
               "auvp_prrt_summary": _cabi.PRRT_SUMMARY_DTYPE, "auvp_astar_summary": _cabi.ASTAR_SUMMARY_DTYPE}
    for name, dt in records.items():
        assert dt.itemsize == sizes[name], name
        want = {f: v for (s, f), v in fields.items() if s == name}
        if name == "auvp_astar_summary":  # the counter's halves are read as the one little-endian uint64 they form
            lo, hi = want.pop("open_scanned_lo"), want.pop("open_scanned_hi")
            assert hi == (lo[0] + 4, 4) and sys.byteorder == "little"
            want["open_scanned"] = (lo[0], 8)
        assert {f: (dt.fields[f][1], dt.fields[f][0].itemsize) for f in dt.names} == want, name
    assert _cabi.ASTAR_SUMMARY_DTYPE["open_scanned"] == np.dtype("<u8")


@needs_gcc
def test_header_compiles_on_its_own(tmp_path):
    (tmp_path / "only.c").write_text('#include "auvplan.h"\n')
    inc = ["-I", os.path.join(REPO, "include")]
    subprocess.run(["gcc", "-std=c99", "-fsyntax-only"] + inc + [str(tmp_path / "only.c")], check=True)
    subprocess.run(["g++", "-fsyntax-only", "-x", "c++"] + inc + [str(tmp_path / "only.c")], check=True)


def test_load_alone_binds_every_prototype():
    """in a fresh process: nothing but _lib.load() has run -- no Context, no PlannerBatch"""
    import __graft_entry__ as ge
    ge.build()
    code = ("import sys\n"
            "sys.path.insert(0, %r)\n"
            "from auv_sim_amd import _cabi, _lib\n"
            "L = _lib.load()\n"
            "for name, (restype, argtypes) in _cabi.PROTOTYPES.items():\n"
            "    fn = getattr(L, name)\n"
            "    assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name\n"
            "v, lib = L.auvp_version(), L.auvp_comm_library()\n"
            "assert isinstance(v, bytes) and isinstance(lib, bytes), (v, lib)\n"
            "print('ok', len(_cabi.PROTOTYPES))\n" % REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok 134", (r.returncode, r.stdout, r.stderr)


def test_bind_skips_what_a_library_lacks():
    """an earlier build lacks the newest entry points: bind sets what is there, and the rest raises AttributeError when called"""
    class Fn:
        restype, argtypes = C.c_int, None

    class Older:
        pass

    lib = Older()
    lib.auvp_version, lib.auvp_rrt_run = Fn(), Fn()
    assert _cabi.bind(lib) is lib
    assert lib.auvp_version.restype is C.c_char_p and lib.auvp_version.argtypes == []
    assert lib.auvp_rrt_run.restype is C.c_int and lib.auvp_rrt_run.argtypes == [C.c_void_p]
    with pytest.raises(AttributeError):
        lib.auvp_replan_begin


def test_no_prototype_is_assigned_anywhere_else():
    # (the stand-in that tests/test_distributed_gloo.py passes as L= is a Python object: it assigns none)
    allowed = {os.path.join("auv_sim_amd", "_cabi.py"): None,
               os.path.join("tests", "test_portable_math.py"): "libm.hypot."}      # libm, not libauvplan
    stray = []
    for top in ("auv_sim_amd", "tests", "tools", "bench_sides"):
        for root, _, files in os.walk(os.path.join(REPO, top)):
            for f in files:
                path = os.path.relpath(os.path.join(root, f), REPO)
                if not f.endswith(".py") or path == os.path.join("tests", "test_cabi_prototypes.py"):
                    continue
                for k, line in enumerate(open(os.path.join(root, f), errors="replace"), 1):
                    if re.search(r"\.(argtypes|restype)\s*=(?!=)", line):
                        if path in allowed and (allowed[path] is None or allowed[path] in line):
                            continue
                        stray.append("%s:%d: %s" % (path, k, line.strip()))
    assert stray == []

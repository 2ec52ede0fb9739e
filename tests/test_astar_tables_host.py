"""The top-n table of astar_fixLenSOG's heuristic, built without a GPU: csrc/astar_tables.h (the pure host function behind the
world's own table and behind the host route of the probability sets' tables) compiled into tests/host/astar_tables_dump.cpp with
g++, once plain and once with the address / undefined-behaviour sanitizers, and its rows compared byte for byte with what
get_top_n_prob computes (astar_fixLenSOG.py:516-531): sorted(row, reverse=True) and a running `total += v` from 0."""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def python_topn(prob):
    """[T, C] -> [T, C + 1], the reference's own operations on Python floats"""
    out = np.zeros((prob.shape[0], prob.shape[1] + 1))
    for t, row in enumerate(prob):
        total = 0
        for i, v in enumerate(sorted(row.tolist(), reverse=True)):
            total += v
            out[t, i + 1] = total
    return out


def awkward_rows(C, seed):
    """[4, C]: ties, zeros of both signs, negative values, one +inf; the rows differ from each other"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.5, 1.0, (4, C))
    if C >= 2:
        p[0, :] = np.round(p[0, :], 1)                # ties
        p[1, ::3] = 0.0
        p[1, 1::3] = -0.0
        p[2, rng.integers(0, C)] = np.inf
        p[3, :] = -np.abs(p[3, :])
        p[3, C // 2] = 0.25
    return p


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("astar_tables")
    out = []
    for name, extra in (("plain", ["-O2"]), ("san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / ("astar_tables_dump_" + name))
        subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + extra + ["-I", os.path.join(REPO, "auv_sim_amd", "csrc"), "-o", exe,
                        os.path.join(REPO, "tests", "host", "astar_tables_dump.cpp")], check=True)
        out.append(exe)
    count = [0]

    def run(exe, prob):
        count[0] += 1
        src, dst = str(d / ("in%d.bin" % count[0])), str(d / ("out%d.bin" % count[0]))
        with open(src, "wb") as f:
            f.write(np.array(prob.shape, dtype=np.int64).tobytes())
            f.write(np.ascontiguousarray(prob, dtype=np.float64).tobytes())
        r = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])   # the sanitizers report on stderr
        return np.fromfile(dst, dtype=np.float64).reshape(prob.shape[0], prob.shape[1] + 1)

    return out, run


@pytest.mark.parametrize("C", [0, 1, 2, 987])
def test_topn_rows_equal_the_reference_loop_byte_for_byte(programs, C):
    (plain, san), run = programs
    prob = awkward_rows(C, seed=C + 1)
    want = python_topn(prob)
    assert np.all(want[:, 0] == 0.0) and not np.signbit(want[:, 0]).any()
    if C == 987:
        assert np.isinf(want[2, 1:]).all() and len(np.unique(prob[0])) < C // 2 and (want[3, 2:] < want[3, 1:-1]).all()
    for exe in (plain, san):
        got = run(exe, prob)
        assert got.tobytes() == want.tobytes(), (C, exe)


def test_no_rows(programs):
    (plain, san), run = programs
    for exe in (plain, san):
        assert run(exe, np.zeros((0, 5))).size == 0

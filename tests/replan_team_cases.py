"""Cases of the team fold (csrc/replan_teams.h), shared by tests/test_replan_teams_host.py (the header on the host, under the
sanitizers) and tests/test_gpu_replan_teams.py (replan_team_kernel through its probe entry).  A case: labels [n] (int32) and
keep [n] (Python ints below 2**64).  The expected outcome comes from rrt_dubins.team_fold / team_csr, the definition."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from auv_sim_amd.rrt_dubins import team_csr, team_fold  # noqa: E402

ALL = (1 << 64) - 1


def case(labels, keep, name=""):
    labels = np.array(labels, dtype=np.int32).reshape(-1)
    keep = [int(k) for k in keep]
    assert len(labels) == len(keep) and all(0 <= k <= ALL for k in keep)
    return dict(labels=labels, keep=keep, name=name)


def expected(c):
    """(team_off, members, folded keep) by the Python definition"""
    off, mem = team_csr(c["labels"])
    return off, mem, team_fold(c["keep"], c["labels"])


def crafted():
    b63 = 1 << 63
    return [
        case([0], [0x3ff], "n = 1"),
        case([-1], [5], "n = 1, negative"),
        case([-1, -5, -1, -2 ** 31], [1, 2, 3, 4], "all labels negative"),
        case([3, 4, 3, -1], [0b110, 0b001, 0b011, 0b111], "a team of one next to a team of two"),
        case([9], [ALL], "a team of one alone"),
        case([7, 1000000, 0, 7, 1000000, 0, 0, 7], [0xff, 0xf0f, 0x33, 0x3c, 0xff0, ALL, 0x31, 0x7e], "labels 7, 1000000, 0 interleaved"),
        case([2 ** 31 - 1, 0, 2 ** 31 - 1, 0], [6, 5, 3, 12], "the largest label"),
        case([1, 1, 1], [ALL, 0, ALL], "a mask of 0 empties the team"),
        case([1, 1, 1, 2, 2], [ALL, ALL, ALL, 0, 0], "masks 2**64 - 1 and 0"),
        case([4, 4], [ALL, ALL], "all ones stay all ones"),
        case([5, 5, 5], [ALL, ALL & ~b63, ALL], "bit 63 leaves"),
        case([5, -1, 5], [b63 | 1, 0, b63 | 2], "bit 63 stays"),
        case([0, 1, 0, 1, -1], [b63, 1 << 32, b63 | (1 << 31), (1 << 32) | (1 << 33), 77], "bits 31, 32, 33 and 63: both halves of the word"),
        case([6, 6, 6, 6], [0x3ff, 0x3fe, 0x3fd, 0x3fb], "every member lacks a bit of its own"),
        case([1, 1], [0xa, 0x5], "disjoint lists"),
    ]


def random_cases(n, seed=20240611, max_n=200):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        m = int(rng.integers(1, max_n + 1)) if k % 7 else int(rng.integers(1, 4))
        kinds = int(rng.integers(1, 9))
        pool = rng.choice(np.array([-3, -1, 0, 1, 2, 5, 64, 1000000, 2 ** 31 - 1, 12345, 7, 99]), size=kinds)
        labels = rng.choice(pool, size=m)
        dense = k % 3  # 0: random words, 1: mostly ones (single bits missing), 2: mostly zeros
        words = rng.integers(0, 1 << 63, size=m, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=m, dtype=np.uint64)
        keep = []
        for w in words:
            w = int(w)
            if dense == 1:
                w = ALL & ~(1 << (w % 64)) if w % 5 else ALL
            elif dense == 2:
                w = (1 << (w % 64)) | (1 << ((w >> 8) % 64))
            keep.append(w)
        out.append(case(labels, keep, "random %d" % k))
    return out


# ---- the host program's files (tests/host/replan_team_check.cpp) ---------------------------------------------------------

def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for c in cases:
            f.write(np.int32(len(c["labels"])).tobytes())
            f.write(c["labels"].astype("<i4").tobytes())
            f.write(np.array(c["keep"], dtype="<u8").tobytes())


def read_results(path, cases):
    """[(team_off, members, keep)]"""
    buf = open(path, "rb").read()
    at, out = 0, []
    for c in cases:
        nt, nm = np.frombuffer(buf, "<i4", 2, at)
        at += 8
        off = np.frombuffer(buf, "<i4", int(nt) + 1, at)
        at += 4 * (int(nt) + 1)
        mem = np.frombuffer(buf, "<i4", int(nm), at)
        at += 4 * int(nm)
        keep = np.frombuffer(buf, "<u8", len(c["labels"]), at)
        at += 8 * len(c["labels"])
        out.append((off, mem, [int(k) for k in keep]))
    assert at == len(buf)
    return out

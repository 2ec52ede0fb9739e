"""Cases of the replanning commit rule (csrc/replan_commit.h), shared by tests/test_replan_commit_host.py (the header on the
host, under the sanitizers) and tests/test_gpu_replan_commit.py (rrt_commit_kernel through the probe entry).  A case: course
[L,7] as rrt_final_course writes it, last [7], keep (a Python int over the habitat table hab [H,3]) and round_span.  The
expected outcome comes from rrt_dubins.first_bucket_commit, the definition of the rule."""
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from auv_sim_amd.rrt_dubins import first_bucket_commit  # noqa: E402

LENGTHS = (1, 2, 63, 64, 65, 129, 300)
NAN, INF = float("nan"), float("inf")


def case(course, last, keep, span, hab, name=""):
    return dict(course=np.ascontiguousarray(course, dtype=np.float64).reshape(-1, 7), last=np.array(last, dtype=np.float64).reshape(7),
                keep=int(keep), span=float(span), hab=np.ascontiguousarray(hab, dtype=np.float64).reshape(-1, 3), name=name)


def expected(c):
    """(sel [L] bool, committed rows [n,7], new keep, new last) by the Python definition: row 0 is the committed state"""
    p = c["course"].copy()
    if len(p) == 0:
        return np.zeros(0, bool), p, c["keep"], c["last"].copy()
    p[0] = c["last"]
    sel, keep = first_bucket_commit(p[:, 4], p[:, :2], float(c["last"][4]), 1.0e300, c["span"], c["keep"], c["hab"])
    rows = p[sel]
    return sel, rows, int(keep), (rows[-1].copy() if len(rows) else c["last"].copy())


def line_course(L, t0, dt, x0=500.0, y0=500.0, step=0.0):
    """L rows on a line from (x0, y0), times t0 + i * dt; the course's own row 0 has v = 0 and the start's time"""
    i = np.arange(L, dtype=np.float64)
    c = np.zeros((L, 7))
    c[:, 0], c[:, 1] = x0 + step * i, y0 + 0.5 * step * i
    c[:, 2], c[:, 3] = 0.1 * i, 1.0
    c[:, 4], c[:, 5], c[:, 6] = t0 + dt * i, i, 2.0 * dt * i
    c[0, 3] = 0.0
    return c


def crafted():
    out = []
    t0, span = 12.5, 30.0
    lo, hi = t0 + 0 * span, t0 + (0 + 1) * span
    last = [500.0, 500.0, 0.3, 1.5, t0, 7.0, 40.0]
    far = [[0.0, 0.0, 3.0], [50.0, 0.0, 4.0]]
    # the lengths around the wavefront's 64 rows: a first bucket that ends inside the course (dt 0.37: 82 rows fit), habitats on it
    for L in LENGTHS:
        c = line_course(L, t0, 0.37, step=0.25)
        hab = [[500.0 + 0.25 * k, 500.0 + 0.125 * k, 0.2] for k in (0, 5, 62, 63, 64, 80, 81, 82, 128, 299)]
        out.append(case(c, last, (1 << len(hab)) - 1, span, hab, "length %d" % L))
        out.append(case(line_course(L, t0, 0.01), last, 3, span, far, "length %d, all selected" % L))
    # the bucket's edges
    c = line_course(8, t0, 1.0)
    c[1:, 4] = [lo, hi, math.nextafter(hi, INF), NAN, t0 - 1.0, t0 + 3.0, math.nextafter(lo, -INF)]
    out.append(case(c, last, 3, span, far, "edges: lo, hi, above hi, nan, below lo, a selected row after unselected ones"))
    for k, t in enumerate((lo, hi, math.nextafter(hi, INF), NAN)):
        c = line_course(3, t0, 1.0)
        c[1, 4] = t
        out.append(case(c, last, 3, span, far, "edge %d alone" % k))
    c = line_course(70, t0, 1.0)
    c[1:, 4] += 1000.0
    out.append(case(c, last, 3, span, far, "only row 0 selected"))
    c = line_course(130, t0, 0.1)
    c[3::2, 4] = NAN  # every other row out: the committed rows are not contiguous
    out.append(case(c, last, 3, span, far, "alternating selection"))
    # row 0's substituted state lies inside a habitat, the course's own row 0 outside
    c = line_course(5, t0, 1.0, x0=900.0, y0=900.0)
    out.append(case(c, [100.0, 100.0, 0.0, 1.0, t0, 0.0, 0.0], 1, span, [[100.5, 100.0, 2.0]], "row 0 substituted"))
    # habitat counts: the last habitat of the table (bits 0, 32, 63) contains a point, the others none
    for H in (0, 1, 33, 64):
        hab = [[10.0 * h, -50.0, 1.0] for h in range(H)]
        c = line_course(4, t0, 1.0)
        if H:
            c[2, 0], c[2, 1] = hab[-1][0] + 0.5, hab[-1][1]
        out.append(case(c, last, (1 << H) - 1, span, hab, "H = %d" % H))
    hab = [[10.0 * h, -50.0, 1.0] for h in range(64)]
    c = line_course(4, t0, 1.0)
    c[1, 0], c[1, 1], c[2, 0], c[2, 1] = 320.0, -50.0, 630.0, -50.0
    out.append(case(c, last, (1 << 64) - 1, span, hab, "bits 32 and 63"))
    out.append(case(c, last, 0, span, hab, "keep == 0"))
    # exactly on the radius: offset (3, 4), size 5
    c = line_course(3, t0, 1.0)
    c[1, 0], c[1, 1] = 13.0, 24.0
    out.append(case(c, last, 1, span, [[10.0, 20.0, 5.0]], "on the radius"))
    # two overlapping kept habitats and one far away: the lower index goes first, then the higher
    c = line_course(4, t0, 1.0)
    c[1, 0], c[1, 1], c[2, 0], c[2, 1] = 0.5, 0.0, 0.6, 0.0
    out.append(case(c, last, 7, span, [[0.0, 0.0, 5.0], [1.0, 0.0, 5.0], [300.0, 300.0, 5.0]], "overlapping habitats"))
    # inside only a habitat whose bit is clear
    out.append(case(c, last, 4, span, [[0.0, 0.0, 5.0], [1.0, 0.0, 5.0], [300.0, 300.0, 5.0]], "inside a habitat that already left"))
    return out


def random_cases(n, seed=20240611):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        L, H = int(rng.integers(1, 301)), int(rng.integers(0, 65))
        hab = np.column_stack([rng.uniform(0, 100, H), rng.uniform(0, 100, H), rng.uniform(1, 15, H)]) if H else np.zeros((0, 3))
        t0, span = float(rng.uniform(0, 500)), float(rng.uniform(1, 120))
        c = np.zeros((L, 7))
        c[:, :2] = np.clip(np.cumsum(rng.normal(0, 2.5, (L, 2)), axis=0) + rng.uniform(10, 90, 2), -5, 105)
        c[:, 2], c[:, 3] = rng.uniform(-3, 3, L), rng.uniform(0, 2, L)
        c[:, 4] = t0 + np.cumsum(rng.uniform(0, 2.0 * span * rng.uniform(0.2, 3.0) / L, L))
        c[:, 5], c[:, 6] = rng.integers(0, 2000, L), np.cumsum(rng.uniform(0, 3, L))
        odd = rng.random(L) < 0.03
        c[odd, 4] = rng.choice([NAN, t0 - 1.0, t0, t0 + span, math.nextafter(t0 + span, INF), INF], int(odd.sum()))
        keep = 0 if rng.random() < 0.05 else int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2 + int(rng.integers(0, 2))
        keep &= (1 << H) - 1
        last = [float(rng.uniform(0, 100)), float(rng.uniform(0, 100)), float(rng.uniform(-3, 3)), float(rng.uniform(0, 2)), t0,
                float(rng.integers(0, 2000)), float(rng.uniform(0, 900))]
        out.append(case(c, last, keep, span, hab, "random %d" % k))
    return out


def write_cases(path, cases):
    """the input format of tests/host/replan_commit_check.cpp"""
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], dtype=np.int32).tobytes())
        for c in cases:
            f.write(np.array([len(c["course"]), len(c["hab"])], dtype=np.int32).tobytes())
            f.write(np.array([c["keep"]], dtype=np.uint64).tobytes())
            f.write(np.array([c["span"]], dtype=np.float64).tobytes())
            f.write(c["last"].tobytes() + c["hab"].tobytes() + c["course"].tobytes())


def read_results(path, cases):
    """[(sel, rows, keep, last)] as the program wrote them"""
    raw = open(path, "rb").read()
    out, pos = [], 0
    for c in cases:
        L = len(c["course"])
        n = int(np.frombuffer(raw, np.int32, 2, pos)[0])
        keep = int(np.frombuffer(raw, np.uint64, 1, pos + 8)[0])
        last = np.frombuffer(raw, np.float64, 7, pos + 16)
        sel = np.frombuffer(raw, np.uint8, L, pos + 72).astype(bool)
        rows = np.frombuffer(raw, np.float64, 7 * n, pos + 72 + L).reshape(n, 7)
        pos += 72 + L + 56 * n
        out.append((sel, rows, keep, last))
    assert pos == len(raw)
    return out


def same(a, b):
    """exact equality of two float arrays, a NaN equal to a NaN (bit patterns are not compared: the rule copies values)"""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)

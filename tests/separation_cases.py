"""Cases of the winner selection of RRT.replanning_batch(team_separation=d) (csrc/replan_apart.h), shared by
tests/test_team_separation_host.py (the Python rule on hand-made tables, its invariants, the header on the host under the
sanitizers) and tests/test_gpu_team_separation.py (rrt_course_ticks_kernel and replan_team_pick_apart_kernel through their probe
entry).

A case is a case of tests/team_pick_cases.py (world, labels, keep, active, K, per candidate a course [L,3] of x, y, t with its
cost, leaf time and bins) plus d, tick and W.  Every case is judged twice: with the claims and without them.  The expected outcome
comes from rrt_dubins.course_ticks / team_pick_separated, the definition."""
import numpy as np

import team_pick_cases as pc
from auv_sim_amd.rrt_dubins import course_ticks, team_pick_separated

REPO = pc.REPO
FULL10 = 0x3ff


def sep_case(d, tick, W, *a, **kw):
    c = pc.case(*a, **kw)
    c.update(d=float(d), tick=float(tick), W=int(W))
    c["ticks"] = [course_ticks(p[:, 2], p[:, :2], c["tick"], c["W"]) for p in c["courses"]]
    return c


def candidates(c):
    """cands[g][k] as team_pick_separated takes them"""
    cands = pc.candidates(c)
    K = c["K"]
    for g, row in enumerate(cands):
        for k, x in enumerate(row):
            if x is not None:
                x["ticks"] = c["ticks"][g * K + k]
    return cands


def expected(c, claims):
    return team_pick_separated(c["labels"], c["keep"], c["active"], candidates(c), c["weights"], c["d"], claims)


def drift(rng, L, start, t0=0.0, step=2.0, dt=(0.3, 2.5)):
    """a course of L points that wanders off from `start` in steps of about `step` metres, one every dt seconds"""
    if L == 0:
        return np.zeros((0, 3))
    xy = np.asarray(start, dtype=np.float64) + np.concatenate([np.zeros((1, 2)), np.cumsum(rng.normal(0.0, step, size=(L - 1, 2)), axis=0)])
    t = t0 + np.concatenate([[0.0], np.cumsum(rng.uniform(dt[0], dt[1], size=L - 1))])
    return np.concatenate([xy, t[:, None]], axis=1)


def _fleet(seed, name, labels, K, lens, d=4.0, tick=1.0, W=64, active=None, keep=None, spread=1.0, t_spread=0.0, **kw):
    """every AUV of a team starts within `spread` metres of its team's point, at times t_spread apart; K drifting courses each"""
    rng = np.random.default_rng(seed)
    labels = list(labels)
    active = list(range(len(labels))) if active is None else list(active)
    keep = [FULL10] * len(labels) if keep is None else keep
    lens = list(lens)
    home = {}
    courses = []
    for g, a in enumerate(active):
        at = home.setdefault(int(labels[a]) if labels[a] >= 0 else -1 - a, rng.uniform([0.0, 0.0], [70.0, 10.0]))
        t0 = float(rng.uniform(0.0, t_spread)) if t_spread else 0.0
        for k in range(K):
            courses.append(drift(rng, lens[(g * K + k) % len(lens)], at + rng.uniform(-spread, spread, size=2), t0=t0))
    return sep_case(d, tick, W, "h10", labels, keep, active, K, courses, name, rng=rng, **kw)


def line(p0, p1, n, t0=0.0, dt=1.0):
    """n points from p0 to p1, one per dt"""
    p = np.linspace(np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64), n)
    return np.concatenate([p, (t0 + dt * np.arange(n))[:, None]], axis=1)


def crafted():
    out = []
    for W in (1, 63, 64, 65, 1024):
        out.append(_fleet(100 + W, "W = %d" % W, [0, 0, 0, -1], 3, [70, 90, 40], W=W, tick=0.0625 if W == 1024 else 1.0))
    for K in (1, 4, 65):
        out.append(_fleet(200 + K, "K = %d" % K, [7, 7, 7, -1], K, [30, 17, 45], W=40))
    sizes = [2, 3, 64, 65]
    labels = np.concatenate([np.full(s, 100 * k + 1, dtype=np.int32) for k, s in enumerate(sizes)] + [np.full(5, -1, dtype=np.int32), [9999]])
    labels = labels[np.random.default_rng(5).permutation(len(labels))]
    out.append(_fleet(301, "teams of 2, 3, 64 and 65 between loners and a team of one", labels, 2, [25, 18], W=30, spread=6.0))
    out.append(_fleet(302, "a member with no leaf in any tree", [0, 0, 0], 3, [30, 30, 30, 0, 0, 0, 30, 30, 30], W=40))
    out.append(_fleet(303, "a member absent from the round", [0, 0, 0, -1], 2, [30, 22], active=[3, 2, 0], W=40))
    out.append(_fleet(304, "rounds that start at different times", [0, 0, 0, 0], 3, [60, 50, 40], W=50, t_spread=20.0))
    # AUV 0 goes east along y = 0, one point per second.  AUV 1's trees, all from the same start:
    east = line([0, 0], [20, 0], 21)
    beside = line([0, 1], [20, 1], 21)           # a metre beside it all the way: 21 conflicts
    leaves = line([0, 1], [0, 41], 21)           # north at 2 m/s: ticks 0 and 1 within 4 m
    slow = line([0, 1], [0, 21], 21)             # north at 1 m/s: ticks 0, 1 and 2
    out.append(sep_case(4.0, 1.0, 32, "h10", [0, 0], [FULL10] * 2, [0, 1], 3, [east, east, east, beside, slow, leaves],
                        "every candidate conflicts: the fewest win", c2=[-1, -0.5, -0.2, -9.0, -5.0, -0.1]))
    far_a, far_b = line([40, 8], [60, 8], 21), line([40, -30], [60, -30], 21)
    out.append(sep_case(4.0, 1.0, 32, "h10", [0, 0], [FULL10] * 2, [0, 1], 3, [east, east, east, far_a, far_b, beside],
                        "equal n, different scores", c2=[-1, -0.5, -0.2, -0.3, -0.7, -9.0]))
    out.append(sep_case(4.0, 1.0, 32, "h10", [0, 0], [FULL10] * 2, [0, 1], 3, [east, east, east, beside, far_b, far_b],
                        "equal n, equal scores: the lowest tree wins", c2=[-1, -0.5, -0.2, -9.0, -0.7, -0.7]))
    out.append(sep_case(4.0, 1.0, 32, "h10", [0, 0], [FULL10] * 2, [0, 1], 3, [east, east, east, far_a, beside, slow],
                        "a NaN score with n = 0 must not win", c2=[-1, -0.5, -0.2, np.nan, -0.4, -0.3]))
    # claims and separation disagree: AUV 0 sits in habitat 0 (at the origin) -- claimed.  AUV 1's tree 0 visits habitat 1 beside
    # AUV 0's course, its tree 1 visits habitat 0 far from it in time: under the claims tree 0 scores better, but it conflicts
    hab = pc.WORLDS["h10"]["habitats"]
    stay0 = line(hab[0][:2], hab[0][:2], 12)
    near1 = np.concatenate([line(hab[0][:2] + [0.5, 0.5], hab[0][:2] + [0.5, 0.5], 6), line(hab[1][:2], hab[1][:2], 6, t0=6.0)])
    late0 = line([30.0, -40.0], [30.0, -40.0], 12)
    out.append(sep_case(3.0, 1.0, 32, "h10", [0, 0], [FULL10] * 2, [0, 1], 2, [stay0, stay0, near1, late0],
                        "claims and separation disagree: n decides", c2=[-1.0, -0.5, -0.5, -0.4]))
    out.append(sep_case(3.0, 1.0, 32, "h10", [0, 0], [FULL10] * 2, [0, 1], 2, [stay0, stay0, near1, late0],
                        "d so small that nothing conflicts", c2=[-1.0, -0.5, -0.5, -0.4]))
    out[-1]["d"] = 1e-9
    # times the rule has to be total for: an infinite and a NaN time, rows before row 0's tick, a non-monotone course
    odd = np.array([[0, 0, 5.0], [1, 0, 3.0], [2, 0, 7.5], [3, 0, np.nan], [4, 0, 6.2], [5, 0, np.inf], [6, 0, -np.inf], [7, 0, 9.0]])
    out.append(sep_case(4.0, 1.0, 16, "h10", [0, 0], [FULL10] * 2, [0, 1], 2, [odd, odd + [0, 1, 0], odd + [0, 2, 0], line([9, 9], [9, 9], 3, t0=5.0)],
                        "NaN, infinite and descending times", c2=[-1.0, -0.5, -0.5, -0.4], leaf_t=[9.0, 9.0, 9.0, 7.0]))
    return out


def random_cases(n, seed=20261020):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        m = int(rng.integers(2, 13))
        labels = rng.choice(np.array([-1, 0, 0, 0, 1, 1, 5]), size=m)
        K = int(rng.integers(1, 5))
        active = [int(a) for a in rng.permutation(m)[:int(rng.integers(1, m + 1))]]
        keep = [int(rng.integers(0, 1 << 10)) if i % 3 else FULL10 for _ in range(m)]
        lens = [int(rng.integers(1, 90)) if rng.uniform() < 0.9 else 0 for _ in range(len(active) * K)]
        W = int(rng.choice([1, 2, 7, 31, 64, 65, 100, 200]))
        tick = float(rng.choice([0.25, 0.5, 1.0, 1.0, 3.0]))
        out.append(_fleet(int(rng.integers(0, 1 << 30)), "random %d" % i, labels, K, lens, d=float(rng.uniform(0.5, 9.0)), tick=tick, W=W,
                          active=active, keep=keep, spread=float(rng.uniform(0.0, 5.0)), t_spread=float(rng.choice([0.0, 0.0, 10.0])),
                          bin_lo=[int(rng.integers(0, 3)) for _ in lens], bin_hi=[int(rng.integers(3, pc.T_BINS + 1)) for _ in lens]))
    return out


# ---- the host program's files (tests/host/replan_apart_check.cpp) ------------------------------------------------------------

def write_cases(path, cases_claims):
    """cases_claims: (case, claims) pairs.  int32 n; per pair: int32 H, T, n, G, K, W, claims, pad; double d, tick; habitats [H,3];
    bins [T,2]; labels [n] i32; keep [n] u64; active [G] i32; weights [3]; per candidate: int32 L, bin_lo, bin_hi, pad; cost [4],
    leaf_t; xyt [L,3]"""
    with open(path, "wb") as f:
        f.write(np.int32(len(cases_claims)).tobytes())
        for c, claims in cases_claims:
            w = pc.WORLDS[c["world"]]
            hab, bins = w["habitats"], w["bins"]
            f.write(np.array([len(hab), len(bins), len(c["labels"]), len(c["active"]), c["K"], c["W"], 1 if claims else 0, 0], dtype="<i4").tobytes())
            f.write(np.array([c["d"], c["tick"]], dtype="<f8").tobytes())
            f.write(hab.astype("<f8").tobytes())
            f.write(bins.astype("<f8").tobytes())
            f.write(c["labels"].astype("<i4").tobytes())
            f.write(np.array(c["keep"], dtype="<u8").tobytes())
            f.write(np.array(c["active"], dtype="<i4").tobytes())
            f.write(np.array(c["weights"], dtype="<f8").tobytes())
            for e, p in enumerate(c["courses"]):
                f.write(np.array([len(p), c["bin_lo"][e], c["bin_hi"][e], 0], dtype="<i4").tobytes())
                f.write(np.array(list(c["cost4"][e]) + [c["leaf_t"][e]], dtype="<f8").tobytes())
                f.write(p.astype("<f8").tobytes())


def read_results(path, cases_claims):
    """per pair: G records {int32 winner (-2: the AUV has no teammate, the program left it alone), pad; cost [4]; u64 claimed; int32
    conflicts, pad}; then every candidate's table: int32 s_lo, n; xy [n,2].  Returns [(records, tables)]"""
    buf = open(path, "rb").read()
    at, out = 0, []
    rec = np.dtype([("winner", "<i4"), ("pad", "<i4"), ("cost", "<f8", (4,)), ("claimed", "<u8"), ("conflicts", "<i4"), ("pad2", "<i4")])
    for c, _ in cases_claims:
        G = len(c["active"])
        r = np.frombuffer(buf, rec, G, at)
        at += rec.itemsize * G
        tables = []
        for _ in c["courses"]:
            s_lo, n = (int(x) for x in np.frombuffer(buf, "<i4", 2, at))
            at += 8
            tables.append((s_lo, np.frombuffer(buf, "<f8", 2 * n, at).reshape(n, 2)))
            at += 16 * n
        out.append((r, tables))
    assert at == len(buf)
    return out

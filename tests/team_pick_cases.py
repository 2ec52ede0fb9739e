"""Cases of the team-aware winner selection of RRT.replanning_batch(team_pick="claims") (csrc/replan_pick.h), shared by
tests/test_team_pick_host.py (the Python rule against the CPU checker, the header on the host under the sanitizers) and
tests/test_gpu_team_pick.py (rrt_course_words_kernel and replan_team_pick_kernel through their probe entry).

A world: habitats [H,3], shark bins [T,2], cells, prob.  A case: its world's name, labels [n], keep [n] (Python ints), active
(group g is AUV active[g]), K, and per candidate e = g*K + k: course [L,3] (x, y, t; L == 0: the tree has no leaf), cost4 (its
cost under the AUV's own list, so that a member that sees claimed == 0 must get exactly it), leaf_t, length, bin_lo / bin_hi;
weights [3].  The expected outcome comes from rrt_dubins.course_habitat_words / team_pick_claims, the definition."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from auv_sim_amd.rrt_dubins import course_habitat_words, rescore, team_pick_claims  # noqa: E402

ALL = (1 << 64) - 1
T_BINS = 6
W_DEFAULT = (-3.0, -3.0, -4.0)


def _grid_world(H, seed):
    """H habitats on a 10-unit grid, 8 per row, with radii 3 .. 7 (neighbours overlap); six bins of 50 s; a 2 x 2 cell grid"""
    rng = np.random.default_rng(seed)
    hab = np.array([[10.0 * (h % 8), 10.0 * (h // 8), float(rng.uniform(3.0, 7.0))] for h in range(H)], dtype=np.float64).reshape(-1, 3)
    bins = np.array([[50.0 * b, 50.0 * (b + 1)] for b in range(T_BINS)])
    cells = np.array([[-20.0, -20.0, 35.0, 35.0], [35.0, -20.0, 100.0, 35.0], [-20.0, 35.0, 35.0, 100.0], [35.0, 35.0, 100.0, 100.0]])
    prob = rng.uniform(0.0, 1.0, size=(T_BINS, 4))
    return dict(habitats=hab, bins=bins, cells=cells, prob=prob)


def worlds():
    w = {"h0": _grid_world(0, 1), "h1": _grid_world(1, 2), "h10": _grid_world(10, 3), "h63": _grid_world(63, 4), "h64": _grid_world(64, 5)}
    o = _grid_world(3, 6)
    o["habitats"] = np.array([[0.0, 0.0, 5.0], [3.0, 0.0, 5.0], [50.0, 50.0, 5.0]])
    w["overlap"] = o
    return w


WORLDS = worlds()


def walk(rng, L, H, t0=0.0, t1=290.0):
    """a random course of L points over the habitats' area, times ascending in [t0, t1]"""
    rows = max((H + 7) // 8, 1)
    x = rng.uniform(-6.0, 76.0, size=L)
    y = rng.uniform(-6.0, 10.0 * rows - 4.0, size=L)
    t = np.sort(rng.uniform(t0, t1, size=L)) if L else np.zeros(0)
    return np.stack([x, y, t], axis=1).reshape(-1, 3)


def through(points, t0=1.0, dt=1.0):
    """a course through the given (x, y) points, one per dt"""
    p = np.array(points, dtype=np.float64).reshape(-1, 2)
    return np.concatenate([p, (t0 + dt * np.arange(len(p)))[:, None]], axis=1)


def case(world, labels, keep, active, K, courses, name="", weights=W_DEFAULT, c2=None, leaf_t=None, bin_lo=None, bin_hi=None, rng=None):
    labels = np.array(labels, dtype=np.int32).reshape(-1)
    keep = [int(k) for k in keep]
    active = [int(a) for a in active]
    E = len(active) * K
    assert len(labels) == len(keep) and len(courses) == E and len(set(active)) == len(active)
    courses = [np.array(c, dtype=np.float64).reshape(-1, 3) for c in courses]
    rng = rng or np.random.default_rng(len(name) + E)
    c2 = [float(rng.uniform(-2.0, 0.0)) for _ in range(E)] if c2 is None else [float(x) for x in c2]
    leaf_t = [float(c[-1, 2]) if len(c) else 0.0 for c in courses] if leaf_t is None else [float(x) for x in leaf_t]
    bin_lo = [0] * E if bin_lo is None else [int(b) for b in bin_lo]
    bin_hi = [T_BINS] * E if bin_hi is None else [int(b) for b in bin_hi]
    c = dict(world=world, labels=labels, keep=keep, active=active, K=K, courses=courses, leaf_t=leaf_t, bin_lo=bin_lo, bin_hi=bin_hi,
             length=[float(len(x)) * 0.5 + e for e, x in enumerate(courses)], weights=[float(x) for x in weights], name=name)
    # the cost the leaf pass would report: under the AUV's own list
    c["words"] = words_of(c)
    c["cost4"] = [rescore(c["words"][e], keep[active[e // K]], c2[e], leaf_t[e], c["weights"])[0] if len(courses[e]) else [np.inf] * 4
                  for e in range(E)]
    return c


def words_of(c):
    w = WORLDS[c["world"]]
    return [course_habitat_words(p[:, :2], p[:, 2], w["bins"], lo, hi, w["habitats"])
            for p, lo, hi in zip(c["courses"], c["bin_lo"], c["bin_hi"])]


def candidates(c):
    """cands[g][k] as team_pick_claims takes them"""
    K = c["K"]
    return [[dict(words=c["words"][g * K + k], cost=c["cost4"][g * K + k], leaf_time=c["leaf_t"][g * K + k])
             if len(c["courses"][g * K + k]) else None for k in range(K)] for g in range(len(c["active"]))]


def expected(c):
    return team_pick_claims(c["labels"], c["keep"], c["active"], candidates(c), c["weights"])


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _simple(world, H, K, lens, seed, name, labels=(0, 0), keep=None, active=None, **kw):
    rng = np.random.default_rng(seed)
    labels = list(labels)
    active = list(range(len(labels))) if active is None else active
    keep = [(1 << H) - 1] * len(labels) if keep is None else keep
    lens = list(lens)
    courses = [walk(rng, lens[(g * K + k) % len(lens)], H) for g in range(len(active)) for k in range(K)]
    return case(world, labels, keep, active, K, courses, name, rng=rng, **kw)


def crafted():
    out = []
    for wn, H in (("h0", 0), ("h1", 1), ("h63", 63), ("h64", 64)):
        out.append(_simple(wn, H, 2, [40, 25, 33], 10 + H, "H = %d" % H, labels=[2, 2, -1, 2]))
    c63 = WORLDS["h64"]["habitats"][63]
    c5 = WORLDS["h64"]["habitats"][5]
    to63, to5 = through([c63[:2]] * 3), through([c5[:2]] * 2)
    far = through([[500.0, 500.0]] * 4)
    out.append(case("h64", [1, 1], [ALL, ALL], [0, 1], 2, [to63, far, to63, to5], "bit 63 claimed", c2=[0, 0, -0.01, 0]))
    out.append(case("h64", [1, 1], [ALL, ALL], [0, 1], 2, [to5, far, to63, to5], "bit 63 not claimed", c2=[0, 0, -0.01, 0]))
    c3 = WORLDS["h10"]["habitats"][3]
    to3 = through([c3[:2]] * 5)
    out.append(case("h10", [4, 4], [0x3ff, 1 << 3], [0, 1], 2, [to3, to3, to3, through([[300.0, 0.0]] * 2)],
                    "claimed empties the member's mask: H' == 0", c2=[-1, -0.5, -0.25, -0.125]))
    out.append(_simple("h10", 10, 5, [1, 63, 64, 65, 200], 21, "course lengths 1, 63, 64, 65, 200", labels=[0, 0, 0]))
    for K in (1, 2, 3, 64, 65):
        out.append(_simple("h10", 10, K, [9, 17, 5], 30 + K, "K = %d" % K, labels=[7, 7, 7, -1]))
    sizes = [2, 3, 64, 65]
    labels = np.concatenate([np.full(s, 100 * k + 1, dtype=np.int32) for k, s in enumerate(sizes)] + [np.full(5, -1, dtype=np.int32), [9999]])
    labels = labels[np.random.default_rng(5).permutation(len(labels))]
    out.append(_simple("h63", 63, 2, [12, 7], 41, "teams of 2, 3, 64 and 65 between loners and a team of one", labels=labels,
                       keep=[((1 << 63) - 1) & ~(1 << (i % 63)) for i in range(len(labels))]))
    out.append(_simple("h10", 10, 3, [14, 14, 14, 0, 0, 0, 20, 20, 20], 51, "a member with no leaf in any tree", labels=[0, 0, 0]))
    out.append(_simple("h10", 10, 2, [0], 54, "no tree of the round has a leaf", labels=[0, 0, -1]))
    out.append(_simple("h10", 10, 2, [30, 20], 52, "a member absent from the round", labels=[0, 0, 0, -1], active=[3, 2, 0]))
    rng = np.random.default_rng(53)
    a, b, c = walk(rng, 30, 10), walk(rng, 30, 10), walk(rng, 30, 10)
    out.append(case("h10", [0, 0], [0x3ff, 0x3ff], [0, 1], 3, [a, b, c, c, b, b], "equal scores: the lower tree wins",
                    c2=[-0.3, -0.2, -0.1, -5.0, -9.0, -9.0]))
    out.append(case("h10", [0, 0], [0x3ff, 0x3ff], [0, 1], 3, [a, b, c, a, b, c], "a NaN c2", c2=[np.nan, -0.2, -0.1, -0.5, np.nan, -0.4]))
    out.append(case("h10", [0, 0], [0x3ff, 0x3ff], [0, 1], 2, [a, b, a, b], "every c2 a NaN", c2=[np.nan] * 4))
    # AUV 0 visits habitat 0 alone; AUV 1's points lie inside habitats 0 and 1: with 0 claimed the hits move to habitat 1
    out.append(case("overlap", [0, 0], [7, 7], [0, 1], 2,
                    [through([[-3.0, 0.0]] * 2), through([[90.0, 90.0]]), through([[1.5, 0.0]] * 4), through([[50.0, 50.0]] * 3)],
                    "inside two habitats, the lower one claimed", c2=[0, 0, 0, 0]))
    # the points of candidate 2 lie inside habitat 0, but at times of bin 0, which is not one of its selected bins 1 .. 2
    out.append(case("overlap", [0, 0], [7, 7], [0, 1], 2,
                    [through([[50.0, 50.0]] * 2, t0=60.0), through([[90.0, 90.0]]), through([[0.0, 0.0]] * 4, t0=5.0), through([[3.0, 0.0]] * 3, t0=70.0)],
                    "inside a habitat, in no selected bin", c2=[0, 0, 0, 0], bin_lo=[1] * 4, bin_hi=[3] * 4))
    many = through([WORLDS["h10"]["habitats"][2][:2]] * 10 + [WORLDS["h10"]["habitats"][6][:2]])  # (eleven hits)
    few = through([WORLDS["h10"]["habitats"][2][:2]] * 4)
    out.append(case("h10", [0, 0], [0x3ff, 0x3ff], [0, 1], 2, [few, many, many, few], "w2 = -0.1: repeated addition, not the product",
                    weights=(-3.0, -0.1, -4.0), leaf_t=[1.0] * 4, c2=[0, 0, 0, 0]))
    out.append(case("h10", [0, 0], [0x3ff, 0x3ff], [0, 1], 2, [few, many, many, few], "w2 = -0.0", weights=(-3.0, -0.0, -4.0), c2=[0, 0, -0.0, 0]))
    zero = through([WORLDS["h10"]["habitats"][2][:2]] * 6, t0=0.0, dt=0.0)
    out.append(case("h10", [0, 0], [0x3ff, 0x3ff], [0, 1], 2, [zero, few, zero, few], "a leaf time of 0", leaf_t=[0.0, 4.0, 0.0, 4.0]))
    return out


def random_cases(n, seed=20241020):
    rng = np.random.default_rng(seed)
    names = ["h10", "h10", "h63", "h64", "overlap", "h1"]
    out = []
    for i in range(n):
        wn = names[int(rng.integers(0, len(names)))]
        H = len(WORLDS[wn]["habitats"])
        m = int(rng.integers(1, 13))
        labels = rng.choice(np.array([-1, 0, 0, 1, 1, 5, 7]), size=m)
        K = int(rng.integers(1, 5))
        active = [int(a) for a in rng.permutation(m)[:int(rng.integers(1, m + 1))]]
        full = (1 << H) - 1
        keep = [(int(rng.integers(0, 1 << 62)) | (int(rng.integers(0, 4)) << 62)) & full if i % 3 else full for _ in range(m)]
        lens = [int(rng.integers(0, 90)) if rng.uniform() < 0.9 else 0 for _ in range(len(active) * K)]
        courses = [walk(rng, L, H, t0=float(rng.uniform(0, 100)), t1=float(rng.uniform(100, 320))) for L in lens]
        lo = [int(rng.integers(0, 3)) for _ in lens]
        hi = [int(rng.integers(3, T_BINS + 1)) for _ in lens]
        w = (-3.0, -3.0, -4.0) if i % 4 else (float(rng.uniform(-3, 3)), float(rng.uniform(-1, 1)), -4.0)
        out.append(case(wn, labels, keep, active, K, courses, "random %d" % i, weights=w, bin_lo=lo, bin_hi=hi, rng=rng))
    return out


# ---- the host program's files (tests/host/replan_pick_check.cpp) -------------------------------------------------------------

def write_cases(path, cases):
    """int32 n_cases; per case: int32 H, T, n, G, K; habitats [H,3] (the program computes the squared thresholds itself); bins [T,2];
    labels [n] i32; keep [n] u64; active [G] i32; weights [3]; per candidate: int32 L, bin_lo, bin_hi, pad; c2, leaf_t; xyt [L,3]"""
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for c in cases:
            w = WORLDS[c["world"]]
            hab, bins = w["habitats"], w["bins"]
            f.write(np.array([len(hab), len(bins), len(c["labels"]), len(c["active"]), c["K"]], dtype="<i4").tobytes())
            f.write(hab.astype("<f8").tobytes())
            f.write(bins.astype("<f8").tobytes())
            f.write(c["labels"].astype("<i4").tobytes())
            f.write(np.array(c["keep"], dtype="<u8").tobytes())
            f.write(np.array(c["active"], dtype="<i4").tobytes())
            f.write(np.array(c["weights"], dtype="<f8").tobytes())
            for e, p in enumerate(c["courses"]):
                f.write(np.array([len(p), c["bin_lo"][e], c["bin_hi"][e], 0], dtype="<i4").tobytes())
                f.write(np.array([c["cost4"][e][3], c["leaf_t"][e]], dtype="<f8").tobytes())
                f.write(p.astype("<f8").tobytes())


def read_results(path, cases):
    """per case: per team member's group in `active` order: int32 winner, pad; cost [4]; u64 claimed; then the words of every
    candidate.  Returns [(winners [G], costs [G,4], claimed [G], words per candidate)]; a group the program did not touch (an AUV
    without a teammate) has winner -2"""
    buf = open(path, "rb").read()
    at, out = 0, []
    rec = np.dtype([("winner", "<i4"), ("pad", "<i4"), ("cost", "<f8", (4,)), ("claimed", "<u8")])
    for c in cases:
        G = len(c["active"])
        r = np.frombuffer(buf, rec, G, at)
        at += rec.itemsize * G
        words = []
        for p in c["courses"]:
            words.append([int(x) for x in np.frombuffer(buf, "<u8", len(p), at)])
            at += 8 * len(p)
        out.append((r["winner"].tolist(), r["cost"].copy(), [int(x) for x in r["claimed"]], words))
    assert at == len(buf)
    return out

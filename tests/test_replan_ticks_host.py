"""k measurements per round along the last committed bucket, without a GPU: csrc/replan_ticks.h (the pure header
replan_measure_ticks_kernel is built from) compiled into tests/host/replan_ticks_check.cpp with g++ -ffp-contract=off, plain and
under the address / undefined-behaviour sanitizers, against the rule restated here -- tick times and chosen rows bit for bit --
and against tracking.tick_times / tick_row, the pieces of the definition tracking.fleet_measurements_ticks.  And
replan_ticks_plan, the host's index checks: the segments of the last commit only, nothing outside the log."""
import math
import os
import shutil
import struct
import subprocess

import pytest

from auv_sim_amd.tracking import tick_row, tick_times

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
KS = (1, 2, 3, 7, 64)
# spans whose k-th part, taken k times, is not the span: the pair must be found again by the test below
UNEVEN = ((97.7, 3), (126.2, 3), (125.3, 7), (100.0, 11))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or _bits(a) == _bits(b)


def rule(times, k, span):
    """the rule of the issue, restated: [(tau_j, row_j)]; row -1 where the segment is empty"""
    if not times:
        return [(0.0, -1)] * k
    lo = times[0]
    out = []
    for j in range(k):
        tau = lo + 1.0 * span if j == k - 1 else lo + (j + 1) * (span / k)
        best = 0
        for i, t in enumerate(times):
            if t <= tau:  # (a NaN on either side: False)
                best = i
        out.append((tau, best))
    return out


def tick_cases():
    """(name, times, k, span)"""
    cases = []
    for k in KS:
        step = 100.0 / k
        cases.append(("ascending, k = %d" % k, [150.0 + 0.37 * i for i in range(300)], k, 100.0))
        cases.append(("n = 0, k = %d" % k, [], k, 100.0))
        cases.append(("n = 1, k = %d" % k, [150.0], k, 100.0))
        cases.append(("65 rows, k = %d" % k, [7.0 + 1.5 * i for i in range(65)], k, 96.0))
        if k > 1:
            # a row whose time IS tick 0's, then one a hair later
            t0 = 150.0 + 1 * step
            cases.append(("a tick equal to a row's time, k = %d" % k, [150.0, 150.0 + 0.5 * step, t0, math.nextafter(t0, math.inf), 260.0], k, 100.0))
    for span, k in UNEVEN:
        cases.append(("k * (span / k) != span: %r / %d" % (span, k), [0.0] + [span * i / 50.0 for i in range(1, 50)] + [0.0 + 1.0 * span], k, span))
        cases.append(("... from lo = 150: %r / %d" % (span, k), [150.0, 150.0 + 0.5 * span, 150.0 + 1.0 * span], k, span))
    cases.append(("two rows with equal times", [10.0, 20.0, 20.0, 20.0, 90.0], 4, 40.0))
    cases.append(("non-ascending times", [10.0, 45.0, 12.0, 30.0, 11.0, 50.0, 40.0], 7, 35.0))
    cases.append(("every later row below lo", [10.0, 5.0, 4.0, 3.0], 3, 30.0))
    cases.append(("a NaN time in the middle", [10.0, 15.0, NAN, 25.0, 40.0], 3, 30.0))
    cases.append(("a NaN time at the end", [10.0, 15.0, NAN], 2, 30.0))
    cases.append(("a NaN lo", [NAN, 15.0, 20.0, 25.0], 3, 30.0))
    cases.append(("no row qualifies but row 0 is not below either", [10.0, 500.0, 600.0], 2, 30.0))
    cases.append(("130 rows, the winner in the last chunk", [1.0 * i for i in range(130)], 64, 129.0))
    return cases


def plan_cases():
    """(name, pieces [(auv, n, src, round)], last_round, n_auvs, members, log_rows, k, expected (status, bad, [(off, n)]))"""
    OK, BAD_K, BAD_MEMBER, BAD_PIECE = 0, 1, 2, 3
    two_rounds = [(0, 30, 0, 0), (1, 40, 100, 0), (2, 10, 200, 0), (0, 25, 300, 1), (2, 5, 400, 1)]
    return [
        ("no commit yet", [], -1, 3, [2, 0, 1], 0, 3, (OK, -1, [(0, 0)] * 3)),
        ("the last round's pieces only; AUV 1 took no part in it", two_rounds, 1, 3, [2, 0, 1], 500, 3,
         (OK, -1, [(400, 5), (300, 25), (0, 0)])),
        ("the round before, had it been the last", two_rounds[:3], 0, 3, [0, 1, 2], 300, 1, (OK, -1, [(0, 30), (100, 40), (200, 10)])),
        ("a piece that ends exactly at the log's end", two_rounds, 1, 3, [0, 1, 2], 405, 64, (OK, -1, [(300, 25), (0, 0), (400, 5)])),
        ("a segment reaching past the log", two_rounds, 1, 3, [0, 1, 2], 404, 3, (BAD_PIECE, 4, [])),
        ("a segment that starts past the log", two_rounds, 1, 3, [0, 1, 2], 310, 3, (BAD_PIECE, 4, [])),
        ("an older piece past the log is nobody's business", [(0, 30, 10 ** 12, 0), (0, 5, 0, 1)], 1, 1, [0], 5, 2, (OK, -1, [(0, 5)])),
        ("a negative offset", [(0, 5, -1, 0)], 0, 1, [0], 100, 2, (BAD_PIECE, 0, [])),
        ("an empty piece", [(0, 0, 3, 0)], 0, 1, [0], 100, 2, (BAD_PIECE, 0, [])),
        ("a piece of an AUV outside the fleet", [(3, 5, 0, 0)], 0, 3, [0, 1, 2], 100, 2, (BAD_PIECE, 0, [])),
        ("an AUV's second piece of the round", [(1, 5, 0, 0), (1, 5, 5, 0)], 0, 3, [0, 1, 2], 100, 2, (BAD_PIECE, 0, [])),
        ("an offset beyond 2^31 rows", [(0, 7, 2 ** 33, 0)], 0, 1, [0], 2 ** 33 + 7, 2, (OK, -1, [(2 ** 33, 7)])),
        ("a member outside the fleet", two_rounds, 1, 3, [0, 3, 1], 500, 3, (BAD_MEMBER, 1, [])),
        ("a negative member", two_rounds, 1, 3, [-1, 0, 1], 500, 3, (BAD_MEMBER, 0, [])),
        ("k = 0", two_rounds, 1, 3, [0, 1, 2], 500, 0, (BAD_K, -1, [])),
        ("k = 65", two_rounds, 1, 3, [0, 1, 2], 500, 65, (BAD_K, -1, [])),
        ("k = -1", two_rounds, 1, 3, [0, 1, 2], 500, -1, (BAD_K, -1, [])),
    ]


def _write(path, ticks, plans):
    with open(path, "w") as f:
        for _, times, k, span in ticks:
            f.write("ticks %d %d %s\n" % (len(times), k, float(span).hex()))
            for i, t in enumerate(times):  # (the other six fields: values the rule must not read as times)
                f.write(" ".join(float(v).hex() for v in (1e3 + i, -1e3 - i, 0.25 * i, 2.0, t, -5.0, 1e6)) + "\n")
        for _, pieces, last_round, n_auvs, members, log_rows, k, _ in plans:
            f.write("plan %d %d %d %d %d %d\n" % (len(pieces), last_round, n_auvs, len(members), log_rows, k))
            for p in pieces:
                f.write("%d %d %d %d\n" % p)
            f.write(" ".join("%d" % m for m in members) + "\n")


def _read(text, ticks, plans):
    words = text.split()
    at = [0]

    def take():
        at[0] += 1
        return words[at[0] - 1]

    got_t, got_p = [], []
    for _ in ticks:
        assert take() == "ticks"
        k = int(take())
        got_t.append([(float.fromhex(take()), int(take())) for _ in range(k)])
    for _ in plans:
        assert take() == "plan"
        status, bad, n = int(take()), int(take()), int(take())
        got_p.append((status, bad, [(int(take()), int(take())) for _ in range(n)]))
    assert at[0] == len(words)
    return got_t, got_p


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("replan_ticks")

    def build(name, flags):
        exe = str(d / name)
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"] + flags +
                       ["-I", os.path.join(REPO, "auv_sim_amd", "csrc"), "-o", exe, os.path.join(REPO, "tests", "host", "replan_ticks_check.cpp")],
                       check=True)
        return exe

    return d, build("replan_ticks_check", []), build("replan_ticks_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_the_uneven_spans_are_uneven():
    """the pairs used really have k * (span / k) != span, and the last tick is lo + 1.0 * span all the same"""
    for span, k in UNEVEN:
        assert k * (span / k) != span, (span, k)
        for lo in (0.0, 150.0):
            taus = tick_times(lo, span, k)
            assert _bits(taus[-1]) == _bits(lo + 1.0 * span)
            assert len(taus) == k and all(a < b for a, b in zip(taus, taus[1:]))
    # ... also where the sum with lo would still show it: the tick a plain (j + 1) * step would give is another double
    assert any(150.0 + k * (span / k) != 150.0 + 1.0 * span for span, k in UNEVEN)


def test_python_definition_equals_the_restated_rule():
    for name, times, k, span in tick_cases():
        want = rule(times, k, span)
        if not times:
            continue
        taus = tick_times(times[0], span, k)
        assert all(_same(a, b[0]) for a, b in zip(taus, want)), name
        assert [tick_row(times, t) for t in taus] == [w[1] for w in want], name


def test_cases_mean_what_they_say():
    by = {name: rule(times, k, span) for name, times, k, span in tick_cases()}
    assert [r for _, r in by["two rows with equal times"]] == [3, 3, 3, 3]                 # the greater index wins
    assert [r for _, r in by["non-ascending times"]] == [4, 4, 4, 4, 4, 6, 6]                 # ... a later row that is early counts
    assert [r for _, r in by["every later row below lo"]] == [3, 3, 3]
    assert [r for _, r in by["a NaN time in the middle"]] == [1, 3, 4]                        # the NaN row is never chosen
    assert [r for _, r in by["a NaN time at the end"]] == [1, 1]
    assert [r for _, r in by["a NaN lo"]] == [0, 0, 0] and all(math.isnan(t) for t, _ in by["a NaN lo"])
    assert [r for _, r in by["no row qualifies but row 0 is not below either"]] == [0, 0]
    assert [r for _, r in by["n = 0, k = 3"]] == [-1, -1, -1]
    assert [r for _, r in by["n = 1, k = 7"]] == [0] * 7
    assert by["a tick equal to a row's time, k = 2"][0][1] == 2                              # t == tau qualifies, the next double does not
    assert by["130 rows, the winner in the last chunk"][-1][1] == 129
    for k in KS:
        assert by["ascending, k = %d" % k][-1][1] == max(i for i in range(300) if 150.0 + 0.37 * i <= 250.0)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_header_reproduces_the_rule(programs, which):
    d, plain, san = programs
    ticks, plans = tick_cases(), plan_cases()
    assert {k for _, _, k, _ in ticks} >= set(KS)
    src = str(d / ("cases_%s.txt" % which))
    _write(src, ticks, plans)
    r = subprocess.run([plain if which == "plain" else san, src], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]  # the sanitizers report on stderr
    got_t, got_p = _read(r.stdout, ticks, plans)
    for (name, times, k, span), got in zip(ticks, got_t):
        want = rule(times, k, span)
        assert len(got) == k and [g[1] for g in got] == [w[1] for w in want], name
        assert all(_same(g[0], w[0]) for g, w in zip(got, want)), name
    for (name, *_, want), got in zip(plans, got_p):
        assert got == want, (name, got, want)

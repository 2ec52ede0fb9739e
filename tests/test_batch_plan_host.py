"""What a batch needs in HBM, worked out without a GPU: csrc/batch_plan.h (the pure host functions behind rrt_prepare_impl,
auvp_rrt_prepare_episodes, prrt_configure, the epoch tags and the random stream's buffer) compiled into
tests/host/batch_plan_check.cpp with g++ and the address / undefined-behaviour / float-cast-overflow sanitizers.

Every expectation is a literal worked out by hand from the formulas the host code had before they moved there:
  K = ceil(max_traj_time / bin_interval) in time-bin mode;  max_pts = floor(freq) + 2;  cap_nodes = max_iter + 1
  cap_points = ceil(points_per_iter max_iter), or ceil(min(max_iter max(floor(freq), 1), freq max_iter / 2 + 8 freq sqrt(max_iter / 12))),
               + floor(freq) + 64
  bin_cap = cap_nodes with time bins, else 1;  past 128 members per bin: bin_over = ceil(cap_nodes / 64) + K + 1 chunks and
  bin_slots = ceil((bin_cap - 128) / 64);  bin_stride = 128 (K + 1) + 64 bin_over + bin_slots (K + 1)
The inputs whose handling was undefined (a NaN horizon, an infinite freq, sizes past an int) go through the same program: the
sanitizers must stay silent and the plan must refuse them."""
import math
import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

INT_MAX = 2147483647
TIMEBIN, PLANTIME, NN = 0, 1, 2
LEAF_LOG, ITER_LOG, PHASE_CLOCKS = 2, 1, 4
# RrtBatchStatus / PrrtBatchStatus / RrtEpisodeRefusal, in the order of the checks
OK, BAD_ARGS, BAD_PARAMS, BIN_INTERVAL, OBSTACLES, FIELD, TOO_MANY_BINS, POINTS, BIN_LISTS = range(9)
P_OK, P_BAD_ARGS, P_OBSTACLES, P_BAD_PARAMS, P_FIELD, P_EMPTY_GRID, P_BUCKETS, P_POINTS, P_STEPS = range(9)
EP_OK, EP_HORIZON, EP_KEEP, EP_BINS = range(4)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    """ask(commands) -> one list of tokens per command, through the sanitized program"""
    d = tmp_path_factory.mktemp("batch_plan")
    exe = str(d / "batch_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "auv_sim_amd", "csrc"), "-o", exe,
                    os.path.join(REPO, "tests", "host", "batch_plan_check.cpp")], check=True)
    count = [0]

    def run(commands):
        count[0] += 1
        src = str(d / ("commands%d.txt" % count[0]))
        with open(src, "w") as f:
            f.write("\n".join(commands) + "\n")
        r = subprocess.run([exe, src], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])   # the sanitizers report on stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(commands)
        return [line.split() for line in lines]

    return run


def num(v):
    return v if isinstance(v, str) else (float(v).hex() if isinstance(v, float) and math.isfinite(v) else str(v))


RRT_FIELDS = ("status", "field", "K", "max_pts", "cap_nodes", "cap_points", "bin_cap", "bin_over", "bin_slots", "bin_stride", "cap_leaves",
              "xy_stride", "flags", "inv_bin_interval", "itlog_n")
RRT_BYTES = ("nodes_f", "nodes_i", "points", "bin_items", "bin_count", "summary", "node_c", "node_q", "node_xy", "itlog_i", "itlog_b", "leaf_c",
             "leaf_i", "leaf_stats", "phase", "mt")


def rrt_cmd(max_iter=10000, freq=30.0, max_traj_time=500.0, bin_interval=5.0, mode=TIMEBIN, E=3, points_per_iter=0.0, flags=0, O=64):
    return "rrt %d %d %s %s %s %d %s %d %d" % (E, max_iter, num(freq), num(max_traj_time), num(bin_interval), mode, num(points_per_iter), flags, O)


def rrt_plan(tokens):
    # (the field's name may hold blanks: it ends where the fixed number of fields behind it begins)
    n_tail = len(RRT_FIELDS) - 2 + len(RRT_BYTES)
    head, tail = tokens[:len(tokens) - n_tail], tokens[len(tokens) - n_tail:]
    out = {"status": int(head[0]), "field": " ".join(head[1:])}
    for k, v in zip(RRT_FIELDS[2:] + RRT_BYTES, tail):
        out[k] = float.fromhex(v) if k == "inv_bin_interval" else int(v)
    return out


def rrt(ask, **kw):
    return rrt_plan(ask([rrt_cmd(**kw)])[0])


# ---- RRT.exploring: plans worked out by hand ---------------------------------------------------------------------------------------

def test_rrt_time_bin_batch_with_chunked_member_lists(ask):
    p = rrt(ask, max_iter=10000)
    want = dict(status=OK, K=100, max_pts=32, cap_nodes=10001, cap_points=157023, bin_cap=10001, bin_over=258, bin_slots=155,
                bin_stride=45095, cap_leaves=1, xy_stride=0, flags=0, inv_bin_interval=1.0 / 5.0, itlog_n=0)
    assert {k: p[k] for k in want} == want
    E = 3
    assert {k: p[k] for k in RRT_BYTES} == dict(
        nodes_f=E * 10001 * 8 * 8, nodes_i=E * 10001 * 4 * 4, points=E * 157023 * 6 * 8, bin_items=E * 45095 * 4, bin_count=E * 101 * 4,
        summary=E * 104, node_c=E * 10001 * 8 * 4, node_q=E * 10001, node_xy=0, itlog_i=0, itlog_b=0, leaf_c=0, leaf_i=0, leaf_stats=64,
        phase=0, mt=E * 624 * 4)


def test_rrt_member_list_seam_at_the_direct_mapped_head(ask):
    # 128 members per bin are direct-mapped (AUVP_BIN_HEAD): 127 iterations need no chunk, 128 need the first
    p = rrt(ask, max_iter=127)
    assert (p["K"], p["cap_nodes"], p["cap_points"], p["bin_over"], p["bin_slots"], p["bin_stride"]) == (100, 128, 2780, 0, 0, 12928)
    p = rrt(ask, max_iter=128)
    assert (p["K"], p["cap_nodes"], p["cap_points"], p["bin_over"], p["bin_slots"], p["bin_stride"]) == (100, 129, 2798, 104, 1, 19685)


def test_rrt_points_per_iter_and_the_leaf_log(ask):
    p = rrt(ask, max_iter=1000, freq=0.5, max_traj_time=50.0, bin_interval=7.0, points_per_iter=1.5, flags=LEAF_LOG)
    assert (p["status"], p["K"], p["max_pts"], p["cap_points"], p["bin_over"], p["bin_slots"], p["bin_stride"], p["cap_leaves"]) == \
        (OK, 8, 2, 1564, 25, 14, 2878, 1001)
    assert (p["flags"], p["inv_bin_interval"]) == (LEAF_LOG, 1.0 / 7.0)
    assert (p["leaf_c"], p["leaf_i"]) == (3 * 1001 * 6 * 8, 3 * 1001 * 4)


def test_rrt_other_sampling_modes_have_no_bins(ask):
    p = rrt(ask, max_iter=513, freq=10.0, mode=NN)
    assert (p["status"], p["K"], p["max_pts"], p["cap_nodes"], p["cap_points"], p["bin_cap"], p["bin_stride"], p["xy_stride"]) == \
        (OK, 0, 12, 514, 3163, 1, 128, 1024)
    assert (p["node_xy"], p["bin_count"]) == (3 * 1024 * 2 * 8, 3 * 4)
    p = rrt(ask, max_iter=10, freq=1.0, mode=PLANTIME)
    assert (p["status"], p["K"], p["max_pts"], p["cap_points"], p["bin_stride"], p["xy_stride"], p["node_xy"]) == (OK, 0, 3, 75, 128, 0, 0)


def test_rrt_logs(ask):
    p = rrt(ask, max_iter=100, flags=ITER_LOG | PHASE_CLOCKS, E=7)
    assert (p["itlog_n"], p["itlog_i"], p["itlog_b"], p["phase"], p["leaf_c"]) == (700, 700 * 2 * 4, 700, 7 * 5 * 8, 0)


def test_rrt_limits(ask):
    p = rrt(ask, max_iter=100, max_traj_time=5242880.0, E=1)          # K = 1 << 20 exactly
    assert (p["status"], p["K"]) == (OK, 1 << 20)
    p = rrt(ask, max_iter=100, max_traj_time=5242881.0, E=1)
    assert (p["status"], p["K"]) == (TOO_MANY_BINS, (1 << 20) + 1)    # (the message prints this K)
    p = rrt(ask, max_iter=2000000, max_traj_time=5242880.0, E=1)
    assert (p["status"], p["K"]) == (BIN_LISTS, 1 << 20)
    p = rrt(ask, max_iter=1400000, max_traj_time=7500.0, E=1)
    assert (p["status"], p["K"], p["bin_stride"]) == (OK, 1500, 34521130)
    assert rrt(ask, points_per_iter=1.0e9)["status"] == POINTS
    assert rrt(ask, points_per_iter=math.inf)["status"] == POINTS
    assert rrt(ask, freq=2.0e9, max_iter=10)["status"] == POINTS      # (floor(freq) still fits an int)


def test_rrt_refusals_there_have_always_been(ask):
    for kw, status in ((dict(E=0), BAD_ARGS), (dict(max_iter=0), BAD_PARAMS), (dict(freq=math.nan), BAD_PARAMS), (dict(freq=-1.0), BAD_PARAMS),
                       (dict(mode=3), BAD_PARAMS), (dict(mode=-1), BAD_PARAMS), (dict(bin_interval=0.0), BIN_INTERVAL),
                       (dict(bin_interval=math.nan), BIN_INTERVAL), (dict(O=1025), OBSTACLES),
                       # ... in their order: the first that applies
                       (dict(E=0, max_iter=0), BAD_ARGS), (dict(max_iter=0, bin_interval=0.0, O=1025), BAD_PARAMS),
                       (dict(bin_interval=0.0, O=1025), BIN_INTERVAL), (dict(O=1025, max_traj_time=math.nan), OBSTACLES)):
        assert rrt(ask, **kw)["status"] == status, kw
    assert rrt(ask, O=1024)["status"] == OK
    assert rrt(ask, bin_interval=0.0, mode=NN)["status"] == OK and rrt(ask, bin_interval=0.0, mode=NN)["inv_bin_interval"] == 0.0


@pytest.mark.parametrize("kw, field", [
    (dict(max_traj_time=math.nan), "max_traj_time / bin_interval"),
    (dict(max_traj_time=math.inf), "max_traj_time / bin_interval"),
    (dict(max_traj_time=1.1e10), "max_traj_time / bin_interval"),      # 2.2e9 bins: past an int
    (dict(max_traj_time=-1.1e10), "max_traj_time / bin_interval"),
    (dict(max_traj_time=1.0, bin_interval=1e-300), "max_traj_time / bin_interval"),
    (dict(freq=math.inf), "freq"),
    (dict(freq=1e300), "freq"),
    (dict(freq=2147483648.0), "freq"),
    (dict(freq=float(INT_MAX - 63), max_iter=1), "freq"),              # floor(freq) + 64 would not fit
    (dict(max_iter=INT_MAX), "max_iter"),
    (dict(points_per_iter=math.nan), "points_per_iter"),
    (dict(E=INT_MAX, max_iter=1000000, freq=1000.0), "points"),      # 2^31 x 5e8 x 48 bytes
])
def test_rrt_inputs_that_were_undefined_are_refused(ask, kw, field):
    p = rrt(ask, **kw)
    assert (p["status"], p["field"]) == (FIELD, field)


def test_rrt_largest_defined_inputs_still_plan(ask):
    # (an int's worth of time bins is defined, and refused as ever; max_iter one below INT_MAX has no bins to overflow outside time-bin mode)
    p = rrt(ask, max_traj_time=1.0e10, E=1)
    assert (p["status"], p["K"]) == (TOO_MANY_BINS, 2000000000)
    p = rrt(ask, max_iter=INT_MAX - 1, freq=0.0, mode=PLANTIME, E=1)
    assert (p["status"], p["cap_nodes"], p["cap_points"], p["max_pts"]) == (OK, INT_MAX, 64, 2)


# ---- per-episode limits ------------------------------------------------------------------------------------------------------------

def limits(ask, cap, bin_interval, H, episodes):
    t = ask(["lim %s %s %d %d %s" % (num(cap), num(bin_interval), H, len(episodes), " ".join("%s %d" % (num(a), k) for a, k in episodes))])[0]
    rows = [(int(t[i]), int(t[i + 1]), float.fromhex(t[i + 2])) for i in range(2, len(t), 3)]
    return int(t[0]), int(t[1]), rows


def test_episode_limits(ask):
    # a horizon equal to the cap, a short one, one a thousandth of a bin long
    assert limits(ask, 500.0, 5.0, 10, [(500.0, 1023), (5.0, 1), (0.005, 0), (5.000001, 512)]) == \
        (-1, EP_OK, [(100, 1023, 500.0), (1, 1, 5.0), (1, 0, 0.005), (2, 512, 5.000001)])
    assert limits(ask, 500.0, 5.0, 10, [(500.0, 1), (500.0000001, 1)])[:2] == (1, EP_HORIZON)     # above the cap
    assert limits(ask, 500.0, 5.0, 10, [(0.0, 1), (-3.0, 1)])[:2] == (0, EP_HORIZON)
    assert limits(ask, 500.0, 5.0, 10, [(1.0, 1), (-3.0, 1)])[:2] == (1, EP_HORIZON)
    assert limits(ask, 500.0, 5.0, 10, [(math.nan, 1)])[:2] == (0, EP_HORIZON)
    assert limits(ask, 500.0, 5.0, 10, [(3.0, 1 << 9), (3.0, 1 << 10)])[:2] == (1, EP_KEEP)       # a bit at H
    assert limits(ask, 500.0, 5.0, 0, [(3.0, 0)])[:2] == (-1, EP_OK)
    assert limits(ask, 500.0, 5.0, 0, [(3.0, 1)])[:2] == (0, EP_KEEP)
    assert limits(ask, 500.0, 5.0, 64, [(3.0, (1 << 64) - 1)]) == (-1, EP_OK, [(1, (1 << 64) - 1, 3.0)])
    assert limits(ask, 500.0, 5.0, 63, [(3.0, 1 << 63)])[:2] == (0, EP_KEEP)
    # the horizon's checks come first, then the habitats', then the number of bins (undefined before: 3e9 bins)
    assert limits(ask, 500.0, 5.0, 10, [(600.0, 1 << 10)])[:2] == (0, EP_HORIZON)
    assert limits(ask, 3.0e10, 10.0, 10, [(3.0e10, 1)])[:2] == (0, EP_BINS)
    assert limits(ask, 3.0e10, 10.0, 10, [(2.0e10, 1)]) == (-1, EP_OK, [(2000000000, 1, 2.0e10)])


# ---- Planner_RRT ------------------------------------------------------------------------------------------------------------------

PRRT_FIELDS = ("rows", "cols", "n_buckets", "delta_theta", "cap_nodes", "max_pts", "cap_points")
PRRT_BYTES = ("nodes", "node_bucket", "points", "occupied", "buckets", "mt", "rng_state", "summary", "step_bucket", "start", "goal", "st_log")


def prrt(ask, rect=(0.0, 0.0, 100.0, 100.0), cell=10.0, subs=4, max_step=2000, freq=10.0, E=4, flags=0, O=64):
    t = ask(["prrt %d %s %s %d %d %s %d %d" % (E, " ".join(num(float(v)) for v in rect), num(cell), subs, max_step, num(freq), flags, O)])[0]
    n_tail = len(PRRT_FIELDS) + len(PRRT_BYTES)
    out = {"status": int(t[0]), "field": " ".join(t[1:len(t) - n_tail])}
    for k, v in zip(PRRT_FIELDS + PRRT_BYTES, t[len(t) - n_tail:]):
        out[k] = float.fromhex(v) if k == "delta_theta" else int(v)
    return out


def test_prrt_plan(ask):
    p = prrt(ask)
    want = dict(status=P_OK, rows=10, cols=10, n_buckets=400, delta_theta=2.0 * math.pi / 4.0, cap_nodes=2001, max_pts=13, cap_points=20064)
    assert {k: p[k] for k in want} == want
    E = 4
    assert {k: p[k] for k in PRRT_BYTES} == dict(
        nodes=E * 2001 * 64, node_bucket=E * 2001 * 4, points=E * 20064 * 4 * 8, occupied=E * 2001 * 4, buckets=E * 400 * 8, mt=E * 624 * 4,
        rng_state=E * 4 * 4, summary=E * 112, step_bucket=E * 4, start=E * 4 * 8, goal=E * 2 * 8, st_log=0)
    assert prrt(ask, flags=ITER_LOG)["st_log"] == E * 2000 * 8 * 4
    # int(height) // int(cell): both truncated first; the origin plays no part; freq below 1 stores one point per step
    p = prrt(ask, rect=(-30.0, 12.5, 75.9, 112.4), cell=10.9, subs=3, freq=0.5, max_step=7)
    assert (p["status"], p["rows"], p["cols"], p["n_buckets"], p["max_pts"], p["cap_points"]) == (P_OK, 9, 10, 270, 3, 7 + 64)


def test_prrt_refusals(ask):
    for kw, status in ((dict(E=0), P_BAD_ARGS), (dict(O=1025), P_OBSTACLES), (dict(cell=0.5), P_BAD_PARAMS), (dict(cell=-3.0), P_BAD_PARAMS),
                       (dict(subs=0), P_BAD_PARAMS), (dict(max_step=0), P_BAD_PARAMS), (dict(freq=math.nan), P_BAD_PARAMS),
                       (dict(freq=-0.5), P_BAD_PARAMS),
                       (dict(rect=(0.0, 0.0, 5.0, 100.0)), P_EMPTY_GRID),                  # narrower than a cell
                       (dict(rect=(0.0, 0.0, 100.0, 9.99)), P_EMPTY_GRID),
                       (dict(rect=(0.0, 0.0, -100.0, 100.0)), P_EMPTY_GRID),
                       (dict(rect=(0.0, 0.0, 5000.0, 5000.0), cell=1.0, subs=2), P_OK),    # 5e7 buckets exactly
                       (dict(rect=(0.0, 0.0, 5000.0, 5001.0), cell=1.0, subs=2), P_BUCKETS),
                       (dict(rect=(0.0, 0.0, 100000.0, 100000.0), cell=1.0), P_BUCKETS),
                       (dict(max_step=(1 << 24) - 2), P_OK), (dict(max_step=(1 << 24) - 1), P_STEPS),
                       (dict(max_step=1000000, freq=2001.0), P_POINTS),
                       (dict(O=1025, cell=math.nan), P_OBSTACLES), (dict(cell=0.5, rect=(0.0, 0.0, math.inf, 1.0)), P_BAD_PARAMS)):
        assert prrt(ask, **kw)["status"] == status, kw


@pytest.mark.parametrize("kw, field", [
    (dict(cell=math.nan), "cell_side_length"), (dict(cell=math.inf), "cell_side_length"), (dict(cell=3.0e9), "cell_side_length"),
    (dict(rect=(0.0, 0.0, math.inf, 100.0)), "rect"), (dict(rect=(0.0, math.nan, 100.0, 100.0)), "rect"),
    (dict(rect=(-2.0e9, 0.0, 2.0e9, 100.0)), "rect"), (dict(rect=(0.0, 0.0, 100.0, 1e300)), "rect"),
    (dict(freq=math.inf), "freq"), (dict(freq=2147483648.0), "freq"), (dict(max_step=INT_MAX), "max_step"),
    (dict(E=INT_MAX, max_step=1 << 23, freq=200.0), "points"),
])
def test_prrt_inputs_that_were_undefined_are_refused(ask, kw, field):
    p = prrt(ask, **kw)
    assert (p["status"], p["field"]) == (P_FIELD, field)


def test_prrt_rng_state_rows(ask):
    t = ask(["rng 5 -1 0 623 624 700"])[0]
    assert [int(v) for v in t] == [0, 624, 0, 0,   0, 624, 0, 0,   623, 1, 0, 0,   0, 0, 0, 0,   0, 0, 0, 0]
    assert ask(["rng 0"])[0] == []


# ---- epoch tags --------------------------------------------------------------------------------------------------------------------

def test_epoch_tag_wraps_at_255_and_clears_on_a_new_allocation(ask):
    t = [int(v) for v in ask(["epoch 260 0"])[0]]
    tags, clears = t[0::2], t[1::2]
    assert [i + 1 for i, c in enumerate(clears) if c] == [1, 256]
    assert tags == list(range(1, 256)) + [1, 2, 3, 4, 5] and 0 not in tags
    t = [int(v) for v in ask(["epoch 12 7"])[0]]
    assert t[0::2] == [1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 5, 6] and [i + 1 for i, c in enumerate(t[1::2]) if c] == [1, 7]


# ---- the random stream's buffer ----------------------------------------------------------------------------------------------------

def test_drawn_memory_keeps_four_blocks_and_the_largest_figures(ask):
    ops = "r 1 100 8  r 2 50 8  r 3 50 8  r 4 50 8  r 1 90 4  r 1 120 2  f 1  r 5 10 1  f 2  f 1  f 3  f 4  f 5  r 6 7 7  f 3  f 1  f 6  f 9"
    t = ask(["drawn " + ops])[0]
    # most and E never shrink; block 5 takes block 2's slot (used longest ago: block 1 was used again), block 6 block 3's
    assert t == ["100", "8", "50", "8", "50", "8", "50", "8", "100", "8", "120", "8", "120", "8", "10", "1", "none", "120", "8", "50", "8",
                 "50", "8", "10", "1", "7", "7", "none", "120", "8", "7", "7", "none"]


def test_stream_bytes_at_the_margin_seams(ask):
    G4 = 4 << 30
    bytes_, padded = 16000000000, 17000000000      # + 1/16
    want = lambda free, held: int(ask(["want %d %d %d" % (free, held, bytes_)])[0][0])  # noqa: E731
    assert want(padded + G4, 0) == padded
    assert want(padded + G4 - 1, 0) == bytes_       # only the exact size fits beside the margin
    assert want(bytes_ + G4, 0) == bytes_
    assert want(bytes_ + G4 - 1, 0) == 0
    assert want(0, 0) == 0
    # what the buffer holds is free again once it is released
    assert want(padded + G4 - 1000, 1000) == padded and want(padded + G4 - 1001, 1000) == bytes_
    assert want(bytes_ + G4 - 1001, 1000) == 0


def test_stream_keeping_equals_the_launch_choice_once_a_figure_was_seen(ask):
    """rrt_stream_keeps (what rrt_prepare_impl keeps the buffer by and rrt_record_drawn takes it by) against
    auvp_rrt_choose_launch's answer with a figure seen.  The two differ, as the host's texts always have, on:
      ROWS_STREAM = 1 with 16 <= max_iter < 1000: the choice streams, the buffer is not kept between batches;
      max_iter >= 65534 (the four-episode kernels' 16-bit node ids): the choice cannot stream, the buffer is kept."""
    from auv_sim_amd import _lib
    modes = {TIMEBIN: "timebin", PLANTIME: "plantime", NN: "nn"}
    grid = [(E, it, mode, lim, rows, stream) for E in (4608, 4609, 12288) for it in (15, 16, 999, 1000, 10000, 65533, 65534)
            for mode in modes for lim in (0, 1) for rows in (-1, 0, 1) for stream in (-1, 0, 1)]
    kept = [int(t[0]) for t in ask(["keep %d 256 %d %d %d %d %d" % g for g in grid])]
    n_kept = n_differ = 0
    for (E, it, mode, lim, rows, stream), keep in zip(grid, kept):
        opts = {k: v for k, v in (("ROWS", rows), ("ROWS_STREAM", stream)) if v >= 0}
        c = _lib.rrt_choose_launch(E, n_cu=256, mode=modes[mode], max_iter=it, K=100 if mode == TIMEBIN else 0, freq=30.0, O=256, H=10, V=4,
                                   T=10, lim=bool(lim), seen_most=46 * it + 1, seen_E=E, options=opts or None)
        chosen = int(c["kind"] == "rows_stream")
        rows_wanted = rows == 1 or (rows < 0 and E > 18 * 256)
        if (stream == 1 and 16 <= it < 1000) or it >= 65534:
            assert keep == int(not lim and mode == TIMEBIN and it >= 1000 and stream != 0 and rows_wanted), (E, it, mode, lim, rows, stream)
            n_differ += keep != chosen
        else:
            assert keep == chosen, (E, it, mode, lim, rows, stream, c["name"])
        n_kept += keep
    assert n_kept > 20 and n_differ > 10

"""The paired A* kernel's hand-over, give-up and batch redo (astar_kernel<3, true>, auvp_astar_batch).

In the paired launch of astar_fixLenSOG wavefronts 0 .. 3 of a workgroup search and wavefront 4 + ((i + 2) & 3) is the partner of
instance i: the searching wavefront posts the popped node through an LDS box, the partner answers with eight neighbours' rows.
Both waits are bounded; an instance whose wait runs out ends with AUVP_ERR_PIPELINE (-9) and auvp_astar_batch searches the whole
batch again on the one-wavefront kernel, on a fresh epoch of the visited words.

Every test starts one fresh child process.  All but the last give it the diagnostic build (libauvplan_diag.so =
-DAUVP_PIPE_DIAG, built by __graft_entry__.build(); auvp_wave.h): AUVP_DIAG_JITTER = "mode,mod,residue,U,seed" sleeps 0 .. U x
s_sleep 1 before every hand-over word of the chosen wavefronts ("2,4,0": wave / 4 == 0, the searchers; "2,4,1": the partners;
"1,8,w": wavefront w alone) and AUVP_DIAG_SPIN replaces the 2^24-poll limit of every wait.  The sweep and the comparison with the
portable checker are tests/experiments/soak_astar_pair.py's; profiles/astar_pair_handover.md records what one run measured."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = os.path.join(REPO, "auv_sim_amd", "libauvplan_diag.so")
SOAK = os.path.join(REPO, "tests", "experiments", "soak_astar_pair.py")
SEARCHERS, PARTNERS = "2,4,0", "2,4,1"
# test c: the longest delay, in units of s_sleep 1 (~64 clocks), before a hand-over word of wavefront 5.  Its searcher polls 400
# times before it gives up.  Measured on the MI355X (profiles/astar_pair_handover.md): no instance gives up at U <= 1 000; at
# 2 000 the two delayed instances give up within their first three expansions -- except in a process's first launch, where one
# of them got through all of its ~250 expansions (400 polls outlasted 2 000 units there); at 4 000 both give up within three
# expansions in every launch.  A wait of W units survives an expansion with probability W / U and a search of 150 m has some
# 200 expansions, so at 4 000 even polls half as fast again as the slowest seen leave (3/4)^200 ~ 1e-25
U_ONE_PARTNER = 4000


def _child(argv, diag=True, jitter=None, spin=None):
    """one fresh process on the diagnostic (or the plain) library; its output, after a clean exit"""
    env = dict(os.environ)
    for k in ("AUVPLAN_LIBRARY", "AUVP_DIAG_JITTER", "AUVP_DIAG_SPIN", "AUVP_ASTAR_PAIR", "AUVP_PIPE_FALLBACK"):
        env.pop(k, None)
    if diag:
        assert os.path.exists(DIAG), "libauvplan_diag.so is built by __graft_entry__.build()"
        env["AUVPLAN_LIBRARY"] = DIAG
    if jitter:
        env["AUVP_DIAG_JITTER"] = jitter
    if spin:
        env["AUVP_DIAG_SPIN"] = str(spin)
    r = subprocess.run([sys.executable] + argv, cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _sweep(cases, seed, **kw):
    """soak_astar_pair.py: (cases, mismatches, instances redone by the pipeline fallback)"""
    last = _child([SOAK, str(cases), str(seed)], **kw).strip().splitlines()[-1]
    print(last)
    return int(last.split(" cases,")[0]), int(last.split("cases,")[1].split()[0]), int(last.split("mismatches,")[1].split()[0])


def _inline(code, **kw):
    """child code that prints one JSON object as its last line"""
    out = _child(["-c", PRELUDE % os.path.join(REPO, "tests", "experiments") + code], **kw)
    facts = json.loads(out.strip().splitlines()[-1])
    print(facts)
    return facts


PRELUDE = r'''
import json, sys
import numpy as np
sys.path.insert(0, %r)
import soak_astar_pair as sp
from auv_sim_amd import _astar_lib as al, _lib, synth
ctx = _lib.Context(0)

def diffs(res, ref, only=None):
    """[instance, first differing field] of every instance (of `only`) that differs from the checker"""
    return [[e, d] for e, d in ((e, sp.first_difference(r, o)) for e, (r, o) in enumerate(zip(res, ref)) if only is None or e in only)
            if d is not None]

def world12(**kw):
    """the world of tests/test_gpu_epoch_wrap.py's A* searches"""
    w = synth.make_world(seed=12, n_obstacles=32, obst_radius=(2.0, 6.0), n_habitats=8, hab_radius=(10.0, 25.0), **kw)
    ctx.set_world(*[w[k] for k in sp.WORLD_KEYS])
    return w

def nine_starts():
    """nine lattice starts (three workgroups, the last one partial), drawn as tests/test_gpu_astar_limits.py::count_world does"""
    rng = np.random.default_rng(1012)
    return np.array([(-290.0 + 10.0 * rng.integers(0, 6), -90.0 + 10.0 * rng.integers(0, 6)) for _ in range(9)])
'''


@pytest.mark.parametrize("stage", [SEARCHERS, PARTNERS], ids=["searchers", "partners"])
def test_delayed_hand_overs_are_waited_for(stage):
    """a pseudo-random delay of 0 .. 32 x s_sleep 1 (~0 .. 2 000 clocks) before every hand-over word of the searching wavefronts
    or of their partners, the default spin limit: a delayed wavefront is waited for, not given up on, and every run of the sweep
    -- the visited arrays included -- equals the checker"""
    cases, bad, redone = _sweep(12, 21, jitter="%s,32,7" % stage)
    assert (cases, bad, redone) == (12, 0, 0)


def test_a_wait_that_runs_out_is_redone_on_the_one_wavefront_kernel():
    """bounded waits of six polls and the partners delayed by up to 64 units: instances end with AUVP_ERR_PIPELINE inside the
    paired launch and auvp_astar_batch searches their batch again -- same results, and the visited words of the launch that gave
    up (a new epoch hides them) must not reach the second search"""
    cases, bad, redone = _sweep(12, 21, jitter="%s,64,3" % PARTNERS, spin=6)
    assert (cases, bad) == (12, 0)
    assert redone > 0


def test_fallback_off_shows_the_status_of_the_delayed_instances_only():
    """wavefront 5 alone delayed, by up to U_ONE_PARTNER units, against a wait of 400 polls: it is the partner of instance 3 of
    its workgroup, so of instances 3 and 7 of a batch of nine.  With PIPE_FALLBACK = 0 those two keep AUVP_ERR_PIPELINE (-9); an
    instance beside them may give up too, but whichever ends with status 0 is complete and right, its visited array included
    (at least one does: the comparison is not empty).  With the default the same batch is redone: nine complete searches, counted."""
    f = _inline(r'''
w = world12()
starts, limits = nine_starts(), np.full(9, 150.0)
ref = sp.checker(w, starts, limits)
ctx.set_option("ASTAR_PAIR", 1)
ctx.set_option("PIPE_FALLBACK", 0)
res0 = sp.gpu_batch(ctx, starts, limits)
fb0, block0 = ctx.pipeline_fallbacks(), ctx.last_launch()[1]
ctx.set_option("PIPE_FALLBACK", None)
res1 = sp.gpu_batch(ctx, starts, limits)
fb1, block1 = ctx.pipeline_fallbacks(), ctx.last_launch()[1]
ok0 = [e for e, r in enumerate(res0) if r["status"] == 0]
print(json.dumps(dict(ref_status=[o["status"] for o in ref], status0=[r["status"] for r in res0], diffs0=diffs(res0, ref, ok0), fb0=fb0,
                      block0=block0, status1=[r["status"] for r in res1], diffs1=diffs(res1, ref), fb1=fb1, block1=block1)))
''', jitter="1,8,5,%d,5" % U_ONE_PARTNER, spin=400)
    assert f["ref_status"] == [0] * 9
    # the fallback off: the status is there to see, nothing was redone, and what finished is right
    st = f["status0"]
    assert st[3] == -9 and st[7] == -9, st
    assert all(s in (0, -9) for s in st), st
    assert st.count(0) >= 1, st
    assert f["diffs0"] == []
    assert f["fb0"][0] == 0 and f["block0"] == 512
    # the default: the batch is searched again, every instance that gave up is counted
    assert f["status1"] == [0] * 9
    assert 2 <= f["fb1"][0] <= 9
    assert f["fb1"][1] - f["fb0"][1] == f["fb1"][0]
    assert f["diffs1"] == []
    assert f["block1"] == 256


def test_the_redo_clears_the_visited_words_at_the_tag_wrap():
    """one handle, E = 2 throughout (the visited table is allocated once), the searches of tests/test_gpu_epoch_wrap.py.  Batch k
    carries tag k: batch 1, from starts one lattice step beside the final batch's, leaves tag-1 words over the cells the final
    batch will visit; batches 2 .. 254 search far away on the one-wavefront kernel, which cannot give up.  Batch 255, paired, with a
    wait of ONE poll and the partners delayed, gives up on its first expansion with tag 255 taken: the redo inside
    auvp_astar_batch has to clear the table before it starts over at tag 1, or batch 1's words count as visited cells -- which
    the checker, seeded with them, shows to change the search.  Batch 256 (tag 2) goes over batch 1's cells once more."""
    f = _inline(r'''
w = world12()
final, beside = np.array([(-280.0, -80.0), (-250.0, -60.0)]), np.array([(-270.0, -80.0), (-240.0, -60.0)])
far = np.array([(-130.0, 70.0), (-140.0, 60.0)])
limits, cap = np.full(2, 80.0), 4000
ref = {k: sp.checker(w, s, limits, cap_nodes=cap) for k, s in (("final", final), ("beside", beside), ("far", far))}
# the test must discriminate: batch 1's words, were they to survive with the redo's tag, change the final batch ...
seeded = sp.checker(w, final, limits, cap_nodes=cap, visited=[o["visited"] for o in ref["beside"]])
# ... and they do survive batches 2 .. 254, which touch none of them
overlap = int(sum((a["visited"] & (b["visited"] | c["visited"])).sum() for a, b, c in zip(ref["far"], ref["beside"], ref["final"])))
ctx.set_option("ASTAR_PAIR", 0)
d1 = diffs(sp.gpu_batch(ctx, beside, limits, cap_nodes=cap), ref["beside"])
between, first = 0, None
for k in range(2, 255):
    got = al.run_batch_arrays(ctx, sp.VARIANT, far, limits=limits, weights=sp.WEIGHTS, cap_nodes=cap)["summ"]
    first = got.copy() if first is None else first
    between += int(not all(np.array_equal(got[n], first[n]) for n in got.dtype.names))
far_ok = [int(first[e]["status"]) == 0 and int(first[e]["n_nodes"]) == ref["far"][e]["n_nodes"] for e in range(2)]
total = ctx.pipeline_fallbacks()[1]
ctx.set_option("ASTAR_PAIR", 1)
res = sp.gpu_batch(ctx, final, limits, cap_nodes=cap)
fb, block = ctx.pipeline_fallbacks(), ctx.last_launch()[1]
ctx.set_option("ASTAR_PAIR", 0)
d256 = diffs(sp.gpu_batch(ctx, beside, limits, cap_nodes=cap), ref["beside"])
print(json.dumps(dict(ref_status=[o["status"] for k in ref for o in ref[k]], n_nodes=[o["n_nodes"] for o in ref["final"]],
                      n_nodes_seeded=[o["n_nodes"] for o in seeded], overlap=overlap, d1=d1, between=between, far_ok=far_ok,
                      total_before=total, fb=fb, block=block, status=[r["status"] for r in res], d255=diffs(res, ref["final"]), d256=d256)))
''', jitter="%s,64,3" % PARTNERS, spin=1)
    assert f["ref_status"] == [0] * 6
    assert any(a != b for a, b in zip(f["n_nodes"], f["n_nodes_seeded"])), (f["n_nodes"], f["n_nodes_seeded"])
    assert f["overlap"] == 0
    assert f["d1"] == [] and f["between"] == 0 and f["far_ok"] == [True, True]
    assert f["total_before"] == 0   # batches 1 .. 254 took one tag each
    assert f["fb"][0] > 0 and f["block"] == 256, (f["fb"], f["block"])
    assert f["status"] == [0, 0] and f["d255"] == []
    assert f["d256"] == []


@pytest.mark.parametrize("case", ["capacity", "time_bins"])
def test_declared_errors_leave_through_the_paired_exit(case):
    """status -2 (node capacity) and -1 (a time stamp past the last time bin: the reference raises) are declared by the searching
    wavefront after it has posted the node, while its partner is working -- the plain library, the paired launch against the
    one-wavefront kernel (every field) and against the checker (status and the expansions before the error).  An error is no
    give-up: nothing is redone."""
    f = _inline(r'''
case = %r
w = world12(**(dict(n_bins=3, bin_len=20) if case == "time_bins" else {}))
starts, limits = nine_starts(), np.full(9, 150.0)
cap = 64 if case == "capacity" else 20000
ref = sp.checker(w, starts, limits, cap_nodes=cap)
total = ctx.pipeline_fallbacks()[1]
ctx.set_option("ASTAR_PAIR", 1)
paired = sp.gpu_batch(ctx, starts, limits, cap_nodes=cap)
fb, block = ctx.pipeline_fallbacks(), ctx.last_launch()[1]
ctx.set_option("ASTAR_PAIR", 0)
single = sp.gpu_batch(ctx, starts, limits, cap_nodes=cap)
print(json.dumps(dict(ref_status=[o["status"] for o in ref], status=[r["status"] for r in paired], fb=fb, total_before=total, block=block,
                      block_single=ctx.last_launch()[1], same=[sp.same_results(a, b) for a, b in zip(paired, single)],
                      d_paired=diffs(paired, ref), d_single=diffs(single, ref), n_exp=[r["n_expansions"] for r in paired])))
''' % case, diag=False)
    # the checker numbers the two errors the other way round (soak_astar_pair.STATUS_TO_CHECKER)
    want, want_ref = (-2, -1) if case == "capacity" else (-1, -2)
    assert f["ref_status"] == [want_ref] * 9   # every instance overflows / leaves the last bin
    assert f["status"] == [want] * 9
    assert min(f["n_exp"]) > 1                 # ... some expansions in: hand-overs had completed before the exit
    assert f["block"] == 512 and f["block_single"] == 256
    assert f["fb"] == [0, f["total_before"]]
    assert f["same"] == [True] * 9
    assert f["d_paired"] == [] and f["d_single"] == []

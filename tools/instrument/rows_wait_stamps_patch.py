#!/usr/bin/env python3
"""Temporary source patch: s_memtime stamps around ONE class of waits of the four-episode RRT body (auv_sim_amd/csrc/rrt_rows_body.h),
picked by -DAUVP_ROWS_WAIT_STAMPS=<class>.  The differences accumulate in one scalar register pair per wave; the total lands in
the summary's nn_scanned (unused in time-bin mode), where tools/rows_wait_probe.py reads it.  Never the product.

  cp auv_sim_amd/csrc/rrt_rows_body.h /tmp/rows_body.orig.h
  python tools/instrument/rows_wait_stamps_patch.py
  python __graft_entry__.py variant exp/libauvplan_ws2.so -DAUVP_ROWS_WAIT_STAMPS=2      (one library per class)
  cp /tmp/rows_body.orig.h auv_sim_amd/csrc/rrt_rows_body.h
  AUVPLAN_LIBRARY=exp/libauvplan_ws2.so python tools/rows_wait_probe.py 2

Classes (profiles/rows_trip_lgkm.md):
  1  the parent's id (the bin-member word, then the id), waited for where the parent's record is requested        -- a pure wait
  2  the parent's record at its first use in pass 0                                                                -- a pure wait
  3  the candidate loop of the cull (both instances): a REGION, the exact tests' arithmetic included
  4  the accepting path, from `if (acc_)` to the trip's last wave_sync: a REGION (the wait before the bin append lies in it;
     it belongs to a register the compiler reuses, not to a value the source can name, so it cannot be stamped alone)
  5  a steer pass's theta chain, from its call to the chain's result: a REGION (the 15 dependent DPP fmacs included)
  6  a steer pass's four chains, from the increments' LDS write to the prefix values read back: a REGION
  7  the stream_ensure calls of a trip (votes and slow path): a REGION
  8  the selection tail, from the selection loop's exit to the member index `ri` the parent-id request is made with: a REGION
     (the two draws after the winner's, the winner's count; nothing else in the wave can run beside it)
  9  a steer pass's tail, from the lanes' own prefix reads to the end of the pass: a REGION (the point stores' issue, the row's
     end state -- profiles/rows_trip_lds.md)
A pure wait is `stamp; empty asm that reads the value; stamp`: the compiler puts the value's s_waitcnt between the stamps (check
the listing: with a read-write operand it copies the registers BEFORE the first stamp and the wait goes with the copies; the
scheduling barriers round the first stamp keep it in front).  A stamp is itself a scalar-memory read that returns through
lgkmcnt, so every stamp pair also drains the LDS reads in flight -- what the stamps cost shows in the stamped kernel's time
beside the unstamped one's.  Class 7 costs the stream kernel 4 spilled scalar registers (no scratch); the others none."""
import os
import sys

p = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
                                                        "auv_sim_amd", "csrc", "rrt_rows_body.h")
s = open(p).read()


def before(anchor, text, count=1):
    global s
    assert s.count(anchor) == count, (s.count(anchor), anchor)
    s = s.replace(anchor, text + anchor)


def after(anchor, text, count=1):
    global s
    assert s.count(anchor) == count, (s.count(anchor), anchor)
    s = s.replace(anchor, anchor + text)


IN = "\n#ifdef AUVP_ROWS_WAIT_STAMPS\n      ROWS_WS_IN(%d);\n#endif\n"
OUT = "\n#ifdef AUVP_ROWS_WAIT_STAMPS\n      ROWS_WS_OUT(%d);\n#endif\n"


def pure(k, asm):
    # (the scheduling barriers keep the copies the compiler makes of the awaited registers -- and their wait -- behind the first stamp)
    return ("\n#ifdef AUVP_ROWS_WAIT_STAMPS\n      if (AUVP_ROWS_WAIT_STAMPS == %d) { __builtin_amdgcn_sched_barrier(0); ROWS_WS_IN(%d); "
            "__builtin_amdgcn_sched_barrier(0); %s; ROWS_WS_OUT(%d); }\n#endif\n" % (k, k, asm, k))


before("  for (int it = 0; it < P.max_iter; it++) {\n    if (!wave_any(live)) break;",
       "#ifdef AUVP_ROWS_WAIT_STAMPS\n  unsigned long long ws_acc = 0ull, ws_t0 = 0ull;\n"
       "#define ROWS_WS_IN(c) do { if (AUVP_ROWS_WAIT_STAMPS == (c)) ws_t0 = __builtin_amdgcn_s_memtime(); } while (0)\n"
       "#define ROWS_WS_OUT(c) do { if (AUVP_ROWS_WAIT_STAMPS == (c)) ws_acc += __builtin_amdgcn_s_memtime() - ws_t0; } while (0)\n#endif\n")
# 1: the parent's id, where the record is requested
before("    double cx = 0.0, cy = 0.0, cth = 0.0, ctt = 0.0, clen = 0.0;\n    if (live) {", pure(1, 'asm volatile("" : : "v"(par))'))
# 2: the record at its first use (pass 0: the theta chain is the first thing that needs cth)
before("      const double th = rows_theta_chain_dpp(cth, phi);",
       "\n#ifdef AUVP_ROWS_WAIT_STAMPS\n      if (AUVP_ROWS_WAIT_STAMPS == 2 && pass == 0) { __builtin_amdgcn_sched_barrier(0); ROWS_WS_IN(2); "
       '__builtin_amdgcn_sched_barrier(0); asm volatile("" : : "v"(cx), "v"(cy), "v"(cth), "v"(ctt), "v"(clen)); ROWS_WS_OUT(2); }\n#endif\n' + IN % 5)
# 5: the theta chain
after("      const double th = rows_theta_chain_dpp(cth, phi);",
      '\n#ifdef AUVP_ROWS_WAIT_STAMPS\n      double th_ws = th;\n      if (AUVP_ROWS_WAIT_STAMPS == 5) { asm volatile("" : "+v"(th_ws)); ROWS_WS_OUT(5); }\n#endif\n')
# 6: the four chains
before("      if (rl < 15) { inc[rl] = dx; inc[18 + rl] = dy; inc[36 + rl] = dt; inc[54 + rl] = mv; }", IN % 6)
after("      if (active) { mx = inc[rl]; my = inc[18 + rl]; mt_ = inc[36 + rl]; ml = inc[54 + rl]; }",
      '\n#ifdef AUVP_ROWS_WAIT_STAMPS\n      if (AUVP_ROWS_WAIT_STAMPS == 6) { asm volatile("" : "+v"(mx), "+v"(my), "+v"(mt_), "+v"(ml)); ROWS_WS_OUT(6); }\n#endif\n')
# 3: the candidate loop
before("        while (wave_any(cm != 0u)) {", IN % 3)
before("      }\n    };\n    if (P.flags & AUVP_KFLAG_TIGHT_CULL)", OUT % 3)
# 4: the accepting path
before("    if (acc_) {\n      // curr_bin", IN % 4)
before("    wave_sync();\n  }\n\n  // ---- epilogue ----", OUT % 4)
# 7: stream_ensure
for a in ("        if (!stream_ensure<MIRROR>(rng, search, 16u, rl) && search)",
          "    if (!stream_ensure<MIRROR>(rng, on0, (uint32_t)(base + 3 * n0_), rl) && on0)",
          "      if (pass != 0 && !stream_ensure<MIRROR>(rng, on, (uint32_t)nwin, rl) && on)"):
    before(a, IN % 7)
after("{ status = AUVP_ST_STREAM; live = false; iters_run = it; search = false; }", OUT % 7)
after("&& on0) { status = AUVP_ST_STREAM; live = false; iters_run = it; }", OUT % 7)
after("&& on) { status = AUVP_ST_STREAM; live = false; iters_run = it; }", OUT % 7)
# 8: the selection tail
before("      // the two draws after the winner's\n#if AUVP_ROWS_BODY_STREAM", IN % 8)
after("        const int ri = (int)py_uniform(0.0, (double)cnt, u1);",
      '\n#ifdef AUVP_ROWS_WAIT_STAMPS\n        if (AUVP_ROWS_WAIT_STAMPS == 8) { asm volatile("" : : "v"(ri)); ROWS_WS_OUT(8); }\n#endif\n')
# 9: a pass's tail
before("      if (active) { mx = inc[rl]; my = inc[18 + rl]; mt_ = inc[36 + rl]; ml = inc[54 + rl]; }", IN % 9)
before("      first_pass = false;\n      wave_sync();",
       '\n#ifdef AUVP_ROWS_WAIT_STAMPS\n      if (AUVP_ROWS_WAIT_STAMPS == 9) { asm volatile("" : : "v"(cx), "v"(cy), "v"(cth), "v"(ctt), "v"(clen)); '
       'ROWS_WS_OUT(9); }\n#endif\n')
# the total, per wave (every row of the wave reports it)
after("      s.rng_after = after; s.leaf_elems = 0; s.n_draw32 = drawn; s.nn_scanned = 0ull;",
      "\n#ifdef AUVP_ROWS_WAIT_STAMPS\n      s.nn_scanned = ws_acc;\n#endif")
open(p, "w").write(s)

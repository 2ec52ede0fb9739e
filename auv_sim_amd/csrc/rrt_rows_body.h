// rrt_rows_body.h -- the body of rrt_rows_kernel (rrt_rows_kernel.h) and of rrt_rows_stream_kernel (rrt_rows_stream_kernel.h),
// included inside both: RRT.exploring, time-bin sampling, four episodes per wavefront.  In scope: the kernel arguments W, P, B,
// n_episodes and the switch AUVP_ROWS_BODY_STREAM, #defined just before the include and #undefined after it:
//   0  the row runs CPython's generator in its LDS block (RowRng: rows_ensure / rows_random_at / rows_advance, counted in 32-bit
//      words) and a steer pass copies the tempered numbers it may look at into a window area of LDS;
//   1  the row reads the numbers rrt_stream_kernel wrote ahead (RowStream: stream_ensure / stream_base + stream_read /
//      stream_advance / stream_top_up, counted in random() numbers) and the window is the ring itself (MIRROR, a constant of
//      the including kernel: the ring's form).
// What differs is marked by the switch: the set-up (LDS plan, `rng`, ROWS_CONSUME), the sixteen draws of a selection round and
// the two after the winner's, how a steer pass gets its window ready and reads it (ROWS_WIN), the stream's top-up, the epilogue.
// Everything else is the one loop.
// The switch is the preprocessor: `rng` has a different type in each kernel and rrt_rows_kernel is not a template, so both arms
// of an `if constexpr` would have to compile for both; and the two accessors are macros because they then expand to the very
// expressions the kernels had as separate texts -- both kernels' machine code is what it was then, which lambdas did not keep.
// (One text in two kernels, not a __device__ function: as rrt_explore_body.h.)
// No include guard: the file is included once inside each of the two kernels, and nowhere else.
  extern __shared__ __align__(16) unsigned char smem[];
  const RrtTables S = rrt_tables_view(smem, W.n_habitats, W.n_poly);
  const int wave = (int)(threadIdx.x >> 6);
  const int lane = lane_id();
  const int row = lane >> 4, rl = lane & 15, rowbase = lane & 48;
  const int K = P.K;
  const int wg_waves = (int)(blockDim.x >> 6);
  // ---- the episode's LDS block: where its random numbers come from, the running-sum scratch, the time-bin counters ----
#if AUVP_ROWS_BODY_STREAM
  const RowsStreamLdsPlan plan = rrt_rows_stream_lds_plan(K, RW_MAX_OBST, rrt_tables_bytes(W.n_habitats, W.n_poly, W.n_bins), wg_waves, MIRROR);
  unsigned char* ebase = smem + plan.tables + (size_t)(wave * RW_ROWS + row) * plan.per_ep;
  double* ring = reinterpret_cast<double*>(ebase);                // [RS_RING (+ RS_MIRROR)] the next random() values of the episode
  double* inc = reinterpret_cast<double*>(ebase + plan.ring);     // [4][18] running sums
  uint16_t* bin_count = reinterpret_cast<uint16_t*>(ebase + plan.ring + plan.scratch);
#else
  const RowsLdsPlan plan = rrt_rows_lds_plan(K, RW_MAX_OBST, rrt_tables_bytes(W.n_habitats, W.n_poly, W.n_bins), wg_waves);
  unsigned char* ebase = smem + plan.tables + (size_t)(wave * RW_ROWS + row) * plan.per_ep;
  uint32_t* mt = reinterpret_cast<uint32_t*>(ebase);
  double* win = reinterpret_cast<double*>(ebase + plan.mt);  // [RW_WIN] tempered random() values of a pass
  double* inc = win;                                         // [4][18] running sums (aliases the window once it is dead)
  uint16_t* bin_count = reinterpret_cast<uint16_t*>(ebase + plan.mt + plan.scratch);
#endif

  rrt_tables_stage(S, W);
  if (threadIdx.x == 0) *S.params = P;
  const RrtParamsDev& Q = *S.params;
  double* olx = reinterpret_cast<double*>(smem + plan.tables + (size_t)wg_waves * RW_ROWS * plan.per_ep);
  double* oly = olx + RW_MAX_OBST;
  float* olr = reinterpret_cast<float*>(oly + RW_MAX_OBST);
  // the tile grouped by median splits (WorldDev::os_*): slot s = entries 16 s .. 16 s + 15, a group of at most 16 + padding
  for (int i = threadIdx.x; i < RW_MAX_OBST; i += blockDim.x) { olx[i] = W.os_x[i]; oly[i] = W.os_y[i]; olr[i] = W.os_r[i]; }
  __syncthreads();

  const int ep = ((int)blockIdx.x * wg_waves + wave) * RW_ROWS + row;
  bool live = ep < n_episodes;  // row-uniform; a row that fails keeps running as a no-op until the wave is done
  const int eps = live ? ep : 0;
  if (!wave_any(live)) return;

  // ---- per-episode views ----
  const int capn = B.cap_nodes, capp = B.cap_points, bcap = B.bin_cap;
  double* nodeF = B.node_f + (size_t)eps * capn * 8;
  int4* nodeI = reinterpret_cast<int4*>(B.node_i) + (size_t)eps * capn;
  uint8_t* nodeQ = B.node_q + (size_t)eps * capn;
  double* ptF = B.points + (size_t)eps * capp * 6;
  const BinLists bins = bin_lists(B, (size_t)eps, K);
  int next_chunk = 0;
  const double* init = B.init + (size_t)eps * 6;

  // ---- the row's random() numbers.  ROWS_CONSUME(on, n): the rows that are `on` have used up the next n of them ----
#if AUVP_ROWS_BODY_STREAM
  RowStream rng;  // the episode's part of the stream written ahead: nothing to seed, the ring fills on first use
  rng.ring = ring;
  rng.src = B.stream + (size_t)eps * (size_t)B.stream_cap;
  rng.pos = 0u; rng.front = 0u; rng.req = 0u;
  rng.cap = (uint32_t)B.stream_cap;
#pragma unroll
  for (int c = 0; c < RS_PEND; c++) rng.pend[c] = rs_piece(0.0);
#ifdef AUVP_STREAM_COUNT_SLOW
  rng.slow = 0u;
#endif
#define ROWS_CONSUME(on, n) stream_advance(rng, on, (uint32_t)(n))
#else
  RowRng rng;  // CPython's generator, its state copied in
  rng.s = mt;
  for (int i = rl; i < 624; i += 16) mt[i] = B.mt[(size_t)eps * 624 + i];
  {
    int idx = B.mt_index ? B.mt_index[eps] : 624;
    idx = idx < 0 ? 0 : (idx > 624 ? 624 : idx);
    rng.pslot = idx == 624 ? 0u : (uint32_t)idx;
    rng.avail = (uint32_t)(624 - idx);
    rng.drawn = 0ull;
  }
#define ROWS_CONSUME(on, n) rows_advance(rng, on, (uint32_t)(2 * (n)))  // (the generator counts 32-bit words: two per number)
#endif
  for (int i = rl; i < K + 2; i += 16) bin_count[i] = 0;
  wave_sync();
  if (live && rl == 0) {
    nodeF[0] = init[0]; nodeF[1] = init[1]; nodeF[2] = init[2]; nodeF[3] = init[3]; nodeF[4] = init[5];
    nodeI[0] = make_int4(0, -1, 0, 0);
    nodeQ[0] = 0;  // the start state is never a leaf candidate
    bins.direct[(K >= 1 ? 1 : 0) * AUVP_BIN_HEAD] = 0;
    bin_count[K >= 1 ? 1 : 0] = 1;
  }
  wave_sync();
  int n_nodes = 1, n_points = 0, status = 0, n_cand = 0, iters_run = 0;
  // lane rl keeps the bounding box of obstacle slot rl: one compare round tells which slots a steer can touch
  double4 sbox_ld = reinterpret_cast<const double4*>(W.os_box)[rl];
  // (the empty statement makes the four components arrive HERE: used first inside the loop, the load stayed pending over the
  // loop's header and its first use in the cull drained the vector-memory counter -- the trip's own point stores with it --
  // in every trip: profiles/rows_trip_waits.md.  No instruction per trip.)
  asm volatile("" : "+v"(sbox_ld.x), "+v"(sbox_ld.y), "+v"(sbox_ld.z), "+v"(sbox_ld.w));
  const double4 sbox = sbox_ld;
  // the obstacles' thresholds are read through the scalar data path (constant address space: the table is written by the host
  // before the launch and by nobody during it), so that no vector-memory load -- and no wait on the one in-order counter the
  // point stores share -- is left in the collision test
  typedef const __attribute__((address_space(4))) double* rows_ost_ptr;
  const rows_ost_ptr ost_s = (rows_ost_ptr)W.os_t;
  const int nv_poly = W.n_poly;

  for (int it = 0; it < P.max_iter; it++) {
    if (!wave_any(live)) break;
    // ------------------------------------------------------------ parent selection (:121-127)
    // lane rl of a row tries draw rl: ran_bin = int(uniform(1, K+1)) until that bin is non-empty; the first success in
    // stream order wins, a key beyond K before it is a KeyError.  14 tries per round leave room for the two draws
    // that follow the successful one.
    int par = 0, n_total = 0, base = 0;
    {
      bool search = live;
      int fo = 0, rb = 0, cnt = 0;
      double u = 0.0;
#if AUVP_ROWS_BODY_STREAM
      StreamBase<MIRROR> sel;  // the round's sixteen numbers: the window at the row's position
#endif
      for (;;) {
        // the round's sixteen draws: the next sixteen numbers of the row's stream
#if AUVP_ROWS_BODY_STREAM
        // (a row whose stream ends before what it asks for gives up, here and below: the host redoes the batch on rrt_rows_kernel)
        if (!stream_ensure<MIRROR>(rng, search, 16u, rl) && search) { status = AUVP_ST_STREAM; live = false; iters_run = it; search = false; }
        sel = stream_base<MIRROR>(rng, 0u, rl);
        if (search) u = stream_read(sel, rl, rl);
#else
        rows_ensure(rng, search, 32u, rl);
        // (they also go to the window area, free at this point: they ARE stream entries 0 .. 15 of the first pass's window
        // -- stream entry e at win[e] -- and the two draws after the winner's are read from there)
        if (search) { u = rows_random_at(rng, (uint32_t)rl); win[rl] = u; }
#endif
        const int rbj = (int)py_uniform(1.0, (double)(K + 1), u);
        const bool cand = search && rl < 14;
        const bool badkey = cand && rbj > K;
        const int cj = (cand && !badkey) ? (int)bin_count[rbj] : 0;
        const uint32_t okm = row_ballot(cj != 0, rowbase), badm = row_ballot(badkey, rowbase);
        const int f_ok = okm ? (__ffs((int)okm) - 1) : 16, f_bad = badm ? (__ffs((int)badm) - 1) : 16;
        if (search) {
          if (f_bad < f_ok) { status = -5; live = false; iters_run = it; search = false; }
          else if (f_ok < 16) { fo = f_ok; search = false; }
        }
        const bool again = search;
        ROWS_CONSUME(again, 14);  // 14 unsuccessful draws
        const int src = rowbase + (again ? 0 : fo);
        // rows that just finished pick up the winner's values (rows still searching read garbage they overwrite later)
        const int rb_n = row_read(rbj, src), cnt_n = row_read(cj, src);
        if (!again && live && cnt == 0) { rb = rb_n; cnt = cnt_n; }
        if (!wave_any(again)) break;
      }
      // the two draws after the winner's
#if AUVP_ROWS_BODY_STREAM
      const double u1 = stream_read(sel, fo + 1, rl), u2 = stream_read(sel, fo + 2, rl);
#else
      wave_sync();  // (win[] was written by other lanes)
      const double u1 = win[fo + 1], u2 = win[fo + 2];
#endif
      if (live) {
        const int ri = (int)py_uniform(0.0, (double)cnt, u1);
        par = bin_member(bins, rb, ri);
        n_total = (int)auvp_floor(py_uniform(0.0, Q.freq, u2) / 1);
        base = fo + 3;
      }
    }
    // ------------------------------------------------------------ steer (:252-295), passes of RW_C sub-arcs
    // A pass of n sub-arcs looks at up to 3 n + 3 numbers, its window: window entry j = random() number b0 + j from the row's
    // position in its stream.  The first pass's window (b0 = base) needs nothing of the parent: it is made ready while the
    // parent's id (and then its record) is still on its way from memory
    const bool on0 = live && 0 < n_total;
    const int n0_ = on0 ? (n_total < RW_C ? n_total : RW_C) : 0;
#if AUVP_ROWS_BODY_STREAM
    // the window is the ring itself -- ring entry (pos + b0 + j) -- so there is nothing to build: the ring only has to reach that far
    if (!stream_ensure<MIRROR>(rng, on0, (uint32_t)(base + 3 * n0_), rl) && on0) { status = AUVP_ST_STREAM; live = false; iters_run = it; }
#else
    // the window is built: the numbers generated, tempered and written to win[].  A later pass's, from win[0] on:
    auto make_window = [&](bool on, int nwin, int b0) {
      rows_ensure(rng, on, (uint32_t)(2 * (b0 + nwin)), rl);
#pragma unroll
      for (int t = 0; t < 3; t++) {
        const int j = rl + 16 * t;
        if (on && j < nwin) win[j] = rows_random_at(rng, (uint32_t)(b0 + j));
      }
      wave_sync();
    };
    {
      // the first pass's: stream entry e at win[e], so window entry j = win[base + j]; entries below 16 are there already
      const int e_end = base + 3 * n0_;
      rows_ensure(rng, on0, (uint32_t)(2 * e_end), rl);
#pragma unroll
      for (int t = 0; t < 3; t++) {
        const int e = 16 + rl + 16 * t;
        if (on0 && e < e_end) win[e] = rows_random_at(rng, (uint32_t)e);
      }
      wave_sync();
    }
#endif
    double cx = 0.0, cy = 0.0, cth = 0.0, ctt = 0.0, clen = 0.0;
    if (live) {
      const double2 a = *reinterpret_cast<const double2*>(nodeF + (size_t)par * 8);
      const double2 b = *reinterpret_cast<const double2*>(nodeF + (size_t)par * 8 + 2);
      cx = a.x; cy = a.y; cth = b.x; ctt = b.y;
      clen = nodeF[(size_t)par * 8 + 4];
    }
#if AUVP_ROWS_BODY_STREAM
    // once per trip: the chunks requested a trip ago go into the ring, the next ones are requested.  Those chunks arrived with
    // the parent's record of the trip before (the first pass's wait for it covers them: they are older), so the write waits for
    // nothing -- as long as every way through a trip passes that wait, which is why the first pass is not skipped (below) and
    // why stream_ensure's slow path settles what it requested.  (At the end of the trip the same write waited for the trip's
    // own point stores: measured 45 % of the wave-cycles waiting instead of 34 %)
    stream_top_up<MIRROR>(rng, live, rl);
#endif
    const double px0 = cx, py0 = cy, clen0 = clen;
    int cnt = 0;  // appended path points of this row's steer
    // the lane's own path point of pass 0 / pass 1 (kept for the exact collision and boundary tests)
    double ptx[2] = {0.0, 0.0}, pty[2] = {0.0, 0.0};
    bool ptv[2] = {false, false};
    bool first_pass = true;
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
      const int c0 = pass * RW_C;
      const bool on = live && c0 < n_total;  // rows with sub-arcs left
      // (the first pass runs whatever the rows ask for: with no row `on` -- every live row drew zero sub-arcs, rare -- it is a
      // pass of zeros that changes nothing, and the parent's record then has ONE place where it is first used.  With a way
      // round the pass the record stayed "on its way" for the compiler on that way, and the ring write above and the trip's
      // tail drained the vector-memory counter -- the point stores with it -- for registers nobody was waiting for:
      // profiles/rows_trip_waits.md)
      if (pass != 0 && !wave_any(on)) break;
      const int n = on ? ((n_total - c0) < RW_C ? (n_total - c0) : RW_C) : 0;
      const int nwin = 3 * n;
#ifdef AUVP_ROWS_PAD
      // EXPERIMENT ONLY (tools/rows_pass_probe.py, profiles/r4_rows_packing.md; never defined in the product build): AUVP_ROWS_PAD
      // extra vector instructions per steer pass -- independent fp64 adds on four registers, results unused -- to measure what
      // a pass can afford to carry before packing the rows' sub-arcs stops paying
      {
        double pd0 = cth, pd1 = cx, pd2 = cy, pd3 = ctt;
#pragma unroll
        for (int q = 0; q < AUVP_ROWS_PAD / 4; q++)
          asm volatile("v_add_f64 %0, %0, 1.0\n\tv_add_f64 %1, %1, 1.0\n\tv_add_f64 %2, %2, 1.0\n\tv_add_f64 %3, %3, 1.0"
                       : "+v"(pd0), "+v"(pd1), "+v"(pd2), "+v"(pd3));
      }
#endif
      const int b0 = first_pass ? base : 0;  // later passes start at the (advanced) head of the stream
      // a later pass gets its window ready here (the first pass's is already: above).  ROWS_WIN(j) = window entry j of this pass
      // (a macro, not a lambda: through a lambda both kernels' code generation changed)
#if AUVP_ROWS_BODY_STREAM
      if (pass != 0 && !stream_ensure<MIRROR>(rng, on, (uint32_t)nwin, rl) && on) { status = AUVP_ST_STREAM; live = false; iters_run = it; }
      // (the selection's draws, b0 of them in the first pass, are part of the window's base: the row's position itself moves
      // when the pass is over, so a row that fails inside it reports the position it had)
      const StreamBase<MIRROR> wb = stream_base<MIRROR>(rng, (uint32_t)b0, rl);
#define ROWS_WIN(j) stream_read(wb, (j), rl)
#else
      if (pass != 0) make_window(on, nwin, b0);
      const double* wp = win + (pass == 0 ? base : 0);
#define ROWS_WIN(j) wp[j]
#endif
      // "taken" predicate for every possible start offset, 48 bits per row
      unsigned long long tpred = 0ull;
#pragma unroll
      for (int t = 0; t < 3; t++) {
        // every lane compares (entries past the window are whatever the scratch holds: never a trap, masked below); the
        // predicate is the AND of two single-compare ballots, taken in scalar registers (nwin = 0 for rows that are not `on`)
        const int j = rl + 16 * t;
        const double dist = py_uniform(0.0, Q.dist_to_end, ROWS_WIN(j));
        const double diff = py_uniform(-Q.diff_max, Q.diff_max, ROWS_WIN(j + 1));
        const unsigned long long fb = __builtin_amdgcn_fcmp(auvp_fabs(dist), auvp_fabs(diff), 2 /* ordered > */) &
                                      __builtin_amdgcn_uicmp((unsigned)(j + 1), (unsigned)nwin, 36 /* unsigned < */);
        tpred |= ((fb >> rowbase) & 0xffffull) << (16 * t);
      }
      // where does sub-arc s start?  pos_s = 2s + (#taken among sub-arcs < s): fixed point of
      //   taken_s = T[2s + c_s],  c_s = popcount(taken below s),  started from "everything taken"
      // (the votes are ballots of ONE compare each -- `__builtin_amdgcn_uicmp` -- with the lanes that do not take part made
      // neutral through their data: a vote on `active && x` costs two more vector instructions, a 0 / 1 and its compare)
      const bool active = rl < n;
      const uint32_t mywin = active ? (uint32_t)(tpred >> (2 * rl)) : 0u;  // bits 0 .. rl are looked at (cbelow <= rl <= 14)
      const uint32_t below_me = active ? ((1u << rl) - 1u) : 0u;
      int cbelow = active ? rl : 0;
      uint32_t tmask;
      for (;;) {
        const unsigned long long tb = __builtin_amdgcn_uicmp((mywin >> cbelow) & 1u, 0u, 33 /* != */);
        tmask = (uint32_t)((tb >> rowbase) & 0xffffull);
        const int cnew = __popc(tmask & below_me);
        const unsigned long long chg = __builtin_amdgcn_uicmp((unsigned)cnew, (unsigned)cbelow, 33 /* != */);
        cbelow = cnew;
        if (chg == 0ull) break;
      }
      const int mypos = 2 * rl + cbelow;
      const int used = 2 * n + __popc(tmask);
      const bool taken = (tmask >> rl) & 1u;
      // what a lane without an arc adds to the five sums: +0.0 for an untaken sub-arc, -0.0 past n (rows_idle_zero: the chains
      // run on over the idle lanes and end with the values of sub-arc n - 1)
      const double zero = rows_idle_zero(active);
      double radius = 0.0, phi = zero, vt = 1.0;
      if (taken) {
        const double dist = py_uniform(0.0, Q.dist_to_end, ROWS_WIN(mypos));
        const double diff = py_uniform(-Q.diff_max, Q.diff_max, ROWS_WIN(mypos + 1));
        const double s1 = dist + diff, s2 = dist - diff;
        radius = auvp_div_plain(s1 + s2, -s1 + s2);
        phi = auvp_div_plain(s1 + s2, 2 * radius);
        vt = py_uniform(0.0, 2 * Q.v, ROWS_WIN(mypos + 2));
      }
#undef ROWS_WIN
#if !AUVP_ROWS_BODY_STREAM
      // the window is dead: its LDS becomes the running-sum scratch.  (Not in the stream variant: the ring shares its LDS with
      // nothing, the running sums have their 576 B to themselves)
      wave_sync();
#endif
      // theta += phi, left to right: lane s ends with (((theta0 + phi_0) + phi_1) + ... + phi_s); untaken and idle lanes add
      // an exact zero (rows_theta_chain_dpp: the phis cross the row's lanes as 64-bit DPP broadcasts, no LDS)
      const double th = rows_theta_chain_dpp(cth, phi);
      const double myth = (rl == 15) ? cth : th;  // lane 15: the pass-entry angle
      double sn, cs;
      auvp_sincos_sk(myth, &sn, &cs);
      double dx = zero, dy = zero, mv = zero, dt = zero;
      {
        const uint32_t below = tmask & ((1u << rl) - 1u);
        const int prev = below ? (31 - __clz((int)below)) : 15;
        const double so = row_read_f64(sn, rowbase + prev), co = row_read_f64(cs, rowbase + prev);
        if (taken) {
          dx = radius * (sn - so);
          dy = radius * (-cs + co);
          mv = auvp_sqrt_plain(dx * dx + dy * dy);
          dt = auvp_div_plain(mv, vt);
        }
      }
      // x += dx; y += dy; t += dt; length += movement: four serial chains per row, lanes 0..3, 18-double rows in LDS (entry 15
      // of a row only fills the last 16-byte pair: rows_sums_chain never adds it, so nobody sets it)
      if (rl < 15) { inc[rl] = dx; inc[18 + rl] = dy; inc[36 + rl] = dt; inc[54 + rl] = mv; }
      wave_sync();
      const double acc = rows_sums_chain(inc, rl, on, rl == 0 ? cx : (rl == 1 ? cy : (rl == 2 ? ctt : clen)));
      // the row's state after this pass = the prefix values of its last sub-arc = where the five chains ended (idle lanes added
      // -0.0): lanes 0 .. 3's sums and lane 14's angle, already in registers -- no LDS read, no ds_bpermute
      // (rows_pass_ends_dpp; rows that are not `on` did not run the four chains and added fifteen times -0.0 to their angle:
      // what they get is the state they had)
      rows_pass_ends_dpp(acc, th, cx, cy, ctt, clen, cth);
      wave_sync();
      double mx = 0.0, my = 0.0, mt_ = 0.0, ml = 0.0;
      if (active) { mx = inc[rl]; my = inc[18 + rl]; mt_ = inc[36 + rl]; ml = inc[54 + rl]; }
      const bool app = taken && (mv >= Q.min_dist);
      const uint32_t amask = row_ballot(app, rowbase);
      const int napp = __popc(amask);
      if (on && (n_points + cnt + napp > capp)) { status = -2; live = false; iters_run = it; }
      const bool wr = app && live;
      if (wr) {
        const int rank = __popc(amask & ((1u << rl) - 1u));
        const size_t gi = (size_t)(n_points + cnt + rank);  // speculative: committed only if the node is accepted
        double* ra = ptF + gi * 3;                       // x, y, traj_t: what the leaf pass reads
        double* rb = ptF + (size_t)capp * 3 + gi * 3;    // theta, v, length
        // (92 GB per launch that this kernel never reads back: non-temporal stores, -0.3 %)
        typedef double nt_f64x2 __attribute__((ext_vector_type(2)));
        nt_f64x2 va, vb; va.x = mx; va.y = my; vb.x = myth; vb.y = vt;
        __builtin_nontemporal_store(va, reinterpret_cast<nt_f64x2*>(ra)); __builtin_nontemporal_store(mt_, ra + 2);
        __builtin_nontemporal_store(vb, reinterpret_cast<nt_f64x2*>(rb)); __builtin_nontemporal_store(ml, rb + 2);
      }
      ptx[pass] = mx; pty[pass] = my; ptv[pass] = wr;
      if (on) cnt += napp;
      ROWS_CONSUME(on && live, b0 + used);  // (a row that just failed keeps its stream position, like the one-episode kernel)
      first_pass = false;
      wave_sync();
    }
    // a steer without sub-arcs consumed only the selection and n_expand draws
    ROWS_CONSUME(live && n_total == 0, base);

    // ------------------------------------------------------------ check_collision (:530-549)
    // conservative cull: the square around the parent's end that holds every prefix position (half-width = the steer's
    // total movement) against each obstacle's bounding square; survivors get the exact test d2 <= T_i on every point
    const double reach = clen - clen0;
    const double bx0 = px0 - reach, by0 = py0 - reach, bx1 = px0 + reach, by1 = py0 + reach;
    const double slack = 0x1p-30 * (auvp_fabs(bx0) + auvp_fabs(bx1) + auvp_fabs(by0) + auvp_fabs(by1) + 1.0);
    const double hx = reach + slack;
    bool hit = false;
    // Two instances of the same loop, picked by a launch-uniform flag: where the host expects dense obstacles the cull goes
    // on with the tight box of the row's path points (and the parent's end) instead of the reach square -- the path
    // wanders inside a fraction of it, and an obstacle can only be hit if its bounding square meets that box.  The
    // sparse instance is the plain loop (the ~100 instructions of the tight box would cost more than they save there).
    // (the extent used by the boundary test below: the reach square, or the tight box once the dense instance has it)
    double ex0 = bx0, ey0 = by0, ex1 = bx1, ey1 = by1;
    auto cull_and_test = [&](auto tight_tag) {
      constexpr bool TIGHT = decltype(tight_tag)::value;
      const double hs = hx + slack;
      const bool slot_hit = live && !(sbox.z < px0 - hs || sbox.x > px0 + hs || sbox.w < py0 - hs || sbox.y > py0 + hs);
      uint32_t sm = row_ballot(slot_hit, rowbase);
      double tcx = px0, tcy = py0, thx = hx, thy = hx;
      if (TIGHT) {  // (dense worlds: nearly every steer has a slot within reach, and the boundary test profits as well)
        double mnx = px0, mxx = px0, mny = py0, mxy = py0;
#pragma unroll
        for (int q = 0; q < 2; q++) {
          if (ptv[q]) {
            mnx = __builtin_fmin(mnx, ptx[q]); mxx = __builtin_fmax(mxx, ptx[q]);
            mny = __builtin_fmin(mny, pty[q]); mxy = __builtin_fmax(mxy, pty[q]);
          }
        }
        mnx = row_min_f64(mnx); mxx = row_max_f64(mxx); mny = row_min_f64(mny); mxy = row_max_f64(mxy);
        const double ts = 0x1p-30 * (auvp_fabs(mnx) + auvp_fabs(mxx) + auvp_fabs(mny) + auvp_fabs(mxy) + 1.0);
        tcx = (mnx + mxx) * 0.5; tcy = (mny + mxy) * 0.5;
        thx = (mxx - mnx) * 0.5 + ts; thy = (mxy - mny) * 0.5 + ts;
        const bool tight = slot_hit && !(sbox.z < mnx - ts || sbox.x > mxx + ts || sbox.w < mny - ts || sbox.y > mxy + ts);
        sm = row_ballot(tight, rowbase);
        ex0 = mnx; ey0 = mny; ex1 = mxx; ey1 = mxy;
      }
      while (wave_any(sm != 0u)) {  // slots some row has to look into (none at all for most steers of a sparse world)
        const bool hs_ = sm != 0u;
        const int j0 = hs_ ? 16 * (__ffs((int)sm) - 1) : 0;
        sm &= sm - 1u;
        const int oi = j0 + rl;
        const double oxj = olx[oi], oyj = oly[oi], orj = (double)olr[oi];
#ifdef AUVP_ROWS_OST_LDS
        // EXPERIMENT ONLY (profiles/rows_trip_waits.md; never defined in the product build): a stand-in threshold from the LDS
        // tile -- NOT the obstacle's, the results are wrong -- to price a collision test without any vector-memory load
        const double otj = orj * orj;
#endif
        const bool cand = hs_ && (TIGHT ? !(auvp_fabs(oxj - tcx) > thx + orj || auvp_fabs(oyj - tcy) > thy + orj)
                                        : !(auvp_fabs(oxj - px0) > hx + orj || auvp_fabs(oyj - py0) > hx + orj));
        uint32_t cm = row_ballot(cand, rowbase);
        n_cand += __popc(cm);
        while (wave_any(cm != 0u)) {
          const bool has = cm != 0u;
          const int cl = has ? (__ffs((int)cm) - 1) : 0;
          cm &= cm - 1u;
          const double ox = row_read_f64(oxj, rowbase + cl), oy = row_read_f64(oyj, rowbase + cl);
#ifdef AUVP_ROWS_OST_LDS
          const double ot = row_read_f64(otj, rowbase + cl);
#else
          // the threshold of each row's candidate, obstacle j0 + cl (row-uniform, 0 .. 255 also for a row without one): four
          // scalar loads, each row keeps its own
          const int oc = j0 + cl;
          const unsigned long long hasm = __builtin_amdgcn_uicmp((unsigned)has, 0u, 33 /* != */);
          double ot = 0.0;
          int rowv = row;
          asm volatile("" : "+v"(rowv));
#pragma unroll
          for (int r = 0; r < RW_ROWS; r++)
            if (hasm & (1ull << (16 * r))) {
              const double t = ost_s[__builtin_amdgcn_readlane(oc, 16 * r)];
              ot = rowv == r ? t : ot;
            }
#endif
#pragma unroll
          for (int q = 0; q < 2; q++) {
            const double ddx = ptx[q] - ox, ddy = pty[q] - oy;
            hit |= has && ptv[q] && (ddx * ddx + ddy * ddy <= ot);
          }
          // the parent's end, path[0], is a path point too
          if (rl == 15) { const double ddx = px0 - ox, ddy = py0 - oy; hit |= has && (ddx * ddx + ddy * ddy <= ot); }
          // a row that has its collision is done with this slot's candidates (they are counted above already)
          if (row_ballot(hit, rowbase) != 0u) cm = 0u;
        }
      }
    };
    if (P.flags & AUVP_KFLAG_TIGHT_CULL) cull_and_test(std::true_type{});
    else cull_and_test(std::false_type{});
    // boundary: strictly inside an axis-aligned rectangle implies Point.within; otherwise the crossing test per point
    const double* sb = S.world->safe_box;
    // (the four bounds are read together and the compares joined without short circuits: as `a && b && ...` every bound was
    // an LDS read of its own behind the compare before it -- four round trips in a row, each with its lgkmcnt(0), in every trip:
    // profiles/rows_trip_lgkm.md.  Without a box the four values are whatever the table holds and the flag decides)
    const double sb0 = sb[0], sb1 = sb[1], sb2 = sb[2], sb3 = sb[3];
    const bool box_inside = (W.has_safe_box != 0) & (ex0 > sb0) & (ey0 > sb1) & (ex1 < sb2) & (ey1 < sb3);
    bool outside = false;
    if (wave_any(live && !box_inside)) {
      // lane = path point (two passes' points + the parent's end on lane 15); edges of the polygon one at a time
      auto crossing_outside = [&](double x, double y) {
        if (nv_poly <= 0) return true;
        int par_ = 0;
        for (int e = 0; e < nv_poly; e++) {
          const int ej = e == 0 ? nv_poly - 1 : e - 1;
          const double xi = S.poly[e][0], yi = S.poly[e][1], xj = S.poly[ej][0], yj = S.poly[ej][1];
          if ((yi > y) != (yj > y)) par_ ^= (x < (xj - xi) * (y - yi) / (yj - yi) + xi) ? 1 : 0;
        }
        return (par_ & 1) == 0;
      };
      const bool need = live && !box_inside;
#pragma unroll
      for (int q = 0; q < 2; q++)
        if (need && ptv[q]) outside |= crossing_outside(ptx[q], pty[q]);
      if (need && rl == 15) outside |= crossing_outside(px0, py0);
    }
    const bool bad = row_ballot(hit || outside, rowbase) != 0u;
    const bool ok = live && !bad;
    // ------------------------------------------------------------ accept (:144-151)
    if (ok && n_nodes >= capn) { status = -2; live = false; iters_run = it; }
    const bool acc_ = ok && live;
    const int me = n_nodes;
    if (acc_) {
      // curr_bin = (t // bin_interval + 1) * bin_interval, exact floor of the true quotient
      double q = auvp_floor(ctt * Q.inv_bin_interval);
      const double r = auvp_fma(-q, Q.bin_interval, ctt);
      if (r < 0.0) q -= 1.0;
      else if (r >= Q.bin_interval) q += 1.0;
      const double fi = q + 1.0;
      const double curr_bin = fi * Q.bin_interval;
      const bool over = curr_bin > Q.max_traj_time;
      bool stored = true;
      if (!over || fi <= (double)K) {
        const int bi = (int)fi;
        const int c = over ? 0 : (int)bin_count[bi];  // an overflowing regular key is reset first (:149-151)
        int32_t* slot = (c >= bcap || c >= 65535) ? nullptr : bin_slot_for_append(bins, bi, c, next_chunk, rl == 0);
        if (!slot) { status = -2; live = false; iters_run = it; stored = false; }
        else if (rl == 0) { *slot = me; bin_count[bi] = (uint16_t)(c + 1); }
      }
      if (stored) {
        if (rl == 0) {
          double* nf = nodeF + (size_t)me * 8;
          *reinterpret_cast<double2*>(nf) = make_double2(cx, cy);
          *reinterpret_cast<double2*>(nf + 2) = make_double2(cth, ctt);
          nf[4] = clen;
          nodeI[me] = make_int4(it, par, n_points, cnt);
          nodeQ[me] = ctt >= Q.max_traj_time - 30 ? 1 : 0;  // a qualifying leaf (:158); ranked by rrt_leaf_kernel
        }
        n_nodes++;
        n_points += cnt;
      }
    }
    wave_sync();
  }

  // ---- epilogue ----
  const bool valid = ep < n_episodes;
  if (live) iters_run = P.max_iter;
  // drawn: 32-bit outputs of the generator the episode consumed; after: the next random(), not consumed (parity probe)
#if AUVP_ROWS_BODY_STREAM
  const unsigned long long drawn = 2ull * rng.pos;  // (two per random())
  // a stream that ends exactly here has no next number: reported like any other end
  if (!stream_ensure<MIRROR>(rng, valid && status == 0, 1u, rl) && valid && status == 0) status = AUVP_ST_STREAM;
  const double after = status == AUVP_ST_STREAM ? 0.0 : stream_read(stream_base<MIRROR>(rng, 0u, rl), rl, rl);
#else
  const unsigned long long drawn = rng.drawn;
  rows_ensure(rng, valid, 2u, rl);
  const double after = rows_random_at(rng, 0u);
#endif
  if (valid) {
    for (int i = rl; i < K + 1; i += 16) B.bin_count[(size_t)ep * (K + 1) + i] = (int32_t)bin_count[i];
    if (rl == 0) {
      RrtSummary& s = B.summary[ep];
#if AUVP_ROWS_BODY_STREAM
      // (the host's "redo this batch" word.  Here, not in the block above: from there rrt_rows_kernel's schedule changed)
      pipe_report(B.pipe_fail, status == AUVP_ST_STREAM ? AUVP_ST_PIPELINE : 0);
#endif
      s.status = status; s.n_nodes = n_nodes; s.n_points = n_points; s.n_leaves = 0;
      s.best_leaf = -1; s.best_path_len = 0; s.iters_run = iters_run; s.n_candidates = n_cand;
      s.best_cost[0] = __builtin_inf(); s.best_cost[1] = 0.0; s.best_cost[2] = 0.0; s.best_cost[3] = 0.0;
      s.best_length = 0.0;
      s.rng_after = after; s.leaf_elems = 0; s.n_draw32 = drawn; s.nn_scanned = 0ull;
#if AUVP_ROWS_BODY_STREAM && defined(AUVP_STREAM_COUNT_SLOW)
      s.nn_scanned = rng.slow;  // EXPERIMENT ONLY (tools/stream_slow_probe.py): the field is unused in time-bin mode
#endif
    }
  }
#undef ROWS_CONSUME

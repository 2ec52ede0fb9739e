// rrt_explore_body.h -- the body of rrt_explore_kernel and rrt_explore_lim_kernel (rrt_explore_kernel.h), included inside
// both.  In scope: the kernel arguments W, P, B, n_episodes, max_pts, lim and the compile-time constants J, MODE, DIAG, LIM.
// (One text in two kernels, not a __device__ function: the function form changed rrt_explore_kernel's register allocation.)
// No include guard: the file is included once inside each of the two kernels, and nowhere else.
  extern __shared__ __align__(16) unsigned char smem[];
  const RrtTables S = rrt_tables_view(smem, W.n_habitats, W.n_poly);
  const int wave = uni((int)(threadIdx.x >> 6));  // wave-uniform: keeps every per-episode address scalar
  const int lane = lane_id();
  const int nfreq = (int)P.freq;
  const int xw = (int)(blockDim.x >> 6);  // episodes per workgroup (RRT_X_WAVES; fewer for batches that would leave CUs idle)
  const RrtLdsPlan plan = rrt_lds_plan(P.K, max_pts, nfreq, J * 64, rrt_tables_bytes(W.n_habitats, W.n_poly, W.n_bins), xw);
  const int C = plan.chunk;
  unsigned char* wbase = smem + plan.tables + (size_t)wave * plan.per_wave;
  double* scratch = reinterpret_cast<double*>(wbase);
  double* u_win = scratch;                         // [3C+3]      (steer, phase 1)
  double* inc = scratch;                           // [(C+1)*4]   (steer, phase 2: aliases u_win)
  double* sc = scratch + (size_t)4 * ((C + 2) & ~1);  // [(C+1)*2]
  double* phi_l = sc + (size_t)2 * ((C + 2) & ~1);    // [CS]
  uint32_t* mt = reinterpret_cast<uint32_t*>(wbase + plan.scratch);
  double(*pts)[2] = reinterpret_cast<double(*)[2]>(wbase + plan.scratch + plan.mt);
  int32_t* bin_count = reinterpret_cast<int32_t*>(wbase + plan.scratch + plan.mt + plan.pts);

  // ---- stage the shared world tables (whole workgroup) ----
  rrt_tables_stage(S, W);
  // The fp64 parameters are read from an LDS copy inside the expansion loop: as kernel arguments they sit in ~24
  // scalar registers for the whole loop, get spilled to vector-register lanes and cost a VALU instruction per
  // reload, whereas an LDS read feeds a vector operand directly (109 -> 92 spilled SGPRs, -4 % VALU instructions).
  if (threadIdx.x == 0) *S.params = P;
  const RrtParamsDev& Q = *S.params;
  // obstacles: SoA tile shared by the episodes of the workgroup, padded to J*64 (slot j, lane l =
  // obstacle j*64 + l); with the bounding-box cull most slots are only touched by 3 reads per expansion
  double* olx = reinterpret_cast<double*>(smem + plan.tables + (size_t)xw * plan.per_wave);
  double* oly = olx + J * 64;
  double* olt = oly + J * 64;
  // cull radius: >= sqrt(T) with margin, rounded up to a float (it only has to be conservative; 1 KB less LDS
  // at 256 obstacles); -inf where nothing can collide
  float* olr = reinterpret_cast<float*>(olt + J * 64);
  for (int i = threadIdx.x; i < J * 64; i += blockDim.x) {
    const bool ok = i < W.n_obstacles;
    const double t = ok ? W.ot[i] : -1.0;  // d2 >= 0 > -1: padding never collides
    olx[i] = ok ? W.ox[i] : 0.0;
    oly[i] = ok ? W.oy[i] : 0.0;
    olt[i] = t;
    const double rd = t >= 0.0 ? auvp_sqrt(t) * (1.0 + 0x1p-30) + 0x1p-40 : -__builtin_inf();
    float rf = (float)rd;
    if ((double)rf < rd) rf = __uint_as_float(__float_as_uint(rf) + 1u);  // rd > 0 here: the next float up
    olr[i] = rf;
  }
  __syncthreads();

  const int ep = (int)blockIdx.x * xw + wave;
  if (ep >= n_episodes) return;  // no workgroup barrier after this point

  // ---- per-episode views (scalar bases) ----
  const int capn = B.cap_nodes, capp = B.cap_points, bcap = B.bin_cap;
  double* nodeF = B.node_f + (size_t)ep * capn * 8;                       // [capn][8] x,y,theta,t,length
  int4* nodeI = reinterpret_cast<int4*>(B.node_i) + (size_t)ep * capn;    // plan_iter,parent,pt_off,pt_cnt
  uint8_t* nodeQ = B.node_q + (size_t)ep * capn;
  double2* nodeXY = MODE == 2 ? reinterpret_cast<double2*>(B.node_xy) + (size_t)ep * (size_t)B.xy_stride : nullptr;
  unsigned long long nn_scanned = 0ull;
  double* ptF = B.points + (size_t)ep * capp * 6;                         // [capp][3] x,y,t then [capp][3] theta,v,length
  const BinLists bins = bin_lists(B, (size_t)ep, P.K);
  int next_chunk = 0;
  const double* init = B.init + (size_t)ep * 6;
  const int K = LIM ? uni(lim[ep].K) : P.K;
  const double mtt_ep = LIM ? lim[ep].max_traj_time : 0.0;  // (LIM: the episode's horizon, read where the body reads Q's)
  const bool log_it = DIAG && (P.flags & 1) != 0;
  const size_t logb = (size_t)ep * P.max_iter;

  WaveRng rng;
  rng.s = mt;
  for (int i = lane; i < 624; i += 64) mt[i] = B.mt[(size_t)ep * 624 + i];
  {
    // words [idx, 624) of the incoming state are generated and unconsumed (CPython's index)
    int idx = B.mt_index ? uni(B.mt_index[ep]) : 624;
    idx = idx < 0 ? 0 : (idx > 624 ? 624 : idx);
    rng.pslot = idx == 624 ? 0u : (uint32_t)idx;
    rng.avail = (uint32_t)(624 - idx);
    rng.drawn = 0ull;
  }
  for (int i = lane; i < K + 2; i += 64) bin_count[i] = 0;
  wave_sync();

  if (MODE == 2) {  // the x,y mirror starts out as +inf everywhere (a scan block is always read whole)
    const double inf = __builtin_inf();
    for (long long i = lane; i < B.xy_stride; i += 64) nodeXY[i] = make_double2(inf, inf);
  }
  // mps_list = [initial]; time_bin[bin_interval].append(initial)  (:105,:114)
  if (lane == 0) {
    if (MODE == 2) nodeXY[0] = make_double2(init[0], init[1]);
    nodeF[0] = init[0]; nodeF[1] = init[1]; nodeF[2] = init[2]; nodeF[3] = init[3]; nodeF[4] = init[5];
    nodeI[0] = make_int4(0, -1, 0, 0);
    nodeQ[0] = 0;  // the start state is never a leaf candidate
    if (MODE == 0) { bins.direct[(K >= 1 ? 1 : 0) * AUVP_BIN_HEAD] = 0; bin_count[K >= 1 ? 1 : 0] = 1; }
  }
  wave_sync();
  int n_nodes = 1, n_points = 0, status = 0;
  int it = 0, n_cand = 0;  // n_cand: obstacles that survived the cull (exact tests run), whole episode
  // optional per-phase shader-clock accounting (AUVP_FLAG_PHASE_CLOCKS): select, steer, collision, accept
  const bool clk = DIAG && (P.flags & 4) != 0;
  unsigned long long tph[5] = {0, 0, 0, 0, 0}, t_prev = 0;
#define AUVP_PHASE(i) do { if (clk) { unsigned long long t_now = __builtin_amdgcn_s_memtime(); tph[i] += t_now - t_prev; t_prev = t_now; } } while (0)

  for (; it < P.max_iter; it++) {
    if (log_it && lane == 0) {
      B.it_parent[logb + it] = -1;
      B.it_accepted[logb + it] = 0;
      B.it_npath[logb + it] = 0;
    }
    // ------------------------------------------------------------ parent selection (:121-139)
    if (clk) t_prev = __builtin_amdgcn_s_memtime();
    int par = 0, par_v = 0;
    // The next 64 random() values of the stream are tempered in one pass (lane j holds number j);
    // the iteration's scalar draws are read out of that window and `base` counts how many of them
    // the selection + n_expand draws consumed.  The steer window continues in the same buffer.
    int base = 0;
    double u_me;
    if (MODE == 0) {
      int rb = 0, cnt = 0, f = -1;
      for (;;) {
        rng_ensure(rng, 128u);
        u_me = rng_random_at(rng, (uint32_t)lane);
        // ran_bin = int(uniform(1, K+1)) until that bin is non-empty (:123-125): every lane tries its
        // own draw, the first success in stream order wins; a key beyond K before it is a KeyError
        const int rbj = (int)py_uniform(1.0, (double)(K + 1), u_me);
        const bool cand = lane < 60;  // leave room for the two draws that follow the successful one
        const bool badkey = cand && rbj > K;
        const int cj = (cand && !badkey) ? bin_count[rbj] : 0;
        const unsigned long long okm = wave_ballot(cj != 0), badm = wave_ballot(badkey);
        const int fo = okm ? (__ffsll((long long)okm) - 1) : 64, fb = badm ? (__ffsll((long long)badm) - 1) : 64;
        if (fb < fo) { status = -5; break; }
        if (fo < 64) {
          f = fo;
          rb = __builtin_amdgcn_readlane(rbj, fo);
          cnt = __builtin_amdgcn_readlane(cj, fo);
          break;
        }
        rng_advance_words(rng, 120u);  // 60 unsuccessful draws (only while most bins are still empty)
      }
      if (uni(status)) break;  // (uni: the compiler cannot see that status is wave-uniform)
      const int ri = uni((int)py_uniform(0.0, (double)cnt, readlane_f64(u_me, f + 1)));
      par_v = bin_member(bins, rb, ri);  // every lane reads the same word; made uniform when the record is fetched
      base = uni(f + 2);
    } else if (MODE == 1) {
      double u = rng_next_random(rng);
      double ran_time = py_uniform(0.0, Q.max_plan_time * Q.freq, u);
      int lo = 0, hi = n_nodes;  // list slicing of get_closest_mps_time (:515-528)
      while (hi - lo > 3) {
        int n = hi - lo;
        double ld = auvp_fabs((double)nodeI[lo + n / 2 - 1].x - ran_time);
        double rd = auvp_fabs((double)nodeI[lo + n / 2 + 1].x - ran_time);
        if (ld >= rd) lo += n / 2; else hi = lo + n / 2;
        lo = uni(lo); hi = uni(hi);
      }
      par = lo;
      par_v = par;
      if (nodeF[(size_t)par * 8 + 3] > Q.max_traj_time) continue;
    } else {
      // get_random_mps (:333-343): x, y, theta, size draws; only x,y are used
      rng_ensure(rng, 8);
      double rx = py_uniform(W.bb[0], W.bb[2], rng_random_at(rng, 0));
      double ry = py_uniform(W.bb[1], W.bb[3], rng_random_at(rng, 1));
      rng_advance_words(rng, 8);
      // get_closest_mps (:505-513): first index with the smallest RN(sqrt(d2)), a streaming scan of the x,y mirror
      nn_scanned += (unsigned long long)n_nodes;
      par = nn_closest(nodeXY, n_nodes, readfirst_f64(rx), readfirst_f64(ry), (P.flags & AUVP_KFLAG_NN_EXACT) != 0);
      par_v = par;
      if (nodeF[(size_t)par * 8 + 3] > Q.max_traj_time) continue;
    }

    AUVP_PHASE(0);
    // ------------------------------------------------------------ steer (:252-295)
    // The parent's record is fetched as late as possible -- right before the first chunk's theta chain: the random
    // window, the "taken" predicate, the draw-offset fixed point and the arc radii need nothing of it, and run while the
    // parent's id and then its record are on their way from memory.
    double cx = 0.0, cy = 0.0, cth = 0.0, ctt = 0.0, clen = 0.0;
    double px0 = 0.0, py0 = 0.0, clen0 = 0.0;  // the parent's end: centre of the collision cull's box
    auto fetch_parent = [&]() {
      par = uni(par_v);
      const double2 a = *reinterpret_cast<const double2*>(nodeF + (size_t)par * 8);
      const double2 b = *reinterpret_cast<const double2*>(nodeF + (size_t)par * 8 + 2);
      cx = readfirst_f64(a.x); cy = readfirst_f64(a.y); cth = readfirst_f64(b.x); ctt = readfirst_f64(b.y);
      clen = readfirst_f64(nodeF[(size_t)par * 8 + 4]);
      px0 = cx; py0 = cy; clen0 = clen;
      if (lane == 0) { pts[0][0] = cx; pts[0][1] = cy; }
    };
    if (MODE != 0) {  // modes 1/2 consumed their selection draws one by one; open the window here
      rng_ensure(rng, 128u);
      u_me = rng_random_at(rng, (uint32_t)lane);
      base = 0;
    }
    const int n_total = uni((int)auvp_floor(py_uniform(0.0, Q.freq, readlane_f64(u_me, base)) / 1));
    base += 1;
    int cnt = 0;  // appended path points
    if (n_total == 0) fetch_parent();
    bool cap_err = false;
    for (int c0 = 0; c0 < n_total; c0 += C) {
      const int n = (n_total - c0) < C ? (n_total - c0) : C;
      const int nwin = 3 * n;
      // window entry j of this chunk = random() number base + j of the stream
      if (c0 == 0) {
        u_win[lane] = u_me;
        if (base + nwin > 64) {
          rng_ensure(rng, (uint32_t)(2 * (base + nwin)));
          for (int jj = 64 + lane; jj < base + nwin; jj += 64) u_win[jj] = rng_random_at(rng, (uint32_t)jj);
        }
      } else {
        base = 0;
        rng_ensure(rng, (uint32_t)(2 * nwin));
        for (int jj = lane; jj < nwin; jj += 64) u_win[jj] = rng_random_at(rng, (uint32_t)jj);
      }
      wave_sync();
      const double* uw = u_win + base;
      // "taken" predicate for every possible start offset
      unsigned long long msk[3] = {0ull, 0ull, 0ull};
#pragma unroll
      for (int t = 0; t < 3; t++) {
        if (64 * t + 1 < nwin) {  // wave-uniform: short steers need one pass only
          int jj = lane + 64 * t;
          bool f = false;
          if (jj + 1 < nwin) {
            double dist = py_uniform(0.0, Q.dist_to_end, uw[jj]);
            double diff = py_uniform(-Q.diff_max, Q.diff_max, uw[jj + 1]);
            f = auvp_fabs(dist) > auvp_fabs(diff);
          }
          msk[t] = wave_ballot(f);
        }
      }
      // Where does sub-arc s start?  pos_s = 2s + (#taken among sub-arcs < s).  Fixed point of
      //   taken_s = T[2s + c_s],  c_s = popcount(taken below s)
      // started from "everything taken"; sub-arcs 0..k are exact after k+1 rounds, and in practice
      // the loop ends after (number of untaken sub-arcs + 1) rounds.
      const bool active = lane < n;
      int cbelow = lane;
      unsigned long long tmask;
      // this lane only ever looks at bits 2*lane .. 3*lane of the 192-bit predicate: cut that window out once
      unsigned long long win;
      {
        const int sh = 2 * lane;
        const unsigned long long lo = sh < 64 ? msk[0] : msk[1], hi = sh < 64 ? msk[1] : msk[2];
        const int s6 = sh & 63;
        win = (lo >> s6) | ((hi << 1) << (63 - s6));
      }
      // (votes as ballots of ONE compare each, the lanes that take no part made neutral through their data: a vote on
      // `active && x` costs two more vector instructions on this chain -- a 0 / 1 and its compare with zero)
      {
        const unsigned long long win_a = active ? win : 0ull;  // bits 0 .. lane are looked at (a chunk has up to 63 sub-arcs)
        const unsigned long long below_me = active ? ((1ull << lane) - 1ull) : 0ull;
        cbelow = active ? lane : 0;
        for (;;) {
          tmask = __builtin_amdgcn_uicmp((uint32_t)(win_a >> cbelow) & 1u, 0u, 33 /* != */);
          const int cnew = __popcll(tmask & below_me);
          const unsigned long long chg = __builtin_amdgcn_uicmp((unsigned)cnew, (unsigned)cbelow, 33 /* != */);
          cbelow = cnew;
          if (chg == 0ull) break;
        }
      }
      const int mypos = 2 * lane + cbelow;
      const int used = 2 * n + __popcll(tmask);
      const bool taken = (tmask >> lane) & 1ull;
      double radius = 0.0, phi = 0.0, vt = 1.0;
      if (taken) {
        double dist = py_uniform(0.0, Q.dist_to_end, uw[mypos]);
        double diff = py_uniform(-Q.diff_max, Q.diff_max, uw[mypos + 1]);
        double s1 = dist + diff, s2 = dist - diff;
        radius = auvp_div_plain(s1 + s2, -s1 + s2);
        phi = auvp_div_plain(s1 + s2, 2 * radius);
        vt = py_uniform(0.0, 2 * Q.v, uw[mypos + 2]);
      }
      wave_sync();  // the window is dead: its LDS becomes the steer scratch
      if (c0 == 0) fetch_parent();
      const int CS = (C + 2) & ~1;  // chain-major: chain c owns inc[c*CS .. c*CS+C], 16-byte aligned rows
      if (lane < CS) phi_l[lane] = phi;  // untaken / idle lanes add an exact 0.0
      wave_sync();
      // theta += phi, left to right, by one lane; prefix angles written back in place
      if (lane == 0) {
        double th = cth;
#pragma unroll 2
        for (int s = 0; s < n; s += 2) {  // two steps per 16-byte access; entries past n hold exact zeros
          double2 v = *reinterpret_cast<double2*>(phi_l + s);
          th = th + v.x; v.x = th;
          th = th + v.y; v.y = th;
          *reinterpret_cast<double2*>(phi_l + s) = v;
        }
      }
      wave_sync();
      const double myth = active ? phi_l[lane] : cth;  // idle lanes evaluate the chunk-entry angle
      double sn, cs;
      auvp_sincos_sk(myth, &sn, &cs);
      if (lane <= C) { sc[2 * lane] = sn; sc[2 * lane + 1] = cs; }
      wave_sync();
      double dx = 0.0, dy = 0.0, mv = 0.0, dt = 0.0;
      if (taken) {
        unsigned long long below = tmask & ((1ull << lane) - 1ull);
        int prev = below ? (63 - __clzll((long long)below)) : C;  // lane C is idle: entry angle
        double so = sc[2 * prev], co = sc[2 * prev + 1];
        dx = radius * (sn - so);
        dy = radius * (-cs + co);
        mv = auvp_sqrt_plain(dx * dx + dy * dy);
        dt = auvp_div_plain(mv, vt);
      }
      if (active) { inc[lane] = dx; inc[CS + lane] = dy; inc[2 * CS + lane] = dt; inc[3 * CS + lane] = mv; }
      else if (lane < CS) { inc[lane] = 0.0; inc[CS + lane] = 0.0; inc[2 * CS + lane] = 0.0; inc[3 * CS + lane] = 0.0; }
      wave_sync();
      // x += dx; y += dy; t += dt; length += movement: four serial chains, one lane each
      if (lane < 4) {
        double acc = lane == 0 ? cx : (lane == 1 ? cy : (lane == 2 ? ctt : clen));
        double* row = inc + lane * CS;
#pragma unroll 2
        for (int s = 0; s < n; s += 2) {  // two steps per 16-byte access (the row is zero past n: adding 0.0 changes nothing)
          double2 v = *reinterpret_cast<double2*>(row + s);
          acc = acc + v.x; v.x = acc;
          acc = acc + v.y; v.y = acc;
          *reinterpret_cast<double2*>(row + s) = v;
        }
      }
      wave_sync();
      double mx = 0.0, my = 0.0, mt_ = 0.0, ml = 0.0;
      if (active) { mx = inc[lane]; my = inc[CS + lane]; mt_ = inc[2 * CS + lane]; ml = inc[3 * CS + lane]; }
      const bool app = taken && (mv >= Q.min_dist);
      const unsigned long long amask = wave_ballot(app);
      const int napp = __popcll(amask);
      if (n_points + cnt + napp > capp || cnt + napp + 1 > max_pts) { cap_err = true; break; }
      if (app) {
        int rank = __popcll(amask & ((1ull << lane) - 1ull));
        size_t gi = (size_t)(n_points + cnt + rank);  // speculative: committed only if the node is accepted
        // two 24-byte records per path point (auvp_types.h): what the leaf pass reads, and the rest
        double* ra = ptF + gi * 3;
        double* rb = ptF + (size_t)capp * 3 + gi * 3;
        *reinterpret_cast<double2*>(ra) = make_double2(mx, my); ra[2] = mt_;
        *reinterpret_cast<double2*>(rb) = make_double2(myth, vt); rb[2] = ml;
        pts[cnt + rank + 1][0] = mx;
        pts[cnt + rank + 1][1] = my;
      }
      cnt += napp;
      if (n > 0) {
        cx = readlane_f64(mx, n - 1); cy = readlane_f64(my, n - 1);
        ctt = readlane_f64(mt_, n - 1); clen = readlane_f64(ml, n - 1);
        cth = readlane_f64(myth, n - 1);
      }
      rng_advance_words(rng, (uint32_t)(2 * (base + used)));
      wave_sync();
    }
    if (n_total == 0) {
      rng_advance_words(rng, (uint32_t)(2 * base));  // selection + n_expand draws only
    }
    if (cap_err) { status = -2; break; }
    wave_sync();
    const int P_n = cnt + 1;

    AUVP_PHASE(1);
    // ------------------------------------------------------------ check_collision (:530-549)
    // Exact cull first: an obstacle whose effective disc does not reach the bounding box of the
    // path cannot be within T_i of any path point (a point in the box is at least as far from the
    // centre as the box is), so a slot of 64 obstacles with no candidate is skipped as a whole.
    // The cull only has to be conservative (a candidate slot runs the exact test below): the obstacle's
    // bounding square of half-width olr >= sqrt(T_i) against the box around its centre, both inflated by
    // 2^-30 relative -- eight orders of magnitude above any rounding in these few operations.
    // The box: every prefix position of the steer lies within the steer's total movement (the growth of the
    // length chain, which adds every sub-arc's chord) of the parent's end -- a square around the parent.  Looser than
    // the exact extent, but at these obstacle densities it still leaves well under one candidate per expansion, and
    // it costs nothing to maintain (tracking min/max in the serial chains was 30 instructions per expansion).
    const double reach = clen - clen0;
    const double bx0 = px0 - reach, by0 = py0 - reach, bx1 = px0 + reach, by1 = py0 + reach;
    double cxm = px0, cym = py0;
    const double slack = 0x1p-30 * (auvp_fabs(bx0) + auvp_fabs(bx1) + auvp_fabs(by0) + auvp_fabs(by1) + 1.0);
    double hx = reach + slack, hy = reach + slack;
    // lane = path point (the usual steer has < 64 of them): the few obstacles that survive the cull are tested one
    // at a time against every point at once, read back from the tile with a wave-uniform address
    int hit = 0;
    const bool pv0 = lane < P_n;
    double2 q0 = make_double2(0.0, 0.0);
    if (pv0) q0 = *reinterpret_cast<const double2*>(&pts[lane][0]);
    // Where the host expects dense obstacles (AUVP_KFLAG_TIGHT_CULL, set at launch) the cull box is the tight box of the
    // path points themselves (the parent's end is pts[0]): four wave reductions, far fewer exact tests
    if ((P.flags & AUVP_KFLAG_TIGHT_CULL) && P_n <= 64) {
      const double inf = __builtin_inf();
      const double mnx = wave_min_f64(pv0 ? q0.x : inf), mxx = wave_max_f64(pv0 ? q0.x : -inf);
      const double mny = wave_min_f64(pv0 ? q0.y : inf), mxy = wave_max_f64(pv0 ? q0.y : -inf);
      const double ts = 0x1p-30 * (auvp_fabs(mnx) + auvp_fabs(mxx) + auvp_fabs(mny) + auvp_fabs(mxy) + 1.0);
      cxm = (mnx + mxx) * 0.5; cym = (mny + mxy) * 0.5;
      hx = (mxx - mnx) * 0.5 + ts; hy = (mxy - mny) * 0.5 + ts;
    }
#pragma unroll
    for (int j = 0; j < J; j++) {
      const double oxj = olx[j * 64 + lane], oyj = oly[j * 64 + lane], orj = (double)olr[j * 64 + lane];
      const bool cand = !(auvp_fabs(oxj - cxm) > hx + orj || auvp_fabs(oyj - cym) > hy + orj);
      unsigned long long cm = wave_ballot(cand);
      n_cand += __popcll(cm);
      while (cm) {
        const int idx = uni(j * 64 + (__ffsll((long long)cm) - 1));
        cm &= cm - 1ull;
        const double ox = olx[idx], oy = oly[idx], ot = olt[idx];
        {
          const double ddx = q0.x - ox, ddy = q0.y - oy;
          const double d2 = ddx * ddx + ddy * ddy;
          hit |= (pv0 && d2 <= ot) ? 1 : 0;
        }
        for (int p = 64 + lane; p < P_n; p += 64) {  // only steers with freq > 63
          const double2 q = *reinterpret_cast<const double2*>(&pts[p][0]);
          const double ddx = q.x - ox, ddy = q.y - oy;
          const double d2 = ddx * ddx + ddy * ddy;
          hit |= (d2 <= ot) ? 1 : 0;
        }
      }
    }
    // polygon: when the path's bounding box lies strictly inside an axis-aligned rectangular boundary
    // every point is strictly inside it and the crossing test would say so too; skip it then
    const double* sb = S.world->safe_box;  // the LDS copy: four doubles less held in scalar registers
    const bool box_inside = W.has_safe_box && bx0 > sb[0] && by0 > sb[1] && bx1 < sb[2] && by1 < sb[3];
    const bool ok = !wave_any(hit != 0) && (box_inside || !any_point_outside(S.poly, W.n_poly, pts, P_n));
    if (log_it && lane == 0) {
      B.it_parent[logb + it] = par;
      B.it_accepted[logb + it] = ok ? 1 : 0;
      B.it_npath[logb + it] = P_n;
    }
    AUVP_PHASE(2);
    if (!ok) continue;
    if (n_nodes >= capn) { status = -2; break; }

    // ------------------------------------------------------------ accept (:144-151)
    const int me = n_nodes;
    if (lane == 0) nodeI[me] = make_int4(it, par, n_points, cnt);
    if (MODE == 0) {
      // curr_bin = (t // bin_interval + 1) * bin_interval, exact floor of the true quotient
      double q = auvp_floor(ctt * Q.inv_bin_interval);  // within one of the true floor; the remainder below settles it
      double r = auvp_fma(-q, Q.bin_interval, ctt);
      if (r < 0.0) q -= 1.0;
      else if (r >= Q.bin_interval) q += 1.0;
      double fi = q + 1.0;
      double curr_bin = fi * Q.bin_interval;
      bool over = curr_bin > (LIM ? mtt_ep : Q.max_traj_time);
      if (!over || fi <= (double)K) {
        int bi = uni((int)fi);
        int c = over ? 0 : uni(bin_count[bi]);  // an overflowing regular key is reset first (:149-151)
        if (c >= bcap) { status = -2; break; }
        int32_t* slot = bin_slot_for_append(bins, bi, c, next_chunk, lane == 0);
        if (!slot) { status = -2; break; }
        if (lane == 0) { *slot = me; bin_count[bi] = c + 1; }
      }
      wave_sync();
    }

    if (lane == 0) {
      double* nf = nodeF + (size_t)me * 8;
      *reinterpret_cast<double2*>(nf) = make_double2(cx, cy);
      *reinterpret_cast<double2*>(nf + 2) = make_double2(cth, ctt);
      nf[4] = clen;
      if (MODE == 2) nodeXY[me] = make_double2(cx, cy);
      nodeQ[me] = ctt >= (LIM ? mtt_ep : Q.max_traj_time) - 30 ? 1 : 0;  // a qualifying leaf (:158); ranked by rrt_leaf_kernel
    }
    n_nodes++;
    n_points += cnt;
    AUVP_PHASE(3);
  }

  if (clk && lane == 0 && B.phase_clocks) {
    for (int i = 0; i < 5; i++) B.phase_clocks[(size_t)ep * 5 + i] = tph[i];
  }
  const unsigned long long drawn = rng.drawn;
  double after = rng_next_random(rng);
  for (int i = lane; i < K + 1; i += 64) B.bin_count[(size_t)ep * ((LIM ? P.K : K) + 1) + i] = bin_count[i];  // (stride: the cap's)
  if (lane == 0) {
    // the tree is complete; rrt_leaf_kernel ranks its qualifying leaves and fills in the rest of the record
    RrtSummary& s = B.summary[ep];
    s.status = status; s.n_nodes = n_nodes; s.n_points = n_points; s.n_leaves = 0;
    s.best_leaf = -1; s.best_path_len = 0; s.iters_run = it; s.n_candidates = n_cand;
    s.best_cost[0] = __builtin_inf(); s.best_cost[1] = 0.0; s.best_cost[2] = 0.0; s.best_cost[3] = 0.0;
    s.best_length = 0.0;
    s.rng_after = after; s.leaf_elems = 0; s.n_draw32 = drawn; s.nn_scanned = nn_scanned;
  }

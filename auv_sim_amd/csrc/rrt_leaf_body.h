// rrt_leaf_body.h -- the body of rrt_leaf_kernel and rrt_leaf_lim_kernel (rrt_explore_kernel.h), included inside both, and of
// rrt_leaf_grid_kernel (leaf_grid_kernels.hip), which defines AUVP_LEAF_GRID around its include and brings set_of and sets.
// In scope: the kernel arguments W, P, B, n_episodes, mark_words, lim and the compile-time constant LIM.
// (One text in three kernels, not a __device__ function: the function form changed rrt_leaf_kernel's register allocation.)
// No include guard: the file is included once inside each of the kernels, and nowhere else.
  __shared__ __align__(16) unsigned char tables[RRT_WORLD_BYTES + RRT_MAX_HAB * 32 + RRT_MAX_POLY * 16 + RRT_MAX_BINS * 16];
  __shared__ double w_term[RRT_LEAF_WAVES][64];
  __shared__ double w_S[RRT_LEAF_WAVES][64];
  __shared__ int32_t w_hits[RRT_LEAF_WAVES][64], w_elems[RRT_LEAF_WAVES][64], w_par[RRT_LEAF_WAVES][64], w_off[RRT_LEAF_WAVES][64];
  __shared__ int32_t w_cpos[RRT_LEAF_WAVES][64], w_ids[RRT_LEAF_WAVES][128];
  __shared__ unsigned long long w_vis[RRT_LEAF_WAVES][64];
  __shared__ __align__(16) uint8_t w_owner[RRT_LEAF_WAVES][2048];  // owner lane of every point of the pass in flight (re-summation: 256 doubles)
  extern __shared__ __align__(16) unsigned char leaf_dyn[];
  const RrtTables St = rrt_tables_view(tables, W.n_habitats, W.n_poly);
  const int wave = uni((int)(threadIdx.x >> 6));
  const int lane = lane_id();
  rrt_tables_stage(St, W);
  const double* grid_lds = nullptr;
  if (rrt_leaf_grid_lds_bytes(W.sg_enabled, W.sg_ncol, W.sg_nrow)) {
    double* g = reinterpret_cast<double*>(leaf_dyn);
    for (int i = threadIdx.x; i < W.sg_ncol; i += blockDim.x) { g[i] = W.sg_x1[i]; g[W.sg_ncol + i] = W.sg_x0[i]; }
    for (int i = threadIdx.x; i < W.sg_nrow; i += blockDim.x) { g[2 * W.sg_ncol + i] = W.sg_y1[i]; g[2 * W.sg_ncol + W.sg_nrow + i] = W.sg_y0[i]; }
    grid_lds = g;
  }
  __syncthreads();
  const int ep = (int)blockIdx.x * RRT_LEAF_WAVES + wave;
  if (ep >= n_episodes) return;  // no workgroup barrier after this point
#ifdef AUVP_LEAF_GRID
  {
    // rrt_leaf_grid_kernel only (the other two kernels never see these lines): the episode's own probability table and the two
    // constants of the error bound that belong to it, swapped into the by-value copy of the world.  The record is fetched at a
    // wave-uniform address and every word goes through readfirstlane: the table's base stays in scalar registers.
    const RrtProbSetDev* rec = sets + uni(set_of[ep]);
    const unsigned long long pb = reinterpret_cast<unsigned long long>(rec->prob);
    W.prob = reinterpret_cast<const double*>(((unsigned long long)(uint32_t)uni((int)(uint32_t)(pb >> 32)) << 32) |
                                             (unsigned long long)(uint32_t)uni((int)(uint32_t)(pb & 0xffffffffull)));
    W.prob_absmax = readfirst_f64(rec->absmax);
    W.prob_one_sign = uni(rec->one_sign);
  }
#endif
  uint32_t* mark = mark_words > 0 ? reinterpret_cast<uint32_t*>(leaf_dyn + rrt_leaf_grid_lds_bytes(W.sg_enabled, W.sg_ncol, W.sg_nrow)) +
                                        (size_t)wave * mark_words
                                  : nullptr;
  double* term = w_term[wave];
  double* c_S = w_S[wave];
  int32_t *c_hits = w_hits[wave], *c_elems = w_elems[wave], *c_par = w_par[wave], *c_off = w_off[wave];
  int32_t *c_cpos = w_cpos[wave], *c_ids = w_ids[wave];
  unsigned long long* c_vis = w_vis[wave];
  uint8_t* c_owner = w_owner[wave];
  const double (*s_bins)[2] = St.bins;
  RrtSummary& sum = B.summary[ep];
  const int status_in = sum.status;
  if (status_in < 0) return;  // the expansion failed: nothing to rank
  const int capn = B.cap_nodes;
  const size_t capp = (size_t)B.cap_points;
  double* nodeF = B.node_f + (size_t)ep * capn * 8;
  const int4* nodeI = reinterpret_cast<const int4*>(B.node_i) + (size_t)ep * capn;
  // the running sums of a node as one 32-byte record {S, hits | elements, visited mask, -}: a child fetches its parent's
  // sums with one read
  double4* nodeC = reinterpret_cast<double4*>(B.node_c) + (size_t)ep * capn;
  const double* ptF = B.points + (size_t)ep * capp * 6;
  const int n_nodes = sum.n_nodes;
  const bool log_leaf = (P.flags & 2) != 0 && B.leaf_cost != nullptr;
  const double init_t = B.init[(size_t)ep * 6 + 3];
  const double w1 = P.w[0], w2 = P.w[1], w3 = P.w[2];
  const double thresh = (LIM ? lim[ep].max_traj_time : P.max_traj_time) - 30;
  const unsigned long long keep = LIM ? lim[ep].keep : ~0ull;
  const double term_max = auvp_fabs(w3) * W.prob_absmax;  // |shark term of one element| <= this
  const bool w2_int = (w2 == auvp_rint(w2) && auvp_fabs(w2) < 1048576.0);
  const int H = LIM ? __popcll(keep) : W.n_habitats;
  wave_sync();

  // cost[0], cost[1] and the scaled shark term of a leaf, given the ordered or unordered sum `c2num`
  auto total_of = [&](int hits, unsigned long long vis, double ctt, double c2num, double& c0, double& c1, double& c2) {
    c0 = 0.0; c1 = 0.0; c2 = c2num;
    // exact: equals `hits` successive rounded additions of an integer weight to 0.0 -- whose sum without a hit, or of a weight
    // of -0.0, is +0.0 and not the product's -0.0: hence the addition to 0.0
    if (w2_int) c1 = 0.0 + w2 * (double)hits;
    else for (int h = 0; h < hits; h++) c1 = c1 + w2;
    if (ctt > 0) { c1 = c1 / ctt; c2 = c2 / ctt; }
    if (H != 0) c0 = w1 * (double)__popcll(vis) / (double)H;
    return ((0.0 + c0) + c1) + c2;
  };

  int n_leaves = 0, best_leaf = -1, best_L = 0;
  long long leaf_elems = 0;
  int st_nodes = 0, st_points = 0, st_resummed = 0, st_releaves = 0;  // RrtBuffers::leaf_stats (wave-uniform: scalar registers)
  double best_tot = __builtin_inf(), best_c0 = 0.0, best_c1 = 0.0, best_c2 = 0.0, best_len = 0.0;
  double min_hi = __builtin_inf();  // smallest upper bound among the qualifying leaves seen so far
  // ---------------------------------------------------------------- 0. which nodes matter
  // Only the qualifying leaves and their ancestors enter any cost (about a quarter of the bench's trees).  Backwards over
  // the nodes, 64 at a time: a node is marked if it qualifies (node_q, from the expansion) or a child marked it; it
  // marks its parent.  Children come after their parents, so one backward sweep settles every mark; parents inside the
  // block in flight are reached by repeating until no lane changes.
  const uint8_t* nodeQ = B.node_q + (size_t)ep * capn;
  if (mark) {
    for (int i = lane; i < mark_words; i += 64) mark[i] = 0u;
    wave_sync();
    // (the parent link and the leaf flag of the NEXT block are requested before this block's rounds: every block was a full
    // memory round trip on its own -- ~150 of them per episode, one after the other)
    const int n_top = ((n_nodes - 1) >> 6) << 6;
    int par_nx = (n_top + lane < n_nodes) ? nodeI[n_top + lane].y : -1;
    uint8_t q_nx = (n_top + lane < n_nodes) ? nodeQ[n_top + lane] : (uint8_t)0;
    for (int n0 = n_top; n0 >= 0; n0 -= 64) {
      const int m = n0 + lane;
      const bool live = m < n_nodes;
      const int par = par_nx;
      const uint8_t q_me = q_nx;
      if (n0 >= 64) { par_nx = nodeI[m - 64].y; q_nx = nodeQ[m - 64]; }  // (blocks below the top one are full)
      bool need = live && m >= 1 && q_me != 0;
      bool pushed = false;
      for (;;) {
        need = need || (live && ((mark[m >> 5] >> (m & 31)) & 1u));
        const bool push = need && !pushed && par >= 0;
        if (push) { atomicOr(&mark[par >> 5], 1u << (par & 31)); pushed = true; }
        // another round only if some lane just marked a parent inside this block
        if (!wave_any(push && par >= n0)) break;
        wave_sync();
      }
      if (need) atomicOr(&mark[m >> 5], 1u << (m & 31));
      wave_sync();
    }
  }

  // ---------------------------------------------------------------- the sweep: marked nodes in creation order, 64 per pass
  int qn = 0, scan = 0;  // ids waiting in c_ids[0..qn); next block of nodes to look at
  for (;;) {
    while (qn < 64 && scan < n_nodes) {
      const int mm = scan + lane;
      const bool f = mm < n_nodes && (!mark || ((mark[mm >> 5] >> (mm & 31)) & 1u));
      const unsigned long long fm = wave_ballot(f);
      if (f) c_ids[qn + __popcll(fm & ((1ull << lane) - 1ull))] = mm;
      qn += __popcll(fm);
      scan += 64;
    }
    wave_sync();
    if (qn == 0) break;
    const int nlive = qn < 64 ? qn : 64;
    const bool live = lane < nlive;
    const int m = live ? c_ids[lane] : 0x7fffffff;
    const int first_id = __builtin_amdgcn_readfirstlane(m);
    int4 r = make_int4(0, -1, 0, 0);
    if (live) r = nodeI[m];
    // ---------------------------------------------------------------- 1. terms of the pass's path elements
    // the runs of the pass's nodes, packed: point slot j of the pass = point c_off[o] + (j - c_cpos[o]) of its owner o
    int incl = live ? r.w : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    const int cpos = incl - (live ? r.w : 0);
    const int n_slots = __builtin_amdgcn_readlane(incl, 63);
    st_nodes = uni(st_nodes + nlive); st_points = uni(st_points + n_slots);
    c_cpos[lane] = live ? cpos : 0x7fffffff;
    c_off[lane] = r.z;
    c_S[lane] = 0.0; c_hits[lane] = 0; c_vis[lane] = 0ull;
    // every node marks its own slots: owner[slot] = its lane (2048 slots here; the search below serves longer passes)
    const bool own_tab = n_slots <= 2048;
    if (own_tab && live)
      for (int k = 0; k < r.w; k++) c_owner[cpos + k] = (uint8_t)lane;
    wave_sync();
    // the node's own record and its parent's running sums are requested now; they are used after the point rounds
    double2 n_xy = make_double2(0.0, 0.0), n_tl = make_double2(0.0, 0.0);
    if (live) {
      n_xy = *reinterpret_cast<const double2*>(nodeF + (size_t)m * 8);
      n_tl = *reinterpret_cast<const double2*>(nodeF + (size_t)m * 8 + 3);  // traj_t, length (unaligned pair)
    }
    const bool par_before = live && r.y >= 0 && r.y < first_id;
    double4 par_rec = make_double4(0.0, 0.0, 0.0, 0.0);
    if (par_before) par_rec = nodeC[r.y];
    // Point rounds, two points per lane and round, software-pipelined: the records of round k + 1 are requested before
    // the terms of round k are evaluated.  owner = the node whose run holds the slot: from the table, or the last node
    // whose first slot is <= the slot (nodes without points share their successor's first slot and are skipped)
    struct Slot { bool v; int o; double2 xy; double t; };
    auto fetch = [&](int j) {
      Slot q;
      q.v = j < n_slots;
      q.o = 0;
      if (own_tab) q.o = q.v ? (int)c_owner[j] : 0;
      else {
#pragma unroll
        for (int st = 32; st >= 1; st >>= 1)
          if (q.o + st < 64 && c_cpos[q.o + st] <= j) q.o += st;
      }
      const int pidx = q.v ? c_off[q.o] + (j - c_cpos[q.o]) : 0;
      const double* rec = ptF + (size_t)pidx * 3;
      // (read once: non-temporal, so that the stream of point records does not push the probability table out of L2 -- 1-3 %)
      typedef double nt_f64x2 __attribute__((ext_vector_type(2)));
      const nt_f64x2 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f64x2*>(rec));
      q.xy = make_double2(v.x, v.y);
      q.t = __builtin_nontemporal_load(rec + 2);
      return q;
    };
    constexpr int NPL = AUVP_LEAF_NPL;  // points per lane and round
    Slot sn[NPL];
#pragma unroll
    for (int u = 0; u < NPL; u++) sn[u] = fetch(u * 64 + lane);
    for (int j0 = 0; j0 < n_slots; j0 += 64 * NPL) {
      Slot c[NPL];
#pragma unroll
      for (int u = 0; u < NPL; u++) c[u] = sn[u];
      if (j0 + 64 * NPL < n_slots) {
#pragma unroll
        for (int u = 0; u < NPL; u++) sn[u] = fetch(j0 + 64 * NPL + u * 64 + lane);
      }
      double tv[NPL];
      int hb[NPL];
      {
        // every element's index arithmetic first, then their dependent global reads (prob, habitat mask) back to back
        CostPre q[NPL];
        double pr[NPL];
        unsigned long long mk[NPL];
#pragma unroll
        for (int u = 0; u < NPL; u++) {
          q[u].tb = -1; q[u].c = -1; q[u].midx = -1;
          if (c[u].v) q[u] = cost_pre(W, St, 0, W.n_bins, c[u].xy.x, c[u].xy.y, c[u].t, grid_lds);
        }
#pragma unroll
        for (int u = 0; u < NPL; u++) {
          pr[u] = 0.0; mk[u] = 0ull;
          if (q[u].c >= 0) pr[u] = W.prob[(size_t)q[u].tb * W.n_cells + q[u].c];
          if (q[u].midx >= 0) mk[u] = W.hg_mask[q[u].midx];
        }
#pragma unroll
        for (int u = 0; u < NPL; u++) cost_post<LIM>(W, St, P.w[2], c[u].xy.x, c[u].xy.y, q[u], pr[u], mk[u], tv[u], hb[u], keep);
      }
#pragma unroll
      for (int u = 0; u < NPL; u++) {
        if (c[u].v) {
          if (tv[u] != 0.0) atomicAdd(&c_S[c[u].o], tv[u]);
          if (hb[u] >= 0) { atomicAdd(&c_hits[c[u].o], 1); atomicOr(&c_vis[c[u].o], 1ull << hb[u]); }
        }
      }
    }
    wave_sync();
    double own = c_S[lane], ntv = 0.0, ctt = 0.0, nlen = 0.0;
    int own_hits = c_hits[lane], nhab = -1;
    unsigned long long own_vis = c_vis[lane];
    if (live) {
      ctt = n_tl.x; nlen = n_tl.y;
      cost_element<LIM>(W, St, 0, W.n_bins, P.w[2], n_xy.x, n_xy.y, ctt, ntv, nhab, true, grid_lds, keep);
      own = own + ntv;
      if (nhab >= 0) { own_hits++; own_vis |= (1ull << nhab); }
    }
    // ---------------------------------------------------------------- 2. running sums down the tree
    // the parent's sums: from memory when it belongs to an earlier pass, else from the lanes of this one
    double pS = 0.0;
    int4 pc = make_int4(0, 0, 0, 0);
    unsigned long long pvis = 0ull;
    if (par_before) {
      const double4 pr = par_rec;
      pS = pr.x;
      const long long he = __double_as_longlong(pr.y);
      pc.x = (int)(he & 0xffffffffll); pc.y = (int)(he >> 32);
      pvis = (unsigned long long)__double_as_longlong(pr.z);
    }
    wave_sync();
    // a parent inside this pass: its lane = its position among the pass's ids (ascending; a marked node's parent is marked)
    int plane = 0;
    if (live && r.y >= first_id) {
#pragma unroll
      for (int st = 32; st >= 1; st >>= 1)
        if (plane + st < nlive && c_ids[plane + st] <= r.y) plane += st;
    }
    c_par[lane] = plane;
    c_S[lane] = pS + own; c_hits[lane] = pc.x + own_hits; c_elems[lane] = pc.y + r.w + 1; c_vis[lane] = pvis | own_vis;
    wave_sync();
    // parents inside this pass: a lane is ready once its parent's entry is final (a parent always has the smaller
    // index, so the lowest pending lane is ready in every round); all ready lanes add their parent's sums at once
    unsigned long long pending = wave_ballot(live && r.y >= first_id);
    while (pending) {
      const int p = c_par[lane];
      const bool mine = (pending >> lane) & 1ull;
      const bool ready = mine && !((pending >> (p & 63)) & 1ull);
      double aS = 0.0;
      int aH = 0, aE = 0;
      unsigned long long aV = 0ull;
      if (ready) { aS = c_S[p]; aH = c_hits[p]; aE = c_elems[p]; aV = c_vis[p]; }
      wave_sync();
      if (ready) { c_S[lane] = aS + c_S[lane]; c_hits[lane] += aH; c_elems[lane] += aE; c_vis[lane] |= aV; }
      wave_sync();
      pending &= ~wave_ballot(ready);
    }
    const double S = c_S[lane];
    const int hits = c_hits[lane], elems = c_elems[lane];
    const unsigned long long vis = c_vis[lane];
    if (live) {
      *reinterpret_cast<double2*>(nodeF + (size_t)m * 8 + 6) = make_double2(ntv, (double)nhab);
      nodeC[m] = make_double4(S, __longlong_as_double(((long long)elems << 32) | (long long)(uint32_t)hits),
                              __longlong_as_double((long long)vis), 0.0);
    }
    // later passes (parents) and the re-summation below read these back: make the stores visible to the wave first
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    wave_sync();
    // ---------------------------------------------------------------- 3. ranking of the pass's qualifying leaves
    bool q = false;
    double lo = __builtin_inf(), hi = __builtin_inf();
    if (live && m >= 1) {  // node 0 is the start state: never a leaf candidate (:144-171)
      q = ctt >= thresh;
      if (q) {
        double c0, c1, c2;
        const double tot = total_of(hits, vis, ctt, S, c0, c1, c2);
        // |S - ordered sum| <= 2 gamma_L L term_max; one more rounding each for the division and the two additions
        const double L = (double)elems;
        const double gam = 2.0 * (L + 2.0) * 0x1p-53;
        // sum|term| <= L term_max; with probabilities of one sign also sum|term| = |exact sum| <= |S| / (1 - gamma_L).
        // The second bound is what separates exact ties: a path without any shark term has S = 0 = the reference's sum.
        double mag = L * term_max;
        if (W.prob_one_sign) { const double ms = auvp_fabs(S) * (1.0 + 0x1p-20); mag = ms < mag ? ms : mag; }
        double e2 = 2.0 * gam * mag;
        if (ctt > 0) e2 = e2 / ctt;
        // e2 == 0: the sums are the same number, and so is everything computed from them
        const double err = e2 == 0.0 ? 0.0 : 1.25 * e2 + 0x1p-50 * (auvp_fabs(c0) + auvp_fabs(c1) + auvp_fabs(c2) + e2);
        lo = tot - err; hi = tot + err;
        if (!(err == err) || !(tot == tot)) { lo = -__builtin_inf(); hi = __builtin_inf(); }  // nan: decide exactly
      }
    }
    const unsigned long long qm = wave_ballot(q);
    if (qm != 0ull) {
    n_leaves += __popcll(qm);
    // exclusive prefix minimum of hi over the lanes (creation order), seeded with the earlier passes
    double pm = hi;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double t = __shfl_up(pm, o, 64);
      if (lane >= o) pm = t < pm ? t : pm;
    }
    double before = __shfl_up(pm, 1, 64);
    if (lane == 0) before = __builtin_inf();
    before = before < min_hi ? before : min_hi;
    leaf_elems += q ? (long long)elems : 0ll;  // (per lane; summed over the wavefront once, where the record is written)
    const bool cand = q && (log_leaf || lo < before);
    unsigned long long cm = wave_ballot(cand);
    min_hi = readlane_f64(pm, 63) < min_hi ? readlane_f64(pm, 63) : min_hi;
    while (cm) {
      const int l = __ffsll((long long)cm) - 1;
      cm &= cm - 1ull;
      const int leaf = __builtin_amdgcn_readlane(m, l);
      const double lo_l = readlane_f64(lo, l);
      if (!log_leaf && !(lo_l < best_tot)) continue;  // an exact total found meanwhile already rules it out
      // ---- the reference's ordered sum: [leaf] + reversed(leaf.path[1:]) + [parent] + reversed(parent.path[1:]) ... root
      // In chunks of up to 64 chain nodes: (A) the parent links are walked on their own -- a chain of dependent reads,
      // nothing else waits on it -- and leave one descriptor per node in LDS (arrays of the pass that are dead by now);
      // (B) the chunk's elements -- a node's own term, then its points last to first -- are evaluated lane = element, every
      // lane busy, into an LDS buffer in the reference's order, RS_CAP at a time; (C) the buffer is summed left to right, one
      // rounded add per element.  The same terms in the same order as a walk that evaluates node after node.  (Built and
      // dropped: skip links -- every node record carrying its depth and its nearest ancestor at a depth that is a multiple of
      // 8, so that a chunk costs 8 + 8 dependent reads instead of 64 -- bit-identical and no faster: profiles/r5_leaf_pass.md.)
      constexpr int RS_CAP = 256;  // elements per window: the owner table's 2 048 bytes as doubles
      double* rs_buf = reinterpret_cast<double*>(c_owner);
      int32_t *d_off = c_off, *d_w = c_cpos, *d_pos = c_par;
      double* d_tv = term;
      double c2num = 0.0;
      int mm = leaf;
      while (mm >= 0) {
        // (A) descriptors
        int nh = 0, cnt = 0;
        while (nh < 64 && mm >= 0) {
          const int4 rr = nodeI[mm];
          const double tvn = nodeF[(size_t)mm * 8 + 6];
          const int par_m = uni(rr.y);
          const int w = par_m >= 0 ? uni(rr.w) : 0;  // the root has no path of its own
          if (lane == 0) { d_off[nh] = rr.z; d_w[nh] = w; d_pos[nh] = cnt; d_tv[nh] = tvn; }
          cnt += 1 + w; nh++;
          mm = par_m;
        }
        wave_sync();
        for (int e0 = 0; e0 < cnt; e0 += RS_CAP) {
          const int ne = (cnt - e0) < RS_CAP ? (cnt - e0) : RS_CAP;
          // (B) the window's elements, 64 per round
          for (int s0 = 0; s0 < ne; s0 += 64) {
            const int sl = e0 + s0 + lane;
            if (s0 + lane < ne) {
              int h = 0;
#pragma unroll
              for (int st = 32; st >= 1; st >>= 1)
                if (h + st < nh && d_pos[h + st] <= sl) h += st;
              const int k = sl - d_pos[h];
              double tv_e = 0.0;
              if (k == 0) tv_e = d_tv[h];  // the node's own state comes before the points that led to it
              else {                        // point w - k: last point first; the term is evaluated again from the record
                const double* rec = ptF + ((size_t)d_off[h] + (size_t)(d_w[h] - k)) * 3;
                const double2 xy = *reinterpret_cast<const double2*>(rec);
                int habp = -1;
                cost_element(W, St, 0, W.n_bins, P.w[2], xy.x, xy.y, rec[2], tv_e, habp, true, grid_lds);
              }
              rs_buf[s0 + lane] = tv_e;
            }
          }
          wave_sync();
          // (C) one rounded add per element, in order
          int i = 0;
          for (; i + 4 <= ne; i += 4) {
            const double2 a = *reinterpret_cast<const double2*>(rs_buf + i), b = *reinterpret_cast<const double2*>(rs_buf + i + 2);
            c2num = c2num + a.x; c2num = c2num + a.y; c2num = c2num + b.x; c2num = c2num + b.y;
          }
          for (; i < ne; i++) c2num = c2num + rs_buf[i];
          wave_sync();
        }
      }
      const int lhits = __builtin_amdgcn_readlane(hits, l), lelems = __builtin_amdgcn_readlane(elems, l);
      st_resummed = uni(st_resummed + lelems); st_releaves = uni(st_releaves + 1);
      const unsigned long long lvis = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(vis >> 32), l) << 32) |
                                      (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(vis & 0xffffffffull), l);
      const double lctt = readlane_f64(ctt, l), llen = readlane_f64(nlen, l);
      double c0, c1, c2;
      double tot = total_of(lhits, lvis, lctt, c2num, c0, c1, c2);
      tot = readfirst_f64(tot);
      if (log_leaf) {
        // position of this leaf among the qualifying ones = leaves before this pass + qualifying lanes below l
        const int pos = n_leaves - __popcll(qm) + __popcll(qm & ((1ull << l) - 1ull));
        if (pos < B.cap_leaves && lane == 0) {
          // number of shark-grid bins in the leaf's sub-dict (:160-165)
          int nsel = 0;
          for (int b = 0; b < W.n_bins; b++) {
            const double b0 = s_bins[b][0], b1 = s_bins[b][1];
            nsel += ((init_t >= b0 && init_t <= b1) || (b0 >= init_t && b1 <= lctt) || (lctt >= b0 && lctt <= b1)) ? 1 : 0;
          }
          double* lc = B.leaf_cost + ((size_t)ep * B.cap_leaves + pos) * 6;
          lc[0] = tot; lc[1] = c0; lc[2] = c1; lc[3] = c2; lc[4] = (double)lelems; lc[5] = (double)nsel;
          B.leaf_iter[(size_t)ep * B.cap_leaves + pos] = nodeI[leaf].x;
        }
      }
      if (tot < best_tot) {
        best_tot = tot; best_leaf = leaf; best_L = lelems;
        best_c0 = c0; best_c1 = c1; best_c2 = c2; best_len = llen;
      }
    }
    }  // qm
    // the ids of the pass are done: the rest of the queue moves to its front
    wave_sync();
    const int carry = (lane + 64 < qn) ? c_ids[lane + 64] : 0;
    wave_sync();
    if (lane + 64 < qn) c_ids[lane] = carry;
    qn = qn > 64 ? qn - 64 : 0;
    wave_sync();
  }
  {
    // (leaf_elems was kept per lane)
    long long el = leaf_elems;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) el += __shfl_xor(el, o, 64);
    leaf_elems = el;
  }
  if (lane == 0) {
    if (B.leaf_stats) {
      atomicAdd(&B.leaf_stats[0], (unsigned long long)st_nodes); atomicAdd(&B.leaf_stats[1], (unsigned long long)st_points);
      atomicAdd(&B.leaf_stats[2], (unsigned long long)st_resummed); atomicAdd(&B.leaf_stats[3], (unsigned long long)st_releaves);
      // [4]: the most 32-bit outputs one episode of the batch drew -- what the host sizes the next batch's pre-generated
      // random stream from (auvplan.hip: option ROWS_STREAM)
      atomicMax(&B.leaf_stats[4], (unsigned long long)sum.n_draw32);
    }
    sum.n_leaves = n_leaves;
    sum.leaf_elems = leaf_elems;
    sum.best_leaf = best_leaf;
    sum.best_path_len = best_L;
    if (best_leaf >= 0) {
      sum.best_cost[0] = best_tot; sum.best_cost[1] = best_c0; sum.best_cost[2] = best_c1; sum.best_cost[3] = best_c2;
      sum.best_length = best_len;
    } else if (status_in == 0) {
      sum.status = 1;  // no qualifying leaf: opt_path stays None (:174)
    }
  }

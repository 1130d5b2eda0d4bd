// slack_kernels.h -- exact arc slack (the max-plus counterpart of the arc posteriors) and beam masks
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.7.
#pragma once

// One workgroup per lattice runs four phases, with a barrier between them (or one launch per phase: `phases`):
//   beta   max-plus sweep of the by-source tile program: beta*(s) = max over the out-arcs of c_a = e_a + (theta + beta*(dst))
//   gap    every canonical arc: gap_a = beta*(src) - c_a (+inf where c_a = -inf, 0 for a self loop), into the workspace
//   delta  min-plus sweep of the by-destination tile program: delta(d) = min over the in-arcs of delta(src) + gap_a
//   arcs   every canonical arc: slack_a = delta(src) + gap_a, keep_a = slack_a <= beam (and < +inf), the count of kept arcs, the rows
// max and min are exact, so the order in which a program presents a state's arcs -- pieces, carry records, partial
// groups and combine records of tree-summed states -- does not change a bit: every packing of a lattice gives the
// same results.  beta* and delta of all rows (scratch rows included) live in LDS, 4 bytes per row each, beside the
// label scores [V + 2] (the null label: -inf, the unit label of carry and combine records: 0).
constexpr int kSlkThreads = 1024;
constexpr int kSlkBeta = 1, kSlkGap = 2, kSlkDelta = 4, kSlkArcs = 8, kSlkAll = 15;
constexpr float kPosInf = __builtin_huge_valf();

// the caller's workspace (nfst_arc_slack_ws_bytes); the row arrays carry beta* and delta from launch to launch when
// the phases run as separate launches
struct SlkWs {
  float *gap;  // [total_arcs]
  float *vb;   // [total_rows] beta*
  float *dl;   // [total_rows] delta
};
struct SlkOut {
  const float *beam;  // [B] or null
  float *best, *vbeta, *state_slack, *slack;
  uint8_t *keep;
  int32_t *n_kept;
};

// c_a with the adds of nfst_kbest, in its order (e_a: Extra::at)
__device__ __forceinline__ float slk_cand(float e, float th, float vd) { return e + (th + vd); }

template <bool kMax>
__device__ __forceinline__ float slk_pick(float a, float b) { return kMax ? fmaxf(a, b) : fminf(a, b); }

// One sweep of a general tile program through the reader of tile_pipeline.h: wave 0 runs the tiles, waves 1 .. 3 pull
// what it will read -- program words, the slot -> arc map and the per-arc values gathered through it -- into the L2
// cache; the other waves go straight to the barrier that follows.
//   kBeta:  val = beta* rows, a slot's candidate is e_a + (tl[label] + val[operand]), a state takes the maximum;
//           arc_x / arc_y are the per-arc extras (arc_w, arc_scores; either may be null)
//   !kBeta: val = delta rows, a slot's candidate is val[operand] + gap_a (0 for a unit-label record, +inf for an empty
//           slot), a state takes the minimum; arc_x is the gap array
// A lane's slots beyond U repeat its last slot (tile_load_arcs): a repeated candidate changes no max or min.
template <bool kBeta>
__device__ __forceinline__ void slk_sweep(const uint32_t *prog, const int32_t *perm, int F, int tiles, int V, float *val,
                                          const float *tl, int *progress, const float *arc_x, const float *arc_y, int wv,
                                          int lane, float *keep_alive) {
  const int U = fmt_u(F), ST = fmt_words(F);
  const Extra ex = {arc_x, arc_y};
  const bool gather = kBeta ? ex.any() : true;
  if (wv > 3) return;
  if (wv > 0) {
    float sink_f = 0.0f;
    int sink_i = 0;
    const int prog_lines = (ST * 4 + 127) / 128, perm_lines = (64 * U * 4 + 127) / 128;
    for (int T = wv - 1; T < tiles; T += 3) {
      while (T > lds_flag_load(progress) + kTileAhead) __builtin_amdgcn_s_sleep(8);
      if (lane < prog_lines) sink_i += (int)prog[(size_t)T * ST + min(lane * 32, ST - 1)];
      if (!gather) {
        if (lane < perm_lines) sink_i += perm[(size_t)T * 64 * U + min(lane * 32, 64 * U - 1)];
      } else {
        for (int j = 0; j < U; ++j) {
          const int ca = perm[(size_t)T * 64 * U + lane * U + j];
          if (ca >= 0) {
            if (arc_x) sink_f += arc_x[ca];
            if (arc_y) sink_f += arc_y[ca];
          }
        }
      }
    }
    if (sink_f == 1.2345e-33f && sink_i == 0x12345678) *keep_alive = 0.0f;  // keeps the loads alive, never true
    return;
  }
  auto sweep = [&](auto compact_tag, auto gather_tag) {
    constexpr bool kCompact = decltype(compact_tag)::value, kGather = decltype(gather_tag)::value;
    auto load_tile = [&](int T, ArcTile &t) { tile_load_arcs<kCompact>(prog, perm, U, ST, T, lane, t); };
    auto step = [&](const ArcTile &cur) {
      const uint32_t ctl = cur.p.ctl();
      uint32_t rcs[4];
      tile_records<kCompact>(cur.p, rcs);
      float xs[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // the per-arc value of the slot: e_a, or gap_a
        const int ca = cur.cas[j];
        if (kBeta) {
          xs[j] = 0.0f;
          if (kGather && ca >= 0) xs[j] = ex.at(ca);
        } else {
          xs[j] = ((int)rec32_label(rcs[j]) == V + 1) ? 0.0f : kPosInf;
          if (ca >= 0) xs[j] = arc_x[ca];
        }
      }
      float acc = kBeta ? kNegInf : kPosInf;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // straight-line: every slot reads its operand (an empty slot has operand 0 and the null label)
        const float o = val[rec32_state(rcs[j])];
        const float c = kBeta ? slk_cand(xs[j], tl[rec32_label(rcs[j])], o) : o + xs[j];
        acc = slk_pick<kBeta>(acc, c);
      }
      // segmented max (kBeta) or min over the state's 2^g lanes
      acc = seg_reduce<6>(acc, (int)ctl_g(ctl), (int)ctl_gmax(__builtin_amdgcn_readfirstlane(ctl)),
                          [](float a, float o) { return slk_pick<kBeta>(a, o); });
      if (ctl_leader(ctl)) val[ctl_state(ctl)] = acc;
    };
    tile_run<ArcTile>(tiles, progress, load_tile, step);
  };
  if (F == kFmtCompact) { if (gather) sweep(std::true_type{}, std::true_type{}); else sweep(std::true_type{}, std::false_type{}); }
  else { if (gather) sweep(std::false_type{}, std::true_type{}); else sweep(std::false_type{}, std::false_type{}); }
}

// LDS: beta* [max_rows] | delta [max_rows] | label scores [V + 2] | progress, kept
__global__ __launch_bounds__(kSlkThreads) void k_arc_slack(nfst_batch lat, nfst_scores sc, SlkWs w, int phases, SlkOut o) {
  extern __shared__ float slk_lds[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Meta m = load_meta(lat.meta, b);
  const int V = lat.vocab, NR = lat.max_rows;
  float *v = slk_lds, *d = v + NR, *tl = d + NR;
  int *progress = (int *)(tl + V + 2), *kept = progress + 1;
  const float *tg = sc.theta + (size_t)sc.theta_stride * b;
  const float *arc_w = lat.weighted ? lat.arc_w : nullptr;
  float *vb = w.vb + m.row_off, *dl = w.dl + m.row_off;

  for (int i = tid; i < V + 2; i += kSlkThreads) tl[i] = i < V ? tg[i] : (i == V ? kNegInf : 0.0f);
  for (int i = tid; i < NR; i += kSlkThreads) {  // (incl. scratch rows)
    v[i] = (phases & kSlkBeta) || i >= m.n_rows ? kNegInf : vb[i];
    d[i] = (phases & kSlkDelta) || i >= m.n_rows ? kPosInf : dl[i];
  }
  if (tid == 0) { *progress = 0; *kept = 0; }
  __syncthreads();

  if (phases & kSlkBeta) {
    if (tid == 0) v[m.sink] = 0.0f;
    __syncthreads();
    slk_sweep<true>(lat.bwd_stream + m.bwd_off, lat.bwd_perm + m.bwd_slot_off, m.bwd_u, m.bwd_tiles, V, v, tl, progress, arc_w,
                    sc.arc_scores, wv, lane, w.gap);
    __syncthreads();
    if (phases != kSlkAll)
      for (int i = tid; i < m.n_rows; i += kSlkThreads) vb[i] = v[i];
  }

  if (phases & kSlkGap) {
    for (int i = tid; i < m.n_arcs; i += kSlkThreads) {
      const int a = m.arc_off + i;
      const int s0 = lat.arc_src[a], d0 = lat.arc_dst[a];
      const float c = slk_cand(Extra{arc_w, sc.arc_scores}.at(a), tl[lat.arc_label[a]], v[d0]);
      // (a self loop lies on no path: gap 0, so that slack = delta(s) + gap serves every arc)
      w.gap[a] = (s0 == d0) ? 0.0f : (c > kNegInf ? v[s0] - c : kPosInf);
    }
    __syncthreads();  // (the gaps, written by this workgroup, are visible to its sweep)
  }

  if (phases & kSlkDelta) {
    if (tid == 0) { d[0] = (v[0] > kNegInf) ? 0.0f : kPosInf; *progress = 0; }
    __syncthreads();
    slk_sweep<false>(lat.fwd_stream + m.fwd_off, lat.fwd_perm + m.fwd_slot_off, m.fwd_u, m.fwd_tiles, V, d, tl, progress, w.gap,
                     nullptr, wv, lane, w.gap);
    __syncthreads();
    if (phases != kSlkAll)
      for (int i = tid; i < m.n_rows; i += kSlkThreads) dl[i] = d[i];
  }

  if (phases & kSlkArcs) {
    const float beam = o.beam ? o.beam[b] : 0.0f;
    int mine = 0;
    for (int base = 0; base < m.n_arcs; base += kSlkThreads) {  // (whole waves take every trip: the ballot below)
      const int i = base + tid;
      bool kp = false;
      if (i < m.n_arcs) {
        const int a = m.arc_off + i;
        const float sl = d[lat.arc_src[a]] + w.gap[a];
        o.slack[a] = sl;
        kp = (sl <= beam) & (sl < kPosInf);  // (an arc on no path of finite score is never kept, whatever the beam)
        if (o.keep) o.keep[a] = kp ? 1 : 0;
      }
      mine += __popcll(__builtin_amdgcn_ballot_w64(kp));
    }
    if (o.n_kept && lane == 0 && mine) atomicAdd(kept, mine);  // (an integer sum: the same whatever the order)
    for (int i = tid; i < m.n_rows; i += kSlkThreads) {
      // rows on no path of finite score: -inf / +inf, whether or not the programs hold them
      const float di = d[i];
      if (o.vbeta) o.vbeta[m.row_off + i] = di < kPosInf ? v[i] : kNegInf;
      if (o.state_slack) o.state_slack[m.row_off + i] = di;
    }
    if (tid == 0) o.best[b] = v[0];
    __syncthreads();
    if (o.n_kept && tid == 0) o.n_kept[b] = *kept;
  }
}

// expect_kernels.h -- forward-backward in the first-order expectation semiring: E[V] and Cov(1_a, V)
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md section 4.5.
#pragma once

// Per-arc value v_a = label_values[b, label] + arc_values[a] + coef * s_a (each term optional), s_a the arc's log
// weight as nfst_scores defines it.
struct ExpVals {
  nfst_scores sc;
  const float *lv;  // [V] (stride 0) or [B, stride]
  int64_t lv_stride;
  const float *av;  // [total_arcs] canonical order
  float coef;
};
// the caller's workspace (nfst_expectation_ws_bytes): slot-ordered arc data of both programs, then the row values of
// both directions (direction 0 = alpha, by destination; 1 = beta, by source)
struct ExpWs {
  double *wm;  // [fwd_slots + bwd_slots] weight of the slot's arc, mantissa (0: empty, carry and combine slots)
  int *we;     // [fwd_slots + bwd_slots] ... and exponent
  float *sv;   // [fwd_slots + bwd_slots] value of the slot's arc
  double *rm;  // [2, total_rows] mantissa of the path mass A
  double *rr;  // [2, total_rows] R = E[prefix (alpha) / suffix (beta) value | the row]
  int *re;     // [2, total_rows] exponent of A
  double *lc;  // [B, V] per-label sums of c_a (float64 atomics)
  unsigned long long *lp;  // [B, V] per-label sums of p_a in fixed point, units of 2^-kExpPostBits (integer atomics)
};
// Per-label sums of the posteriors are summed exactly, as integers: then their value does not depend on the order of
// the atomic adds, and two launches with the same posteriors give the same bits (KL(p||p) has a gradient of exactly 0).
// A posterior is at most 1 and a label's sum at most the length of a path (< 8192 = 2^13 rows): 2^(13 + 44) < 2^64.
// Rounding each p_a to 2^-44 costs < 3e-14 per arc.
constexpr int kExpPostBits = 44;

__device__ __forceinline__ double exp_arc_score(const nfst_batch &lat, const nfst_scores &sc, int b, int a, int l) {
  double s = (double)sc.theta[sc.theta_stride * b + l];
  if (lat.weighted) s += (double)lat.arc_w[a];
  if (sc.arc_scores) s += (double)sc.arc_scores[a];
  return s;
}
// The sweeps and the per-arc pass use the same float32 rounding of v_a, so that E[V | a] and E[V] agree.  An arc of
// weight zero (s below -9e7, exp_split64) has no value: coef * s would be -inf or NaN there.
__device__ __forceinline__ float exp_arc_value(const ExpVals &x, int b, int a, int l, double s) {
  double v = 0.0;
  if (x.lv) v += (double)x.lv[x.lv_stride * b + l];
  if (x.av) v += (double)x.av[a];
  if (x.coef != 0.0f && s > -9.0e7) v += (double)x.coef * s;
  return (float)v;
}

// Pass 1, grid (B, 2, kExpParts): the weight (float64 mantissa, exponent) and the value of every slot of a lattice's
// program, in slot order, so that the sweep streams them next to the program words instead of gathering per canonical
// arc and has no exp on its dependency chain.  kExpParts workgroups share a program (the gathers are latency-bound).
constexpr int kExpPrepThreads = 256, kExpParts = 16;
__global__ __launch_bounds__(kExpPrepThreads) void k_expect_prep(nfst_batch lat, ExpVals x, ExpWs w) {
  const int b = blockIdx.x, dir = blockIdx.y;
  const Meta m = load_meta(lat.meta, b);
  const int F = dir ? m.bwd_u : m.fwd_u, tiles = dir ? m.bwd_tiles : m.fwd_tiles;
  const int32_t *perm = dir ? lat.bwd_perm + m.bwd_slot_off : lat.fwd_perm + m.fwd_slot_off;
  const int64_t so = dir ? lat.fwd_slots + m.bwd_slot_off : (int64_t)m.fwd_slot_off;
  const int n = tiles * 64 * fmt_u(F);
  for (int i = blockIdx.z * kExpPrepThreads + threadIdx.x; i < n; i += kExpPrepThreads * kExpParts) {
    const int a = perm[i];
    ME64 wt = {0.0, kEZero};
    float v = 0.0f;
    if (a >= 0) {
      const int l = lat.arc_label[a];
      const double s = exp_arc_score(lat, x.sc, b, a, l);
      wt = exp_split64(s);
      v = exp_arc_value(x, b, a, l, s);
    }
    w.wm[so + i] = wt.m;
    w.we[so + i] = wt.e;
    w.sv[so + i] = v;
  }
}

// the two numerators of a row, reduced together; their partner in a stage of the ladder, member by member
struct ExpSums { double M, N; };
template <int S>
__device__ __forceinline__ ExpSums wave_partner(ExpSums x) { return {wave_partner<S>(x.M), wave_partner<S>(x.N)}; }

// Pass 2, grid (B, 2): one workgroup per lattice and direction sweeps the general tile program (the reader of
// tile_pipeline.h).  Per row it carries the path mass A as (float64 mantissa, int32 exponent) -- the precise
// flavour of DESIGN.md section 2, for every program -- and R = E[value of the path so far | the row] in float64:
//   A(row) = sum_in A(op) w_a,   R(row) = sum_in A(op) w_a (R(op) + v_a) / A(row).
// A tile's slots and the state's lanes reduce both numerators with one shared exponent; R is the ratio of the two
// sums, so it stays bounded whatever the path masses.  Carry records and the combine records of tree-summed states
// (unit label V + 1) have weight one and value zero: they pass the (A, R) of the row they read on unchanged.
// LDS: 20 bytes per row (16-byte (mantissa, R) record + exponent) + 16: max_rows <= 8191 in 160 KiB.
constexpr int kExpThreads = 256;
__global__ __launch_bounds__(kExpThreads) void k_expect_sweep(nfst_batch lat, ExpWs w) {
  extern __shared__ double2 exl[];
  const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Meta m = load_meta(lat.meta, b);
  double2 *mr = exl;                     // (mantissa of A, R)
  int *ex = (int *)(mr + lat.max_rows);  // exponent of A
  int *progress = ex + lat.max_rows;
  for (int i = tid; i < lat.max_rows; i += kExpThreads) {  // (incl. scratch rows)
    mr[i] = make_double2(0.0, 0.0);
    ex[i] = kEZero;
  }
  if (tid == 0) *progress = 0;
  __syncthreads();
  if (tid == 0) {
    mr[dir ? m.sink : 0] = make_double2(0.5, 0.0);  // A = 1, R = 0 at the start (alpha) / the sink (beta)
    ex[dir ? m.sink : 0] = 1;
  }
  __syncthreads();
  const int F = dir ? m.bwd_u : m.fwd_u, U = fmt_u(F), ST = fmt_words(F);
  const int tiles = dir ? m.bwd_tiles : m.fwd_tiles;
  const uint32_t *prog = dir ? lat.bwd_stream + m.bwd_off : lat.fwd_stream + m.fwd_off;
  const int64_t so = dir ? lat.fwd_slots + m.bwd_slot_off : (int64_t)m.fwd_slot_off;
  const double *wm = w.wm + so;
  const int *we = w.we + so;
  const float *sv = w.sv + so;
  const int V = lat.vocab;
  if (wv > 0) {
    // waves 1 .. 3 pull the tiles the sweep will read into the L2 cache, a bounded distance ahead of it
    int sink_i = 0;
    double sink_d = 0.0;
    const int prog_lines = (ST * 4 + 127) / 128, wm_lines = (64 * U * 8 + 127) / 128, sv_lines = (64 * U * 4 + 127) / 128;
    for (int T = wv - 1; T < tiles; T += kExpThreads / 64 - 1) {
      while (T > lds_flag_load(progress) + kTileAhead) __builtin_amdgcn_s_sleep(8);
      if (lane < prog_lines) sink_i += (int)prog[(size_t)T * ST + min(lane * 32, ST - 1)];
      if (lane < wm_lines) sink_d += wm[(size_t)T * 64 * U + min(lane * 16, 64 * U - 1)];
      if (lane < sv_lines) {
        sink_d += (double)sv[(size_t)T * 64 * U + min(lane * 32, 64 * U - 1)];
        sink_i += we[(size_t)T * 64 * U + min(lane * 32, 64 * U - 1)];
      }
    }
    if (sink_i == 0x12345678 && sink_d == 1.2345e-300) w.rr[0] = 0.0;  // keeps the loads alive, never true
  } else {
    struct ExpTile { TileWords p; double m[4]; int e[4]; float v[4]; };
    auto sweep = [&](auto compact_tag) {
      constexpr bool kCompact = decltype(compact_tag)::value;
      // (not tile_load_arcs: three slot arrays in slot order, 16-byte loads in the compact tile)
      auto load_tile = [&](int T, ExpTile &t) {
        const size_t sb = (size_t)T * 64 * U + (size_t)lane * U;
        if (kCompact) {  // control word + four 24-bit records per lane; four slots per lane (32 + 16 + 16 bytes, aligned)
          t.p.x = *reinterpret_cast<const uint4 *>(prog + (size_t)T * ST + lane * 4);
          const double2 m01 = *reinterpret_cast<const double2 *>(wm + sb), m23 = *reinterpret_cast<const double2 *>(wm + sb + 2);
          const int4 e4 = *reinterpret_cast<const int4 *>(we + sb);
          const float4 v4 = *reinterpret_cast<const float4 *>(sv + sb);
          t.m[0] = m01.x; t.m[1] = m01.y; t.m[2] = m23.x; t.m[3] = m23.y;
          t.e[0] = e4.x; t.e[1] = e4.y; t.e[2] = e4.z; t.e[3] = e4.w;
          t.v[0] = v4.x; t.v[1] = v4.y; t.v[2] = v4.z; t.v[3] = v4.w;
          return;
        }
        t.p.x.x = prog[(size_t)T * ST + lane];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int jj = min(j, U - 1);
          t.p.w[j] = prog[(size_t)T * ST + 64 + lane * U + jj];
          t.m[j] = wm[sb + jj];
          t.e[j] = we[sb + jj];
          t.v[j] = sv[sb + jj];
        }
      };
      auto step = [&](const ExpTile &cur) {
        const uint32_t ctl = cur.p.ctl();
        uint32_t rcs[4];
        tile_records<kCompact>(cur.p, rcs);
        double tm[4], tr[4];
        int te[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int other = (int)rec32_state(rcs[j]), l = (int)rec32_label(rcs[j]);
          ME64 wt = {cur.m[j], cur.e[j]};  // (empty slot: weight zero)
          double v = (double)cur.v[j];
          if (l == V + 1) { wt.m = 1.0; wt.e = 0; v = 0.0; }  // carry / combine record
          if (j >= U) wt.m = 0.0;
          const double2 o = mr[other];
          tm[j] = o.x * wt.m;
          te[j] = ex[other] + wt.e;
          tr[j] = (tm[j] != 0.0) ? tm[j] * (o.y + v) : 0.0;
        }
        const int E = max(max(te[0], te[1]), max(te[2], te[3]));
        const int gl = (int)ctl_g(ctl);
        const int gmax = (int)ctl_gmax(__builtin_amdgcn_readfirstlane(ctl));
        const int Eg = seg_reduce<6>(E, gl, gmax, OpMax{});
        ExpSums s = {0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s.M += __builtin_amdgcn_ldexp(tm[j], te[j] - Eg);
          s.N += __builtin_amdgcn_ldexp(tr[j], te[j] - Eg);
        }
        seg_ladder<6>(s, gl, gmax, [](ExpSums &x, const ExpSums &o, bool take) {
          x.M = take ? x.M + o.M : x.M;
          x.N = take ? x.N + o.N : x.N;
        });
        if (ctl_leader(ctl)) {
          const uint32_t sid = ctl_state(ctl);
          const Rec64 a = me_pack64(s.M, Eg);
          mr[sid] = make_double2(a.m, (s.M != 0.0) ? s.N / s.M : 0.0);
          ex[sid] = a.e;
        }
      };
      tile_run<ExpTile>(tiles, progress, load_tile, step);
    };
    if (F == kFmtCompact) sweep(std::true_type{});
    else sweep(std::false_type{});
  }
  __syncthreads();
  const int64_t ro = (int64_t)dir * lat.total_rows + m.row_off;
  for (int i = tid; i < m.n_rows; i += kExpThreads) {
    const double2 v = mr[i];
    w.rm[ro + i] = v.x;
    w.rr[ro + i] = v.y;
    w.re[ro + i] = ex[i];
  }
}

// Pass 3, grid (B, kExpParts): every canonical arc (arc_sd / arc_l16)
//   p_a = A_alpha(src) w_a A_beta(dst) / Z,  E[V | a] = R_alpha(src) + v_a + R_beta(dst),  c_a = p_a (E[V | a] - E[V]),
// E[V] = R_beta(start).  Self loops (the sink's pad loop) lie on no path: p = c = 0, as in nfst_forward_backward.
// Per-arc and per-lattice outputs are written once each (bit-identical across launches); the per-label sums are
// atomics into the workspace (exact integers for p, float64 for c), turned into float32 by k_expect_labels.
constexpr int kExpArcThreads = 256;
__global__ __launch_bounds__(kExpArcThreads) void k_expect_arcs(nfst_batch lat, ExpVals x, ExpWs w, double *logz64, double *ev64,
                                                                float *ev32, float *posterior, float *cov, bool want_lc,
                                                                bool want_lp) {
  const int b = blockIdx.x;
  const Meta m = load_meta(lat.meta, b);
  const int64_t TR = lat.total_rows;
  const double *am = w.rm + m.row_off, *ar = w.rr + m.row_off, *bm = w.rm + TR + m.row_off, *br = w.rr + TR + m.row_off;
  const int *ae = w.re + m.row_off, *be = w.re + TR + m.row_off;
  const double zm = bm[0], ev = br[0];
  const int ze = be[0];
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    logz64[b] = (zm > 0.0) ? log(zm) + (double)ze * 0.693147180559945309417232 : -__builtin_huge_val();
    ev64[b] = ev;
    if (ev32) ev32[b] = (float)ev;
#ifdef NFST_DEBUG_EXPECT
    // both directions compute E[V]: R_alpha(sink) == R_beta(start) up to rounding
    assert(!(zm > 0.0) || fabs(ar[m.sink] - ev) <= 1e-9 * (1.0 + fabs(ev)) + 1e-9);
#endif
  }
  const double rz = (zm > 0.0) ? 1.0 / zm : 0.0;
  const int V = lat.vocab;
  for (int i = blockIdx.y * kExpArcThreads + threadIdx.x; i < m.n_arcs; i += kExpArcThreads * kExpParts) {
    const int a = m.arc_off + i;
    const uint32_t sd = lat.arc_sd[a];
    const int s0 = (int)(sd & 0xffffu), d0 = (int)(sd >> 16), l = (int)lat.arc_l16[a];
    double p = 0.0, c = 0.0;
    if (s0 != d0) {
      const double s = exp_arc_score(lat, x.sc, b, a, l);
      const ME64 wt = exp_split64(s);
      const double pm = am[s0] * wt.m * bm[d0] * rz;
      if (pm != 0.0) {
        p = __builtin_amdgcn_ldexp(pm, ae[s0] + wt.e + be[d0] - ze);
        c = p * ((ar[s0] + (double)exp_arc_value(x, b, a, l, s) + br[d0]) - ev);
      }
    }
    if (posterior) posterior[a] = (float)p;
    if (cov) cov[a] = (float)c;
    if (want_lc && c != 0.0) atomicAdd(w.lc + (size_t)b * V + l, c);
    if (want_lp && p != 0.0)
      atomicAdd(w.lp + (size_t)b * V + l, (unsigned long long)llrint(__builtin_amdgcn_ldexp(p, kExpPostBits)));
  }
}

// Pass 4 (only when per-label sums are asked for): the workspace sums as float32 [B, V]
__global__ __launch_bounds__(256) void k_expect_labels(ExpWs w, int64_t n, float *label_cov, float *label_post) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (label_cov) label_cov[i] = (float)w.lc[i];
  if (label_post) label_post[i] = (float)__builtin_amdgcn_ldexp((double)w.lp[i], -kExpPostBits);
}

// positional_expect_kernels.h -- the first-order expectation semiring on the time-synchronous sweeps
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.13.
#pragma once

// k_positional_expect is k_positional in kPosModeAlpha with a second sum beside every path mass.  The arc at position t
// of a path carries
//     v_t(a) = pos_values[b, t, l] + label_values[b, l] + arc_values[a] + coef (s_a + pos[b, t, l])      (l = label_a)
// in float64.  Backwards in time every (t, s) keeps beta_t(s) and R_t(s) = E[value of the rest of the path | s at t];
// forwards alpha_t(s) and R^alpha_t(s) = E[value so far | s at t].  A step accumulates sum x and sum x (R(other) + v)
// under ONE exponent (section 4.5: two numerators under one shared exponent); R is their ratio.  The path mass goes
// through exactly the operations of PosSum::plus / combine / norm in the order of k_positional, and the numerator never
// enters it: log Z, pos_post and arc_post are the bits of nfst_positional.
// The per-arc part of v (arc_values + coef (arc_w + arc_scores)) is a double per arc in the workspace, the per-label part
// a double per label in the step's table.  A term whose weight mantissa is zero is skipped before its value is read.
struct PosExpVals {
  const float *pv;  // [T, V] (stride 0) or [B, T, V]
  int64_t pv_stride;
  const float *lv;  // [V] (stride 0) or [B, V]
  int64_t lv_stride;
  const float *av;  // [total_arcs]
  double coef;
};
struct PosExpWs {
  double *br;    // [(T + 1) * total_rows] R_t(s) beside the stored beta rows
  double *av;    // [total_arcs] the position-independent part of an arc's value (only read when the launch has one)
  double *acc2;  // [total_arcs] per in-entry: sum over t of c_{a,t}
};
struct PosExpOut {
  double *logz64;
  float *logz32;
  double *ev64;
  float *ev32;
  float *pos_post, *arc_post, *pos_cov, *arc_cov;
};

// PosSum::plus on the mass, and the numerator N kept under the mass's exponent
__device__ __forceinline__ void pos_exp_plus(ME64 &acc, double &N, ME64 x, double val) {
  if (x.e > acc.e) {
    acc.m = __builtin_amdgcn_ldexp(acc.m, acc.e - x.e);
    N = __builtin_amdgcn_ldexp(N, acc.e - x.e);
    acc.e = x.e;
  }
  const double xm = __builtin_amdgcn_ldexp(x.m, x.e - acc.e);
  acc.m += xm;
  N += xm * val;
}
// PosSum::combine on the mass; the numerators are aligned and added the same way (commutative: both partners agree)
__device__ __forceinline__ void pos_exp_combine(ME64 &acc, double &N, int o) {
  const double om = __shfl_xor(acc.m, o), oN = __shfl_xor(N, o);
  const int oe = __shfl_xor(acc.e, o);
  const int E = max(acc.e, oe);
  acc.m = __builtin_amdgcn_ldexp(acc.m, acc.e - E) + __builtin_amdgcn_ldexp(om, oe - E);
  N = __builtin_amdgcn_ldexp(N, acc.e - E) + __builtin_amdgcn_ldexp(oN, oe - E);
  acc.e = E;
}

// the label table of position t: the split weights by pos_fill_table<PosSum>, then the per-label part of the value
// (every thread reads back the entries it wrote itself: no barrier in between)
__device__ __forceinline__ void pos_exp_fill_table(const PosSum::Rows &tab, double *tv, const float *theta, const float *pos_t,
                                                   const float *lv, const float *pv_t, double coef, int V) {
  pos_fill_table<PosSum>(tab, theta, pos_t, V);
  for (int l = threadIdx.x; l < V; l += kPosThreads) {
    double v = 0.0;
    if (tab.m[l] != 0.0) {  // (a label of weight zero has no value: coef * s would be -inf or NaN there)
      if (pv_t) v += (double)pv_t[l];
      if (lv) v += (double)lv[l];
      if (coef != 0.0) v += coef * (pos_t ? (double)theta[l] + (double)pos_t[l] : (double)theta[l]);
    }
    tv[l] = v;
  }
}

// LDS: two rows of (float64 mass, float64 R, int32 exponent), the label table (float64 weight, float64 value, int32
// exponent), two label histograms (64-bit fixed point for p, float64 for p e) and one int per thread:
// 40 max_rows + 36 vocab + 4 kPosThreads bytes.  STAGED: + 4 (max_rows + 1) + 4 (arcs of the largest lattice) bytes.
template <bool EXTRA, bool STAGED>
__global__ __launch_bounds__(kPosThreads) void k_positional_expect(nfst_batch lat, PosIn in, PosExpVals x, PosWs w, PosExpWs xw,
                                                                   PosExpOut o) {
  extern __shared__ double pos_lds[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const Meta m = load_meta(lat.meta, b);
  const int R = lat.max_rows, V = lat.vocab, T = in.T, n = m.n_rows;
  double *vm = pos_lds, *vr = vm + 2 * R, *tm = vr + 2 * R, *tv = tm + V;
  unsigned long long *hist = (unsigned long long *)(tv + V);
  double *hcov = (double *)(hist + V);
  int *ve = (int *)(hcov + V), *te = ve + 2 * R, *scan = te + V;
  int *rp_l = scan + kPosThreads;
  uint32_t *recs = (uint32_t *)(rp_l + R + 1);
  typedef typename std::conditional<STAGED, PosArcsLds, PosArcsGlobal>::type Arcs;
  const PosSum::Rows val = {vm, ve}, tab = {tm, te};
  const float *theta = in.sc.theta + (size_t)in.sc.theta_stride * b;
  const float *pos_b = in.pos ? in.pos + (size_t)in.pos_stride * b : nullptr;
  const float *pv_b = x.pv ? x.pv + (size_t)x.pv_stride * b : nullptr;
  const float *lv_b = x.lv ? x.lv + (size_t)x.lv_stride * b : nullptr;
  const bool by_step = pos_b != nullptr || pv_b != nullptr;  // the table changes from position to position
  const bool arc_val = x.av != nullptr || (EXTRA && x.coef != 0.0);
  const int G = pos_group(m);
  const int slots = kPosThreads / G, slot = tid / G, gl = tid % G;

  // ---- once per launch: the weights and values of the per-arc terms, the arcs by (destination, canonical arc) -----
  if (EXTRA || arc_val) {
    for (int a = m.arc_off + tid; a < m.arc_off + m.n_arcs; a += kPosThreads) {
      double e = 0.0, v = 0.0;
      if (EXTRA) {
        if (lat.weighted) e += (double)lat.arc_w[a];
        if (in.sc.arc_scores) e += (double)in.sc.arc_scores[a];
        const ME64 ew = exp_split64(e);
        w.ewm[a] = ew.m;
        w.ewe[a] = ew.e;
        if (x.coef != 0.0 && ew.m != 0.0) v = x.coef * e;
      }
      if (x.av) v += (double)x.av[a];
      if (arc_val) xw.av[a] = v;
    }
  }
  // without any of the four optional outputs there is no forward pass: no by-destination order, no stored rows
  const bool need_alpha = o.pos_post || o.arc_post || o.pos_cov || o.arc_cov;
  int *in_ptr = w.in_ptr + m.row_off + b;
  if (need_alpha) {
    pos_in_order(lat, m, (int *)vm, scan, in_ptr, w);
    for (int i = tid; i < m.n_arcs; i += kPosThreads) xw.acc2[m.arc_off + i] = 0.0;
  }

  // ---- backwards in time ----------------------------------------------------------------------------------------
  const size_t ro = (size_t)(T + 1) * m.row_off;
  double *sbm = w.bm + ro, *sbr = xw.br + ro;
  int *sbe = w.be + ro;
  auto ext = [&](int a, ME64 y) -> ME64 {
    if (EXTRA) { y.m *= w.ewm[a]; y.e += w.ewe[a]; }
    return y;
  };
  Arcs out_arcs;
  if constexpr (STAGED) {
    pos_stage_out(lat, m, b, rp_l, recs);  // (the pass begins with a barrier)
    out_arcs = {rp_l, recs, m.arc_off};
  } else {
    out_arcs = {lat.row_ptr + m.row_off + b, lat.arc_dst, lat.arc_label, m.arc_off, m.arc_off + m.n_arcs};
  }
  for (int i = tid; i < n; i += kPosThreads) {
    const ME64 v = i == m.sink ? PosSum::one() : PosSum::zero();
    val.set((T & 1) * R + i, v);
    vr[(T & 1) * R + i] = 0.0;
    if (need_alpha) {
      sbm[(size_t)T * n + i] = v.m;
      sbe[(size_t)T * n + i] = v.e;
      sbr[(size_t)T * n + i] = 0.0;
    }
  }
  if (!by_step) pos_exp_fill_table(tab, tv, theta, nullptr, lv_b, nullptr, x.coef, V);
  for (int t = T - 1; t >= 0; --t) {
    if (by_step)
      pos_exp_fill_table(tab, tv, theta, pos_b ? pos_b + (size_t)t * V : nullptr, lv_b, pv_b ? pv_b + (size_t)t * V : nullptr, x.coef, V);
    __syncthreads();  // the table and the row of position t + 1 are complete
    const int nxt = ((t + 1) & 1) * R, cur = (t & 1) * R;
    for (int base = 0; base < n; base += slots) {
      const int s = base + slot;
      const bool act = s < n && s != m.sink;
      const int a0 = act ? out_arcs.lo(s) : 0, a1 = act ? out_arcs.hi(s) : 0;
      ME64 acc = PosSum::zero();
      double N = 0.0;
      for (int a = a0 + gl; a < a1; a += G) {
        const uint32_t rec = out_arcs.rec(a);
        const int d = (int)(rec & 0xffffu), l = (int)(rec >> 16);
        if (d == s) continue;  // self loops are on no path
        const ME64 y = ext(a, PosSum::times(tab.get(l), val.get(nxt + d)));
        if (y.m != 0.0) pos_exp_plus(acc, N, y, vr[nxt + d] + tv[l] + (arc_val ? xw.av[a] : 0.0));
      }
      for (int og = 1; og < G; og <<= 1) pos_exp_combine(acc, N, og);
      if (gl == 0 && s < n) {
        const bool sink = s == m.sink;
        const ME64 v = sink ? PosSum::one() : PosSum::norm(acc);
        const double r = (!sink && acc.m != 0.0) ? N / acc.m : 0.0;
        val.set(cur + s, v);
        vr[cur + s] = r;
        if (need_alpha) {
          sbm[(size_t)t * n + s] = v.m;
          sbe[(size_t)t * n + s] = v.e;
          sbr[(size_t)t * n + s] = r;
        }
      }
    }
    __syncthreads();  // (the next step overwrites the table and the row of position t + 1)
  }
  const ME64 z = val.get(0);  // beta_0(0) is in row 0 of the pair (position 0)
  const double ev = z.m > 0.0 ? vr[0] : 0.0;
  const double logz = z.m > 0.0 ? log(z.m) + (double)z.e * 0.693147180559945309417232 : -__builtin_huge_val();
  if (tid == 0) {
    o.logz64[b] = logz;
    if (o.logz32) o.logz32[b] = (float)logz;
    o.ev64[b] = ev;
    if (o.ev32) o.ev32[b] = (float)ev;
  }
  if (!need_alpha) return;
  __syncthreads();  // (everyone has read beta_0(0) and R_0(0))

  // ---- forwards in time -------------------------------------------------------------------------------------------
  const double rz = z.m > 0.0 ? 1.0 / z.m : 0.0;
  const bool want_p = o.pos_post != nullptr || o.arc_post != nullptr, want_c = o.pos_cov != nullptr || o.arc_cov != nullptr;
  for (int i = tid; i < n; i += kPosThreads) {
    val.set(i, i == 0 ? PosSum::one() : PosSum::zero());
    vr[i] = 0.0;
  }
  for (int l = tid; l < V; l += kPosThreads) {
    hist[l] = 0ull;
    hcov[l] = 0.0;
  }
  const int2 *in_rec = w.in_rec + m.arc_off;
  double *acc_e = w.acc + m.arc_off, *acc_c = xw.acc2 + m.arc_off;
  if constexpr (STAGED) {  // the same LDS, now by destination: (src | label << 16) of every in-entry
    const int n_in = in_ptr[n];
    for (int d = tid; d <= n; d += kPosThreads) rp_l[d] = in_ptr[d];
    for (int j = tid; j < n_in; j += kPosThreads) recs[j] = (uint32_t)in_rec[j].y;
  }
  for (int t = 0; t < T; ++t) {
    if (by_step)
      pos_exp_fill_table(tab, tv, theta, pos_b ? pos_b + (size_t)t * V : nullptr, lv_b, pv_b ? pv_b + (size_t)t * V : nullptr, x.coef, V);
    __syncthreads();
    const int cur = (t & 1) * R, nxt = ((t + 1) & 1) * R;
    const double *brm = sbm + (size_t)(t + 1) * n, *brr = sbr + (size_t)(t + 1) * n;
    const int *bre = sbe + (size_t)(t + 1) * n;
    for (int base = 0; base < n; base += slots) {
      const int d = base + slot;
      const bool act = d < n;
      const int j0 = act ? (STAGED ? rp_l[d] : in_ptr[d]) : 0, j1 = act ? (STAGED ? rp_l[d + 1] : in_ptr[d + 1]) : 0;
      const double bmd = act ? brm[d] * rz : 0.0;
      const int bed = act ? bre[d] - z.e : 0;
      const double rest = act ? brr[d] - ev : 0.0;  // R_{t+1}(d) - E[V]
      ME64 acc = PosSum::zero();
      double N = 0.0;
      for (int j = j0 + gl; j < j1; j += G) {
        int2 rec;
        if (STAGED) {
          rec.y = (int)recs[j];
          rec.x = (EXTRA || arc_val) ? in_rec[j].x : 0;
        } else {
          rec = in_rec[j];
        }
        const int l = rec.y >> 16, s = rec.y & 0xffff;
        const ME64 y = ext(m.arc_off + rec.x, PosSum::times(tab.get(l), val.get(cur + s)));
        if (y.m == 0.0) continue;  // (PosSum::plus adds nothing either; the value is not read)
        const double sofar = vr[cur + s] + tv[l] + (arc_val ? xw.av[m.arc_off + rec.x] : 0.0);  // R^alpha_t(src) + v_t(a)
        pos_exp_plus(acc, N, y, sofar);
        const double pm = y.m * bmd;
        if (pm != 0.0) {
          const double p = __builtin_amdgcn_ldexp(pm, y.e + bed);
          if (want_p) {
            if (o.pos_post) atomicAdd(&hist[l], (unsigned long long)llrint(__builtin_amdgcn_ldexp(p, kPosPostBits)));
            if (o.arc_post) acc_e[j] += p;  // (entry j belongs to this lane at every step)
          }
          if (want_c) {
            const double c = p * (sofar + rest);
            if (o.pos_cov) atomicAdd(&hcov[l], c);  // (float64 LDS atomics: the order of the adds is not fixed)
            if (o.arc_cov) acc_c[j] += c;
          }
        }
      }
      for (int og = 1; og < G; og <<= 1) pos_exp_combine(acc, N, og);
      if (gl == 0 && act) {
        val.set(nxt + d, PosSum::norm(acc));
        vr[nxt + d] = acc.m != 0.0 ? N / acc.m : 0.0;
      }
    }
    __syncthreads();
    if (o.pos_post || o.pos_cov) {
      const size_t row = ((size_t)b * T + t) * V;
      for (int l = tid; l < V; l += kPosThreads) {
        if (o.pos_post) o.pos_post[row + l] = (float)__builtin_amdgcn_ldexp((double)hist[l], -kPosPostBits);
        if (o.pos_cov) o.pos_cov[row + l] = (float)hcov[l];
        hist[l] = 0ull;
        hcov[l] = 0.0;
      }
    }
  }
  if (o.arc_post || o.arc_cov) {
    for (int i = tid; i < m.n_arcs; i += kPosThreads)
      if (lat.arc_src[m.arc_off + i] == lat.arc_dst[m.arc_off + i]) {
        if (o.arc_post) o.arc_post[m.arc_off + i] = 0.0f;
        if (o.arc_cov) o.arc_cov[m.arc_off + i] = 0.0f;
      }
    const int n_in = in_ptr[n];
    for (int j = tid; j < n_in; j += kPosThreads) {
      if (o.arc_post) o.arc_post[m.arc_off + in_rec[j].x] = (float)acc_e[j];
      if (o.arc_cov) o.arc_cov[m.arc_off + in_rec[j].x] = (float)acc_c[j];
    }
  }
}

// positional_expect_kernels.h -- the first-order expectation semiring on the time-synchronous sweeps
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.13.
#pragma once

// k_positional_expect is k_positional in kPosModeAlpha with a second sum beside every path mass.  The arc at position t
// of a path carries
//     v_t(a) = pos_values[b, t, l] + label_values[b, l] + arc_values[a] + coef (s_a + pos[b, t, l])      (l = label_a)
// in float64.  Backwards in time every (t, s) keeps beta_t(s) and R_t(s) = E[value of the rest of the path | s at t];
// forwards alpha_t(s) and R^alpha_t(s) = E[value so far | s at t].  A step accumulates sum x and sum x (R(other) + v)
// under ONE exponent (section 4.5: two numerators under one shared exponent); R is their ratio.
// The kernel is pos_sum_sweep -- the body of k_positional, step loops included -- with PosExpRider: the path mass goes
// through the one PosSum::plus / combine / norm of those loops and the rider only follows its exponent, so log Z,
// pos_post and arc_post are the bits of nfst_positional by construction, not by two copies that agree.
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

// the per-label part of the value beside the label table of position t (every thread reads back the weights it wrote
// itself in pos_fill_table: no barrier in between)
__device__ __forceinline__ void pos_exp_fill_table(const PosSum::Rows &tab, double *tv, const float *theta, const float *pos_t,
                                                   const float *lv, const float *pv_t, double coef, int V) {
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

// The rider of the expectation sweep (PosNoRider documents the hooks): the numerator N of the lane's running sum, kept
// under the exponent of the mass `acc` that the loop itself accumulates; R rows `vr` and values `tv` beside the LDS rows
// and the label table; the R rows of the stored beta rows; a float64 histogram and a per-entry sum for the c_{a,t}.
struct PosExpRider {
  const float *pv, *lv;  // of this lattice, or nullptr
  double coef;
  const float *av_in;  // arc_values, or nullptr
  double *av;          // the workspace's value per arc; nullptr: no arc has one
  double *sbr;         // the stored R rows of this lattice
  double *acc_c;       // per in-entry of this lattice
  float *pos_cov, *arc_cov;
  double *ev64;
  float *ev32;
  double *vr, *tv, *hcov;      // LDS
  double N = 0.0, v = 0.0, rest = 0.0, ev = 0.0;  // v: the value of the term just taken (R(other state) + v_t(a)); rest: R_{t+1}(d) - E[V]
  __device__ __forceinline__ bool by_step() const { return pv != nullptr; }
  __device__ __forceinline__ bool arc_val() const { return av != nullptr; }
  __device__ __forceinline__ bool by_label() const { return pos_cov != nullptr; }
  __device__ __forceinline__ bool by_arc() const { return arc_cov != nullptr; }
  __device__ __forceinline__ void arc(int a, double e, bool live) {
    if (!av) return;
    double x = (coef != 0.0 && live) ? coef * e : 0.0;
    if (av_in) x += (double)av_in[a];
    av[a] = x;
  }
  __device__ __forceinline__ void fill(const PosSum::Rows &tab, const float *theta, const float *pos_t, int t, int V) {
    pos_exp_fill_table(tab, tv, theta, pos_t, lv, pv ? pv + (size_t)t * V : nullptr, coef, V);
  }
  __device__ __forceinline__ void start(bool fwd, size_t st_i) {
    N = 0.0;
    rest = fwd ? sbr[st_i] - ev : 0.0;
  }
  __device__ __forceinline__ void term(const ME64 &was, const ME64 &acc, const ME64 &y, int i, int l, int a) {
    v = vr[i] + tv[l] + (av ? av[a] : 0.0);
    if (y.e > was.e) N = __builtin_amdgcn_ldexp(N, was.e - y.e);  // (the move PosSum::plus made: acc.e is y.e now)
    N += __builtin_amdgcn_ldexp(y.m, y.e - acc.e) * v;
  }
  // the partner's numerator comes as it is, beside its mass (no shuffle waits for another), and both are brought under
  // the common exponent here (commutative: both partners agree)
  __device__ __forceinline__ void combine(const ME64 &was, const ME64 &acc, int o) {
    const double oN = __shfl_xor(N, o);
    const int oe = __shfl_xor(was.e, o);
    N = __builtin_amdgcn_ldexp(N, was.e - acc.e) + __builtin_amdgcn_ldexp(oN, oe - acc.e);
  }
  __device__ __forceinline__ void row(int i, const ME64 &acc, bool live, bool store, size_t st_i) {
    const double r = (live && acc.m != 0.0) ? N / acc.m : 0.0;
    vr[i] = r;
    if (store) sbr[st_i] = r;
  }
  __device__ __forceinline__ void beta_done(int b, const ME64 &z) {  // R_0(0) is in row 0 of the pair
    ev = z.m > 0.0 ? vr[0] : 0.0;
    if (threadIdx.x == 0) {
      ev64[b] = ev;
      if (ev32) ev32[b] = (float)ev;
    }
  }
  __device__ __forceinline__ void post(double p, int j, int l) {
    const double c = p * (v + rest);
    if (pos_cov) atomicAdd(&hcov[l], c);  // (float64 LDS atomics: the order of the adds is not fixed)
    if (arc_cov) acc_c[j] += c;
  }
  __device__ __forceinline__ void drain_label(size_t i, int l) {
    if (pos_cov) pos_cov[i] = (float)hcov[l];
    hcov[l] = 0.0;
  }
  __device__ __forceinline__ void drain_arc(int a, int j) {
    if (arc_cov) arc_cov[a] = j < 0 ? 0.0f : (float)acc_c[j];
  }
};

// LDS: pos_lds_layout with one double beside every row value, table entry and histogram bin:
// 40 max_rows + 36 vocab + 4 kPosThreads bytes.  STAGED: + 4 (max_rows + 1) + 4 (arcs of the largest lattice) bytes.
template <bool EXTRA, bool STAGED>
__global__ __launch_bounds__(kPosThreads) void k_positional_expect(nfst_batch lat, PosIn in, PosExpVals x, PosWs w, PosExpWs xw,
                                                                   PosExpOut o) {
  extern __shared__ double pos_lds[];
  const int b = blockIdx.x;
  const Meta m = load_meta(lat.meta, b);
  const PosLds L = pos_lds_layout(pos_lds, lat.max_rows, lat.vocab, 1);
  // without any of the four optional outputs there is no forward pass: no by-destination order, no stored rows
  const bool need_alpha = o.pos_post || o.arc_post || o.pos_cov || o.arc_cov;
  const bool arc_val = x.av != nullptr || (EXTRA && x.coef != 0.0);
  PosExpRider rd = {x.pv ? x.pv + (size_t)x.pv_stride * b : nullptr, x.lv ? x.lv + (size_t)x.lv_stride * b : nullptr, x.coef, x.av,
                    arc_val ? xw.av : nullptr, xw.br + (size_t)(in.T + 1) * m.row_off, xw.acc2 + m.arc_off, o.pos_cov, o.arc_cov,
                    o.ev64, o.ev32, L.xr, L.xt, L.xh};
  if (need_alpha) {  // (barriers follow before either is added to)
    for (int l = threadIdx.x; l < lat.vocab; l += kPosThreads) rd.hcov[l] = 0.0;
    for (int i = threadIdx.x; i < m.n_arcs; i += kPosThreads) rd.acc_c[i] = 0.0;
  }
  const PosOut po = {o.logz64, o.logz32, nullptr, o.pos_post, o.arc_post};
  pos_sum_sweep<EXTRA, STAGED>(lat, in, w, po, need_alpha ? kPosModeAlpha : kPosModeLogz, L, rd);
}

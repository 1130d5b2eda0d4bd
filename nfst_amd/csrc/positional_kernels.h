// positional_kernels.h -- time-synchronous sweeps: arc scores that depend on the position of the arc on the path
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.10.
#pragma once

// A path a_0 .. a_{L-1} from state 0 to the sink takes arc a_t "at position t" and scores it
//     s_a + pos[b, t, label(a)]          (s_a as nfst_scores defines it; pos optional)
// Only paths of L <= T arcs count.  Both kernels advance ALL states one position per step (the level-scheduled
// sweeps cannot: a state of these lattices is reached at many path lengths), one workgroup per lattice, on the
// canonical arrays only (row_ptr, arc_src, arc_dst, arc_label, arc_w):
//   k_positional          sum-product: beta_t(s) = total weight of the ways to finish from s with at most T - t arcs,
//                         backwards in time (log Z_T = log beta_0(0)); on request alpha_t forwards in time over a
//                         by-destination order built once per launch, with the posteriors of every (position, label)
//                         and every arc and the weight of every path length
//   k_positional_viterbi  the same backward pass in max-plus (plain float32), then one thread walks the best path
//   k_positional_walk     exact draws: one wave per walk reads the beta rows that k_positional stored (kPosModeRows: the
//                         backward pass alone, no forward pass); k_positional_score is the forced walk of given marks
// The backward pass is ONE function template over the semiring (PosSum / PosMax), not a copy, and the forward pass is
// one function too (pos_alpha_pass).  An op that carries a second quantity beside the semiring's value -- the expectation
// sweep of positional_expect_kernels.h -- does not copy the loops either: it hands them a rider (PosNoRider below lists
// the hooks), and k_positional and k_positional_expect are both pos_sum_sweep, with the empty rider and with PosExpRider.
//
// Arithmetic of the sum-product kernel: (float64 mantissa, int32 exponent) THROUGHOUT, for every T -- label weights by
// exp_split64, sums in float64.  float32 mantissas would repeat one rounding error per label at every position
// (1.5e-5 at 900 levels); this op is bound by its barriers, not by its multiplies (section 4.10),
// so there is no float32 flavour and no threshold in T.  Per step exp(theta[l] + pos[b, t, l]) is split once per LABEL
// into an LDS table; the weights of per-arc extras are split once per launch into the workspace: no transcendental per
// arc and step.
//
// A state's arcs are shared by a group of G lanes (G = 1 .. 64, a power of two chosen per lattice from its mean degree);
// the group's partial sums are combined by butterfly shuffles in a fixed order: no float atomics anywhere, the same bits
// at every launch and for every packing.
constexpr int kPosThreads = 1024;
constexpr int kPosPostBits = kExpPostBits;  // per-label posterior sums in fixed point, as label_post of nfst_expectation
// what a launch of k_positional does after the backward pass: nothing (log Z only), the forward pass over the stored
// beta rows (posteriors, lengths), or nothing but with every beta row stored for k_positional_walk
constexpr int kPosModeLogz = 0, kPosModeAlpha = 1, kPosModeRows = 2;
constexpr int kPosWalkWaves = 4;  // walks (waves) per workgroup of k_positional_walk

struct PosIn {
  nfst_scores sc;
  const float *pos;    // [T, V] (stride 0) or [B, T, V] (stride T * V); nullptr: no position term
  int64_t pos_stride;
  int T;
};
// the caller's workspace (nfst_positional_ws_bytes); lattice b owns rows (T + 1) * row_off .. of the stored rows
struct PosWs {
  double *ewm;   // [total_arcs] weight of the arc's extras (arc_w + arc_scores), mantissa ...
  int *ewe;      // [total_arcs] ... and exponent (only read when the batch has extras)
  double *bm;    // [(T + 1) * total_rows] beta_t(s), mantissa ...
  int *be;       // [(T + 1) * total_rows] ... and exponent
  int *in_ptr;   // [total_rows + n_lattices] first in-entry of every state (relative to the lattice), then the end
  int *in_tmp;   // [total_arcs] the in-entries before they are put in canonical order
  int2 *in_rec;  // [total_arcs] in-entries by (destination, canonical arc): (arc in lattice, src | label << 16)
  double *acc;   // [total_arcs] per in-entry: sum over t of P(the arc is at position t)
  float *vb;     // [(T + 1) * total_rows] max-plus rows of k_positional_viterbi
};
struct PosOut {
  double *logz64;
  float *logz32;
  double *len_logz;  // [B, T + 1]
  float *pos_post;   // [B, T, V]
  float *arc_post;   // [total_arcs]
};
struct PosVitOut {
  float *best;
  int32_t *paths, *path_arcs, *lengths;
  int pad;
};

// ---- the two semirings of the backward pass ---------------------------------------------------------------------
struct PosSum {  // sum-product in (float64 mantissa, exponent)
  typedef ME64 V;
  struct Rows {  // the values of two positions, and the label table of the current step, in LDS
    double *m;
    int *e;
    __device__ __forceinline__ V get(int i) const { return {m[i], e[i]}; }
    __device__ __forceinline__ void set(int i, V v) const { m[i] = v.m; e[i] = v.e; }
  };
  struct Store {  // the stored rows of one lattice in the workspace
    double *m;
    int *e;
    __device__ __forceinline__ void set(size_t i, V v) const { m[i] = v.m; e[i] = v.e; }
    __device__ __forceinline__ bool on() const { return m != nullptr; }
  };
  static __device__ __forceinline__ V zero() { return {0.0, kEZero}; }
  static __device__ __forceinline__ V one() { return {0.5, 1}; }
  static __device__ __forceinline__ V label(float th) { return exp_split64((double)th); }
  static __device__ __forceinline__ V label(float th, float p) { return exp_split64((double)th + (double)p); }
  static __device__ __forceinline__ V times(V lab, V nxt) { return {lab.m * nxt.m, lab.e + nxt.e}; }
  static __device__ __forceinline__ bool live(V x) { return x.m != 0.0; }  // (plus adds nothing otherwise)
  static __device__ __forceinline__ void plus(V &acc, V x) {
    if (x.m != 0.0) {
      if (x.e > acc.e) { acc.m = __builtin_amdgcn_ldexp(acc.m, acc.e - x.e); acc.e = x.e; }
      acc.m += __builtin_amdgcn_ldexp(x.m, x.e - acc.e);
    }
  }
  // the same value in both partners of a butterfly stage: the sum is commutative
  static __device__ __forceinline__ void combine(V &acc, int o) {
    const double om = __shfl_xor(acc.m, o);
    const int oe = __shfl_xor(acc.e, o);
    const int E = max(acc.e, oe);
    acc.m = __builtin_amdgcn_ldexp(acc.m, acc.e - E) + __builtin_amdgcn_ldexp(om, oe - E);
    acc.e = E;
  }
  static __device__ __forceinline__ V norm(V acc) {
    const Rec64 r = me_pack64(acc.m, acc.e);
    return {r.m, r.e};
  }
};
struct PosMax {  // max-plus in plain float32: c = e_a + ((theta[l] + pos[b, t, l]) + vb_{t+1}(dst)), in this order
  typedef float V;
  struct Rows {
    float *v;
    __device__ __forceinline__ V get(int i) const { return v[i]; }
    __device__ __forceinline__ void set(int i, V x) const { v[i] = x; }
  };
  struct Store {
    float *v;
    __device__ __forceinline__ void set(size_t i, V x) const { v[i] = x; }
    __device__ __forceinline__ bool on() const { return v != nullptr; }
  };
  static __device__ __forceinline__ V zero() { return kNegInf; }
  static __device__ __forceinline__ V one() { return 0.0f; }
  static __device__ __forceinline__ V label(float th) { return th; }
  static __device__ __forceinline__ V label(float th, float p) { return th + p; }
  static __device__ __forceinline__ V times(V lab, V nxt) { return lab + nxt; }
  static __device__ __forceinline__ bool live(V) { return true; }
  static __device__ __forceinline__ void plus(V &acc, V x) { acc = x > acc ? x : acc; }
  static __device__ __forceinline__ void combine(V &acc, int o) {
    const float x = __shfl_xor(acc, o);
    acc = x > acc ? x : acc;
  }
  static __device__ __forceinline__ V norm(V acc) { return acc; }
};

// lanes per state: the largest power of two <= the mean out-degree (n_dp / n_reach, rounded down), doubled while it
// is below that mean and twice as many lanes per state still fit the workgroup (lanes would idle otherwise)
__device__ __forceinline__ int pos_group(const Meta &m) {
  const int n = max(m.n_reach, 1), avg = m.n_dp / n;
  int g = 1;
  while (g < 64 && g * 2 <= avg) g <<= 1;
  while (g < 64 && g < avg && m.n_rows * g * 2 <= kPosThreads) g <<= 1;
  return g;
}

// The arcs of the step loops: read from the canonical arrays in HBM / L2, or -- when the lattice's arcs fit next to the
// value rows (the launcher decides) -- from 4-byte records staged in LDS once per pass, so that a step touches no
// global memory but the stored rows.  A record is (other state | label << 16): rows < 2^13, labels < 2^15.
struct PosArcsGlobal {
  const int32_t *rp, *other, *label;  // rp: the lattice's row pointers (absolute arcs)
  int a_lo, a_hi;
  __device__ __forceinline__ int lo(int s) const { return max(rp[s], a_lo); }
  __device__ __forceinline__ int hi(int s) const { return min(rp[s + 1], a_hi); }
  __device__ __forceinline__ uint32_t rec(int a) const { return (uint32_t)other[a] | ((uint32_t)label[a] << 16); }
};
struct PosArcsLds {
  const int *rp;         // LDS: first entry of every state, relative to the lattice, then the end
  const uint32_t *recs;  // LDS
  int a_lo;
  __device__ __forceinline__ int lo(int s) const { return rp[s] + a_lo; }
  __device__ __forceinline__ int hi(int s) const { return rp[s + 1] + a_lo; }
  __device__ __forceinline__ uint32_t rec(int a) const { return recs[a - a_lo]; }
};
// stage the out-arcs of a lattice (before a barrier of the caller)
__device__ __forceinline__ void pos_stage_out(const nfst_batch &lat, const Meta &m, int b, int *rp_l, uint32_t *recs) {
  const int32_t *rp = lat.row_ptr + m.row_off + b;
  const int a_lo = m.arc_off, a_hi = m.arc_off + m.n_arcs;
  for (int s = threadIdx.x; s <= m.n_rows; s += kPosThreads) rp_l[s] = min(max(rp[s], a_lo), a_hi) - a_lo;
  for (int i = threadIdx.x; i < m.n_arcs; i += kPosThreads)
    recs[i] = (uint32_t)lat.arc_dst[a_lo + i] | ((uint32_t)lat.arc_label[a_lo + i] << 16);
}

template <bool STAGED>
using PosArcs = typename std::conditional<STAGED, PosArcsLds, PosArcsGlobal>::type;
// the out-arcs of a lattice for the backward pass (STAGED: staged here, before the barrier the pass begins with)
template <bool STAGED>
__device__ __forceinline__ PosArcs<STAGED> pos_out_arcs(const nfst_batch &lat, const Meta &m, int b, int *rp_l, uint32_t *recs) {
  if constexpr (STAGED) {
    pos_stage_out(lat, m, b, rp_l, recs);
    return {rp_l, recs, m.arc_off};
  } else {
    return {lat.row_ptr + m.row_off + b, lat.arc_dst, lat.arc_label, m.arc_off, m.arc_off + m.n_arcs};
  }
}

// ---- riders -------------------------------------------------------------------------------------------------------
// The step loops below exist once.  What an op carries through them BESIDE the value of the semiring -- the numerator of
// the expectation sweep (PosExpRider, positional_expect_kernels.h) -- is a rider: a policy class whose hooks sit where
// the second quantity needs a line.  The value itself goes through S::plus / combine / norm in the loop, never through a
// hook, so a rider cannot change a bit of it.  PosNoRider has no state and only empty hooks: with it the loops compile
// to the plain sum-product and max-plus sweeps.
struct PosNoRider {
  // what the loops do for the rider's sake: refill the label table at every position, read the arc of every in-entry,
  // drain per label and step, drain per arc (either drain: the posterior terms are computed)
  static constexpr bool by_step() { return false; }
  static constexpr bool arc_val() { return false; }
  static constexpr bool by_label() { return false; }
  static constexpr bool by_arc() { return false; }
  // once per launch and arc: the sum e of the arc's extras; live: its weight is not zero
  __device__ __forceinline__ void arc(int, double, bool) {}
  // the label table of position t is filled (by this thread for the labels of its stride)
  template <class Rows>
  __device__ __forceinline__ void fill(const Rows &, const float *, const float *, int, int) {}
  // a state's sum begins; fwd: in the forward pass, for a state whose stored row is st_i
  __device__ __forceinline__ void start(bool, size_t) {}
  // `acc` took the term y from (row i of the other state, label l, arc a); `was` is acc before
  template <class V>
  __device__ __forceinline__ void term(const V &, const V &, const V &, int, int, int) {}
  // `acc` took the partner's sum of butterfly stage o; `was` is acc before
  template <class V>
  __device__ __forceinline__ void combine(const V &, const V &, int) {}
  // the value of LDS row i is acc (live) or a constant (not live); store: it also goes to the stored row st_i
  template <class V>
  __device__ __forceinline__ void row(int, const V &, bool, bool, size_t) {}
  // beta_0(0) = z of lattice b is known
  template <class V>
  __device__ __forceinline__ void beta_done(int, const V &) {}
  // the term just taken has posterior p; it is in-entry j with label l
  __device__ __forceinline__ void post(double, int, int) {}
  // after every step: label l goes to output element i; after the last: in-entry j (-1: a self loop) to arc a
  __device__ __forceinline__ void drain_label(size_t, int) {}
  __device__ __forceinline__ void drain_arc(int, int) {}
};

// the label table of position t: one entry per label, shared by every arc of the step
template <class S>
__device__ __forceinline__ void pos_fill_table(const typename S::Rows &tab, const float *theta, const float *pos_t, int V) {
  for (int l = threadIdx.x; l < V; l += kPosThreads) tab.set(l, pos_t ? S::label(theta[l], pos_t[l]) : S::label(theta[l]));
}
template <class S, class Rd>
__device__ __forceinline__ void pos_step_table(const typename S::Rows &tab, const float *theta, const float *pos_b, int t, int V, Rd &rd) {
  const float *pos_t = pos_b ? pos_b + (size_t)t * V : nullptr;
  pos_fill_table<S>(tab, theta, pos_t, V);
  rd.fill(tab, theta, pos_t, t, V);
}

// The backward pass, positions T .. 0: val holds two rows of R values (the row of position t is at (t & 1) * R).
// ext(a) multiplies (adds, in max-plus) the per-arc extras in.  Row t of the lattice goes to `st` when it is on.
template <class S, class Arcs, class ExtF, class Rd>
__device__ __forceinline__ void pos_beta_pass(const nfst_batch &lat, const Meta &m, const Arcs &arcs, const float *theta,
                                              const float *pos_b, int T, int R, int G, const typename S::Rows &val,
                                              const typename S::Rows &tab, const typename S::Store &st, ExtF ext, Rd &rd) {
  typedef typename S::V Val;
  const int tid = threadIdx.x, n = m.n_rows, V = lat.vocab;
  const int slots = kPosThreads / G, slot = tid / G, gl = tid % G;
  const bool by_step = pos_b != nullptr || rd.by_step();  // the table changes from position to position
  for (int i = tid; i < n; i += kPosThreads) {
    const Val v = i == m.sink ? S::one() : S::zero();
    val.set((T & 1) * R + i, v);
    if (st.on()) st.set((size_t)T * n + i, v);
    rd.row((T & 1) * R + i, v, false, st.on(), (size_t)T * n + i);
  }
  if (!by_step) pos_step_table<S>(tab, theta, pos_b, 0, V, rd);
  for (int t = T - 1; t >= 0; --t) {
    if (by_step) pos_step_table<S>(tab, theta, pos_b, t, V, rd);
    __syncthreads();  // the table and the row of position t + 1 are complete
    const int nxt = ((t + 1) & 1) * R, cur = (t & 1) * R;
    for (int base = 0; base < n; base += slots) {
      const int s = base + slot;
      const bool act = s < n && s != m.sink;
      const int a0 = act ? arcs.lo(s) : 0, a1 = act ? arcs.hi(s) : 0;
      Val acc = S::zero();
      rd.start(false, 0);
      for (int a = a0 + gl; a < a1; a += G) {
        const uint32_t rec = arcs.rec(a);
        const int d = (int)(rec & 0xffffu), l = (int)(rec >> 16);
        if (d == s) continue;  // self loops are on no path
        const Val y = ext(a, S::times(tab.get(l), val.get(nxt + d))), was = acc;
        if (!S::live(y)) continue;  // (no hook sees a term of no mass: what lies behind it is never read)
        S::plus(acc, y);
        rd.term(was, acc, y, nxt + d, l, a);
      }
      for (int o = 1; o < G; o <<= 1) {
        const Val was = acc;
        S::combine(acc, o);
        rd.combine(was, acc, o);
      }
      if (gl == 0 && s < n) {
        const bool sink = s == m.sink;
        const Val v = sink ? S::one() : S::norm(acc);
        val.set(cur + s, v);
        if (st.on()) st.set((size_t)t * n + s, v);
        rd.row(cur + s, acc, !sink, st.on(), (size_t)t * n + s);
      }
    }
    __syncthreads();  // (the next step overwrites the table and the row of position t + 1)
  }
}

// The arcs of a lattice by (destination, canonical arc), built once per launch for the forward passes: in_ptr gets the
// first in-entry of every state (relative to the lattice) and the end, w.in_rec the entries, and w.acc is zeroed.
// cnt: 2 n + 1 ints of LDS scratch, scan: one int per thread.  Integers throughout: the result does not depend on the
// order of the atomic adds.
__device__ __forceinline__ void pos_in_order(const nfst_batch &lat, const Meta &m, int *cnt, int *scan, int *in_ptr, const PosWs &w) {
  const int tid = threadIdx.x, n = m.n_rows;
  int *fill = cnt + n + 1;
  for (int i = tid; i <= n; i += kPosThreads) cnt[i] = 0;
  __syncthreads();
  for (int i = tid; i < m.n_arcs; i += kPosThreads) {
    const int a = m.arc_off + i, s = lat.arc_src[a], d = lat.arc_dst[a];
    if (s != d) atomicAdd(&cnt[d], 1);  // (integers: the order does not matter)
    w.acc[a] = 0.0;
  }
  __syncthreads();
  const int chunk = (n + kPosThreads - 1) / kPosThreads, c0 = min(tid * chunk, n), c1 = min(c0 + chunk, n);
  int part = 0;
  for (int i = c0; i < c1; ++i) part += cnt[i];
  scan[tid] = part;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < kPosThreads; ++i) { const int v = scan[i]; scan[i] = run; run += v; }
    cnt[n] = run;
    in_ptr[n] = run;
  }
  __syncthreads();
  int run = scan[tid];
  for (int i = c0; i < c1; ++i) {
    const int v = cnt[i];
    cnt[i] = run;
    fill[i] = run;
    in_ptr[i] = run;
    run += v;
  }
  __syncthreads();
  for (int i = tid; i < m.n_arcs; i += kPosThreads) {
    const int a = m.arc_off + i, s = lat.arc_src[a], d = lat.arc_dst[a];
    if (s != d) w.in_tmp[m.arc_off + atomicAdd(&fill[d], 1)] = i;
  }
  __syncthreads();
  // a state's in-entries were filled in any order: every arc finds its rank among them (stable, canonical order)
  for (int i = tid; i < m.n_arcs; i += kPosThreads) {
    const int a = m.arc_off + i, s = lat.arc_src[a], d = lat.arc_dst[a];
    if (s == d) continue;
    const int j0 = cnt[d], j1 = cnt[d + 1];
    int rank = 0;
    for (int j = j0; j < j1; ++j) rank += w.in_tmp[m.arc_off + j] < i;
    w.in_rec[m.arc_off + j0 + rank] = make_int2(i, s | (lat.arc_label[a] << 16));
  }
  __syncthreads();
}

// once per launch: the weight of every arc's extras (arc_w + arc_scores) into the workspace
template <bool EXTRA, class Rd>
__device__ __forceinline__ void pos_arc_extras(const nfst_batch &lat, const Meta &m, const nfst_scores &sc, const PosWs &w, Rd &rd) {
  if (!EXTRA && !rd.arc_val()) return;
  for (int a = m.arc_off + threadIdx.x; a < m.arc_off + m.n_arcs; a += kPosThreads) {
    double e = 0.0;
    bool live = false;
    if (EXTRA) {
      if (lat.weighted) e += (double)lat.arc_w[a];
      if (sc.arc_scores) e += (double)sc.arc_scores[a];
      const ME64 x = exp_split64(e);
      w.ewm[a] = x.m;
      w.ewe[a] = x.e;
      live = x.m != 0.0;
    }
    rd.arc(a, e, live);
  }
}

// The forward pass, positions 0 .. T, over the in-entries of pos_in_order and the beta rows `st` that the backward pass
// stored: alpha_t in `val`, the posterior of every term  p = alpha_t(src) w beta_{t+1}(dst) / z  into the label
// histogram (fixed point) and the lane-owned per-entry sums, the mass of every path length from the sink's row.
// STAGED: the LDS of the out-arc records now holds (src | label << 16) of every in-entry.
template <bool EXTRA, bool STAGED, class ExtF, class Rd>
__device__ __forceinline__ void pos_alpha_pass(const nfst_batch &lat, const Meta &m, int b, const float *theta, const float *pos_b, int T,
                                               int R, int G, const PosSum::Rows &val, const PosSum::Rows &tab, const PosSum::Store &st,
                                               ExtF ext, ME64 z, const PosWs &w, const int *in_ptr, int *rp_l, uint32_t *recs,
                                               unsigned long long *hist, const PosOut &o, Rd &rd) {
  const int tid = threadIdx.x, n = m.n_rows, V = lat.vocab;
  const int slots = kPosThreads / G, slot = tid / G, gl = tid % G;
  const double rz = z.m > 0.0 ? 1.0 / z.m : 0.0;
  const bool by_step = pos_b != nullptr || rd.by_step();
  const bool want_p = o.pos_post != nullptr || o.arc_post != nullptr || rd.by_label() || rd.by_arc();
  for (int i = tid; i < n; i += kPosThreads) {
    const ME64 v = i == 0 ? PosSum::one() : PosSum::zero();
    val.set(i, v);
    rd.row(i, v, false, false, 0);
  }
  for (int l = tid; l < V; l += kPosThreads) hist[l] = 0ull;
  const int2 *in_rec = w.in_rec + m.arc_off;
  double *acc_e = w.acc + m.arc_off;
  if constexpr (STAGED) {
    const int n_in = in_ptr[n];
    for (int d = tid; d <= n; d += kPosThreads) rp_l[d] = in_ptr[d];
    for (int j = tid; j < n_in; j += kPosThreads) recs[j] = (uint32_t)in_rec[j].y;
  }
  for (int t = 0; t < T; ++t) {
    if (by_step) pos_step_table<PosSum>(tab, theta, pos_b, t, V, rd);
    __syncthreads();
    const int cur = (t & 1) * R, nxt = ((t + 1) & 1) * R;
    const double *brm = st.m + (size_t)(t + 1) * n;
    const int *bre = st.e + (size_t)(t + 1) * n;
    for (int base = 0; base < n; base += slots) {
      const int d = base + slot;
      const bool act = d < n;
      const int j0 = act ? (STAGED ? rp_l[d] : in_ptr[d]) : 0, j1 = act ? (STAGED ? rp_l[d + 1] : in_ptr[d + 1]) : 0;
      const double bmd = act ? brm[d] * rz : 0.0;
      const int bed = act ? bre[d] - z.e : 0;
      ME64 acc = PosSum::zero();
      rd.start(act, (size_t)(t + 1) * n + d);
      for (int j = j0 + gl; j < j1; j += G) {
        int2 rec;
        if (STAGED) {
          rec.y = (int)recs[j];
          rec.x = (EXTRA || rd.arc_val()) ? in_rec[j].x : 0;
        } else {
          rec = in_rec[j];
        }
        const int l = rec.y >> 16, s = rec.y & 0xffff;
        const ME64 x = ext(m.arc_off + rec.x, PosSum::times(tab.get(l), val.get(cur + s))), was = acc;
        if (!PosSum::live(x)) continue;
        PosSum::plus(acc, x);
        rd.term(was, acc, x, cur + s, l, m.arc_off + rec.x);
        if (want_p) {
          const double pm = x.m * bmd;
          if (pm != 0.0) {
            const double p = __builtin_amdgcn_ldexp(pm, x.e + bed);
            if (o.pos_post) atomicAdd(&hist[l], (unsigned long long)llrint(__builtin_amdgcn_ldexp(p, kPosPostBits)));
            if (o.arc_post) acc_e[j] += p;  // (entry j belongs to this lane at every step)
            rd.post(p, j, l);
          }
        }
      }
      for (int og = 1; og < G; og <<= 1) {
        const ME64 was = acc;
        PosSum::combine(acc, og);
        rd.combine(was, acc, og);
      }
      if (gl == 0 && act) {
        const ME64 v = PosSum::norm(acc);
        val.set(nxt + d, v);
        rd.row(nxt + d, acc, true, false, 0);
        if (d == m.sink && o.len_logz)  // the paths of exactly t + 1 arcs
          o.len_logz[(size_t)b * (T + 1) + t + 1] = v.m > 0.0 ? log(v.m) + (double)v.e * 0.693147180559945309417232 : -__builtin_huge_val();
      }
    }
    __syncthreads();
    if (o.pos_post || rd.by_label()) {
      const size_t row = ((size_t)b * T + t) * V;
      for (int l = tid; l < V; l += kPosThreads) {
        if (o.pos_post) o.pos_post[row + l] = (float)__builtin_amdgcn_ldexp((double)hist[l], -kPosPostBits);
        hist[l] = 0ull;
        rd.drain_label(row + l, l);
      }
    }
  }
  if (o.arc_post || rd.by_arc()) {  // self loops are on no path; every other arc is one in-entry
    for (int i = tid; i < m.n_arcs; i += kPosThreads)
      if (lat.arc_src[m.arc_off + i] == lat.arc_dst[m.arc_off + i]) {
        if (o.arc_post) o.arc_post[m.arc_off + i] = 0.0f;
        rd.drain_arc(m.arc_off + i, -1);
      }
    const int n_in = in_ptr[n];
    for (int j = tid; j < n_in; j += kPosThreads) {
      if (o.arc_post) o.arc_post[m.arc_off + in_rec[j].x] = (float)acc_e[j];
      rd.drain_arc(m.arc_off + in_rec[j].x, j);
    }
  }
}

// The LDS of the sum-product sweep: two rows of (float64, int32) values, the label table (float64, int32), the label
// histogram (64-bit) and one int per thread for the prefix sums; a rider gets X doubles beside every row value, table
// entry and histogram bin (xr, xt, xh): (24 + 16 X) max_rows + (20 + 16 X) vocab + 4 kPosThreads bytes.
// STAGED: + 4 (max_rows + 1) + 4 (arcs of the largest lattice) bytes for the arc records.
struct PosLds {
  double *vm, *xr, *tm, *xt;
  unsigned long long *hist;
  double *xh;
  int *ve, *te, *scan, *rp_l;
  uint32_t *recs;
};
__device__ __forceinline__ PosLds pos_lds_layout(double *base, int R, int V, int X) {
  PosLds L;
  L.vm = base, L.xr = L.vm + 2 * R, L.tm = L.vm + (1 + X) * 2 * R, L.xt = L.tm + V;
  L.hist = (unsigned long long *)(L.tm + (1 + X) * V), L.xh = (double *)(L.hist + V);
  L.ve = (int *)(L.hist + (1 + X) * V), L.te = L.ve + 2 * R, L.scan = L.te + V, L.rp_l = L.scan + kPosThreads;
  L.recs = (uint32_t *)(L.rp_l + R + 1);
  return L;
}

// One launch of the sum-product sweep for lattice blockIdx.x: the once-per-launch work, the backward pass, log Z, and in
// kPosModeAlpha the forward pass.  k_positional and k_positional_expect are this function with their rider.
template <bool EXTRA, bool STAGED, class Rd>
__device__ __forceinline__ void pos_sum_sweep(const nfst_batch &lat, const PosIn &in, const PosWs &w, const PosOut &o, int mode,
                                              const PosLds &L, Rd &rd) {
  const int b = blockIdx.x;
  const bool need_alpha = mode == kPosModeAlpha, store = mode != kPosModeLogz;
  const Meta m = load_meta(lat.meta, b);
  const int R = lat.max_rows, T = in.T;
  const PosSum::Rows val = {L.vm, L.ve}, tab = {L.tm, L.te};
  const float *theta = in.sc.theta + (size_t)in.sc.theta_stride * b;
  const float *pos_b = in.pos ? in.pos + (size_t)in.pos_stride * b : nullptr;
  const int G = pos_group(m);
  pos_arc_extras<EXTRA>(lat, m, in.sc, w, rd);
  int *in_ptr = w.in_ptr + m.row_off + b;
  if (need_alpha) pos_in_order(lat, m, (int *)L.vm, L.scan, in_ptr, w);  // (the value rows are not in use yet: 8 n + 4 <= 16 max_rows bytes)
  const size_t ro = (size_t)(T + 1) * m.row_off;
  const PosSum::Store st = {store ? w.bm + ro : nullptr, store ? w.be + ro : nullptr};
  auto ext = [&](int a, ME64 x) -> ME64 {
    if (EXTRA) { x.m *= w.ewm[a]; x.e += w.ewe[a]; }
    return x;
  };
  pos_beta_pass<PosSum>(lat, m, pos_out_arcs<STAGED>(lat, m, b, L.rp_l, L.recs), theta, pos_b, T, R, G, val, tab, st, ext, rd);
  const ME64 z = val.get(0);  // beta_0(0) is in row 0 of the pair (position 0)
  const double logz = z.m > 0.0 ? log(z.m) + (double)z.e * 0.693147180559945309417232 : -__builtin_huge_val();
  if (threadIdx.x == 0) {
    o.logz64[b] = logz;
    if (o.logz32) o.logz32[b] = (float)logz;
    if (o.len_logz) o.len_logz[(size_t)b * (T + 1)] = m.sink == 0 ? 0.0 : -__builtin_huge_val();  // (the empty path, where state 0 is the sink)
  }
  rd.beta_done(b, z);
  if (!need_alpha) return;
  __syncthreads();  // (everyone has read beta_0(0))
  pos_alpha_pass<EXTRA, STAGED>(lat, m, b, theta, pos_b, T, R, G, val, tab, st, ext, z, w, in_ptr, L.rp_l, L.recs, L.hist, o, rd);
}

template <bool EXTRA, bool STAGED>
__global__ __launch_bounds__(kPosThreads) void k_positional(nfst_batch lat, PosIn in, PosWs w, PosOut o, int mode) {
  extern __shared__ double pos_lds[];
  PosNoRider rd;
  pos_sum_sweep<EXTRA, STAGED>(lat, in, w, o, mode, pos_lds_layout(pos_lds, lat.max_rows, lat.vocab, 0), rd);
}

// Max-plus: the same backward pass, every row stored; then thread 0 reads the path forwards from state 0: at position
// t the smallest canonical arc whose candidate has the bits of vb_t(state).  LDS: 8 max_rows + 4 vocab + 16 bytes
// (STAGED: + the arc records, as k_positional).
template <bool STAGED>
__global__ __launch_bounds__(kPosThreads) void k_positional_viterbi(nfst_batch lat, PosIn in, PosWs w, PosVitOut o) {
  extern __shared__ double pos_lds[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const Meta m = load_meta(lat.meta, b);
  const int R = lat.max_rows, V = lat.vocab, T = in.T, n = m.n_rows;
  float *vv = (float *)pos_lds, *tf = vv + 2 * R;
  int *len_s = (int *)(tf + V), *rp_l = len_s + 4;
  uint32_t *recs = (uint32_t *)(rp_l + R + 1);
  const PosMax::Rows val = {vv}, tab = {tf};
  const float *theta = in.sc.theta + (size_t)in.sc.theta_stride * b;
  const float *pos_b = in.pos ? in.pos + (size_t)in.pos_stride * b : nullptr;
  const Extra ex = {lat.weighted ? lat.arc_w : nullptr, in.sc.arc_scores};
  float *rows = w.vb + (size_t)(T + 1) * m.row_off;
  const PosMax::Store st = {rows};
  auto ext = [&](int a, float x) -> float { return ex.at(a) + x; };
  PosNoRider rd;
  pos_beta_pass<PosMax>(lat, m, pos_out_arcs<STAGED>(lat, m, b, rp_l, recs), theta, pos_b, T, R, pos_group(m), val, tab, st, ext, rd);
  int32_t *po = o.paths + (size_t)b * T;
  int32_t *ao = o.path_arcs ? o.path_arcs + (size_t)b * T : nullptr;
  if (tid == 0) {
    const int32_t *rp = lat.row_ptr + m.row_off + b;
    const float v0 = rows[0];
    o.best[b] = v0;
    int s = 0, len = 0;
    if (v0 > kNegInf) {
      for (int t = 0; t < T && s != m.sink; ++t) {
        const float v = rows[(size_t)t * n + s];
        const float *nx = rows + (size_t)(t + 1) * n;
        const int a0 = max(rp[s], m.arc_off), a1 = min(rp[s + 1], m.arc_off + m.n_arcs);
        int pick = -1;
        for (int a = a0; a < a1 && pick < 0; ++a) {
          const int d = lat.arc_dst[a], l = lat.arc_label[a];
          if (d == s) continue;
          const float lab = pos_b ? theta[l] + pos_b[(size_t)t * V + l] : theta[l];
          if (ex.at(a) + (lab + nx[d]) == v) pick = a;
        }
        if (pick < 0) break;  // (never: some arc attains the maximum)
        po[len] = lat.arc_label[pick];
        if (ao) ao[len] = pick;
        ++len;
        s = lat.arc_dst[pick];
      }
    }
    o.lengths[b] = len;
    *len_s = len;
  }
  __syncthreads();
  for (int t = *len_s + tid; t < T; t += kPosThreads) {
    po[t] = o.pad;
    if (ao) ao[t] = -1;
  }
}

// ------------------------------------------------------------------ draws and forced scores
// k_positional_walk draws from p_T(pi) = exp(S_T(pi)) / Z_T over the paths of at most T arcs, after a launch of
// k_positional in kPosModeRows has stored every beta row.  One wave per walk (b, k), kPosWalkWaves walks per workgroup,
// the grid over all B * K walks.  At position t in state s the lanes take the out-arcs of s in canonical order, 64 per
// round: lane i computes x_i = w_t(a_i) * beta_{t+1}(dst) (exp_split64 on demand, the extras' weights from the
// workspace; zero for a self loop), the wave scans the x_i inclusively by the six butterfly stages of wave_ops.h, and
// the first lane with x_i > 0 whose running sum exceeds u * beta_t(s) wins (a ballot).  The running sum is carried
// from round to round.  If rounding leaves nobody above the target the last arc of positive weight is taken.
// beta_T is zero off the sink, so the arc at position T - 1 enters the sink: no walk overruns T.  Nothing is shared
// between walks and nothing is accumulated with atomics: a walk is a function of its own uniforms.
struct PosWalkOut {
  const double *logz64;  // [B], written by the k_positional launch before this one
  int32_t *paths, *path_arcs, *lengths;
  float *logq;
  int pad;
};

// a + b rescaled to the larger exponent, as PosSum::combine: the same bits whichever operand comes first
__device__ __forceinline__ ME64 pos_add(ME64 a, ME64 b) {
  const int E = max(a.e, b.e);
  return {__builtin_amdgcn_ldexp(a.m, a.e - E) + __builtin_amdgcn_ldexp(b.m, b.e - E), E};
}
// a > b
__device__ __forceinline__ bool pos_above(ME64 a, ME64 b) {
  const int E = max(a.e, b.e);
  return __builtin_amdgcn_ldexp(a.m, a.e - E) > __builtin_amdgcn_ldexp(b.m, b.e - E);
}
// Stage S of the inclusive scan over a wave: groups of 2^S lanes, each lane with its prefix `pre` inside the group and
// the group's total `tot` (the same bits in all its lanes), merge in pairs; the upper group adds the lower one's total.
template <int S>
__device__ __forceinline__ void pos_scan_stage(ME64 &pre, ME64 &tot, int lane) {
  const ME64 o = {wave_partner<S>(tot.m), wave_partner<S>(tot.e)};
  const ME64 up = pos_add(o, pre);
  const bool upper = (lane >> S) & 1;
  pre.m = upper ? up.m : pre.m;
  pre.e = upper ? up.e : pre.e;
  tot = pos_add(tot, o);
}

template <bool EXTRA>
__global__ __launch_bounds__(kPosWalkWaves * 64) void k_positional_walk(nfst_batch lat, PosIn in, PosWs w, int K, const float *uniforms,
                                                                       uint64_t seed, PosWalkOut o) {
  const int lane = threadIdx.x & 63;
  const int64_t walk = (int64_t)blockIdx.x * kPosWalkWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (walk >= (int64_t)lat.n_lattices * K) return;  // (a whole wave: the lanes of a walk stay together throughout)
  const int b = (int)(walk / K);
  const Meta m = load_meta(lat.meta, b);
  const int T = in.T, V = lat.vocab, n = m.n_rows;
  const float *theta = in.sc.theta + (size_t)in.sc.theta_stride * b;
  const float *pos_b = in.pos ? in.pos + (size_t)in.pos_stride * b : nullptr;
  const float *arc_w = lat.weighted ? lat.arc_w : nullptr;
  const int32_t *rp = lat.row_ptr + m.row_off + b;
  const int a_lo = m.arc_off, a_hi = m.arc_off + m.n_arcs;
  const size_t ro = (size_t)(T + 1) * m.row_off;
  const double *bm = w.bm + ro;
  const int *be = w.be + ro;
  int32_t *po = o.paths + (size_t)walk * T;
  int32_t *ao = o.path_arcs ? o.path_arcs + (size_t)walk * T : nullptr;
  const double logz = o.logz64[b];
  int s = 0, len = 0;
  double tot = 0.0;
  float ublk[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (logz > -__builtin_huge_val()) {
    for (int t = 0; t < T && s != m.sink; ++t) {
      float u;
      if (uniforms) {
        u = uniforms[(size_t)walk * T + t];
      } else {  // one Philox block serves four steps
        if ((t & 3) == 0) philox_uniform4(seed, (uint32_t)walk, (uint32_t)(t >> 2), ublk);
        u = (t & 3) == 0 ? ublk[0] : ((t & 3) == 1 ? ublk[1] : ((t & 3) == 2 ? ublk[2] : ublk[3]));
      }
      const ME64 target = {(double)u * bm[(size_t)t * n + s], be[(size_t)t * n + s]};
      const double *nm = bm + (size_t)(t + 1) * n;
      const int *ne = be + (size_t)(t + 1) * n;
      const int a0 = max(rp[s], a_lo), a1 = min(rp[s + 1], a_hi);
      ME64 run = PosSum::zero();
      int chosen = -1, last = -1;
      for (int c = a0; c < a1 && chosen < 0; c += 64) {
        const int a = c + lane;
        ME64 x = PosSum::zero();
        if (a < a1) {
          const int d = lat.arc_dst[a];
          if (d != s) {  // self loops are on no path
            const int l = lat.arc_label[a];
            x = PosSum::times(pos_b ? PosSum::label(theta[l], pos_b[(size_t)t * V + l]) : PosSum::label(theta[l]), {nm[d], ne[d]});
            if (EXTRA) { x.m *= w.ewm[a]; x.e += w.ewe[a]; }
            if (x.m == 0.0) x.e = kEZero;
          }
        }
        ME64 pre = x, sum = x;
        pos_scan_stage<0>(pre, sum, lane);
        pos_scan_stage<1>(pre, sum, lane);
        pos_scan_stage<2>(pre, sum, lane);
        pos_scan_stage<3>(pre, sum, lane);
        pos_scan_stage<4>(pre, sum, lane);
        pos_scan_stage<5>(pre, sum, lane);
        const bool live = x.m > 0.0;
        const unsigned long long hit = __ballot(live && pos_above(pos_add(run, pre), target));
        const unsigned long long any = __ballot(live);
        if (hit) chosen = c + __builtin_ctzll(hit);
        else if (any) last = c + 63 - __builtin_clzll(any);
        run = pos_add(run, sum);
      }
      if (chosen < 0) chosen = last;
      if (chosen < 0) break;  // (never: beta_t(s) > 0 on a walk, so some arc of s has positive weight)
      const int l = lat.arc_label[chosen];
      double x = (double)theta[l];
      if (pos_b) x += (double)pos_b[(size_t)t * V + l];
      if (EXTRA) {
        if (arc_w) x += (double)arc_w[chosen];
        if (in.sc.arc_scores) x += (double)in.sc.arc_scores[chosen];
      }
      tot += x;
      if (lane == 0) {
        po[len] = l;
        if (ao) ao[len] = chosen;
      }
      ++len;
      s = __builtin_amdgcn_readfirstlane(lat.arc_dst[chosen]);
    }
  }
  if (lane == 0) {  // (log Z_T = -inf: no path of finite weight within T, the empty result)
    o.lengths[walk] = len;
    o.logq[walk] = len > 0 ? (float)(tot - logz) : 0.0f;
  }
  for (int t = len + lane; t < T; t += 64) {
    po[t] = o.pad;
    if (ao) ao[t] = -1;
  }
}

// The forced walk of marks [B, K, T] from state 0, one thread per (b, k): the mark at position t takes the arc of the
// current state with that label (the arcs of a state are sorted by label) and scores s_a + pos[b, t, label], summed in
// float64.  The sink's pad loop scores nothing and ends the count of `lengths`; a mark without an arc gives -inf and
// end state 0, as k_score_paths.
__global__ __launch_bounds__(64) void k_positional_score(nfst_batch lat, PosIn in, const int32_t *marks, int K, float *path_score,
                                                         int32_t *end_state, int32_t *lengths) {
  const int b = blockIdx.x;
  const int k = blockIdx.y * 64 + threadIdx.x;
  if (k >= K) return;
  const Meta m = load_meta(lat.meta, b);
  const int T = in.T, V = lat.vocab;
  const float *theta = in.sc.theta + (size_t)in.sc.theta_stride * b;
  const float *pos_b = in.pos ? in.pos + (size_t)in.pos_stride * b : nullptr;
  const Extra ex = {lat.weighted ? lat.arc_w : nullptr, in.sc.arc_scores};
  const int32_t *rp = lat.row_ptr + m.row_off + b;
  const int a_lo = m.arc_off, a_hi = m.arc_off + m.n_arcs;
  const size_t walk = (size_t)b * K + k;
  const int32_t *mk = marks + walk * T;
  int s = 0, len = 0;
  bool counting = true;
  double tot = 0.0;
  for (int t = 0; t < T; ++t) {
    const int l = mk[t];
    const int a = (l >= 0 && l < V) ? find_arc(lat.arc_label, max(rp[s], a_lo), min(rp[s + 1], a_hi), l) : -1;
    if (a < 0) { tot = (double)kNegInf; s = 0; break; }
    const int d = lat.arc_dst[a];
    if (d != s) {
      double x = (double)theta[l];
      if (pos_b) x += (double)pos_b[(size_t)t * V + l];
      if (ex.arc_w) x += (double)ex.arc_w[a];
      if (ex.arc_scores) x += (double)ex.arc_scores[a];
      tot += x;
      len += counting;
    } else {
      counting = false;
    }
    s = d;
  }
  path_score[walk] = (float)tot;
  end_state[walk] = s;
  lengths[walk] = len;
}

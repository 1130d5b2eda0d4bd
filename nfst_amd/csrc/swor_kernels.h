// swor_kernels.h -- k distinct paths per lattice drawn without replacement (stochastic beam search, Gumbel top-k)
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.15.
#pragma once

// k_swor: one workgroup per lattice, the whole search in one launch, on the canonical arrays only (row_ptr, arc_label,
// arc_dst, arc_w).  A slot is a prefix: its state, the float64 score S of its arcs and its perturbed score G.  A step
// expands every slot by the out-arcs of its state (a slot at the sink is its own single candidate); candidate e of the
// flat index (slot ascending, then canonical arc) is worth
//     phi = (S + e_a) + logbeta[dst_a] - log Z,   g = phi - log(-log x)            (x: the candidate's uniform + 2^-25)
// and, conditioned on the parent's G (M = the largest g of the parent's candidates, whose first holder inherits G itself),
//     v = G - g + log(1 - exp(g - M)),   G~ = G - max(v, 0) - log1p(exp(-|v|))     (G~ = g under G = +inf, the root)
// all in float64; log(1 - exp(d)) is evaluated as log(-expm1(d)).  The k largest G~ survive, equal ones by flat index,
// and take the next slots in flat order.  Phases of a step:
//   1  wave 0: the slots' arc ranges, a wave scan for every slot's first candidate, "some slot is off the sink"
//   2  g of every candidate into the key buffer (LDS up to `cap` candidates, the caller's workspace beyond: the kernel
//      is compiled for both), M and its first holder per slot (a wave per slot: wave_max), then the buffer is
//      overwritten with the keys: the order-preserving bits of G~, 0 = dropped.  A key is computed once per step
//   3  beam_select (beam_kernels.h): the threshold select over the keys and the compaction in flat order; the largest
//      key that loses goes to kappa
//   4  wave 0 writes the new slots and their back pointers (parent slot, arc) into the workspace
// After the last step wave 0 ranks the slots by (G desc, slot asc) and walks the back pointers.  No atomics.
//
// The kernel has two flavours, which differ only in where a candidate's score and continuation mass come from
// (SworFlavour below); the step loop is written once.  k_swor<false> is nfst_swor as above.  k_swor<true> is
// nfst_positional_swor: the arc at step t also scores pos[b, t, label], S' = (S + e_a) + pos[b, t, label_a], and the
// continuation is log beta_{t+1}(dst_a) of the rows a launch of k_positional in kPosModeRows stored, read as
// log(m) + e ln 2 per candidate (-inf at m = 0); Z is log Z_T of that launch and max_len is T.  beta_T is zero off the
// sink, so a candidate that cannot finish within T arcs has phi = -inf and is dropped like any other: the search ends
// within T steps by itself and the length check below never fires.
constexpr int kSworThreads = kBeamThreads, kSworMaxK = kBeamMaxK;
constexpr int kSworKeyBits = 64;

struct SworIn {
  const float *logbeta;  // k_swor<false>: [total_rows] of nfst_backward (k_swor<true>: unused)
  const double *logz64;
  const float *uniforms;
  uint64_t seed;
  int max_degree, k, max_len, pad;
};
// k_swor<true> takes SworIn and, behind it, the position scores of PosIn and the stored beta rows of PosWs
struct SworPosIn {
  SworIn in;
  const float *pos;  // (null: no position term)
  int64_t pos_stride;
  const double *bm;
  const int *be;
};
// the caller's workspace (nfst_swor_ws_bytes)
struct SworWs {
  int2 *back;       // [n_lattices, max_len, k] (parent slot, canonical arc or -1) of every step's slots
  uint64_t *spill;  // [n_lattices, k * vocab] keys of a step with more than kBeamLdsCand candidates (null if none can have)
};
struct SworOut {
  int32_t *paths, *path_arcs, *lengths;
  float *logp;
  double *gumbel, *kappa;
  int32_t *n_paths, *status;
};

// per-slot facts of a lattice's search (LDS)
struct SworSlots {
  double S[kSworMaxK], G[kSworMaxK], M[kSworMaxK];
  int st[kSworMaxK], len[kSworMaxK];  // state, arcs so far
  int off[kSworMaxK + 1];             // first candidate of every slot in the flat index; off[n] = their number
  int r0[kSworMaxK], am[kSworMaxK];   // first canonical arc of the slot's state; the flat index of the first holder of M
  int n, open;                        // slots; some slot is off the sink
};

// order-preserving bits of a double ("greater" as unsigned integers; -0.0 and +0.0 alike) and back
__device__ __forceinline__ uint64_t swor_ord(double x) {
  x = x == 0.0 ? 0.0 : x;
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  return u ^ (uint64_t)(((int64_t)u >> 63) | (int64_t)0x8000000000000000ull);
}
__device__ __forceinline__ double swor_unord(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? k ^ 0x8000000000000000ull : ~k));
}
// the slot j with off[j] <= e < off[j + 1]
__device__ __forceinline__ int swor_slot_of(const SworSlots &sl, int e) {
  int lo = 0, hi = sl.n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (sl.off[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// Where a candidate's score and its continuation mass come from.  score: the prefix score with arc a (float32 score e,
// label l) appended at step t; rest: the log of the mass of the continuations of state dst after step t.
template <bool POS>
struct SworFlavour;
template <>
struct SworFlavour<false> {
  typedef SworIn Arg;
  const float *logbeta;
  int row_off;
  static __device__ __forceinline__ const SworIn &common(const Arg &a) { return a; }
  __device__ __forceinline__ SworFlavour(const Arg &a, const Meta &m, int, int) : logbeta(a.logbeta), row_off(m.row_off) {}
  __device__ __forceinline__ double score(double S, float e, int, int) const { return S + (double)e; }
  __device__ __forceinline__ double rest(int, int dst) const { return (double)logbeta[row_off + dst]; }
};
template <>
struct SworFlavour<true> {
  typedef SworPosIn Arg;
  const float *pos_b;
  const double *bm;
  const int *be;
  int n, V;
  static __device__ __forceinline__ const SworIn &common(const Arg &a) { return a.in; }
  __device__ __forceinline__ SworFlavour(const Arg &a, const Meta &m, int b, int vocab)
      : pos_b(a.pos ? a.pos + (size_t)a.pos_stride * b : nullptr), bm(a.bm + (size_t)(a.in.max_len + 1) * m.row_off),
        be(a.be + (size_t)(a.in.max_len + 1) * m.row_off), n(m.n_rows), V(vocab) {}
  __device__ __forceinline__ double score(double S, float e, int t, int l) const {
    const double x = S + (double)e;
    return pos_b ? x + (double)pos_b[(size_t)t * V + l] : x;
  }
  __device__ __forceinline__ double rest(int t, int dst) const {
    const size_t i = (size_t)(t + 1) * n + dst;
    const double mt = bm[i];
    return mt > 0.0 ? log(mt) + (double)be[i] * 0.693147180559945309417232 : -__builtin_huge_val();
  }
};

template <bool POS>
__global__ __launch_bounds__(kSworThreads) void k_swor(nfst_batch lat, nfst_scores sc, typename SworFlavour<POS>::Arg arg, SworWs ws, SworOut out,
                                                       int cap) {
  const SworIn &in = SworFlavour<POS>::common(arg);
  extern __shared__ uint64_t swor_keys[];  // [cap]
  __shared__ SworSlots sl;
  __shared__ int cnt[2][kBeamWaves * 3];
  __shared__ int win_e[kSworMaxK];  // a winner's flat index; at the end: the length of every output entry
  __shared__ uint64_t win_k[kSworMaxK];
  __shared__ uint64_t red[kBeamWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, K = in.k, L = in.max_len;
  const Meta m = load_meta(lat.meta, b);
  const double kInf = __builtin_huge_val();
  const double Z = in.logz64[b];
  const SworFlavour<POS> fl(arg, m, b, lat.vocab);
  const float *theta = sc.theta + (size_t)sc.theta_stride * b;
  const float *arc_w = lat.weighted ? lat.arc_w : nullptr;
  const int32_t *rp = lat.row_ptr + m.row_off + b;
  int2 *back = ws.back + (size_t)b * L * K;
  uint64_t *spill = ws.spill ? ws.spill + (size_t)b * K * lat.vocab : nullptr;
  const size_t row = (size_t)b * K;

  bool live = fabs(Z) < kInf;  // (false for NaN too; the same in every thread)
  int t = 0, n = 0;
  uint64_t kap = 0;  // the largest key this thread saw lose, 0 = none
  if (live) {
    if (tid == 0) { sl.st[0] = 0; sl.S[0] = 0.0; sl.G[0] = kInf; sl.len[0] = 0; sl.n = 1; }
    __syncthreads();

    // phases 2 to 4 of a step on `total` candidates whose keys live in `keys` (LDS or the workspace)
    const auto step = [&](uint64_t *keys, int total) __attribute__((always_inline)) {
      for (int e = tid; e < total; e += kSworThreads) {
        const int j = swor_slot_of(sl, e), s = sl.st[j], r = e - sl.off[j];
        double g = -kInf;
        if (s == m.sink) {
          g = 0.0;  // (the slot itself: no noise, its key is G)
        } else {
          const int a = sl.r0[j] + r, l = lat.arc_label[a], dst = lat.arc_dst[a];
          if (dst != s && l >= 0 && l < lat.vocab && dst >= 0 && dst < m.n_rows) {
            const double phi = fl.score(sl.S[j], arc_score(theta, arc_w, sc.arc_scores, l, a), t, l) + fl.rest(t, dst) - Z;
            if (phi > -kInf) {
              float u4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
              bool have = true;
              if (in.uniforms) {
                if (r < in.max_degree) u4[0] = in.uniforms[(((size_t)b * L + t) * K + j) * in.max_degree + r];
                else { have = false; *out.status = NFST_ERR_ARG; }
              } else {
                philox_uniform4(in.seed, (uint32_t)b, (uint32_t)t, (uint32_t)j, (uint32_t)r, u4);
              }
              if (have) g = phi - log(-log((double)u4[0] + 0x1p-25));
            }
          }
        }
        keys[e] = (uint64_t)__double_as_longlong(g);
      }
      __syncthreads();
      for (int j = wv; j < n; j += kBeamWaves) {  // a wave per slot: its candidates are contiguous
        const int e0 = sl.off[j], e1 = sl.off[j + 1];
        double mx = -kInf;
        for (int e = e0 + lane; e < e1; e += 64) mx = fmax(mx, __longlong_as_double((long long)keys[e]));
        mx = wave_max(mx);
        int first = -INT_MAX;
        for (int e = e0 + lane; e < e1; e += 64)
          if (first == -INT_MAX && __longlong_as_double((long long)keys[e]) == mx) first = -e;
        first = -wave_max(first);
        if (lane == 0) { sl.M[j] = mx; sl.am[j] = first; }
      }
      __syncthreads();
      for (int e = tid; e < total; e += kSworThreads) {
        const int j = swor_slot_of(sl, e);
        const double g = __longlong_as_double((long long)keys[e]), G = sl.G[j];
        uint64_t key = 0;
        if (sl.st[j] == m.sink) {
          key = swor_ord(G);
        } else if (g > -kInf) {
          double gt = g;
          if (G < kInf) {
            gt = G;
            if (e != sl.am[j]) {
              const double v = G - g + log(-expm1(g - sl.M[j]));
              gt = G - fmax(v, 0.0) - log1p(exp(-fabs(v)));
            }
          }
          key = swor_ord(gt);
        }
        keys[e] = key;
      }
      __syncthreads();
      int n_cand;
      const int n_win = beam_select<kSworKeyBits, true>([&](int e) { return keys[e]; }, total, K, cnt,
                                    [&](int pos, int e, uint64_t k) { win_e[pos] = e; win_k[pos] = k; },
                                    [&](uint64_t k) { kap = k > kap ? k : kap; }, n_cand);
      if (tid < 64) {  // wave 0: winner i becomes slot i (LDS accesses of one wave execute in order: reads, then writes)
        int ns = 0, nl = 0, pj = -1, pa = -1;
        double nS = 0.0, nG = 0.0;
        if (tid < n_win) {
          const int e = win_e[tid];
          pj = swor_slot_of(sl, e);
          ns = sl.st[pj]; nS = sl.S[pj]; nG = sl.G[pj]; nl = sl.len[pj];
          if (ns != m.sink) {
            pa = sl.r0[pj] + (e - sl.off[pj]);
            const int l = lat.arc_label[pa];
            nS = fl.score(nS, arc_score(theta, arc_w, sc.arc_scores, l, pa), t, l);
            ns = lat.arc_dst[pa];
            nG = swor_unord(win_k[tid]);
            ++nl;
          }
        }
        asm volatile("" ::: "memory");
        if (tid < n_win) {
          sl.st[tid] = ns; sl.S[tid] = nS; sl.G[tid] = nG; sl.len[tid] = nl;
          back[(size_t)t * K + tid] = make_int2(pj, pa);
        }
        if (tid == 0) sl.n = n_win;
      }
      __syncthreads();
    };

    for (;; ++t) {
      if (tid < 64) {  // phase 1 (wave 0: at most 64 slots)
        const int ns = sl.n;
        int deg = 0;
        bool off_sink = false;
        if (tid < ns) {
          const int s = sl.st[tid];
          int r0 = 0;
          if (s == m.sink) deg = 1;
          else { r0 = rp[s]; deg = rp[s + 1] - r0; off_sink = true; }
          sl.r0[tid] = r0;
        }
        int incl = deg;
        for (int d = 1; d < 64; d <<= 1) {
          const int o = __shfl_up(incl, d);
          if (tid >= d) incl += o;
        }
        if (tid < ns) sl.off[tid] = incl - deg;
        if (tid == 63) sl.off[ns] = incl;  // (lanes from ns on add nothing)
        const bool open = __any(off_sink);
        if (tid == 0) sl.open = open ? 1 : 0;
      }
      __syncthreads();
      // (every thread reads the same LDS words after the barrier: the workgroup leaves the loop together)
      n = sl.n;
      const int total = sl.off[n];
      if (!sl.open) break;
      if (t >= L) {  // max_len steps have passed and some slot is off the sink
        if (tid == 0) *out.status = NFST_ERR_LENGTH;
        live = false;
        break;
      }
      if (total <= cap) {
        step(swor_keys, total);
      } else if (spill && (int64_t)total <= (int64_t)K * lat.vocab) {
        step(spill, total);
      } else {  // (never on a valid batch: a state has at most one arc per label)
        if (tid == 0) *out.status = NFST_ERR_ARG;
        live = false;
        break;
      }
    }
  }
  if (!live) n = 0;

  // kappa: the largest key any thread saw lose
  kap = kb_wave_max(kap);
  if (lane == 0) red[wv] = kap;
  // ranks by (G desc, slot asc); entry `rank` is slot i.  Entries from n on are empty
  int rank = tid, len = 0;
  if (tid < 64) {
    double G = -kInf, lp = -kInf;
    if (tid < n) {
      G = sl.G[tid];
      len = sl.len[tid];
      lp = sl.S[tid] - Z;
      rank = 0;
      for (int q = 0; q < n; ++q) {
        const double o = sl.G[q];
        rank += (o > G || (o == G && q < tid)) ? 1 : 0;
      }
      len = len < L ? len : L;  // (a slot has one arc per step: never more than max_len)
    }
    if (tid < K) {
      out.lengths[row + rank] = len;
      out.logp[row + rank] = (float)lp;
      out.gumbel[row + rank] = G;
      win_e[rank] = len;
    }
  }
  __syncthreads();
  if (tid == 0) {
    uint64_t kmax = 0;
    for (int w = 0; w < kBeamWaves; ++w) kmax = red[w] > kmax ? red[w] : kmax;
    out.kappa[b] = (n > 0 && kmax != 0) ? swor_unord(kmax) : -kInf;
    out.n_paths[b] = n;
  }
  if (tid < n) {  // (wave 0) the path of slot tid, from its last arc to its first
    int32_t *po = out.paths + (row + rank) * L;
    int32_t *ao = out.path_arcs ? out.path_arcs + (row + rank) * L : nullptr;
    int cur = tid, at = len;
    for (int tt = t - 1; tt >= 0 && cur >= 0 && cur < K; --tt) {
      const int2 bp = back[(size_t)tt * K + cur];
      if (bp.y >= 0 && at > 0) {
        --at;
        po[at] = lat.arc_label[bp.y];
        if (ao) ao[at] = bp.y;
      }
      cur = bp.x;
    }
  }
  for (int i = tid; i < K * L; i += kSworThreads) {  // the rest of every row
    const int ent = i / L;
    if (i - ent * L >= win_e[ent]) {
      out.paths[row * L + i] = in.pad;
      if (out.path_arcs) out.path_arcs[row * L + i] = -1;
    }
  }
}

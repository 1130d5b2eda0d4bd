// string_prefix_kernels.h -- the exact log weight of the paths whose output string starts with a given prefix, and of its
// extensions by one symbol
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.23.
#pragma once

// Three kernels behind k_kbest_levels, on the canonical arrays only; float64 log-sums as in string_logprob_kernels.h:
//   k_string_prefix       the backward sweep of H, which is G (k_string_logprob) with "anything may follow" at column n:
//                         the same grid (B x Y, candidate m in workgroup m mod Y), the same items -- one wave per (state,
//                         candidate, strip of 64 columns) -- and one barrier per level.  Columns j < n follow G's
//                         recurrence; at j = n in keep mode every out-arc, kept or not, carries H[d][n]; in marker mode
//                         H0[s][n] takes H1[d][n] over a marker arc and H0[d][n] over any other, H1[s][n] takes H0[d][n]
//                         over every arc; the sink holds H0 = 0 at column n and H1 = -inf (a marker with nothing behind it
//                         spells nothing).  log_prefix = H0[state 0][0].  Workgroup 0 carries log Z of every row with
//                         sl_item_z, as k_string_logprob does.  Without lengths (y_len == nullptr) every candidate is the
//                         empty prefix: with M = 1 and N = 0 column 0 of a state then holds zn0 (and zn1), the log weight
//                         of its continuations that do not end on a marker.
//   k_string_label_index  one workgroup per lattice: the arcs whose source state 0 reaches, without self loops, by (label,
//                         canonical arc id).  Integer counts in LDS and a scan over the labels give every label's first
//                         entry; then wave w places the arcs of the labels l with l mod 16 == w, taking the arcs of the
//                         lattice 64 at a time in ascending order: the lanes of one label find their places from a ballot
//                         (the label's fill position + the number of lower lanes with that label).  One pass over the
//                         arcs per wave whatever a label's share of them, no barrier, and the list is a function of the
//                         canonical arrays only.
//   k_string_next         behind the unchanged k_string_logprob_index and k_string_logprob_fwd (F and az) and behind
//                         k_string_prefix's zn rows: one workgroup per (lattice, candidate), whose waves take the labels
//                         in turn, one wave per (lattice, candidate, label v): the arcs a: s -> d of label v in list
//                         order, term (F[s][n] + w_a) + z[d] (keep mode, v kept) or (F1[s][n] + w_a) + zn0[d] (marker
//                         mode), summed by sp_wave_lse.  After a barrier wave 0 forms log_prefix from eos = F0[sink][n]
//                         and the V values of next in the same way (term 0 is eos, term 1 + v is next[v]).
// sp_wave_lse: term i sits on lane i mod 64 of strip i / 64.  First the greatest term (exact in any order), then per
// strip the 64 values exp(term - greatest) (0 outside the list, for -inf and for NaN) in the tree of row_reduce<64>, the
// strips' sums added to 0.0 in ascending order; the result is greatest + log(sum), -inf if there is no term above -inf.
// No atomics on values: the same bits at every launch, for every grid Y, under every packing and for every slicing.
constexpr int kSpIndexThreads = 1024, kSpIndexWaves = kSpIndexThreads / 64;
constexpr int kSpNextThreads = 1024, kSpNextWaves = kSpNextThreads / 64;

// the part of nfst_string_next's workspace behind the level arrays and the tables of the prefix sweep (SlWs, SlgWs)
struct SpWs {
  double *zn;     // [total_rows, planes] column 0 of k_string_prefix on the empty prefix (M = 1, N = 0)
  double *zn_lp;  // [B] that run's log_prefix (not an output)
  int *lab_ptr;   // [B, vocab + 1] first entry of every label (relative to the lattice), then the end
  int *lab_list;  // [total_arcs] per lattice from arc_off: canonical arc ids by (label, id)
};

// One item of H: sl_item (string_logprob_kernels.h) with the open column j == n.
template <bool MK>
__device__ __forceinline__ void sp_item(const nfst_batch &lat, const Meta &m, const float *theta, const Extra &ex, const SlIn &in,
                                        const int32_t *rp, double *cells, int64_t stride_row, int64_t cand, const int32_t *y, int n,
                                        int s, int p, int lane) {
  const int j = 64 * p + lane, N1 = in.N + 1;
  const bool in_row = j <= n, has_tok = j < n, open = j == n;
  double *out = cells + (size_t)s * stride_row + cand;
  if (s == m.sink) {  // the empty rest of a path is a rest behind the whole prefix; a marker with nothing behind it spells nothing
    if (in_row) {
      out[j] = open ? 0.0 : kNegInf64;
      if (MK) out[N1 + j] = kNegInf64;
    }
    return;
  }
  const int ytok = has_tok ? y[j] : -1;
  double m0 = kNegInf64, s0 = 0.0, m1 = kNegInf64, s1 = 0.0;
  const int a0 = rp[s], deg = rp[s + 1] - a0;
  for (int base = 0; base < deg; base += 64) {
    const SlArcs a = sl_load_arcs(lat, theta, ex, in, s, a0 + base + lane, base + lane < deg);
    const int cnt = deg - base < 64 ? deg - base : 64;
    for (int q = 0; q < cnt; ++q) {
      const int d = read_lane(a.dv, q);
      if (d == s) continue;  // (a self loop is on no path; the same in every lane)
      const int l = read_lane(a.lv, q), kq = read_lane(a.kv, q);
      const double sc = read_lane(a.sv, q);
      const double *row = cells + (size_t)d * stride_row + cand;
      const bool match = has_tok && ytok == l;
      if (!MK) {
        double v = kNegInf64;
        if (!kq || open) {
          if (in_row) v = row[j];
        } else if (match) {
          v = row[j + 1];
        }
        sl_add(m0, s0, sc + v);
      } else {
        double v0 = kNegInf64, v1 = kNegInf64;
        if (in_row) v0 = row[(kq ? N1 : 0) + j];
        if (match) v1 = row[j + 1];
        else if (open) v1 = row[j];
        sl_add(m0, s0, sc + v0);
        sl_add(m1, s1, sc + v1);
      }
    }
  }
  if (in_row) {
    out[j] = sl_log(m0, s0);
    if (MK) out[N1 + j] = sl_log(m1, s1);
  }
}

template <bool MK>
__global__ __launch_bounds__(kSlThreads) void k_string_prefix(nfst_batch lat, nfst_scores sc, SlIn in, SlWs w, double *log_prefix,
                                                              double *logz, int32_t *status) {
  extern __shared__ int sl_lds[];
  const int b = blockIdx.x, yb = blockIdx.y, Y = gridDim.y, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Meta m = load_meta(lat.meta, b);
  const int n_lev = w.n_lev[b];
  const int n_reach = w.lev[m.row_off + b + n_lev];
  int *order = sl_lds, *lev = order + lat.max_rows;
  for (int i = tid; i < n_reach; i += kSlThreads) order[i] = w.order[m.row_off + i];
  for (int i = tid; i <= n_lev; i += kSlThreads) lev[i] = w.lev[m.row_off + b + i];
  __syncthreads();
  const int32_t *rp = lat.row_ptr + m.row_off + b;
  const float *theta = sc.theta + (size_t)sc.theta_stride * b;
  const Extra ex = {lat.weighted ? lat.arc_w : nullptr, sc.arc_scores};
  double *cells = w.cells + (size_t)m.row_off * w.stride_row;
  double *z = w.z + m.row_off;
  const int32_t *ys = in.y + (size_t)b * in.M * in.N;
  const int32_t *yl = in.y_len ? in.y_len + (size_t)b * in.M : nullptr;  // (none: every candidate is the empty prefix)
  const int m_loc = in.M > yb ? (in.M - yb + Y - 1) / Y : 0;  // the candidates yb, yb + Y, ...
  const int strips = (in.N >> 6) + 1;                        // columns 0 .. N
  const int cell_items = m_loc * strips, per_state = cell_items + (yb == 0 ? 1 : 0);
  for (int L = n_lev - 1; L >= 0; --L) {
    const int lo = lev[L], hi = lev[L + 1];
    const int64_t items = (int64_t)(hi - lo) * per_state;
    for (int64_t it = wv; it < items; it += kSlWaves) {
      const int si = (int)(it / per_state), r = (int)(it - (int64_t)si * per_state);
      const int s = __builtin_amdgcn_readfirstlane(order[lo + si]);
      if (r == cell_items) {
        sl_item_z(lat, m, theta, ex, in, rp, z, s, lane);
        continue;
      }
      const int mi = r / strips, p = r - mi * strips, mc = yb + mi * Y;
      const int n = yl ? yl[mc] : 0;
      if (n < 0 || n > in.N || 64 * p > n) continue;  // (a bad length: none of the candidate's tokens is read)
      sp_item<MK>(lat, m, theta, ex, in, rp, cells, w.stride_row, (int64_t)mc * w.stride_m, ys + (size_t)mc * in.N, n, s, p, lane);
    }
    __syncthreads();  // (the rows of this level are visible to the waves of the next one)
  }
  for (int mi = tid; mi < m_loc; mi += kSlThreads) {
    const int mc = yb + mi * Y, n = yl ? yl[mc] : 0;
    const bool ok = n >= 0 && n <= in.N;
    if (!ok) *status = NFST_ERR_LENGTH;
    log_prefix[(size_t)b * in.M + mc] = ok ? cells[(size_t)mc * w.stride_m] : kNegInf64;  // H0[state 0][0]
  }
  if (yb == 0 && tid == 0) logz[b] = z[0];
}

// LDS: label counts, then fill positions (4 bytes per label + 4), reach flags (4 bytes per row), one int per thread for
// the scan.  Integers throughout: the counts do not depend on the order of the atomic adds, and a label's entries are
// placed by one wave in ascending arc order.
__global__ __launch_bounds__(kSpIndexThreads) void k_string_label_index(nfst_batch lat, SlWs w, SpWs g) {
  extern __shared__ int sp_lds[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Meta m = load_meta(lat.meta, b);
  const int n = m.n_rows, V = lat.vocab;
  int *cnt = sp_lds, *reach = cnt + V + 1, *scan = reach + lat.max_rows;
  const int n_reach = w.lev[m.row_off + b + w.n_lev[b]];
  int *lab_ptr = g.lab_ptr + (size_t)b * (V + 1), *lab_list = g.lab_list + m.arc_off;
  for (int i = tid; i <= V; i += kSpIndexThreads) cnt[i] = 0;
  for (int i = tid; i < n; i += kSpIndexThreads) reach[i] = 0;
  __syncthreads();
  for (int i = tid; i < n_reach; i += kSpIndexThreads) reach[w.order[m.row_off + i]] = 1;
  __syncthreads();
  // an arc counts when it is no self loop and state 0 reaches its source
  for (int i = tid; i < m.n_arcs; i += kSpIndexThreads) {
    const int a = m.arc_off + i, s = lat.arc_src[a];
    if (s != lat.arc_dst[a] && reach[s] != 0) atomicAdd(&cnt[lat.arc_label[a]], 1);
  }
  __syncthreads();
  const int chunk = (V + kSpIndexThreads - 1) / kSpIndexThreads, c0 = min(tid * chunk, V), c1 = min(c0 + chunk, V);
  int part = 0;
  for (int i = c0; i < c1; ++i) part += cnt[i];
  scan[tid] = part;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < kSpIndexThreads; ++i) { const int v = scan[i]; scan[i] = run; run += v; }
    lab_ptr[V] = run;
  }
  __syncthreads();
  int run = scan[tid];
  for (int i = c0; i < c1; ++i) {
    const int v = cnt[i];
    cnt[i] = run;  // from here on the label's fill position
    lab_ptr[i] = run;
    run += v;
  }
  __syncthreads();
  volatile int *fill = cnt;  // (a label's position is read and advanced by its one wave, batch after batch)
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int base = 0; base < m.n_arcs; base += 64) {
    const int i = base + lane;
    int l = -1;
    if (i < m.n_arcs) {
      const int a = m.arc_off + i, s = lat.arc_src[a];
      if (s != lat.arc_dst[a] && reach[s] != 0) l = lat.arc_label[a];
    }
    const bool mine = l >= 0 && (l & (kSpIndexWaves - 1)) == wv;
    unsigned long long rem = __builtin_amdgcn_ballot_w64(mine);
    while (rem) {  // (the same in every lane) one label of this batch per trip, led by its lowest lane
      const int lead = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(rem));
      const int L = read_lane(l, lead);
      const bool in_grp = mine && l == L;
      const unsigned long long grp = __builtin_amdgcn_ballot_w64(in_grp);
      const int at = fill[L];
      if (in_grp) lab_list[at + __popcll(grp & below)] = m.arc_off + i;
      if (lane == lead) fill[L] = at + __popcll(grp);
      rem &= ~grp;
    }
  }
}

// log of the sum of exp(term(i)), i < cnt, over the lanes of a wave (the header comment states the order).  Every lane of
// the wave calls it with the same cnt; term(i) is evaluated twice.
template <class T>
__device__ __forceinline__ double sp_wave_lse(int cnt, int lane, T term) {
  double mx = kNegInf64;
  for (int base = 0; base < cnt; base += 64) {
    const int i = base + lane;
    const double t = i < cnt ? term(i) : kNegInf64;
    mx = t > mx ? t : mx;  // (NaN adds nothing)
  }
  mx = wave_max(mx);
  if (!(mx > kNegInf64)) return kNegInf64;
  double sum = 0.0;
  for (int base = 0; base < cnt; base += 64) {
    const int i = base + lane;
    const double t = i < cnt ? term(i) : kNegInf64;
    sum += row_reduce<64>(slg_exp(t - mx), OpSum{});
  }
  return mx + log(sum);
}

// grid (B, y): the workgroups of a lattice take its candidates in turn.  F of a candidate is read where it exists: state
// 0 reaches the source (az > -inf; otherwise the arc adds nothing).
template <bool MK>
__global__ __launch_bounds__(kSpNextThreads) void k_string_next(nfst_batch lat, nfst_scores sc, SlIn in, SlWs w, SlgWs g, SpWs p,
                                                                double *next, double *eos, double *log_prefix, int32_t *status) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Meta m = load_meta(lat.meta, b);
  const int V = lat.vocab, N1 = in.N + 1, planes = MK ? 2 : 1;
  const float *theta = sc.theta + (size_t)sc.theta_stride * b;
  const float *arc_w = lat.weighted ? lat.arc_w : nullptr;
  const double *fcells = g.fcells + (size_t)m.row_off * w.stride_row;
  const double *az = g.az + m.row_off, *zn = p.zn + (size_t)m.row_off * planes;
  const int *lp = p.lab_ptr + (size_t)b * (V + 1), *list = p.lab_list + m.arc_off;
  const int32_t *yl = in.y_len + (size_t)b * in.M;
  for (int mc = blockIdx.y; mc < in.M; mc += gridDim.y) {
    const int n = yl[mc];
    double *nx = next + ((size_t)b * in.M + mc) * V;
    if (n < 0 || n > in.N) {  // (the same in every thread) a bad length: -inf, and none of the candidate's cells is read
      for (int v = tid; v < V; v += kSpNextThreads) nx[v] = kNegInf64;
      if (tid == 0) {
        *status = NFST_ERR_LENGTH;
        eos[(size_t)b * in.M + mc] = kNegInf64;
        log_prefix[(size_t)b * in.M + mc] = kNegInf64;
      }
      continue;
    }
    const double *f = fcells + (size_t)mc * w.stride_m + (MK ? N1 : 0) + n;  // F[.][n] (marker mode: F1), one row apart
    for (int v = wv; v < V; v += kSpNextWaves) {
      const bool on_tape = MK || in.keep[v] != 0;
      const int e0 = lp[v], cnt = on_tape ? lp[v + 1] - e0 : 0;
      const double th = (double)theta[v];
      const double r = sp_wave_lse(cnt, lane, [&](int i) {
        const int a = list[e0 + i], s = lat.arc_src[a];
        if (!(az[s] > kNegInf64)) return kNegInf64;
        double wa = th;
        if (arc_w) wa += (double)arc_w[a];
        if (sc.arc_scores) wa += (double)sc.arc_scores[a];
        return (f[(size_t)s * w.stride_row] + wa) + zn[(size_t)lat.arc_dst[a] * planes];
      });
      if (lane == 0) nx[v] = r;
    }
    __syncthreads();  // (next of this candidate is visible to wave 0)
    if (wv == 0) {
      const double e = az[m.sink] > kNegInf64 ? fcells[(size_t)m.sink * w.stride_row + (size_t)mc * w.stride_m + n] : kNegInf64;
      const double r = sp_wave_lse(V + 1, lane, [&](int i) { return i == 0 ? e : nx[i - 1]; });
      if (lane == 0) {
        eos[(size_t)b * in.M + mc] = e;
        log_prefix[(size_t)b * in.M + mc] = r;
      }
    }
  }
}

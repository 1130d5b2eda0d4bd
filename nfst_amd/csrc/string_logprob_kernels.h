// string_logprob_kernels.h -- the exact log weight of the paths of a lattice whose output tape spells a given string
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.21.
#pragma once

// k_string_logprob behind k_kbest_levels (kbest_kernels.h), on the canonical arrays only: the sum-semiring sibling of
// k_lattice_edit_sweep.  A state holds for every candidate string y (n tokens) one row G[s][0 .. n] of float64 log
// weights, j = the tokens of y already spelled (marker mode: two rows, G0 "the arc into s was no active marker" and G1
// "it was one").  The levels run in reverse; the work of a level is its (state, candidate, strip of 64 columns) items,
// one wave each.  Per out-arc the lane of column j loads G[d][j] or G[d][j + 1] from the row of the destination in the
// workspace -- the shifted operand is a load at the next address -- and folds arc score + operand into a running
// log-sum (sl_add: one exp per term, arcs in canonical order).  The candidates are independent of each other, so they are
// dealt to the gridDim.y workgroups of a lattice (candidate m belongs to workgroup m mod gridDim.y), each of which runs
// the whole sweep on its own candidates; workgroup 0 also carries log Z, one more item per state.  A barrier ends a level.
// LDS: order and level starts of the lattice (8 bytes per row).  No atomics: the same bits at every launch, for every
// grid and under every packing.
constexpr int kSlThreads = 1024, kSlWaves = kSlThreads / 64;
constexpr double kNegInf64 = -__builtin_huge_val();

// the caller's workspace (nfst_string_logprob_ws_bytes)
struct SlWs {
  double *cells;  // [total_rows, M, planes, N + 1]
  double *z;      // [total_rows] log of the weight of all paths from the row to the sink
  int *order;     // the level arrays of k_kbest_levels
  int *lev;
  int *n_lev;
  int64_t stride_m, stride_row;  // planes (N + 1), M planes (N + 1)
};
struct SlIn {
  const int32_t *y, *y_len;  // [B, M, N], [B, M]
  int M, N;
  const uint8_t *keep;  // [vocab] or null
  int marker;           // or -1
};

// the running log-sum (m, s): the sum so far is exp(m) s.  A term of -inf (or NaN) adds nothing.
__device__ __forceinline__ void sl_add(double &m, double &s, double t) {
  if (t > kNegInf64) {
    const double e = exp(-fabs(t - m));  // (m = -inf: 0)
    const bool up = t > m;
    s = up ? fma(s, e, 1.0) : s + e;
    m = up ? t : m;
  }
}
__device__ __forceinline__ double sl_log(double m, double s) { return m > kNegInf64 ? m + log(s) : kNegInf64; }

// the out-arcs of a state, 64 at a time on the lanes: destination, label, "the label is on the tape" (keep mode) or "the
// label is the marker" (marker mode), and the arc's score in float64, theta[label] + arc_w + arc_scores in this order
struct SlArcs {
  int dv, lv, kv;
  double sv;
};
__device__ __forceinline__ SlArcs sl_load_arcs(const nfst_batch &lat, const float *theta, const Extra &ex, const SlIn &in, int s, int ai, bool live) {
  SlArcs a = {s, 0, 0, 0.0};
  if (live) {
    a.dv = lat.arc_dst[ai];
    a.lv = lat.arc_label[ai];
    a.kv = in.keep ? (in.keep[a.lv] != 0) : (a.lv == in.marker);
    a.sv = (double)theta[a.lv];
    if (ex.arc_w) a.sv += (double)ex.arc_w[ai];
    if (ex.arc_scores) a.sv += (double)ex.arc_scores[ai];
  }
  return a;
}

// One item: columns 64 p + lane of the rows of state s for the candidate whose rows start at `cand` (an offset into a
// state's cells), n tokens y.  Every lane of the wave calls it with the same arguments.
template <bool MK>
__device__ __forceinline__ void sl_item(const nfst_batch &lat, const Meta &m, const float *theta, const Extra &ex, const SlIn &in,
                                        const int32_t *rp, double *cells, int64_t stride_row, int64_t cand, const int32_t *y, int n,
                                        int s, int p, int lane) {
  const int j = 64 * p + lane, N1 = in.N + 1;
  const bool in_row = j <= n, has_tok = j < n;
  double *out = cells + (size_t)s * stride_row + cand;
  if (s == m.sink) {  // the empty rest of a path spells the empty rest of y; a marker with nothing behind it spells nothing
    if (in_row) {
      out[j] = j == n ? 0.0 : kNegInf64;
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
        if (!kq) {
          if (in_row) v = row[j];
        } else if (match) {
          v = row[j + 1];
        }
        sl_add(m0, s0, sc + v);
      } else {
        double v0 = kNegInf64, v1 = kNegInf64;
        if (in_row) v0 = row[(kq ? N1 : 0) + j];
        if (match) v1 = row[j + 1];
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

// log Z of the rest of the lattice behind state s: the recurrence without a tape (every lane computes the same value)
__device__ __forceinline__ void sl_item_z(const nfst_batch &lat, const Meta &m, const float *theta, const Extra &ex, const SlIn &in,
                                          const int32_t *rp, double *z, int s, int lane) {
  double mz = kNegInf64, sz = 0.0;
  if (s == m.sink) {
    mz = 0.0;
    sz = 1.0;
  } else {
    const int a0 = rp[s], deg = rp[s + 1] - a0;
    for (int base = 0; base < deg; base += 64) {
      const SlArcs a = sl_load_arcs(lat, theta, ex, in, s, a0 + base + lane, base + lane < deg);
      const int cnt = deg - base < 64 ? deg - base : 64;
      for (int q = 0; q < cnt; ++q) {
        const int d = read_lane(a.dv, q);
        if (d == s) continue;
        sl_add(mz, sz, read_lane(a.sv, q) + z[d]);
      }
    }
  }
  if (lane == 0) z[s] = sl_log(mz, sz);
}

template <bool MK>
__global__ __launch_bounds__(kSlThreads) void k_string_logprob(nfst_batch lat, nfst_scores sc, SlIn in, SlWs w, double *log_num,
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
  const int32_t *yl = in.y_len + (size_t)b * in.M;
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
      const int n = yl[mc];
      if (n < 0 || n > in.N || 64 * p > n) continue;  // (a bad length: none of the candidate's tokens is read)
      sl_item<MK>(lat, m, theta, ex, in, rp, cells, w.stride_row, (int64_t)mc * w.stride_m, ys + (size_t)mc * in.N, n, s, p, lane);
    }
    __syncthreads();  // (the rows of this level are visible to the waves of the next one)
  }
  for (int mi = tid; mi < m_loc; mi += kSlThreads) {
    const int mc = yb + mi * Y, n = yl[mc];
    const bool ok = n >= 0 && n <= in.N;
    if (!ok) *status = NFST_ERR_LENGTH;
    log_num[(size_t)b * in.M + mc] = ok ? cells[(size_t)mc * w.stride_m] : kNegInf64;  // G0[state 0][0]
  }
  if (yb == 0 && tid == 0) logz[b] = z[0];
}

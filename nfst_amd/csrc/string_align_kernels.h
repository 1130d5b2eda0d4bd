// string_align_kernels.h -- the alignments of a lattice to given output strings: the best one and exact draws
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.24.
#pragma once

// Both ops answer from the suffix table of string_logprob_kernels.h, G[s][j] over (state, tokens of y already spelled),
// in the same workspace (SlWs) and behind the same k_kbest_levels:
//   k_string_viterbi_sweep   the max-plus sibling of k_string_logprob: the same items, the same grid, the same barrier
//                            per level; per arc an add and a max, no exp and no log Z item.  V[s][j] is the score of the
//                            best rest of a path from s that spells y[j:].
//   k_string_walk            one wave per walk from (state 0, column 0, plane 0) to the sink.  The lanes take the
//                            out-arcs of the state 64 at a time, each forms its term from the one cell its arc leads to.
//                            SAMPLE: the weights exp(term - cell of the state) are scanned inclusively over the wave,
//                            the running sum is carried from chunk to chunk and the first lane of positive weight
//                            whose running sum exceeds u wins (a ballot); if rounding leaves none, the last arc of
//                            positive weight.  Otherwise: the first lane whose term equals the state's cell, which
//                            holds by construction (the sweep's only operations are this add and a max).
// Only the canonical arrays are read, nothing is shared between walks and there are no atomics: the same bits at every
// launch, for every grid, under every packing and for every slicing of the candidates.
constexpr int kSaWalkWaves = 4;  // walks (waves) per workgroup of k_string_walk

// One item of the max sweep: sl_item with max for the running log-sum.
template <bool MK>
__device__ __forceinline__ void sa_item(const nfst_batch &lat, const Meta &m, const float *theta, const Extra &ex, const SlIn &in,
                                        const int32_t *rp, double *cells, int64_t stride_row, int64_t cand, const int32_t *y, int n,
                                        int s, int p, int lane) {
  const int j = 64 * p + lane, N1 = in.N + 1;
  const bool in_row = j <= n, has_tok = j < n;
  double *out = cells + (size_t)s * stride_row + cand;
  if (s == m.sink) {
    if (in_row) {
      out[j] = j == n ? 0.0 : kNegInf64;
      if (MK) out[N1 + j] = kNegInf64;
    }
    return;
  }
  const int ytok = has_tok ? y[j] : -1;
  double b0 = kNegInf64, b1 = kNegInf64;
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
        b0 = fmax(b0, sc + v);
      } else {
        double v0 = kNegInf64, v1 = kNegInf64;
        if (in_row) v0 = row[(kq ? N1 : 0) + j];
        if (match) v1 = row[j + 1];
        b0 = fmax(b0, sc + v0);
        b1 = fmax(b1, sc + v1);
      }
    }
  }
  if (in_row) {
    out[j] = b0;
    if (MK) out[N1 + j] = b1;
  }
}

template <bool MK>
__global__ __launch_bounds__(kSlThreads) void k_string_viterbi_sweep(nfst_batch lat, nfst_scores sc, SlIn in, SlWs w) {
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
  const int32_t *ys = in.y + (size_t)b * in.M * in.N;
  const int32_t *yl = in.y_len + (size_t)b * in.M;
  const int m_loc = in.M > yb ? (in.M - yb + Y - 1) / Y : 0;  // the candidates yb, yb + Y, ...
  const int strips = (in.N >> 6) + 1;                        // columns 0 .. N
  const int per_state = m_loc * strips;
  for (int L = n_lev - 1; L >= 0; --L) {
    const int lo = lev[L], hi = lev[L + 1];
    const int64_t items = (int64_t)(hi - lo) * per_state;
    for (int64_t it = wv; it < items; it += kSlWaves) {
      const int si = (int)(it / per_state), r = (int)(it - (int64_t)si * per_state);
      const int s = __builtin_amdgcn_readfirstlane(order[lo + si]);
      const int mi = r / strips, p = r - mi * strips, mc = yb + mi * Y;
      const int n = yl[mc];
      if (n < 0 || n > in.N || 64 * p > n) continue;  // (a bad length: none of the candidate's tokens is read)
      sa_item<MK>(lat, m, theta, ex, in, rp, cells, w.stride_row, (int64_t)mc * w.stride_m, ys + (size_t)mc * in.N, n, s, p, lane);
    }
    __syncthreads();  // (the rows of this level are visible to the waves of the next one)
  }
}

struct SaWalk {
  int K, m0;              // walks per candidate; the slice's first candidate among the caller's (the Philox counter's)
  const float *uniforms;  // [B, M, K, max_len] or null
  uint64_t seed;
  int max_len, pad;
};
struct SaOut {
  int32_t *paths, *path_arcs, *align;  // [B, M, K, max_len]
  int32_t *lengths;                    // [B, M, K]
  double *score;                       // [B, M, K]
  double *logq;                        // [B, M, K] (SAMPLE)
  int32_t *status;
};

// Stage S of the inclusive scan over a wave, as pos_scan_stage: groups of 2^S lanes, each lane with its prefix `pre`
// inside the group and the group's total `tot` (the same bits in all its lanes), merge in pairs.
template <int S>
__device__ __forceinline__ void sa_scan_stage(double &pre, double &tot, int lane) {
  const double o = wave_partner<S>(tot);
  pre = ((lane >> S) & 1) ? o + pre : pre;
  tot = tot + o;
}

template <bool MK, bool SAMPLE>
__global__ __launch_bounds__(kSaWalkWaves * 64) void k_string_walk(nfst_batch lat, nfst_scores sc, SlIn in, SlWs w, SaWalk wk, SaOut o) {
  const int lane = threadIdx.x & 63;
  const int64_t walk = (int64_t)blockIdx.x * kSaWalkWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (walk >= (int64_t)lat.n_lattices * in.M * wk.K) return;  // (a whole wave: the lanes of a walk stay together throughout)
  const int64_t bm = walk / wk.K;  // the walks of one (lattice, candidate) are neighbours: their cells share cache lines
  const int k = (int)(walk - bm * wk.K), b = (int)(bm / in.M), mc = (int)(bm - (int64_t)b * in.M);
  const Meta m = load_meta(lat.meta, b);
  const int N1 = in.N + 1, n = in.y_len[bm];
  int32_t *po = o.paths + (size_t)walk * wk.max_len;
  int32_t *ao = o.path_arcs + (size_t)walk * wk.max_len;
  int32_t *go = o.align + (size_t)walk * wk.max_len;
  int len = 0;
  double total = kNegInf64, lq = 0.0;
  if (n < 0 || n > in.N) {  // (the sweep has written no cell of this candidate)
    if (lane == 0) *o.status = NFST_ERR_LENGTH;
  } else {
    const int32_t *rp = lat.row_ptr + m.row_off + b;
    const int32_t *y = in.y + (size_t)bm * in.N;
    const float *theta = sc.theta + (size_t)sc.theta_stride * b;
    const Extra ex = {lat.weighted ? lat.arc_w : nullptr, sc.arc_scores};
    const double *cells = w.cells + (size_t)m.row_off * w.stride_row + (size_t)mc * w.stride_m;
    const float *us = SAMPLE && wk.uniforms ? wk.uniforms + (size_t)walk * wk.max_len : nullptr;
    const double top = cells[0];  // G0[state 0][0]: log_num (SAMPLE) or the best score
    double cur = top;
    if (cur > kNegInf64) {
      int s = 0, j = 0, f = 0;
      double sum = 0.0;
      bool cut = false;
      float ublk[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int t = 0; s != m.sink && t < m.n_rows; ++t) {  // (a step advances the level of the state)
        float u = 0.0f;
        if (SAMPLE) {
          if (us) {
            u = t < wk.max_len ? us[t] : 0.0f;  // (beyond max_len the walk is cut and reported)
          } else {  // one Philox block serves four steps
            if ((t & 3) == 0) philox_uniform4(wk.seed, (uint32_t)b, (uint32_t)(t >> 2), (uint32_t)(wk.m0 + mc), (uint32_t)k, ublk);
            u = (t & 3) == 0 ? ublk[0] : ((t & 3) == 1 ? ublk[1] : ((t & 3) == 2 ? ublk[2] : ublk[3]));
          }
        }
        const int a0 = rp[s], deg = rp[s + 1] - a0;
        const int ytok = j < n ? y[j] : -1;
        double run = 0.0;
        int take = -1, t_dst = 0, t_lab = 0, t_j = 0, t_f = 0, l_dst = 0, l_lab = 0, l_j = 0, l_f = 0, last = -1;
        double t_sc = 0.0, l_sc = 0.0;
        for (int base = 0; base < deg && take < 0; base += 64) {
          const SlArcs a = sl_load_arcs(lat, theta, ex, in, s, a0 + base + lane, base + lane < deg);
          // the cell the arc leads to: column nj, plane nf (marker mode); an arc off the string leads nowhere
          bool ok = a.dv != s;
          int nj = j, nf = 0;
          if (!MK) {
            if (a.kv) {
              ok = ok && j < n && ytok == a.lv;
              nj = j + 1;
            }
          } else if (f) {
            ok = ok && j < n && ytok == a.lv;
            nj = j + 1;
          } else {
            nf = a.kv;
          }
          double term = kNegInf64;
          if (ok) term = a.sv + cells[(size_t)a.dv * w.stride_row + (MK && nf ? N1 : 0) + nj];
          unsigned long long hit;
          if (SAMPLE) {
            const double x = ok ? exp(term - cur) : 0.0;  // (a term of -inf: 0)
            const bool pos = x > 0.0;
            double pre = pos ? x : 0.0, tot = pre;  // (a NaN weighs nothing)
            sa_scan_stage<0>(pre, tot, lane);
            sa_scan_stage<1>(pre, tot, lane);
            sa_scan_stage<2>(pre, tot, lane);
            sa_scan_stage<3>(pre, tot, lane);
            sa_scan_stage<4>(pre, tot, lane);
            sa_scan_stage<5>(pre, tot, lane);
            hit = __ballot(pos && run + pre > (double)u);
            const unsigned long long any = __ballot(pos);
            if (!hit && any) {  // (a chunk whose weights are all 0 is not chosen from)
              const int wl = 63 - __builtin_clzll(any);
              last = a0 + base + wl;
              l_dst = read_lane(a.dv, wl), l_lab = read_lane(a.lv, wl), l_j = read_lane(nj, wl), l_f = read_lane(nf, wl);
              l_sc = read_lane(a.sv, wl);
            }
            run += tot;
          } else {
            hit = __ballot(ok && term == cur);
          }
          if (hit) {
            const int wl = __builtin_ctzll(hit);
            take = a0 + base + wl;
            t_dst = read_lane(a.dv, wl), t_lab = read_lane(a.lv, wl), t_j = read_lane(nj, wl), t_f = read_lane(nf, wl);
            t_sc = read_lane(a.sv, wl);
          }
        }
        if (SAMPLE && take < 0 && last >= 0) take = last, t_dst = l_dst, t_lab = l_lab, t_j = l_j, t_f = l_f, t_sc = l_sc;
        if (take < 0) break;  // (never: a cell above -inf has an arc whose term is above -inf)
        if (len < wk.max_len) {
          if (lane == 0) {
            po[len] = t_lab;
            ao[len] = take;
            go[len] = t_j > j ? j : -1;
          }
          ++len;
        } else {
          cut = true;
        }
        sum += t_sc;
        s = t_dst, j = t_j, f = t_f;
        cur = cells[(size_t)s * w.stride_row + (MK && f ? N1 : 0) + j];
      }
      if (cut && lane == 0) *o.status = NFST_ERR_LENGTH;
      total = SAMPLE ? sum : top;
      lq = SAMPLE ? sum - top : 0.0;
    }
  }
  if (lane == 0) {
    o.lengths[walk] = len;
    o.score[walk] = total;
    if (SAMPLE) o.logq[walk] = lq;
  }
  for (int t = len + lane; t < wk.max_len; t += 64) {
    po[t] = wk.pad;
    ao[t] = -1;
    go[t] = -1;
  }
}

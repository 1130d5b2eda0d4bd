// string_extend_kernels.h -- prefix states: one column of the prefix table F per hypothesis, carried from symbol to symbol
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.25.
#pragma once

// A prefix state holds, for M hypotheses of every lattice, column n of k_string_logprob_fwd's table F for the
// hypothesis' prefix of n symbols: cell (row, plane, m) at ((row_off + row) planes + plane) M + m, float64 -- the
// hypotheses of one state are adjacent, and a child's gather from its parent's column stays inside one row.  Rows that
// state 0 does not reach are never written and never read.  Two kernels behind the context that nfst_string_prefix_open
// leaves (level arrays, in-arc lists, label lists, zn, az: the unchanged kernels of string_prefix_kernels.h and
// string_logprob_grad_kernels.h), on the canonical arrays only:
//   k_string_extend      grid (B, ceil(M_out / 64)): one ascending level sweep of one column for up to 64 child
//                        hypotheses per workgroup.  With Mp = the next power of two >= the workgroup's hypotheses, a wave
//                        item is 64 / Mp states of the level x Mp hypotheses; a lane owns one cell (F0 and F1 in marker
//                        mode) and walks the in-arc list of its state itself, in the list's order, with slg_item's
//                        recurrence at column n + 1 (the shifted operand is the parent's cell of the source state, the
//                        other one the child's own cell of the source state, written one level earlier).  The lanes of
//                        one state load the same arc, so those loads are broadcast; M = 1 puts 64 states on a wave and
//                        M = 64 reads every arc once per wave.  Order and level starts sit in LDS; one barrier ends a
//                        level.  A workgroup whose hypotheses are all dead writes its -inf without a sweep.
//   k_string_state_next  k_string_next with F[.][n] read from the state: the same terms, label lists, az guard and
//                        sp_wave_lse, so the same bits.
// A cell is computed by one lane in a fixed order and nothing is accumulated across lanes: no atomics, the same bits at
// every launch, for every grid and block size, under every packing and for every slicing of the children.
constexpr int kSeMaxM = 1024;

struct SeIn {
  const double *parent;         // the parents' state (null: M_in == 0)
  const int32_t *par, *sym;     // [B, M_out]: the parent slot (-2: the empty prefix, -1: dead) and the symbol
  double *out;                  // the children's state
  int M_in, M_out;
};

template <bool MK>
__global__ __launch_bounds__(kSlThreads) void k_string_extend(nfst_batch lat, nfst_scores sc, SlIn in, SlWs w, SlgWs g, SeIn x,
                                                              int32_t *status) {
  extern __shared__ int se_lds[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, threads = blockDim.x, waves = threads >> 6;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Meta m = load_meta(lat.meta, b);
  const int n_lev = w.n_lev[b];
  const int n_reach = w.lev[m.row_off + b + n_lev];
  int *order = se_lds, *lev = order + lat.max_rows;
  for (int i = tid; i < n_reach; i += threads) order[i] = w.order[m.row_off + i];
  for (int i = tid; i <= n_lev; i += threads) lev[i] = w.lev[m.row_off + b + i];
  __syncthreads();
  constexpr int planes = MK ? 2 : 1;
  // the hypotheses m_lo .. m_lo + m_cnt - 1 of this workgroup on the low bits of the lane, the states of an item above
  const int m_lo = 64 * blockIdx.y, m_cnt = x.M_out - m_lo < 64 ? x.M_out - m_lo : 64;
  int shift = 0;
  while ((1 << shift) < m_cnt) ++shift;
  const int h = lane & ((1 << shift) - 1), sub = lane >> shift, per_item = 64 >> shift;
  const bool has = h < m_cnt;
  const int mc = m_lo + h;
  int par = -1, sym = 0;
  if (has) {
    par = x.par[(size_t)b * x.M_out + mc];
    sym = x.sym[(size_t)b * x.M_out + mc];
    if (par < -2 || par >= x.M_in || (par >= 0 && (sym < 0 || sym >= lat.vocab))) {  // the slot is dead, the others go on
      *status = NFST_ERR_INDEX;
      par = -1;
    }
  }
  const bool live = par != -1, root = par == -2;
  double *out = x.out + (size_t)m.row_off * planes * x.M_out + mc;
  // (every wave holds the same hypotheses: the vote is the same in all of them)
  if (__builtin_amdgcn_ballot_w64(live) == 0) {
    for (int64_t i = tid; i < (int64_t)n_reach * planes * m_cnt; i += threads) {
      const int r = (int)(i / (planes * m_cnt)), q = (int)(i - (int64_t)r * planes * m_cnt);
      x.out[((size_t)(m.row_off + order[r]) * planes + q / m_cnt) * x.M_out + m_lo + q % m_cnt] = kNegInf64;
    }
    return;
  }
  const double *from = par >= 0 ? x.parent + (size_t)m.row_off * planes * x.M_in + par : nullptr;  // (no parent, no match)
  const int *ip = g.in_ptr + m.row_off + b, *in_list = g.in_list + m.arc_off;
  const float *theta = sc.theta + (size_t)sc.theta_stride * b;
  const float *arc_w = lat.weighted ? lat.arc_w : nullptr;
  const size_t so = (size_t)planes * x.M_out, si = (size_t)planes * x.M_in;  // a row's cells in the two states
  for (int L = 0; L < n_lev; ++L) {
    const int lo = lev[L], cnt = lev[L + 1] - lo;
    for (int it = wv * per_item + sub; it < cnt; it += waves * per_item) {
      if (!has) continue;
      const int s = order[lo + it];
      double c0 = kNegInf64, c1 = kNegInf64;
      if (live && s == 0) {
        c0 = root ? 0.0 : kNegInf64;  // the empty prefix has spelled nothing, behind no marker
      } else if (live) {
        double m0 = kNegInf64, s0 = 0.0, m1 = kNegInf64, s1 = 0.0;
        for (int e = ip[s], e1 = ip[s + 1]; e < e1; ++e) {
          const int ai = in_list[e], u = lat.arc_src[ai], l = lat.arc_label[ai];
          const bool kq = in.keep ? (in.keep[l] != 0) : (l == in.marker);
          double wa = (double)theta[l];
          if (arc_w) wa += (double)arc_w[ai];
          if (sc.arc_scores) wa += (double)sc.arc_scores[ai];
          const bool match = !root && sym == l;
          if (!MK) {
            double v = kNegInf64;
            if (!kq) v = out[u * so];
            else if (match) v = from[u * si];
            sl_add(m0, s0, wa + v);
          } else {
            const double f0 = out[u * so];
            const double v1 = match ? from[u * si + x.M_in] : kNegInf64;
            sl_add(m0, s0, wa + (kq ? kNegInf64 : f0));
            sl_add(m0, s0, wa + v1);
            sl_add(m1, s1, wa + (kq ? f0 : kNegInf64));
          }
        }
        c0 = sl_log(m0, s0);
        c1 = sl_log(m1, s1);
      }
      out[s * so] = c0;
      if (MK) out[s * so + x.M_out] = c1;
    }
    __syncthreads();  // (the cells of this level are visible to the waves of the next one)
  }
}

// grid (B, y): the workgroups of a lattice take its hypotheses in turn.  A dead slot's cells are -inf, and so is all it gets.
template <bool MK>
__global__ __launch_bounds__(kSpNextThreads) void k_string_state_next(nfst_batch lat, nfst_scores sc, SlIn in, SlgWs g, SpWs p,
                                                                      const double *state, int M, double *next, double *eos,
                                                                      double *log_prefix) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Meta m = load_meta(lat.meta, b);
  constexpr int planes = MK ? 2 : 1;
  const int V = lat.vocab;
  const float *theta = sc.theta + (size_t)sc.theta_stride * b;
  const float *arc_w = lat.weighted ? lat.arc_w : nullptr;
  const double *az = g.az + m.row_off, *zn = p.zn + (size_t)m.row_off * planes;
  const int *lp = p.lab_ptr + (size_t)b * (V + 1), *list = p.lab_list + m.arc_off;
  const size_t row = (size_t)planes * M;
  for (int mc = blockIdx.y; mc < M; mc += gridDim.y) {
    double *nx = next + ((size_t)b * M + mc) * V;
    const double *cells = state + (size_t)m.row_off * row + mc;
    const double *f = cells + (MK ? M : 0);  // F[.][n] (marker mode: F1), one row apart
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
        return (f[(size_t)s * row] + wa) + zn[(size_t)lat.arc_dst[a] * planes];
      });
      if (lane == 0) nx[v] = r;
    }
    __syncthreads();  // (next of this hypothesis is visible to wave 0)
    if (wv == 0) {
      const double e = az[m.sink] > kNegInf64 ? cells[(size_t)m.sink * row] : kNegInf64;
      const double r = sp_wave_lse(V + 1, lane, [&](int i) { return i == 0 ? e : nx[i - 1]; });
      if (lane == 0) {
        eos[(size_t)b * M + mc] = e;
        log_prefix[(size_t)b * M + mc] = r;
      }
    }
  }
}

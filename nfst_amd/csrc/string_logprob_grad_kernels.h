// string_logprob_grad_kernels.h -- the gradient of nfst_string_logprob's log_num and logz in every arc's score
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.22.
#pragma once

// Three kernels behind k_kbest_levels and the unchanged k_string_logprob (string_logprob_kernels.h), which leaves the
// suffix table G (and z, log Z of the rest of the lattice behind every state) in the workspace; canonical arrays only:
//   k_string_logprob_index  one workgroup per lattice: the arcs whose source state 0 reaches, without self loops, by
//                           (destination, canonical arc id) -- the in-arc lists that the prefix sweep pulls over -- and
//                           az = -inf for every row ("state 0 does not reach it" until the sweep says otherwise)
//   k_string_logprob_fwd    the mirror image of k_string_logprob on the same grid (B x Y, candidate m in workgroup m mod
//                           Y): the levels in ascending order, one wave per (state, candidate, strip of 64 columns), which
//                           pulls F[s][j] (+ the arc's score) over the in-arcs of the state in that list's order with
//                           sl_add; the shifted operand is a load at j - 1.  Marker mode: per in-arc first the F0 term,
//                           then the F1 term go into F0[d][j]; the F0 term of a marker arc goes into F1[d][j].  Workgroup
//                           0 also carries az, the log weight of all prefixes.  A barrier ends a level.
//   k_string_logprob_arcs   one launch over the arcs of the batch, whatever Y was: one wave per arc loops over the
//                           candidates in ascending order and over the strips of a candidate in ascending order; lane j
//                           forms its term, the wave adds the 64 terms in the fixed tree of row_reduce<64> (wave_ops.h),
//                           the strips' sums are added one after the other, and lane 0 does the ordered accumulation
//                           over the candidates and the one store.
// No atomics on values: the same bits at every launch, for every grid Y, under every packing and for every slicing of
// the candidates (nfst_hip.h states the order of every sum).
constexpr int kSlgIndexThreads = 1024, kSlgArcThreads = 256, kSlgArcWaves = kSlgArcThreads / 64;

// the part of the caller's workspace behind SlWs (nfst_string_logprob_grad_ws_bytes)
struct SlgWs {
  double *fcells;   // [total_rows, M, planes, N + 1] the prefix table F, laid out as SlWs::cells
  double *az;       // [total_rows] log of the weight of all path prefixes from state 0 to the row (-inf: none)
  double *log_num;  // [B, M], [B]: the outputs of k_string_logprob
  double *logz;
  int *in_ptr;      // [total_rows + n_lattices] first in-entry of every state (relative to the lattice), then the end
  int *in_list;     // [total_arcs] per lattice from arc_off: canonical arc ids by (destination, id)
  int *in_tmp;      // [total_arcs] the same entries in the order they were found
};

__device__ __forceinline__ double slg_exp(double t) { return t > kNegInf64 ? exp(t) : 0.0; }  // (-inf and NaN: nothing)

// LDS: in-entry counts, fill positions and reach flags (12 bytes per row), one int per thread for the scan.  Integers
// throughout: the result does not depend on the order of the atomic adds.
__global__ __launch_bounds__(kSlgIndexThreads) void k_string_logprob_index(nfst_batch lat, SlWs w, SlgWs g) {
  extern __shared__ int slg_lds[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const Meta m = load_meta(lat.meta, b);
  const int n = m.n_rows;
  int *cnt = slg_lds, *fill = cnt + n + 1, *reach = fill + n, *scan = reach + n;
  const int n_reach = w.lev[m.row_off + b + w.n_lev[b]];
  int *in_ptr = g.in_ptr + m.row_off + b, *in_list = g.in_list + m.arc_off, *in_tmp = g.in_tmp + m.arc_off;
  for (int i = tid; i <= n; i += kSlgIndexThreads) cnt[i] = 0;
  for (int i = tid; i < n; i += kSlgIndexThreads) {
    reach[i] = 0;
    g.az[m.row_off + i] = kNegInf64;
  }
  __syncthreads();
  for (int i = tid; i < n_reach; i += kSlgIndexThreads) reach[w.order[m.row_off + i]] = 1;
  __syncthreads();
  // an arc counts when it is no self loop, state 0 reaches its source and it does not lead back into state 0
  auto counts = [&](int a, int &d) {
    const int s = lat.arc_src[a];
    d = lat.arc_dst[a];
    return s != d && d != 0 && reach[s] != 0;
  };
  for (int i = tid; i < m.n_arcs; i += kSlgIndexThreads) {
    int d;
    if (counts(m.arc_off + i, d)) atomicAdd(&cnt[d], 1);
  }
  __syncthreads();
  const int chunk = (n + kSlgIndexThreads - 1) / kSlgIndexThreads, c0 = min(tid * chunk, n), c1 = min(c0 + chunk, n);
  int part = 0;
  for (int i = c0; i < c1; ++i) part += cnt[i];
  scan[tid] = part;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < kSlgIndexThreads; ++i) { const int v = scan[i]; scan[i] = run; run += v; }
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
  for (int i = tid; i < m.n_arcs; i += kSlgIndexThreads) {
    int d;
    if (counts(m.arc_off + i, d)) in_tmp[atomicAdd(&fill[d], 1)] = i;
  }
  __syncthreads();
  // a state's in-entries were filled in any order: every arc finds its rank among them (canonical order)
  for (int i = tid; i < m.n_arcs; i += kSlgIndexThreads) {
    int d;
    if (!counts(m.arc_off + i, d)) continue;
    const int j0 = cnt[d], j1 = cnt[d + 1];
    int rank = 0;
    for (int j = j0; j < j1; ++j) rank += in_tmp[j] < i;
    in_list[j0 + rank] = m.arc_off + i;
  }
}

// the in-arcs of a state, 64 at a time on the lanes: SlArcs with dv = the arc's source
__device__ __forceinline__ SlArcs slg_load_in_arcs(const nfst_batch &lat, const float *theta, const Extra &ex, const SlIn &in,
                                                   const int *in_list, int e, bool live) {
  SlArcs a = {0, 0, 0, 0.0};
  if (live) {
    const int ai = in_list[e];
    a.dv = lat.arc_src[ai];
    a.lv = lat.arc_label[ai];
    a.kv = in.keep ? (in.keep[a.lv] != 0) : (a.lv == in.marker);
    a.sv = (double)theta[a.lv];
    if (ex.arc_w) a.sv += (double)ex.arc_w[ai];
    if (ex.arc_scores) a.sv += (double)ex.arc_scores[ai];
  }
  return a;
}

// One item of the prefix sweep: columns 64 p + lane of the rows of state s for the candidate whose rows start at `cand`,
// n tokens y.  Every lane of the wave calls it with the same arguments.
template <bool MK>
__device__ __forceinline__ void slg_item(const nfst_batch &lat, const float *theta, const Extra &ex, const SlIn &in, const int *ip,
                                         const int *in_list, double *fcells, int64_t stride_row, int64_t cand, const int32_t *y,
                                         int n, int s, int p, int lane) {
  const int j = 64 * p + lane, N1 = in.N + 1;
  const bool in_row = j <= n;
  double *out = fcells + (size_t)s * stride_row + cand;
  if (s == 0) {  // the empty prefix has spelled nothing, behind no marker
    if (in_row) {
      out[j] = j == 0 ? 0.0 : kNegInf64;
      if (MK) out[N1 + j] = kNegInf64;
    }
    return;
  }
  const int yprev = (in_row && j >= 1) ? y[j - 1] : -1;  // (labels are not negative: -1 matches none)
  double m0 = kNegInf64, s0 = 0.0, m1 = kNegInf64, s1 = 0.0;
  const int e0 = ip[s], deg = ip[s + 1] - e0;
  for (int base = 0; base < deg; base += 64) {
    const SlArcs a = slg_load_in_arcs(lat, theta, ex, in, in_list, e0 + base + lane, base + lane < deg);
    const int cnt = deg - base < 64 ? deg - base : 64;
    for (int q = 0; q < cnt; ++q) {
      const int u = read_lane(a.dv, q), l = read_lane(a.lv, q), kq = read_lane(a.kv, q);
      const double sc = read_lane(a.sv, q);
      const double *row = fcells + (size_t)u * stride_row + cand;
      const bool match = yprev == l;
      if (!MK) {
        double v = kNegInf64;
        if (!kq) {
          if (in_row) v = row[j];
        } else if (match) {
          v = row[j - 1];
        }
        sl_add(m0, s0, sc + v);
      } else {
        double v0 = kNegInf64, v1 = kNegInf64, vm = kNegInf64;
        if (in_row) {
          const double f0 = row[j];
          if (kq) vm = f0;
          else v0 = f0;
        }
        if (match) v1 = row[N1 + j - 1];
        sl_add(m0, s0, sc + v0);
        sl_add(m0, s0, sc + v1);
        sl_add(m1, s1, sc + vm);
      }
    }
  }
  if (in_row) {
    out[j] = sl_log(m0, s0);
    if (MK) out[N1 + j] = sl_log(m1, s1);
  }
}

// log of the weight of all prefixes that end in state s (every lane computes the same value)
__device__ __forceinline__ void slg_item_z(const nfst_batch &lat, const float *theta, const Extra &ex, const SlIn &in, const int *ip,
                                           const int *in_list, double *az, int s, int lane) {
  double mz = kNegInf64, sz = 0.0;
  if (s == 0) {
    mz = 0.0;
    sz = 1.0;
  } else {
    const int e0 = ip[s], deg = ip[s + 1] - e0;
    for (int base = 0; base < deg; base += 64) {
      const SlArcs a = slg_load_in_arcs(lat, theta, ex, in, in_list, e0 + base + lane, base + lane < deg);
      const int cnt = deg - base < 64 ? deg - base : 64;
      for (int q = 0; q < cnt; ++q) sl_add(mz, sz, read_lane(a.sv, q) + az[read_lane(a.dv, q)]);
    }
  }
  if (lane == 0) az[s] = sl_log(mz, sz);
}

template <bool MK>
__global__ __launch_bounds__(kSlThreads) void k_string_logprob_fwd(nfst_batch lat, nfst_scores sc, SlIn in, SlWs w, SlgWs g) {
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
  const int *ip = g.in_ptr + m.row_off + b, *in_list = g.in_list + m.arc_off;
  const float *theta = sc.theta + (size_t)sc.theta_stride * b;
  const Extra ex = {lat.weighted ? lat.arc_w : nullptr, sc.arc_scores};
  double *fcells = g.fcells + (size_t)m.row_off * w.stride_row;
  double *az = g.az + m.row_off;
  const int32_t *ys = in.y + (size_t)b * in.M * in.N;
  const int32_t *yl = in.y_len + (size_t)b * in.M;
  const int m_loc = in.M > yb ? (in.M - yb + Y - 1) / Y : 0;  // the candidates yb, yb + Y, ...
  const int strips = (in.N >> 6) + 1;                        // columns 0 .. N
  const int cell_items = m_loc * strips, per_state = cell_items + (yb == 0 ? 1 : 0);
  for (int L = 0; L < n_lev; ++L) {
    const int lo = lev[L], hi = lev[L + 1];
    const int64_t items = (int64_t)(hi - lo) * per_state;
    for (int64_t it = wv; it < items; it += kSlWaves) {
      const int si = (int)(it / per_state), r = (int)(it - (int64_t)si * per_state);
      const int s = __builtin_amdgcn_readfirstlane(order[lo + si]);
      if (r == cell_items) {
        slg_item_z(lat, theta, ex, in, ip, in_list, az, s, lane);
        continue;
      }
      const int mi = r / strips, p = r - mi * strips, mc = yb + mi * Y;
      const int n = yl[mc];
      if (n < 0 || n > in.N || 64 * p > n) continue;  // (a bad length: none of the candidate's tokens is read)
      slg_item<MK>(lat, theta, ex, in, ip, in_list, fcells, w.stride_row, (int64_t)mc * w.stride_m, ys + (size_t)mc * in.N, n, s, p, lane);
    }
    __syncthreads();  // (the rows of this level are visible to the waves of the next one)
  }
}

// The arc pass.  grid (B, y): the waves of a lattice's workgroups take its arcs in turn.  F and G of a candidate are
// read where both exist: state 0 reaches the source (az > -inf; otherwise the arc gives 0) and so the destination.
template <bool MK>
__global__ __launch_bounds__(kSlgArcThreads) void k_string_logprob_arcs(nfst_batch lat, nfst_scores sc, SlIn in, SlWs w, SlgWs g,
                                                                        const double *g_num, const double *g_z, int accumulate,
                                                                        double *grad_arc) {
  const int b = blockIdx.x, lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const Meta m = load_meta(lat.meta, b);
  const float *theta = sc.theta + (size_t)sc.theta_stride * b;
  const double *gcells = w.cells + (size_t)m.row_off * w.stride_row, *fcells = g.fcells + (size_t)m.row_off * w.stride_row;
  const double *z = w.z + m.row_off, *az = g.az + m.row_off;
  const int32_t *ys = in.y + (size_t)b * in.M * in.N;
  const int32_t *yl = in.y_len + (size_t)b * in.M;
  const double *ln = g.log_num + (size_t)b * in.M, *gn = g_num + (size_t)b * in.M;
  const int N1 = in.N + 1;
  for (int i = blockIdx.y * kSlgArcWaves + wv; i < m.n_arcs; i += gridDim.y * kSlgArcWaves) {
    const int a = m.arc_off + i;
    const int s = lat.arc_src[a], d = lat.arc_dst[a], l = lat.arc_label[a];
    const bool kq = in.keep ? (in.keep[l] != 0) : (l == in.marker);
    double wa = (double)theta[l];
    if (lat.weighted) wa += (double)lat.arc_w[a];
    if (sc.arc_scores) wa += (double)sc.arc_scores[a];
    const bool dead = s == d || !(az[s] > kNegInf64);  // a self loop, or state 0 does not reach the arc
    double acc = 0.0;
    if (accumulate) acc = grad_arc[a];
    else if (!dead && z[0] > kNegInf64) acc = g_z[b] * slg_exp(((az[s] + wa) + z[d]) - z[0]);
    if (!dead) {
      const double *fs = fcells + (size_t)s * w.stride_row, *gd = gcells + (size_t)d * w.stride_row;
      for (int mc = 0; mc < in.M; ++mc) {
        const double gm = gn[mc], lnum = ln[mc];
        const int n = yl[mc];
        if (gm == 0.0 || n < 0 || n > in.N || !(lnum > kNegInf64)) continue;  // (the same in every lane)
        const int32_t *y = ys + (size_t)mc * in.N;
        const double *f0 = fs + (size_t)mc * w.stride_m, *g0 = gd + (size_t)mc * w.stride_m;
        double post = 0.0;
        for (int p = 0; 64 * p <= n; ++p) {
          const int j = 64 * p + lane;
          const bool in_row = j <= n, match = j < n && y[j] == l;
          double e = 0.0;
          if (!MK) {
            if (!kq) {
              if (in_row) e = slg_exp(((f0[j] + wa) + g0[j]) - lnum);
            } else if (match) {
              e = slg_exp(((f0[j] + wa) + g0[j + 1]) - lnum);
            }
          } else {
            if (in_row) e = slg_exp(((f0[j] + wa) + g0[(kq ? N1 : 0) + j]) - lnum);
            if (match) e += slg_exp(((f0[N1 + j] + wa) + g0[j + 1]) - lnum);
          }
          post += row_reduce<64>(e, OpSum{});
        }
        acc += gm * post;
      }
    }
    if (lane == 0) grad_arc[a] = acc;
  }
}

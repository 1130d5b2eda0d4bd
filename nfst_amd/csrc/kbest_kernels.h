// kbest_kernels.h -- exact k best paths per lattice (max-plus with k-best lists)
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md section 4.6.
#pragma once

// Three kernels, one workgroup per lattice each, on the canonical arrays only (row_ptr, arc_src, arc_dst, arc_label,
// arc_w; tile programs and chunked programs are not read):
//   k_kbest_levels  Kahn's algorithm in LDS over the arcs without self loops: a topological order of the states that
//                   state 0 reaches, cut into levels (longest distance from state 0)
//   k_kbest_sweep   the levels in reverse: every state merges its successors' lists, each shifted by its arc's score,
//                   into its own top k (one wave per state, one lane per out-arc holding that list's head); the merge
//                   is kb_merge_state, which k_positional_kbest_sweep (positional_kbest_kernels.h) shares
//   k_kbest_walk    k lanes follow the back pointers from state 0 and write labels, arcs and lengths
// A list entry is (float score, uint32 payload), payload = arc_in_lattice << 6 | rank in the successor's list; the
// sink's one entry is (0.0f, kKbSinkPay).  A list shorter than k ends with an entry of score -inf.
constexpr int kKbMaxK = 64;
constexpr int kKbLevelThreads = 1024, kKbSweepThreads = 1024, kKbSweepWaves = kKbSweepThreads / 64;
constexpr uint32_t kKbSinkPay = 0xffffffffu;

// the caller's workspace (nfst_kbest_ws_bytes)
struct KbWs {
  uint2 *lists;  // [total_rows, k] (score bits, payload)
  int *order;    // [total_rows] per lattice from row_off: the reachable states by level
  int *lev;      // [total_rows + n_lattices] per lattice from row_off + b: first position of every level, then the end
  int *n_lev;    // [n_lattices] levels
};

// order-preserving bits of a float ("greater" as unsigned integers); the key of a candidate puts them above the
// complement of its payload: one unsigned compare orders (score desc, arc asc, rank asc).  0 = no candidate.
__device__ __forceinline__ uint32_t kb_ord(float x) {
  const uint32_t u = __float_as_uint(x);
  return u ^ (uint32_t)(((int)u >> 31) | (int)0x80000000);
}
__device__ __forceinline__ uint64_t kb_key(float c, uint32_t pay) {
  return c > kNegInf ? (((uint64_t)kb_ord(c) << 32) | (uint32_t)~pay) : 0ull;  // (-inf and NaN are no candidates)
}

// Pass 1: levels.  LDS: in-degree, order and level starts, 12 bytes per row.
__global__ __launch_bounds__(kKbLevelThreads) void k_kbest_levels(nfst_batch lat, KbWs w) {
  extern __shared__ int kb_lds[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const Meta m = load_meta(lat.meta, b);
  const int n = m.n_rows;
  int *indeg = kb_lds, *order = indeg + n, *lev = order + n, *tail = lev + n + 1;
  const int32_t *rp = lat.row_ptr + m.row_off + b;
  for (int i = tid; i < n; i += kKbLevelThreads) indeg[i] = 0;
  __syncthreads();
  for (int a = m.arc_off + tid; a < m.arc_off + m.n_arcs; a += kKbLevelThreads) {
    const int s = lat.arc_src[a], d = lat.arc_dst[a];
    if (s != d) atomicAdd(&indeg[d], 1);
  }
  if (tid == 0) { order[0] = 0; lev[0] = 0; *tail = 1; }
  __syncthreads();
  int lo = 0, hi = 1, L = 0;
  while (lo < hi) {
    for (int i = lo + tid; i < hi; i += kKbLevelThreads) {
      const int s = order[i];
      for (int a = rp[s]; a < rp[s + 1]; ++a) {
        const int d = lat.arc_dst[a];
        if (d != s && atomicSub(&indeg[d], 1) == 1) order[atomicAdd(tail, 1)] = d;
      }
    }
    __syncthreads();
    const int nh = *tail;
    __syncthreads();  // (everyone has read the tail before the next level appends to it)
    ++L;
    if (tid == 0) lev[L] = hi;
    lo = hi;
    hi = nh;
  }
  // L levels: lev[0 .. L) are their starts, lev[L] = the number of reachable states
  __syncthreads();
  for (int i = tid; i < lo; i += kKbLevelThreads) w.order[m.row_off + i] = order[i];
  for (int i = tid; i <= L; i += kKbLevelThreads) w.lev[m.row_off + b + i] = lev[i];
  if (tid == 0) w.n_lev[b] = L;
}

// maximum of a 64-bit key over the wave: the four DPP stages of wave_ops.h on its halves leave every 16-lane row with
// its maximum, the four rows are combined in scalar registers
struct KbKey { uint32_t hi, lo; };
template <int S>
__device__ __forceinline__ KbKey wave_partner(KbKey x) { return {wave_partner<S>(x.hi), wave_partner<S>(x.lo)}; }
__device__ __forceinline__ uint64_t kb_wave_max(uint64_t key) {
  const KbKey x = butterfly<4>(KbKey{(uint32_t)(key >> 32), (uint32_t)key}, [](KbKey a, KbKey o) {
    return (((uint64_t)o.hi << 32) | o.lo) > (((uint64_t)a.hi << 32) | a.lo) ? o : a;
  });
  uint64_t r = 0;
#pragma unroll
  for (int row = 0; row < 4; ++row) {
    const uint64_t v = ((uint64_t)(uint32_t)read_lane((int)x.hi, row * 16) << 32) | (uint32_t)read_lane((int)x.lo, row * 16);
    r = v > r ? v : r;
  }
  return r;
}

// The merge of one state s (not the sink) into its list `out`, by one wave.  The out-arcs a0 .. a0 + d of s go to the
// lanes in chunks: the first chunk has 64 arcs, every further one 63 arcs and, in lane 63, the list merged so far (the
// "carry", in LDS).  A lane holds its list's head (and the entry after it, loaded ahead); each pop is a wave maximum of
// the lanes' keys, and the winning lane advances.  `lists` holds the successors' lists (k entries per state), lab(l) the
// label term of a candidate, buf0 two k-entry buffers of this wave in LDS.
template <class LabF>
__device__ __forceinline__ void kb_merge_state(const nfst_batch &lat, const Meta &m, const Extra &ex, LabF lab, const uint2 *lists,
                                               int k, int s, int a0, int d, uint2 *buf0, int lane, uint2 *out) {
  const uint2 kNone = make_uint2(__float_as_uint(kNegInf), 0u);
  int cnt = 0, sel = 0;
  for (int base = 0; base < d || base == 0; base += (base == 0 ? 64 : 63)) {
    const uint2 *prev = buf0 + sel * 64;
    uint2 *cur = buf0 + (sel ^ 1) * 64;
    const bool carry = base > 0 && lane == 63;
    const int pc = cnt;  // entries of the carry list
    const int a = a0 + base + lane;
    const bool live = !carry && base + lane < d;
    // this lane's list: its head (score c, payload) and the entry after it
    int r = 0;
    float c = kNegInf, e = 0.0f, th = 0.0f;
    uint32_t pay = 0, arel = 0;
    const uint2 *lst = nullptr;
    uint2 nxt = kNone;
    if (live) {
      const int dst = lat.arc_dst[a];
      if (dst != s) {
        th = lab(lat.arc_label[a]);
        e = ex.at(a);
        lst = lists + (size_t)dst * k;
        const uint2 h = lst[0];
        if (k > 1) nxt = lst[1];
        arel = (uint32_t)(a - m.arc_off);
        c = e + (th + __uint_as_float(h.x));  // the adds of k_viterbi, in its order
        pay = arel << 6;
      }
    } else if (carry && pc > 0) {
      const uint2 h = prev[0];
      c = __uint_as_float(h.x);
      pay = h.y;
    }
    uint64_t key = kb_key(c, pay);
    cnt = 0;
    for (; cnt < k; ++cnt) {
      const uint64_t mx = kb_wave_max(key);
      if (mx == 0) break;
      if (key == mx) {
        cur[cnt] = make_uint2(__float_as_uint(c), pay);
        ++r;
        if (carry) {
          const uint2 h = r < pc ? prev[r] : kNone;
          c = __uint_as_float(h.x);
          pay = h.y;
        } else {
          const uint2 h = nxt;
          if (r + 1 < k) nxt = lst[r + 1];
          c = r < k ? e + (th + __uint_as_float(h.x)) : kNegInf;
          pay = (arel << 6) | (uint32_t)r;
        }
        key = kb_key(c, pay);
      }
    }
    // LDS accesses of one wave execute in order; the next chunk's carry and the copy below read `cur`
    asm volatile("" ::: "memory");
    sel ^= 1;
  }
  if (lane < k) out[lane] = lane < cnt ? buf0[sel * 64 + lane] : kNone;
  asm volatile("" ::: "memory");
}

// Pass 2: the backward k-best sweep.  A wave owns one state of a level at a time (kb_merge_state).  LDS: order and level
// starts of the lattice (8 bytes per row) and two k-entry buffers per wave.
__global__ __launch_bounds__(kKbSweepThreads) void k_kbest_sweep(nfst_batch lat, nfst_scores sc, int k, KbWs w) {
  extern __shared__ int kb_lds[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Meta m = load_meta(lat.meta, b);
  const int n_lev = w.n_lev[b];
  const int n_reach = w.lev[m.row_off + b + n_lev];
  uint2 *bufs = (uint2 *)kb_lds;  // [kKbSweepWaves][2][64]
  int *order = (int *)(bufs + kKbSweepWaves * 2 * 64), *lev = order + lat.max_rows;
  for (int i = tid; i < n_reach; i += kKbSweepThreads) order[i] = w.order[m.row_off + i];
  for (int i = tid; i <= n_lev; i += kKbSweepThreads) lev[i] = w.lev[m.row_off + b + i];
  __syncthreads();
  const int32_t *rp = lat.row_ptr + m.row_off + b;
  const float *theta = sc.theta + (size_t)sc.theta_stride * b;
  const Extra ex = {lat.weighted ? lat.arc_w : nullptr, sc.arc_scores};
  uint2 *lists = w.lists + (size_t)m.row_off * k;
  const uint2 kNone = make_uint2(__float_as_uint(kNegInf), 0u);
  uint2 *buf0 = bufs + wv * 128;
  for (int L = n_lev - 1; L >= 0; --L) {
    const int lo = lev[L], hi = lev[L + 1];
    for (int i = lo + wv; i < hi; i += kKbSweepWaves) {
      const int s = order[i];
      uint2 *out = lists + (size_t)s * k;
      if (s == m.sink) {
        if (lane < k) out[lane] = lane == 0 ? make_uint2(__float_as_uint(0.0f), kKbSinkPay) : kNone;
        continue;
      }
      const int a0 = rp[s];
      kb_merge_state(lat, m, ex, [&](int l) { return theta[l]; }, lists, k, s, a0, rp[s + 1] - a0, buf0, lane, out);
    }
    __syncthreads();  // (the lists of this level are visible to the waves of the next one)
  }
}

// Pass 3: the paths.  Lane j < k walks entry j of state 0's list.
__global__ __launch_bounds__(64) void k_kbest_walk(nfst_batch lat, int k, KbWs w, float *best, int32_t *paths,
                                                   int32_t *path_arcs, int32_t *lengths, int32_t *n_paths, int max_len,
                                                   int pad, int32_t *status) {
  const int b = blockIdx.x, j = threadIdx.x;
  const Meta m = load_meta(lat.meta, b);
  const uint2 *lists = w.lists + (size_t)m.row_off * k;
  float sc = kNegInf;
  if (j < k) sc = __uint_as_float(lists[j].x);  // state 0 is reachable: its list exists
  const bool found = j < k && sc > kNegInf;
  const int np = __popcll(__builtin_amdgcn_ballot_w64(found));
  if (j == 0) n_paths[b] = np;
  if (j >= k) return;
  const size_t row = (size_t)b * k + j;
  best[row] = found ? sc : kNegInf;
  int32_t *po = paths + row * max_len;
  int32_t *ao = path_arcs ? path_arcs + row * max_len : nullptr;
  int len = 0;
  if (found) {
    uint32_t pay = lists[j].y;
    while (pay != kKbSinkPay) {
      if ((pay >> 6) >= (uint32_t)m.n_arcs || (pay & 63u) >= (uint32_t)k) break;  // (never on a valid batch)
      if (len >= max_len) { *status = NFST_ERR_LENGTH; break; }
      const int a = m.arc_off + (int)(pay >> 6);
      po[len] = lat.arc_label[a];
      if (ao) ao[len] = a;
      ++len;
      pay = lists[(size_t)lat.arc_dst[a] * k + (pay & 63u)].y;
    }
  }
  lengths[row] = len;
  for (int t = len; t < max_len; ++t) {
    po[t] = pad;
    if (ao) ao[t] = -1;
  }
}

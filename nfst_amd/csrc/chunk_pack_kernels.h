// chunk_pack_kernels.h -- the chunk cutter on the device (include/nfst_hip.h, nfst_pack_chunks_device_*).
// Part of the single translation unit kernels.hip (device code in an anonymous namespace), after pack_kernels.h.
//
// A batch packed on the device (the reference's trainer hands set_masks tables that already live on the GPU) gets its
// chunked programs cut where it is: the device packer has just computed every state's depth and height and its in- and
// out-arc lists (k_pack_lattice, still in its workspace), which is all chunk_pack.cpp's cut() needs.  The same cuts,
// BIT-IDENTICAL to nfst_pack_chunks:
//   k_chunk_plan   one workgroup per (lattice, direction): positions = reachable states by (level, state id) (a bitonic sort of
//                  64-bit keys in LDS, the order of std::stable_sort by level), the reach of every arc and the deepest operand
//                  below every cut (atomicMin in LDS over the <= 63 positions an arc crosses), entry counts by a block scan;
//                  every plan of chunk_cost.h's search on a lane of its own (<= 126), the cheapest by (cycles, loop index);
//                  the winner again on one lane, writing its chunk starts.  Summary per program, positions, entry counts,
//                  chunk starts and chunk offsets in the cutter's workspace.
//   (host: nfst_pack_chunks_device_layout, the layout routine of nfst_pack_chunks)
//   k_chunk_emit   one workgroup per (lattice, direction): tab, pos, and the entries and labels of every position (a lane per
//                  position, its arcs in canonical order), chunks padded to multiples of eight.
#pragma once

#include "chunk_cost.h"

// cutter workspace: per lattice and direction four int32 arrays of n_rows + 2 entries (positions, entries before a
// position, chunk starts, chunk offsets), in front of lattice b: 8 (row_off[b] + 2 b) words
__host__ __device__ inline int64_t cp_ws_words(int64_t n_lattices, int64_t total_rows) { return 8 * (total_rows + 2 * n_lattices); }

struct CpArgs {
  // the device packer's workspace and the arc-list layout it was sized with (nfst_arcs_device)
  const int32_t *pk_ws;
  const int64_t *row_off, *arc_off;
  int64_t in_rows, in_arcs;
  int32_t n_lattices;
  // the packed batch (device)
  const int32_t *meta, *arc_src, *arc_dst, *arc_label;
  // cuts
  int32_t threads, max_chunks;
  int64_t lds_bytes;
  int32_t *ws;
  int32_t *summary;  // [2 B, NFST_CHK_SUM_WORDS]
  // emit: the layout's chunk meta (device) and the arrays
  const int32_t *cmeta;
  int32_t *tab, *pos;
  uint32_t *stream;
  uint16_t *label;
};

// what one (lattice, direction) workgroup reads: the packer's views of the lattice and the cutter's own arrays
struct CpView {
  int n, n_r, arc_base;
  const int32_t *level, *reach, *ptr, *list, *operand;
  int32_t *order, *pre, *starts, *cbeg;
};
__device__ __forceinline__ CpView cp_view(const CpArgs &a, int b, int dir) {
  const int32_t *m = a.meta + (size_t)b * NFST_META_WORDS;
  CpView v;
  v.n = m[NFST_META_N_ROWS];
  v.n_r = m[NFST_META_N_REACH];
  v.arc_base = m[NFST_META_ARC_OFF];
  // (k_pack_lattice's layout: g_dep, g_hei, ..., in_ptr, out_ptr of n + 2 entries; in- and out-arc lists by canonical id)
  const int32_t *wrow = a.pk_ws + (size_t)kPkRowArrays * (a.row_off[b] + 2 * b);
  const int rs = v.n + 2;
  const int64_t a0 = a.arc_off[b], A_in = a.arc_off[b + 1] - a0;
  const int32_t *warc = a.pk_ws + (size_t)kPkRowArrays * (a.in_rows + 2 * a.n_lattices) + (size_t)kPkArcArrays * a0;
  v.reach = wrow;                                    // depth >= 0: reachable from the start
  v.level = dir ? wrow + rs : wrow;                  // longest path to the sink / from the start
  v.ptr = dir ? wrow + 5 * rs : wrow + 4 * rs;       // out- / in-arc list pointers
  v.list = dir ? warc + 3 * A_in : warc + 2 * A_in;  // out- / in-arc lists
  v.operand = (dir ? a.arc_dst : a.arc_src) + v.arc_base;
  int32_t *w = a.ws + (size_t)8 * (a.row_off[b] + 2 * b) + (size_t)dir * 4 * rs;
  v.order = w; v.pre = w + rs; v.starts = w + 2 * rs; v.cbeg = w + 3 * rs;
  return v;
}

// dynamic LDS of k_chunk_plan for lattices of up to `rows` rows: sort keys, position of every state (int16), low, pre
__host__ __device__ inline int64_t cp_plan_lds(int rows) {
  int np2 = 1;
  while (np2 < rows) np2 <<= 1;
  return (int64_t)np2 * 8 + (((int64_t)rows * 2 + 15) & ~(int64_t)15) + 2 * (((int64_t)rows + 2) * 4 + 8);
}

__global__ __launch_bounds__(kPkThreads) void k_chunk_plan(CpArgs a, int rows) {
  extern __shared__ unsigned long long cp_lds[];
  __shared__ int red[64];
  __shared__ int sh[8];
  __shared__ double cyc_s[128];
  __shared__ int ok_s[128];
  const int b = blockIdx.x >> 1, dir = blockIdx.x & 1, tid = threadIdx.x;
  const int32_t *m = a.meta + (size_t)b * NFST_META_WORDS;
  int32_t *sum = a.summary + (size_t)blockIdx.x * NFST_CHK_SUM_WORDS;
  const CpView v = cp_view(a, b, dir);
  const int n = v.n, n_r = v.n_r;
  auto refuse = [&]() {
    if (tid < NFST_CHK_SUM_WORDS) sum[tid] = 0;
  };
  // (the refusals of nfst_pack_chunks before the cut: too many arcs for an entry's 24 bits, fewer than two positions)
  if (m[NFST_META_N_ARCS] >= (1 << 24) || n_r < 2 || n > rows) { refuse(); return; }
  int np2 = 1;
  while (np2 < rows) np2 <<= 1;
  unsigned long long *keys = cp_lds;
  int16_t *posof = reinterpret_cast<int16_t *>(keys + np2);
  int32_t *low = reinterpret_cast<int32_t *>(posof + ((rows + 7) & ~7));
  int32_t *pre = low + ((rows + 2 + 1) & ~1);
  // ---- positions: reachable states by (level, id) -- unreachable ones sort behind them
  for (int s = tid; s < n; s += kPkThreads)
    keys[s] = v.reach[s] >= 0 ? ((unsigned long long)v.level[s] << 16) | (unsigned long long)s : (1ull << 40) | (unsigned long long)s;
  for (int s = tid; s < n; s += kPkThreads) posof[s] = -1;
  if (tid == 0) { sh[0] = 0; sh[1] = 0; sh[2] = 1; }
  __syncthreads();
  pk_sort(keys, n);
  auto order = [&](int p) { return (int)(keys[p] & 0xffffull); };
  for (int p = tid; p < n_r; p += kPkThreads) {
    const int s = order(p);
    posof[s] = (int16_t)p;
    v.order[p] = s;
  }
  for (int x = tid; x <= n_r; x += kPkThreads) low[x] = x;
  // position 0 must be the start (alpha) / the sink (beta)
  if (tid == 0 && order(0) != (dir ? m[NFST_META_SINK] : 0)) sh[0] = 1;
  // entries of positions [1, p): one per arc, one for a position without arcs
  const int total = pk_scan<false>(n_r, [&](int p) {
    if (p == 0) return 0;
    const int s = order(p);
    return max(v.ptr[s + 1] - v.ptr[s], 1);
  }, pre, red);
  if (tid == 0) pre[n_r] = total;
  // ---- the reach of every arc, and per cut the deepest operand below it
  int w_t = 0, bad = 0;
  for (int p = tid + 1; p < n_r && !bad; p += kPkThreads) {
    const int s = order(p);
    for (int j = v.ptr[s]; j < v.ptr[s + 1]; ++j) {
      const int q = posof[v.operand[v.list[j]]];
      if (q < 0 || q >= p || p - q > nfst_chunk::kMaxReach) { bad = 1; break; }
      w_t = max(w_t, p - q);
      for (int x = q + 1; x <= p; ++x) atomicMin(&low[x], q);
    }
  }
  if (bad) atomicOr(&sh[0], 1);
  if (w_t) atomicMax(&sh[1], w_t);
  __syncthreads();
  if (sh[0]) { refuse(); return; }
  int fb_t = 1;
  for (int x = tid + 1; x < n_r; x += kPkThreads) fb_t = max(fb_t, x - low[x]);
  if (fb_t > 1) atomicMax(&sh[2], fb_t);
  __syncthreads();
  const int R = max(4, nfst_chunk::pow2_at_least(sh[1] + 1)), Fb = sh[2], K = 2 * Fb;
  // ---- every plan on a lane of its own
  if (tid < 128) {
    int ok = 0;
    double cyc = 0.0;
    if (tid < K) {
      int pc, pf;
      ok = nfst_chunk::plan_cut(nfst_chunk::plan_ft(Fb, tid), nfst_chunk::plan_lane_cap(tid), n_r, pre, low, R, a.threads, a.lds_bytes,
                                a.max_chunks, [](int) {}, &pc, &pf, &cyc) ? 1 : 0;
    }
    ok_s[tid] = ok;
    cyc_s[tid] = cyc;
  }
  __syncthreads();
  // the cheapest by (cycles, loop index): the plan the host loop keeps
  if (tid < 64) {
    int bk = -1;
    double bc = 0.0;
    for (int k = tid; k < 128; k += 64)
      if (ok_s[k] && (bk < 0 || cyc_s[k] < bc)) { bk = k; bc = cyc_s[k]; }
    for (int off = 32; off > 0; off >>= 1) {
      const int ok = __shfl_xor(bk, off);
      const double oc = __shfl_xor(bc, off);
      if (ok >= 0 && (bk < 0 || oc < bc || (oc == bc && ok < bk))) { bk = ok; bc = oc; }
    }
    if (tid == 0) sh[3] = bk;
  }
  __syncthreads();
  const int best = sh[3];
  if (best < 0) { refuse(); return; }
  // ---- the winner again, writing its chunk starts
  if (tid == 0) {
    int C = 0, F = 0, n_st = 0;
    double cyc = 0.0;
    int32_t *starts = v.starts;
    nfst_chunk::plan_cut(nfst_chunk::plan_ft(Fb, best), nfst_chunk::plan_lane_cap(best), n_r, pre, low, R, a.threads, a.lds_bytes,
                         a.max_chunks, [&](int st) { starts[n_st++] = st; }, &C, &F, &cyc);
    const bool fits = !(C * F > a.threads || nfst_chunk::lds_need(C, F, R) > a.lds_bytes || F > R);
    sh[4] = fits ? C : 0;
    sh[5] = F;
    unsigned long long bits = (unsigned long long)__double_as_longlong(cyc);
    sum[NFST_CHK_SUM_CYCLES] = (int32_t)(uint32_t)bits;
    sum[NFST_CHK_SUM_CYCLES + 1] = (int32_t)(uint32_t)(bits >> 32);
  }
  __syncthreads();
  const int C = sh[4];
  if (C == 0) { refuse(); return; }
  // chunk offsets in the program's stream: entries of every chunk, padded to a multiple of eight
  const int entries = pk_scan<false>(C, [&](int c) {
    const int e = pre[c + 1 < C ? v.starts[c + 1] : n_r] - pre[v.starts[c]];
    return (e + 7) / 8 * 8;
  }, v.cbeg, red);
  for (int x = tid; x <= n_r; x += kPkThreads) v.pre[x] = pre[x];
  if (tid == 0) {
    v.cbeg[C] = entries;
    sum[NFST_CHK_SUM_OK] = 1; sum[NFST_CHK_SUM_C] = C; sum[NFST_CHK_SUM_F] = sh[5]; sum[NFST_CHK_SUM_R] = R;
    sum[NFST_CHK_SUM_NPOS] = n_r; sum[NFST_CHK_SUM_ENTRIES] = entries;
  }
}

__global__ __launch_bounds__(kPkThreads) void k_chunk_emit(CpArgs a) {
  extern __shared__ int32_t cp_posof[];
  const int b = blockIdx.x >> 1, dir = blockIdx.x & 1, tid = threadIdx.x;
  const CpView v = cp_view(a, b, dir);
  const int32_t *cm = a.cmeta + (size_t)blockIdx.x * NFST_CHK_META_WORDS;
  const int C = cm[NFST_CHK_C], R = cm[NFST_CHK_R], n_r = cm[NFST_CHK_NPOS];
  int32_t *tab = a.tab + (size_t)cm[NFST_CHK_TAB_OFF] * 4, *pos = a.pos + cm[NFST_CHK_POS_OFF];
  uint32_t *stream = a.stream + cm[NFST_CHK_STREAM_OFF];
  uint16_t *label = a.label + cm[NFST_CHK_STREAM_OFF];
  const int32_t *arc_label = a.arc_label + v.arc_base;
  for (int s = tid; s < v.n; s += kPkThreads) cp_posof[s] = -1;
  __syncthreads();
  for (int p = tid; p < n_r; p += kPkThreads) {
    const int s = v.order[p];
    cp_posof[s] = p;
    pos[p] = s;
  }
  for (int c = tid; c < C; c += kPkThreads) {
    const int e0 = v.cbeg[c], e1 = v.cbeg[c + 1];
    tab[c * 4 + 0] = v.starts[c]; tab[c * 4 + 1] = e0; tab[c * 4 + 2] = e1 - e0; tab[c * 4 + 3] = 0;
    // (a chunk's entries are walked eight at a time without a bounds test: padded with zero-weight entries)
    const int end = c + 1 < C ? v.starts[c + 1] : n_r;
    for (int k = e0 + v.pre[end] - v.pre[v.starts[c]]; k < e1; ++k) { stream[k] = NFST_CHK_ZERO; label[k] = 0; }
  }
  __syncthreads();
  for (int p = tid + 1; p < n_r; p += kPkThreads) {
    int lo = 0, hi = C - 1;  // the chunk of position p: the last start <= p (starts[0] = 1)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (v.starts[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const int at = v.cbeg[lo] + v.pre[p] - v.pre[v.starts[lo]];
    const int s = v.order[p];
    const int j0 = v.ptr[s], cnt = v.ptr[s + 1] - j0;
    if (cnt == 0) { stream[at] = NFST_CHK_LAST | NFST_CHK_ZERO; label[at] = 0; }
    for (int j = 0; j < cnt; ++j) {
      const int arc = v.list[j0 + j];
      const int q = cp_posof[v.operand[arc]];
      stream[at + j] = (uint32_t)(q & (R - 1)) | (j + 1 == cnt ? NFST_CHK_LAST : 0u) | ((uint32_t)arc << 8);
      label[at + j] = (uint16_t)arc_label[arc];
    }
  }
}

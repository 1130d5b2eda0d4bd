// lattice_edit_kernels.h -- the edit distance between a reference string and a whole lattice, with the oracle path
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.18.
#pragma once

// Two kernels behind k_kbest_levels (kbest_kernels.h), one workgroup per lattice each, on the canonical arrays only:
//   k_lattice_edit_sweep  the levels in reverse: a state's row E[s][0 .. n] of cells (dist, score) lies on the lanes in
//                         strips of 64 columns, one wave per (state, strip).  Per out-arc the wave loads the successor's
//                         strip from the workspace, takes the column j + 1 from the lane above (one DPP move per word;
//                         lane 63 loads its neighbour, the boundary element of the strip) and folds the insertion and
//                         the match/substitution into a 64-bit key, smaller = better.  The deletion chain
//                         E[j] = min_{k >= j} (C[k] + (k - j)) is a suffix minimum of the keys of C[k] + k (le_suffix_min)
//                         inside a strip and, through the strips' minima in LDS, over the strips behind it, with j
//                         subtracted afterwards.
//   k_lattice_edit_walk   one wave follows the cells from (state 0, column 0): lanes over the out-arcs of the state, a
//                         ballot picks the first candidate that reproduces the cell (arcs in canonical order, match or
//                         substitution before insertion, the deletion last)
// A cell is (int32 dist, float32 score bits); dist = kLeNoDist marks a cell that no candidate path reaches.  SC = false
// (no scores given) computes with every term 0.0f and reads neither theta nor per-arc extras.  No atomics: the same bits
// at every launch.
constexpr int kLeThreads = 1024, kLeWaves = kLeThreads / 64;
constexpr int kLeNoDist = 0x3fffffff;
constexpr uint64_t kLeNone = ~0ull;

// the caller's workspace (nfst_lattice_edit_ws_bytes)
struct LeWs {
  int2 *cells;  // [total_rows, stride] (dist, score bits)
  int *order;   // the level arrays of k_kbest_levels
  int *lev;
  int *n_lev;
  int stride;   // R + 1
};
struct LeIn {
  const int32_t *ref, *ref_len;
  int R;
};
struct LeOut {
  int32_t *distance;
  float *score;
  int32_t *paths, *path_arcs, *align, *lengths, *counts;
  int max_len, pad;
  int32_t *status;
};

// (dist asc, score desc) as one unsigned compare: dist above the complement of the score's order-preserving bits.  A
// score of -inf or NaN is no candidate.
__device__ __forceinline__ uint64_t le_key(int dist, float c) {
  return c > kNegInf ? (((uint64_t)(uint32_t)dist << 32) | (uint32_t)~kb_ord(c)) : kLeNone;
}
// the candidate that extends the cell (sd, sv) by an arc of terms (e, th) at `add` more edits
template <bool SC>
__device__ __forceinline__ uint64_t le_extend(int sd, int sv, int add, float e, float th) {
  const float c = SC ? e + (th + __int_as_float(sv)) : 0.0f;  // the adds of nfst_kbest, in its order
  return sd != kLeNoDist ? le_key(sd + add, c) : kLeNone;
}
__device__ __forceinline__ int2 le_cell(uint64_t key) {
  const uint32_t o = ~(uint32_t)key;  // kb_ord of the score
  const uint32_t u = (o >> 31) ? (o ^ 0x80000000u) : ~o;
  return key == kLeNone ? make_int2(kLeNoDist, 0) : make_int2((int)(key >> 32), (int)u);
}

__device__ __forceinline__ KbKey le_split(uint64_t k) { return {(uint32_t)(k >> 32), (uint32_t)k}; }
__device__ __forceinline__ uint64_t le_join(KbKey k) { return ((uint64_t)k.hi << 32) | k.lo; }
__device__ __forceinline__ uint64_t le_min(uint64_t a, uint64_t b) { return b < a ? b : a; }

// One stage of the suffix scan over aligned blocks of 2^S lanes: `tot` is the minimum of the lane's block (the same in
// all its lanes), `suf` the minimum over the lanes of the block from this one on.  The partner of stage S lies in the
// other half of the block of 2^(S + 1) lanes; a lane of the lower half has all of the upper half behind it.
template <int S>
__device__ __forceinline__ void le_scan_stage(uint64_t &suf, uint64_t &tot, int lane) {
  const uint64_t o = le_join(wave_partner<S>(le_split(tot)));
  suf = (lane >> S) & 1 ? suf : le_min(suf, o);
  tot = le_min(tot, o);
}
// min over the lanes l' >= lane of key, and of `carry`; carry takes the wave's minimum in.
// The four DPP stages of wave_ops.h scan every row of 16 lanes; the four row minima are combined in scalar registers.
__device__ __forceinline__ uint64_t le_suffix_min(uint64_t key, int lane, uint64_t &carry) {
  uint64_t suf = key, tot = key;
  le_scan_stage<0>(suf, tot, lane);
  le_scan_stage<1>(suf, tot, lane);
  le_scan_stage<2>(suf, tot, lane);
  le_scan_stage<3>(suf, tot, lane);
  const KbKey t = le_split(tot);
  uint64_t row[4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
    row[r] = ((uint64_t)(uint32_t)read_lane((int)t.hi, r * 16) << 32) | (uint32_t)read_lane((int)t.lo, r * 16);
  const uint64_t a3 = carry, a2 = le_min(row[3], a3), a1 = le_min(row[2], a2), a0 = le_min(row[1], a1);
  carry = le_min(row[0], a0);
  const int r = lane >> 4;
  return le_min(suf, r == 3 ? a3 : r == 2 ? a2 : r == 1 ? a1 : a0);
}

// C[s][64 p + lane], the best candidate through the out-arcs of state s (not yet the deletion chain), as a key; the sink
// holds (n - j, 0.0f).  Every lane of the wave calls it with the same s and p.
template <bool SC>
__device__ __forceinline__ uint64_t le_fold(const nfst_batch &lat, const Meta &m, const float *theta, const Extra &ex, const int32_t *rp,
                                            const int32_t *ref, const int2 *cells, int stride, int n, int s, int p, int lane) {
  const int j = 64 * p + lane;
  const bool in_row = j <= n, has_tok = j < n;
  if (s == m.sink) return in_row ? le_key(n - j, 0.0f) : kLeNone;
  const int rtok = has_tok ? ref[j] : 0;
  const int a0 = rp[s], deg = rp[s + 1] - a0;
  uint64_t acc = kLeNone;
  for (int base = 0; base < deg; base += 64) {
    // the arcs of this chunk, one per lane; the loop below takes them one by one from the lanes
    const int ai = a0 + base + lane;
    const bool live = base + lane < deg;
    const int dv = live ? lat.arc_dst[ai] : s;
    const int lv = live ? lat.arc_label[ai] : 0;
    float thv = 0.0f, ev = 0.0f;
    if (SC && live) {
      thv = theta[lv];
      ev = ex.at(ai);
    }
    const int cnt = deg - base < 64 ? deg - base : 64;
    for (int q = 0; q < cnt; ++q) {
      const int d = read_lane(dv, q);
      if (d == s) continue;  // (a self loop is on no path; the same in every lane)
      const int l = read_lane(lv, q);
      const float th = read_lane(thv, q), e = read_lane(ev, q);
      const int2 *row = cells + (size_t)d * stride;
      int2 cd = make_int2(kLeNoDist, 0), bd = make_int2(kLeNoDist, 0);
      if (in_row) cd = row[j];
      if (lane == 63 && j + 1 <= n) bd = row[j + 1];  // the boundary element: column 0 of the strip behind
      const int nd = wave_shl1(cd.x, bd.x), nv = wave_shl1(cd.y, bd.y);  // E[d][j + 1]
      const uint64_t ki = le_extend<SC>(cd.x, cd.y, 1, e, th);
      const uint64_t ks = has_tok ? le_extend<SC>(nd, nv, l != rtok ? 1 : 0, e, th) : kLeNone;
      acc = le_min(acc, le_min(ki, ks));
    }
  }
  return acc;
}

// Pass 2: the backward sweep.  The work of a level is its (state, strip) items, dealt to the waves in turn, in blocks of
// at most kLeItems items (whole states).  An item folds its strip (le_fold), scans the keys of C[k] + k inside the strip
// and leaves the strip's minimum in LDS; with one strip per row that is the row, and the cell is stored at once.  With
// more strips the scanned keys go to the row's cells as they are, and behind a barrier the same wave takes the item
// again, folds the minima of the strips behind it in and stores the cells.  LDS: the strip minima (8 kLeItems bytes),
// then order and level starts of the lattice (8 bytes per row).  A lattice whose reference length lies outside [0, R]
// sets the status and is left alone: none of its tokens is read.
constexpr int kLeItems = 1024;
template <bool SC>
__global__ __launch_bounds__(kLeThreads) void k_lattice_edit_sweep(nfst_batch lat, nfst_scores sc, LeIn in, LeWs w, int32_t *status) {
  extern __shared__ uint64_t le_lds[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = in.ref_len[b];
  if (n < 0 || n > in.R) {  // (the same in every thread of the workgroup: nobody waits at a barrier)
    if (tid == 0) *status = NFST_ERR_LENGTH;
    return;
  }
  const Meta m = load_meta(lat.meta, b);
  const int n_lev = w.n_lev[b];
  const int n_reach = w.lev[m.row_off + b + n_lev];
  uint64_t *tot = le_lds;
  int *order = (int *)(tot + kLeItems), *lev = order + lat.max_rows;
  for (int i = tid; i < n_reach; i += kLeThreads) order[i] = w.order[m.row_off + i];
  for (int i = tid; i <= n_lev; i += kLeThreads) lev[i] = w.lev[m.row_off + b + i];
  __syncthreads();
  const int32_t *rp = lat.row_ptr + m.row_off + b;
  const int32_t *ref = in.ref + (size_t)b * in.R;
  const float *theta = SC ? sc.theta + (size_t)sc.theta_stride * b : nullptr;
  const Extra ex = {SC && lat.weighted ? lat.arc_w : nullptr, SC ? sc.arc_scores : nullptr};
  int2 *cells = w.cells + (size_t)m.row_off * w.stride;
  const int strips = (n >> 6) + 1;  // columns 0 .. n: at most 17
  const int per = kLeItems / strips;  // states of a block
  for (int L = n_lev - 1; L >= 0; --L) {
    const int lo = lev[L], hi = lev[L + 1];
    for (int s0 = lo; s0 < hi; s0 += per) {
      const int items = (hi - s0 < per ? hi - s0 : per) * strips;
      for (int it = wv; it < items; it += kLeWaves) {
        const int si = it / strips, p = it - si * strips, j = 64 * p + lane;
        const int s = __builtin_amdgcn_readfirstlane(order[s0 + si]);
        const uint64_t acc = le_fold<SC>(lat, m, theta, ex, rp, ref, cells, w.stride, n, s, p, lane);
        // the deletion chain inside the strip: keys of C[k] + k, suffix minimum (j is subtracted when the cell is stored)
        uint64_t mn = kLeNone;
        const uint64_t key = le_suffix_min(acc == kLeNone ? kLeNone : acc + ((uint64_t)(uint32_t)j << 32), lane, mn);
        int2 *out = cells + (size_t)s * w.stride;
        if (strips == 1) {
          if (j <= n) out[j] = le_cell(key == kLeNone ? kLeNone : key - ((uint64_t)(uint32_t)j << 32));
        } else {
          if (j <= n) ((uint64_t *)out)[j] = key;
          if (lane == 0) tot[it] = mn;
        }
      }
      if (strips > 1) {
        __syncthreads();  // (the strip minima are in LDS)
        for (int it = wv; it < items; it += kLeWaves) {  // the same items on the same waves
          const int si = it / strips, p = it - si * strips, j = 64 * p + lane;
          const int s = __builtin_amdgcn_readfirstlane(order[s0 + si]);
          uint64_t behind = kLeNone;
          for (int p2 = p + 1; p2 < strips; ++p2) behind = le_min(behind, tot[it - p + p2]);
          int2 *out = cells + (size_t)s * w.stride;
          if (j <= n) {
            const uint64_t key = le_min(((uint64_t *)out)[j], behind);
            out[j] = le_cell(key == kLeNone ? kLeNone : key - ((uint64_t)(uint32_t)j << 32));
          }
        }
      }
      __syncthreads();  // (the rows of this block are visible to the waves of the next one; the minima may be overwritten)
    }
  }
}

// Pass 3: the oracle path.  One wave; state, column and cell are the same in every lane.
template <bool SC>
__global__ __launch_bounds__(64) void k_lattice_edit_walk(nfst_batch lat, nfst_scores sc, LeIn in, LeWs w, LeOut o) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const Meta m = load_meta(lat.meta, b);
  const int n = in.ref_len[b];
  int32_t *po = o.paths + (size_t)b * o.max_len;
  int32_t *ao = o.path_arcs ? o.path_arcs + (size_t)b * o.max_len : nullptr;
  int32_t *go = o.align ? o.align + (size_t)b * o.max_len : nullptr;
  int len = 0, dist = -1, n_sub = 0, n_ins = 0, n_del = 0;
  float best = kNegInf;
  if (n >= 0 && n <= in.R) {  // (otherwise the sweep has set the status and written no cell)
    const int32_t *rp = lat.row_ptr + m.row_off + b;
    const int32_t *ref = in.ref + (size_t)b * in.R;
    const float *theta = SC ? sc.theta + (size_t)sc.theta_stride * b : nullptr;
    const Extra ex = {SC && lat.weighted ? lat.arc_w : nullptr, SC ? sc.arc_scores : nullptr};
    const int2 *cells = w.cells + (size_t)m.row_off * w.stride;
    int s = 0, j = 0;
    int2 cur = cells[0];
    if (cur.x != kLeNoDist) {
      dist = cur.x;
      best = __int_as_float(cur.y);
      for (int it = 0; s != m.sink && it <= m.n_rows + n; ++it) {  // (a step advances the state or the column)
        const int a0 = rp[s], deg = rp[s + 1] - a0;
        const int tok = j < n ? ref[j] : 0;
        int take = -1, t_sub = 0, t_neq = 0, t_dst = 0, t_lab = 0;
        for (int base = 0; base < deg && take < 0; base += 64) {
          const int ai = a0 + base + lane;
          const bool live = base + lane < deg;
          const int d = live ? lat.arc_dst[ai] : s;
          int l = 0, neq = 0;
          bool sub_ok = false, ins_ok = false;
          if (d != s) {
            l = lat.arc_label[ai];
            float th = 0.0f, e = 0.0f;
            if (SC) {
              th = theta[l];
              e = ex.at(ai);
            }
            const int2 *row = cells + (size_t)d * w.stride;
            const int2 cd = row[j];
            if (j < n) {
              const int2 cn = row[j + 1];
              neq = l != tok ? 1 : 0;
              const int2 c = le_cell(le_extend<SC>(cn.x, cn.y, neq, e, th));
              sub_ok = c.x != kLeNoDist && c.x == cur.x && c.y == cur.y;
            }
            const int2 c = le_cell(le_extend<SC>(cd.x, cd.y, 1, e, th));
            ins_ok = c.x != kLeNoDist && c.x == cur.x && c.y == cur.y;
          }
          const uint64_t hit = __builtin_amdgcn_ballot_w64(sub_ok || ins_ok);
          if (hit) {
            const int wl = __builtin_ctzll(hit);
            take = a0 + base + wl;
            t_sub = read_lane(sub_ok ? 1 : 0, wl);
            t_neq = read_lane(neq, wl);
            t_dst = read_lane(d, wl);
            t_lab = read_lane(l, wl);
          }
        }
        if (take < 0) {  // the deletion of r[j]
          if (j >= n) break;  // (never on cells the sweep wrote)
          ++j;
          ++n_del;
        } else {
          if (len < o.max_len) {
            if (lane == 0) {
              po[len] = t_lab;
              if (ao) ao[len] = take;
              if (go) go[len] = t_sub ? j : -1;
            }
            ++len;
          } else if (lane == 0) {
            *o.status = NFST_ERR_LENGTH;  // (cut here; the counts still cover the whole path)
          }
          if (t_sub) {
            n_sub += t_neq;
            ++j;
          } else {
            ++n_ins;
          }
          s = t_dst;
        }
        cur = cells[(size_t)s * w.stride + j];
      }
      n_del += n - j;  // at the sink the rest of r is deleted
    }
  }
  if (lane == 0) {
    o.distance[b] = dist;
    if (o.score) o.score[b] = best;
    o.lengths[b] = len;
    if (o.counts) {
      o.counts[3 * b] = n_sub;
      o.counts[3 * b + 1] = n_ins;
      o.counts[3 * b + 2] = n_del;
    }
  }
  for (int t = len + lane; t < o.max_len; t += 64) {
    po[t] = o.pad;
    if (ao) ao[t] = -1;
    if (go) go[t] = -1;
  }
}

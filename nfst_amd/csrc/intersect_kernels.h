// intersect_kernels.h -- the product of every lattice with a deterministic automaton over the labels
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.8.
#pragma once

// Two kernels, one 1024-thread workgroup per lattice each, on the canonical arrays only (row_ptr, arc_dst, arc_label),
// after k_kbest_levels has written the level order of the lattice to the workspace:
//   k_intersect_count  the sets of automaton states per lattice state as 64-bit masks in LDS: fwd (reached from (0, 0)),
//                      level by level, then live = fwd restricted to the pairs that reach a final pair of the sink, in
//                      reverse level order; the row id of every state's first pair, the pair of every product row and
//                      the out-arc count of every product row, turned into offsets by block prefix sums
//   k_intersect_write  one lane per product row (one wave per heavy row) writes the row's arcs at its offset
// A union into another state's mask is an LDS atomic OR: it does not depend on the order, so the masks are the same from
// launch to launch.  The backward pass keeps bwd(s) only inside fwd(s) -- q in fwd(s) with delta[q][l] = t has t in
// fwd(d), so t in bwd(d) iff t in live(d): the mask it propagates is live itself, and fwd + live are the 16 bytes per row.
// The automaton is label-major: delta[l * 64 + q] (int8, -1 = no transition): one arc's label is one 64-byte line.
constexpr int kIsThreads = 1024, kIsWaves = kIsThreads / 64;
constexpr int kIsGroup = 8;   // lanes that share the out-arcs of one lattice state in the mask passes
constexpr int kIsHeavy = 64;  // a state (or product row) with more arcs than this is swept by a whole wave
static_assert(kIsThreads == kPkThreads, "the block scans of pack_kernels.h are written for this block size");

typedef unsigned long long is_mask;

// the caller's workspace (nfst_intersect_ws_bytes)
struct IsWs {
  int *order;     // [total_rows] per lattice from row_off: the reachable states by level (k_kbest_levels)
  int *lev;       // [total_rows + n_lattices] per lattice from row_off + b: first position of every level, then the end
  int *n_lev;     // [n_lattices]
  is_mask *live;  // [total_rows]
  int *first;     // [total_rows] product row of the state's first pair
  int *pair;      // [n_lattices, NFST_MAX_ROWS] state << 6 | q of every product row
  int *aoff;      // [n_lattices, NFST_MAX_ROWS] first arc of every product row, relative to the lattice's first
  int *n_out;     // [n_lattices] product rows (0: none, or beyond the limit: nothing to write)
};
struct IsDfa {
  const int8_t *delta;  // [V, 64] (+ delta_stride per lattice)
  int64_t delta_stride;
  const is_mask *fin;   // final states as a mask (+ fin_stride per lattice)
  int64_t fin_stride;
};
struct IsOut {
  const int64_t *row_off, *arc_off;  // [n_lattices] first row / arc of every lattice in the outputs
  int32_t *src, *label, *dst;
  int64_t *arc_map;
  int32_t *arc_q, *row_state, *row_q;
};

// { delta[q][l] >= 0 : q in m }; row = the label's 64-byte line
__device__ __forceinline__ is_mask is_image(is_mask m, const int8_t *row) {
  is_mask r = 0;
  while (m) {
    const int q = __builtin_ctzll(m);
    m &= m - 1;
    const int t = row[q];
    if (t >= 0) r |= 1ull << (t & 63);
  }
  return r;
}
// { q in m : delta[q][l] in tgt }
__device__ __forceinline__ is_mask is_preimage(is_mask m, is_mask tgt, const int8_t *row) {
  is_mask r = 0;
  while (m) {
    const int q = __builtin_ctzll(m);
    m &= m - 1;
    const int t = row[q];
    if (t >= 0 && ((tgt >> (t & 63)) & 1)) r |= 1ull << q;
  }
  return r;
}
// the product row that canonical arc a of row `self` = (s, q) leads to, or -1 if the product has no such arc
__device__ __forceinline__ int is_dst_row(const nfst_batch &lat, int a, int s, int q, int sink, int self, const int8_t *delta,
                                          const is_mask *live, const int *first) {
  const int d = lat.arc_dst[a];
  if (d == s) return self;
  const int t = delta[(size_t)lat.arc_label[a] * 64 + q];
  if (t < 0) return -1;
  const is_mask lv = live[d];
  if (!((lv >> (t & 63)) & 1)) return -1;
  return first[d] + (d == sink ? 0 : __popcll(lv & ((1ull << (t & 63)) - 1)));
}

// LDS: fwd and live, 16 bytes per row (the first-pair row ids take fwd's place once live is known), 64 words of scan scratch
__global__ __launch_bounds__(kIsThreads) void k_intersect_count(nfst_batch lat, IsDfa dfa, IsWs w, int32_t *counts,
                                                                int32_t *status) {
  extern __shared__ is_mask is_lds[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = tid / kIsGroup, sub = tid % kIsGroup;
  const Meta m = load_meta(lat.meta, b);
  const int n = m.n_rows;
  is_mask *fwd = is_lds, *live = fwd + n;
  int *red = (int *)(live + n);
  const int32_t *rp = lat.row_ptr + m.row_off + b;
  const int8_t *delta = dfa.delta + dfa.delta_stride * b;
  const is_mask fin = dfa.fin[dfa.fin_stride * b];
  const int *order = w.order + m.row_off, *lev = w.lev + m.row_off + b;
  const int n_lev = w.n_lev[b];
  const int n_reach = lev[n_lev];
  for (int i = tid; i < n; i += kIsThreads) {
    fwd[i] = i == 0 ? 1ull : 0ull;
    live[i] = 0;
  }
  if (tid == 0) red[0] = 0;
  __syncthreads();
  // does any reachable state need a wave of its own?  (most lattices: no, and the second loop of every level is skipped)
  bool hv = false;
  for (int i = tid; i < n_reach; i += kIsThreads) {
    const int s = order[i];
    hv |= rp[s + 1] - rp[s] > kIsHeavy;
  }
  if (hv) red[0] = 1;  // (every writer stores the same word)
  __syncthreads();
  const bool any_heavy = red[0] != 0;

  // fwd, level by level: the sources of a level are final, its destinations lie on later levels
  for (int L = 0; L < n_lev; ++L) {
    const int lo = lev[L], hi = lev[L + 1];
    for (int i = lo + grp; i < hi; i += kIsThreads / kIsGroup) {
      const int s = order[i], a0 = rp[s], a1 = rp[s + 1];
      const is_mask f = fwd[s];
      if (a1 - a0 > kIsHeavy || !f) continue;
      for (int a = a0 + sub; a < a1; a += kIsGroup) {
        const int d = lat.arc_dst[a];
        if (d == s) continue;
        const is_mask im = is_image(f, delta + (size_t)lat.arc_label[a] * 64);
        if (im) atomicOr(&fwd[d], im);
      }
    }
    if (any_heavy)
      for (int i = lo + wv; i < hi; i += kIsWaves) {
        const int s = order[i], a0 = rp[s], a1 = rp[s + 1];
        const is_mask f = fwd[s];
        if (a1 - a0 <= kIsHeavy || !f) continue;
        for (int a = a0 + lane; a < a1; a += 64) {
          const int d = lat.arc_dst[a];
          if (d == s) continue;
          const is_mask im = is_image(f, delta + (size_t)lat.arc_label[a] * 64);
          if (im) atomicOr(&fwd[d], im);
        }
      }
    __syncthreads();
  }

  // live, in reverse level order: the destinations of a level's out-arcs are final
  for (int L = n_lev - 1; L >= 0; --L) {
    const int lo = lev[L], hi = lev[L + 1];
    for (int i = lo + grp; i < hi; i += kIsThreads / kIsGroup) {
      const int s = order[i], a0 = rp[s], a1 = rp[s + 1];
      const is_mask f = fwd[s];
      if (s == m.sink) {
        if (sub == 0) live[s] = f & fin;
        continue;
      }
      if (a1 - a0 > kIsHeavy || !f) continue;
      is_mask acc = 0;
      for (int a = a0 + sub; a < a1; a += kIsGroup) {
        const int d = lat.arc_dst[a];
        if (d == s) continue;
        acc |= is_preimage(f & ~acc, live[d], delta + (size_t)lat.arc_label[a] * 64);
      }
      if (acc) atomicOr(&live[s], acc);
    }
    if (any_heavy)
      for (int i = lo + wv; i < hi; i += kIsWaves) {
        const int s = order[i], a0 = rp[s], a1 = rp[s + 1];
        const is_mask f = fwd[s];
        if (s == m.sink || a1 - a0 <= kIsHeavy || !f) continue;
        is_mask acc = 0;
        for (int a = a0 + lane; a < a1; a += 64) {
          const int d = lat.arc_dst[a];
          if (d == s) continue;
          acc |= is_preimage(f & ~acc, live[d], delta + (size_t)lat.arc_label[a] * 64);
        }
        if (acc) atomicOr(&live[s], acc);
      }
    __syncthreads();
  }

  // rows: the pairs in (state, q) order, all pairs of the sink as one row
  int *first = (int *)fwd;  // (fwd is not read again)
  const int R = pk_scan<false>(n, [&](int s) { return s == m.sink ? (int)(live[s] != 0) : __popcll(live[s]); }, first, red);
  for (int i = tid; i < n; i += kIsThreads) {
    w.live[m.row_off + i] = live[i];
    w.first[m.row_off + i] = first[i];
  }
  if (R == 0 || R > NFST_MAX_ROWS) {  // (the whole block takes this branch)
    if (tid == 0) {
      counts[2 * b] = R;
      counts[2 * b + 1] = 0;
      status[b] = R ? NFST_ERR_LIMIT : NFST_OK;
      w.n_out[b] = 0;
    }
    return;
  }
  int *pair = w.pair + (size_t)b * NFST_MAX_ROWS, *aoff = w.aoff + (size_t)b * NFST_MAX_ROWS;
  for (int s = tid; s < n; s += kIsThreads) {
    is_mask v = live[s];
    int r = first[s];
    if (s == m.sink) v &= ~v + 1;  // (its row carries the smallest live q)
    while (v) {
      pair[r++] = (s << 6) | __builtin_ctzll(v);
      v &= v - 1;
    }
  }
  __syncthreads();  // (the pairs, in global memory, are read by other lanes of the block)

  // out-arcs per product row: a lane per row; the heavy rows of a wave's 64 then take the whole wave, one after the other
  for (int r0 = wv * 64; r0 < R; r0 += kIsThreads) {
    const int r = r0 + lane;
    int s = 0, q = 0, a0 = 0, a1 = 0, cnt = 0;
    if (r < R) {
      const int p = pair[r];
      s = p >> 6, q = p & 63, a0 = rp[s], a1 = rp[s + 1];
    }
    const bool heavy = a1 - a0 > kIsHeavy;
    if (!heavy)
      for (int a = a0; a < a1; ++a) cnt += is_dst_row(lat, a, s, q, m.sink, r, delta, live, first) >= 0;
    is_mask hm = __builtin_amdgcn_ballot_w64(heavy);
    while (hm) {
      const int hl = __builtin_ctzll(hm);
      hm &= hm - 1;
      const int hs = __shfl(s, hl), hq = __shfl(q, hl), h0 = __shfl(a0, hl), h1 = __shfl(a1, hl);
      int tot = 0;
      for (int base = h0; base < h1; base += 64) {
        const int a = base + lane;
        const bool e = a < h1 && is_dst_row(lat, a, hs, hq, m.sink, r0 + hl, delta, live, first) >= 0;
        tot += __popcll(__builtin_amdgcn_ballot_w64(e));
      }
      if (lane == hl) cnt = tot;
    }
    if (r < R) aoff[r] = cnt;
  }
  __syncthreads();
  const int A = pk_scan<false>(R, [&](int r) { return aoff[r]; }, aoff, red);
  if (tid == 0) {
    counts[2 * b] = R;
    counts[2 * b + 1] = A;
    status[b] = NFST_OK;
    w.n_out[b] = R;
  }
}

__global__ __launch_bounds__(kIsThreads) void k_intersect_write(nfst_batch lat, IsDfa dfa, IsWs w, IsOut o) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int R = w.n_out[b];
  if (R == 0) return;
  const Meta m = load_meta(lat.meta, b);
  const int32_t *rp = lat.row_ptr + m.row_off + b;
  const int8_t *delta = dfa.delta + dfa.delta_stride * b;
  const is_mask *live = w.live + m.row_off;
  const int *first = w.first + m.row_off;
  const int *pair = w.pair + (size_t)b * NFST_MAX_ROWS, *aoff = w.aoff + (size_t)b * NFST_MAX_ROWS;
  const int64_t R0 = o.row_off[b], A0 = o.arc_off[b];
  auto emit = [&](int64_t k, int a, int r, int s, int q, int dr) {
    o.src[k] = r;
    o.label[k] = lat.arc_label[a];
    o.dst[k] = dr;
    o.arc_map[k] = a;
    o.arc_q[k] = (dr == r && s == m.sink) ? 0 : q;
  };
  for (int r0 = wv * 64; r0 < R; r0 += kIsThreads) {
    const int r = r0 + lane;
    int s = 0, q = 0, a0 = 0, a1 = 0, pos = 0;
    if (r < R) {
      const int p = pair[r];
      s = p >> 6, q = p & 63, a0 = rp[s], a1 = rp[s + 1], pos = aoff[r];
      o.row_state[R0 + r] = s;
      o.row_q[R0 + r] = q;
    }
    const bool heavy = a1 - a0 > kIsHeavy;
    if (!heavy)
      for (int a = a0; a < a1; ++a) {
        const int dr = is_dst_row(lat, a, s, q, m.sink, r, delta, live, first);
        if (dr >= 0) emit(A0 + pos++, a, r, s, q, dr);
      }
    is_mask hm = __builtin_amdgcn_ballot_w64(heavy);
    while (hm) {
      const int hl = __builtin_ctzll(hm);
      hm &= hm - 1;
      const int hs = __shfl(s, hl), hq = __shfl(q, hl), h0 = __shfl(a0, hl), h1 = __shfl(a1, hl);
      int hp = __shfl(pos, hl);
      for (int base = h0; base < h1; base += 64) {
        const int a = base + lane;
        const int dr = a < h1 ? is_dst_row(lat, a, hs, hq, m.sink, r0 + hl, delta, live, first) : -1;
        const is_mask bal = __builtin_amdgcn_ballot_w64(dr >= 0);
        if (dr >= 0) emit(A0 + hp + __popcll(bal & ((1ull << lane) - 1)), a, r0 + hl, hs, hq, dr);
        hp += __popcll(bal);
      }
    }
  }
}

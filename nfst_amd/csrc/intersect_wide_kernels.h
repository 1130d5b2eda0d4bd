// intersect_wide_kernels.h -- the product of every lattice with a sparse deterministic automaton of up to 4096 states
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.19.
#pragma once

// The wide route beside intersect_kernels.h: the same product, rows and arcs, with sets of automaton states of
// W = ceil(max_q / 64) 64-bit words instead of one.  Two kernels, one 1024-thread workgroup per lattice each, on the
// canonical arrays only, after k_kbest_levels has written the level order of the lattice to the workspace:
//   k_intersect_wide_count  fwd and live as [rows][W] words in the global workspace (16 W bytes per row: beyond LDS at
//                           the row limit), fwd level by level, live in reverse level order; then the rank of every
//                           word inside its state (it takes fwd's place), the first product row of every state, the
//                           pair and the out-arc count of every product row, turned into offsets by block prefix sums
//   k_intersect_wide_write  one lane per product row (one wave per heavy row) writes the row's arcs at its offset
// The automaton is sparse: delta(q, l) = exc_dst[k] for the k in [exc_off[q], exc_off[q + 1]) with exc_label[k] == l (a
// binary search: the labels ascend inside a state), else dflt[q]; -1 = no transition.
// Memory model: inside k_intersect_wide_count EVERY access to fwd and live is an agent-scope
// atomic -- store, OR or load -- so all of them are served by the L2 of the XCD the workgroup runs on, never by the
// CU's vector L1 (which a read-modify-write done in L2 does not refresh).  A level's ORs are complete before the next
// level reads them: every wave waits for its outstanding memory operations (vmcnt(0)) in front of the barrier.  A union
// does not depend on the order of the ORs, so the words are the same from launch to launch.  The write kernel is a
// later launch and reads them with plain loads.
constexpr int kIwThreads = 1024, kIwWaves = kIwThreads / 64;
constexpr int kIwHeavy = 64;     // a product row with more arcs than this is swept by a whole wave
constexpr int kIwMaxQ = 4096;    // one 64-bit word per lane of a wave
constexpr int kIwQBits = 12;     // pair = state << 12 | q: 13 + 12 bits
static_assert(kIwThreads == kPkThreads, "the block scans of pack_kernels.h are written for this block size");
static_assert(kIwMaxQ == 64 * 64 && (1 << kIwQBits) == kIwMaxQ && NFST_MAX_ROWS <= (1 << (31 - kIwQBits)), "pair layout");

// the caller's workspace (nfst_intersect_wide_ws_bytes)
struct IwWs {
  int *order;     // [total_rows] per lattice from row_off: the reachable states by level (k_kbest_levels)
  int *lev;       // [total_rows + n_lattices] per lattice from row_off + b: first position of every level, then the end
  int *n_lev;     // [n_lattices]
  is_mask *fwd;   // [total_rows, W] reached from (0, 0); after the mask passes: live bits in the state's words before this one
  is_mask *live;  // [total_rows, W]
  int *first;     // [total_rows] product row of the state's first pair
  int *pair;      // [n_lattices, NFST_MAX_ROWS] state << 12 | q of every product row
  int *aoff;      // [n_lattices, NFST_MAX_ROWS] first arc of every product row, relative to the lattice's first
  int *n_out;     // [n_lattices] product rows (0: none, or beyond the limit: nothing to write)
  int W;          // words per state
};
struct IwDfa {
  const int32_t *q_off, *dflt, *exc_off, *exc_label, *exc_dst;
  const uint8_t *fin;
  int per;  // 0: one automaton for the batch, 1: one per lattice
};
// the automaton of one lattice: dflt, exc_off and fin start at its state 0 (exc_off holds positions in exc_label / exc_dst)
struct IwAut {
  const int32_t *dflt, *exc_off, *exc_label, *exc_dst;
  const uint8_t *fin;
  int Q;
};
__device__ __forceinline__ IwAut iw_automaton(const IwDfa &d, int b) {
  const int a = d.per ? b : 0, base = d.q_off[a];
  return {d.dflt + base, d.exc_off + base, d.exc_label, d.exc_dst, d.fin + base, d.q_off[a + 1] - base};
}
// delta(q, l), or -1; a target outside 0 .. Q-1 (the caller's to rule out) counts as no transition, so that no word
// beyond a state's W is ever addressed
__device__ __forceinline__ int iw_delta(const IwAut &A, int q, int l) {
  int lo = A.exc_off[q];
  const int end = A.exc_off[q + 1];
  int hi = end;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (A.exc_label[mid] < l) lo = mid + 1;
    else hi = mid;
  }
  const int t = (lo < end && A.exc_label[lo] == l) ? A.exc_dst[lo] : A.dflt[q];
  return (unsigned)t < (unsigned)A.Q ? t : -1;
}
// final states q of word w as a mask
__device__ __forceinline__ is_mask iw_final_word(const IwAut &A, int w) {
  is_mask r = 0;
  for (int q = w * 64; q < min(A.Q, w * 64 + 64); ++q) r |= (is_mask)(A.fin[q] != 0) << (q & 63);
  return r;
}

__device__ __forceinline__ is_mask iw_ld(const is_mask *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void iw_st(is_mask *p, is_mask v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void iw_or(is_mask *p, is_mask v) { __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// every memory operation of every wave of the block, the atomics without a return value included, is complete
__device__ __forceinline__ void iw_sync() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// the product row that canonical arc a of row `self` = (s, q) leads to, or -1 if the product has no such arc
// (AT: inside the count kernel, where the words are read by atomic loads)
template <bool AT>
__device__ __forceinline__ int iw_dst_row(const nfst_batch &lat, int a, int s, int q, int sink, int self, const IwAut &A, int W,
                                          const is_mask *live, const is_mask *rank, const int *first) {
  const int d = lat.arc_dst[a];
  if (d == s) return self;
  const int t = iw_delta(A, q, lat.arc_label[a]);
  if (t < 0) return -1;
  const size_t x = (size_t)d * W + (t >> 6);
  const is_mask lv = AT ? iw_ld(live + x) : live[x];
  if (!((lv >> (t & 63)) & 1)) return -1;
  if (d == sink) return first[d];
  const int before = (int)(AT ? iw_ld(rank + x) : rank[x]);
  return first[d] + before + __popcll(lv & ((1ull << (t & 63)) - 1));
}

// LDS: 64 words of scan scratch
__global__ __launch_bounds__(kIwThreads) void k_intersect_wide_count(nfst_batch lat, IwDfa dfa, IwWs w, int32_t *counts,
                                                                     int32_t *status) {
  __shared__ int red[64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Meta m = load_meta(lat.meta, b);
  const int n = m.n_rows, W = w.W;
  const IwAut A = iw_automaton(dfa, b);
  if (A.Q < 1 || A.Q > 64 * W) {  // (the whole block: an automaton larger than the caller's max_q)
    if (tid == 0) {
      counts[2 * b] = counts[2 * b + 1] = 0;
      status[b] = NFST_ERR_ARG;
      w.n_out[b] = 0;
    }
    return;
  }
  is_mask *fwd = w.fwd + (size_t)m.row_off * W, *live = w.live + (size_t)m.row_off * W;
  int *first = w.first + m.row_off;
  const int32_t *rp = lat.row_ptr + m.row_off + b;
  const int *order = w.order + m.row_off, *lev = w.lev + m.row_off + b;
  const int n_lev = w.n_lev[b];
  for (size_t i = tid; i < (size_t)n * W; i += kIwThreads) {
    iw_st(fwd + i, i == 0 ? 1ull : 0ull);
    iw_st(live + i, 0ull);
  }
  iw_sync();
  // a wave takes a state: lane = (word of the state's set, slot among its out-arcs); Wp = W rounded up to a power of two
  int Wp = 1;
  while (Wp < W) Wp <<= 1;
  const int wl = lane & (Wp - 1), slot = lane / Wp, n_slot = 64 / Wp;

  // fwd, level by level: the sources of a level are final, its destinations lie on later levels
  for (int L = 0; L < n_lev; ++L) {
    const int lo = lev[L], hi = lev[L + 1];
    for (int i = lo + wv; i < hi; i += kIwWaves) {
      const int s = order[i], a0 = rp[s], a1 = rp[s + 1];
      const is_mask f = wl < W ? iw_ld(fwd + (size_t)s * W + wl) : 0ull;
      if (!f) continue;
      for (int a = a0 + slot; a < a1; a += n_slot) {
        const int d = lat.arc_dst[a];
        if (d == s) continue;
        const int l = lat.arc_label[a];
        is_mask *to = fwd + (size_t)d * W;
        int cw = -1;  // the images are gathered per destination word: a chain's land in one or two
        is_mask cb = 0;
        for (is_mask r = f; r; r &= r - 1) {
          const int t = iw_delta(A, wl * 64 + __builtin_ctzll(r), l);
          if (t < 0) continue;
          if ((t >> 6) != cw) {
            if (cb) iw_or(to + cw, cb);
            cw = t >> 6, cb = 0;
          }
          cb |= 1ull << (t & 63);
        }
        if (cb) iw_or(to + cw, cb);
      }
    }
    iw_sync();
  }

  // live, in reverse level order: the destinations of a level's out-arcs are final.  As in the narrow kernel the mask
  // that travels is live itself: q in fwd(s) with delta(q, l) = t has t in fwd(d), so t in bwd(d) iff t in live(d)
  for (int L = n_lev - 1; L >= 0; --L) {
    const int lo = lev[L], hi = lev[L + 1];
    for (int i = lo + wv; i < hi; i += kIwWaves) {
      const int s = order[i], a0 = rp[s], a1 = rp[s + 1];
      const is_mask f = wl < W ? iw_ld(fwd + (size_t)s * W + wl) : 0ull;
      if (!f) continue;
      if (s == m.sink) {
        if (slot == 0) iw_st(live + (size_t)s * W + wl, f & iw_final_word(A, wl));
        continue;
      }
      is_mask acc = 0;
      for (int a = a0 + slot; a < a1; a += n_slot) {
        const int d = lat.arc_dst[a];
        if (d == s) continue;
        const int l = lat.arc_label[a];
        const is_mask *of = live + (size_t)d * W;
        int cw = -1;
        is_mask cv = 0;
        for (is_mask r = f & ~acc; r; r &= r - 1) {
          const int t = iw_delta(A, wl * 64 + __builtin_ctzll(r), l);
          if (t < 0) continue;
          if ((t >> 6) != cw) cw = t >> 6, cv = iw_ld(of + cw);
          if ((cv >> (t & 63)) & 1) acc |= r & (~r + 1);
        }
      }
      if (acc) iw_or(live + (size_t)s * W + wl, acc);
    }
    iw_sync();
  }

  // rows: the pairs in (state, q) order, all pairs of the sink as one row.  The live bits in front of every word of a
  // state take fwd's place (fwd is not read again), the pairs per state are scanned into the state's first row.
  is_mask *rank = fwd;
  for (int s = tid; s < n; s += kIwThreads) {
    int c = 0;
    for (int x = 0; x < W; ++x) {
      iw_st(rank + (size_t)s * W + x, (is_mask)c);
      c += __popcll(iw_ld(live + (size_t)s * W + x));
    }
    first[s] = s == m.sink ? (int)(c != 0) : c;
  }
  iw_sync();
  const int R = pk_scan<false>(n, [&](int s) { return first[s]; }, first, red);
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
  for (int s = tid; s < n; s += kIwThreads) {
    int r = first[s];
    for (int x = 0; x < W; ++x) {
      is_mask v = iw_ld(live + (size_t)s * W + x);
      if (s == m.sink && v) {  // (its row carries the smallest live q)
        pair[r] = (s << kIwQBits) | (x * 64 + __builtin_ctzll(v));
        break;
      }
      for (; v; v &= v - 1) pair[r++] = (s << kIwQBits) | (x * 64 + __builtin_ctzll(v));
    }
  }
  iw_sync();  // (the pairs and first, in global memory, are read by other lanes of the block)

  // out-arcs per product row: a lane per row; the heavy rows of a wave's 64 then take the whole wave, one after the other
  for (int r0 = wv * 64; r0 < R; r0 += kIwThreads) {
    const int r = r0 + lane;
    int s = 0, q = 0, a0 = 0, a1 = 0, cnt = 0;
    if (r < R) {
      const int p = pair[r];
      s = p >> kIwQBits, q = p & (kIwMaxQ - 1), a0 = rp[s], a1 = rp[s + 1];
    }
    const bool heavy = a1 - a0 > kIwHeavy;
    if (!heavy)
      for (int a = a0; a < a1; ++a) cnt += iw_dst_row<true>(lat, a, s, q, m.sink, r, A, W, live, rank, first) >= 0;
    is_mask hm = __builtin_amdgcn_ballot_w64(heavy);
    while (hm) {
      const int hl = __builtin_ctzll(hm);
      hm &= hm - 1;
      const int hs = __shfl(s, hl), hq = __shfl(q, hl), h0 = __shfl(a0, hl), h1 = __shfl(a1, hl);
      int tot = 0;
      for (int base = h0; base < h1; base += 64) {
        const int a = base + lane;
        const bool e = a < h1 && iw_dst_row<true>(lat, a, hs, hq, m.sink, r0 + hl, A, W, live, rank, first) >= 0;
        tot += __popcll(__builtin_amdgcn_ballot_w64(e));
      }
      if (lane == hl) cnt = tot;
    }
    if (r < R) aoff[r] = cnt;
  }
  iw_sync();
  const int T = pk_scan<false>(R, [&](int r) { return aoff[r]; }, aoff, red);
  if (tid == 0) {
    counts[2 * b] = R;
    counts[2 * b + 1] = T;
    status[b] = NFST_OK;
    w.n_out[b] = R;
  }
}

__global__ __launch_bounds__(kIwThreads) void k_intersect_wide_write(nfst_batch lat, IwDfa dfa, IwWs w, IsOut o) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int R = w.n_out[b];
  if (R == 0) return;
  const Meta m = load_meta(lat.meta, b);
  const int W = w.W;
  const IwAut A = iw_automaton(dfa, b);
  const int32_t *rp = lat.row_ptr + m.row_off + b;
  const is_mask *live = w.live + (size_t)m.row_off * W, *rank = w.fwd + (size_t)m.row_off * W;
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
  for (int r0 = wv * 64; r0 < R; r0 += kIwThreads) {
    const int r = r0 + lane;
    int s = 0, q = 0, a0 = 0, a1 = 0, pos = 0;
    if (r < R) {
      const int p = pair[r];
      s = p >> kIwQBits, q = p & (kIwMaxQ - 1), a0 = rp[s], a1 = rp[s + 1], pos = aoff[r];
      o.row_state[R0 + r] = s;
      o.row_q[R0 + r] = q;
    }
    const bool heavy = a1 - a0 > kIwHeavy;
    if (!heavy)
      for (int a = a0; a < a1; ++a) {
        const int dr = iw_dst_row<false>(lat, a, s, q, m.sink, r, A, W, live, rank, first);
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
        const int dr = a < h1 ? iw_dst_row<false>(lat, a, hs, hq, m.sink, r0 + hl, A, W, live, rank, first) : -1;
        const is_mask bal = __builtin_amdgcn_ballot_w64(dr >= 0);
        if (dr >= 0) emit(A0 + hp + __popcll(bal & ((1ull << lane) - 1)), a, r0 + hl, hs, hq, dr);
        hp += __popcll(bal);
      }
    }
  }
}

// beam_kernels.h -- one step of lattice-constrained beam search, and the backtrack of a finished search
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.9.
#pragma once

// k_beam_step: one workgroup per lattice on the canonical arrays only (row_ptr, arc_label, arc_dst, arc_w).  The K
// slots of the lattice's beam expand by the arcs out of their states; a candidate is (slot j, arc a with label l):
//     c = beam_score[j] + (x + w_a),  x = scores[j, l] (0.0f for l = pad),  w_a = arc_w[a] or 0.0f;   r = c + lookahead[dst_a]
// The best K by (r desc, j asc, l asc) survive.  A candidate is one 64-bit key, 0 = none:
//     key = order-preserving bits of r << 21 | (63 - j) << 15 | (32767 - l)
// (a state's arcs carry distinct labels, so keys are unique and "greater key" is the total order).  Phases:
//   1  K lanes read their slot (state, previous mark, score, arc range); a wave scan gives every slot's first candidate
//   2  the candidates' keys go to LDS, one per (slot, arc) in a flat index over all threads -- when there are more than
//      `cap` of them (kBeamLdsCand, or K * vocab if that is smaller) nothing is kept and every later pass computes the
//      keys again from global memory
//   3  threshold select: the K-th largest key, two bits per pass from the top (three thresholds counted at once with
//      wave ballots, one barrier per pass; 27 passes, none when at most K candidates exist)
//   4  the keys >= the threshold are compacted (ballot prefix per wave, wave totals through LDS) and wave 0 ranks them:
//      lane i counts the winners above its own, finds its arc again by label and stores the rank's outputs
// No atomics but one add per workgroup into n_open.
constexpr int kBeamMaxK = 64, kBeamThreads = 256, kBeamWaves = kBeamThreads / 64;
constexpr int kBeamLdsCand = 7680;  // candidates whose keys are kept in LDS (60 KiB: with the static part under 64 KiB)
constexpr int kBeamKeyBits = 54;    // 32 + 6 + 15 = 53 used

struct BeamIn {
  const int64_t *state, *inp;
  const float *beam_score, *scores, *lookahead;
  int pad, bos, eos, has_to_end, K;
};
struct BeamOut {
  float *score;
  int32_t *parent;
  int64_t *symbol, *next_state;
  int32_t *n_candidates, *n_open;
};

// per-slot facts of a lattice's beam (LDS)
struct BeamSlots {
  int off[kBeamMaxK + 1];  // first candidate of every slot in the flat index; off[K] = their number
  int r0[kBeamMaxK];       // first canonical arc of the slot's state
  float bs[kBeamMaxK];     // beam score
  int ended[kBeamMaxK];    // the previous mark is eos or pad
};

__device__ __forceinline__ uint64_t beam_key(float r, int j, int l) {
  r = r == 0.0f ? 0.0f : r;  // -0.0 and +0.0 rank alike
  return ((uint64_t)kb_ord(r) << 21) | ((uint64_t)(63 - j) << 15) | (uint64_t)(32767 - l);
}

// everything a candidate needs; score() is the one place where c and r are computed
struct BeamCand {
  const nfst_batch &lat;
  const BeamIn &in;
  const BeamSlots &sl;
  int n0, row_off, n_rows;

  // the candidate of slot j over arc a: false when it is illegal or dropped
  __device__ __forceinline__ bool score(int j, int a, int &l, int &dst, float &c, float &r) const {
    l = lat.arc_label[a];
    dst = lat.arc_dst[a];
    if (l < 0 || l >= lat.vocab || dst < 0 || dst >= n_rows) return false;  // (never on a valid batch)
    const bool ended = sl.ended[j] != 0;
    if (l == in.bos || (ended ? (l != in.pad) : (l == in.pad))) return false;
    if (in.has_to_end && !ended && l != in.eos) return false;
    const float x = l == in.pad ? 0.0f : in.scores[(size_t)(n0 + j) * lat.vocab + l];
    const float w = lat.weighted ? lat.arc_w[a] : 0.0f;
    c = sl.bs[j] + (x + w);
    r = in.lookahead ? c + in.lookahead[row_off + dst] : c;
    return c > kNegInf && r > kNegInf;  // (NaN fails both)
  }
  // the key of flat candidate e < off[K]
  __device__ __forceinline__ uint64_t key(int e) const {
    int lo = 0, hi = in.K;  // the slot j with off[j] <= e < off[j + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (sl.off[mid] <= e) lo = mid; else hi = mid;
    }
    int l, dst;
    float c, r;
    return score(lo, sl.r0[lo] + (e - sl.off[lo]), l, dst, c, r) ? beam_key(r, lo, l) : 0ull;
  }
};

// The selection below is shared with k_swor (swor_kernels.h).  Its key source is a parameter: key(e) is the 64-bit key of
// flat candidate e < total, 0 = none, the same value every time it is asked.
//
// FLAT chooses how the candidates go to the threads.  false (k_beam_step, whose winners are ranked by key afterwards): e =
// base + tid, 256 at a time.  true (k_swor, whose winners keep their order): every wave reads one contiguous share of the
// flat index, 64 candidates at a time, so "the waves in order, each in the order it reads" is flat order and the
// compaction keeps it.
__device__ __forceinline__ int beam_share(int total) { return (total + kBeamThreads - 1) / kBeamThreads * 64; }
__device__ __forceinline__ int beam_share_end(int total, int wv) {
  const int e1 = beam_share(total) * (wv + 1);
  return e1 < total ? e1 : total;
}

// how many keys are >= t1, t2, t3 (t1 <= t2 <= t3): wave ballots, then the waves' counts through cnt (LDS, [waves][3])
template <bool FLAT, class KeyF>
__device__ __forceinline__ void beam_count(KeyF key, int total, uint64_t t1, uint64_t t2, uint64_t t3, int *cnt, int &c1, int &c2,
                                           int &c3) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int a1 = 0, a2 = 0, a3 = 0;
  const int e1 = FLAT ? beam_share_end(total, wv) : total;
  for (int base = FLAT ? beam_share(total) * wv : 0; base < e1; base += FLAT ? 64 : kBeamThreads) {  // (the same trips in every lane: the ballots see whole waves)
    const int e = base + (FLAT ? lane : tid);
    uint64_t k = 0;
    if (e < e1) k = key(e);
    a1 += __popcll(__ballot(k >= t1));
    a2 += __popcll(__ballot(k >= t2));
    a3 += __popcll(__ballot(k >= t3));
  }
  if (lane == 0) { cnt[wv * 3] = a1; cnt[wv * 3 + 1] = a2; cnt[wv * 3 + 2] = a3; }
  __syncthreads();
  c1 = c2 = c3 = 0;
#pragma unroll
  for (int w = 0; w < kBeamWaves; ++w) { c1 += cnt[w * 3]; c2 += cnt[w * 3 + 1]; c3 += cnt[w * 3 + 2]; }
}

// phases 3 and 4 up to the compacted winners: the min(K, candidates) largest keys of KEY_BITS bits, of equal keys the
// first in the order the threads read them (FLAT: the smaller flat index).  keep(pos, e, k) receives winner e with key k
// and its position among the winners in that order, drop(k) every other candidate's key; returns the winners' number
// and the candidates' number.  (The keys of k_beam_step are unique: every key >= the threshold wins.)
template <int KEY_BITS, bool FLAT, class KeyF, class KeepF, class DropF>
__device__ __forceinline__ int beam_select(KeyF key, int total, int K, int (*cnt)[kBeamWaves * 3], KeepF keep, DropF drop, int &n_cand) {
  const int tid = threadIdx.x, wv = tid >> 6;
  int c1, c2, c3, par = 0;
  // (consecutive passes write alternating count buffers: a buffer is written again only after the barrier of the pass between)
  beam_count<FLAT>(key, total, 1, 1, 1, cnt[par], c1, c2, c3);
  par ^= 1;
  n_cand = c1;
  const int want = n_cand < K ? n_cand : K;
  if (want == 0) return 0;
  uint64_t thr = 1;  // the largest t with `want` or more keys >= t: the want-th largest key
  if (n_cand > K) {
    thr = 0;
    for (int sh = KEY_BITS - 2; sh >= 0; sh -= 2) {
      beam_count<FLAT>(key, total, thr | (1ull << sh), thr | (2ull << sh), thr | (3ull << sh), cnt[par], c1, c2, c3);
      par ^= 1;
      thr |= (uint64_t)(c3 >= want ? 3 : c2 >= want ? 2 : c1 >= want ? 1 : 0) << sh;
    }
  }
  // compaction: the waves' totals first (keys >= thr, keys > thr), then every wave writes behind the waves before it
  const uint64_t above = thr + 1 ? thr + 1 : thr;  // (a threshold of all ones has nothing above it; no key is all ones)
  beam_count<FLAT>(key, total, thr, above, above, cnt[par], c1, c2, c3);
  const int ties = n_cand > K ? want - c2 : c1 - c2;  // keys equal to the threshold that win: the first in flat order
  int gt = 0, eq = 0;
  for (int w = 0; w < wv; ++w) { gt += cnt[par][w * 3 + 1]; eq += cnt[par][w * 3] - cnt[par][w * 3 + 1]; }
  const int e1 = FLAT ? beam_share_end(total, wv) : total;
  for (int base = FLAT ? beam_share(total) * wv : 0; base < e1; base += FLAT ? 64 : kBeamThreads) {
    const int e = base + (FLAT ? (tid & 63) : tid);
    uint64_t k = 0;
    if (e < e1) k = key(e);
    const uint64_t mg = __ballot(k > thr), me = __ballot(k == thr);
    const int g = gt + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mg >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mg, 0u));
    const int q = eq + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(me >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)me, 0u));
    const int pos = g + (q < ties ? q : ties);
    if ((k > thr || (k == thr && q < ties)) && pos < kBeamMaxK) keep(pos, e, k);
    else if (k != 0) drop(k);
    gt += __popcll(mg);
    eq += __popcll(me);
  }
  __syncthreads();
  return want;
}

__global__ __launch_bounds__(kBeamThreads) void k_beam_step(nfst_batch lat, BeamIn in, BeamOut out, int cap) {
  extern __shared__ uint64_t beam_keys[];  // [cap]
  __shared__ BeamSlots sl;
  __shared__ int cnt[2][kBeamWaves * 3];
  __shared__ uint64_t win[kBeamMaxK];
  const int b = blockIdx.x, tid = threadIdx.x, K = in.K;
  const Meta m = load_meta(lat.meta, b);
  const int n0 = b * K;
  // phase 1 (wave 0: K <= 64 lanes)
  if (tid < 64) {
    int deg = 0;
    if (tid < K) {
      const int64_t s = in.state[n0 + tid], p = in.inp[n0 + tid];
      const float bs = in.beam_score[n0 + tid];
      int r0 = 0;
      if (bs > kNegInf && s >= 0 && s < m.n_rows) {  // a live slot
        const int32_t *rp = lat.row_ptr + m.row_off + b;
        r0 = rp[s];
        deg = rp[s + 1] - r0;
      }
      sl.r0[tid] = r0;
      sl.bs[tid] = bs;
      sl.ended[tid] = (p == in.eos || p == in.pad) ? 1 : 0;
    }
    int incl = deg;
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (tid >= d) incl += o;
    }
    if (tid < K) sl.off[tid] = incl - deg;
    if (tid == K - 1) sl.off[K] = incl;
  }
  __syncthreads();
  const int total = sl.off[K];
  const BeamCand cd{lat, in, sl, n0, m.row_off, m.n_rows};
  int n_cand = 0, n_win = 0;
  const auto keep = [&](int pos, int, uint64_t k) { win[pos] = k; };
  if (total <= cap) {  // (the same in every thread of the workgroup)
    for (int e = tid; e < total; e += kBeamThreads) beam_keys[e] = cd.key(e);
    __syncthreads();
    n_win = beam_select<kBeamKeyBits, false>([&](int e) { return beam_keys[e]; }, total, K, cnt, keep, [](uint64_t) {}, n_cand);
  } else {
    n_win = beam_select<kBeamKeyBits, false>([&](int e) { return cd.key(e); }, total, K, cnt, keep, [](uint64_t) {}, n_cand);
  }
  if (tid >= 64) return;
  // wave 0: lane i ranks winner i and stores the outputs of its rank; the lanes from n_win to K store the empty ranks
  const int i = tid;
  int rank = i, par = -1, l = in.pad, dst = 0;
  float c = kNegInf;
  if (i < n_win) {
    const uint64_t mine = win[i];
    rank = 0;
    for (int q = 0; q < n_win; ++q) rank += win[q] > mine ? 1 : 0;
    const int j = 63 - (int)((mine >> 15) & 63u), lab = 32767 - (int)(mine & 32767u);
    const int r0 = sl.r0[j], r1 = r0 + (sl.off[j + 1] - sl.off[j]);
    const int a = find_arc(lat.arc_label, r0, r1, lab);
    float r;
    if (a >= 0 && cd.score(j, a, l, dst, c, r)) par = j;
    else { c = kNegInf; l = in.pad; dst = 0; }  // (never: the key came from this arc)
  }
  if (i < K) {
    out.score[n0 + rank] = c;
    out.parent[n0 + rank] = par;
    out.symbol[n0 + rank] = l;
    out.next_state[n0 + rank] = dst;
  }
  if (out.n_candidates && i == 0) out.n_candidates[b] = n_cand;
  if (out.n_open) {
    const int open = __popcll(__ballot(i < K && par >= 0 && l != in.pad));
    if (i == 0 && open > 0) atomicAdd(out.n_open, open);
  }
}

// Backtrack: thread n = (lattice, final rank) follows parent[t, n] from the last step to the first, once to count the
// marks other than pad and once to write them from the back; the rest of the row is pad.
__global__ void k_beam_backtrack(const int32_t *parent, const int64_t *symbol, const float *score, int n_steps, int n_lattices,
                                 int K, int max_len, int pad, int32_t *paths, int32_t *lengths) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, N = (int64_t)n_lattices * K;
  if (n >= N) return;
  const int64_t base = n - n % K;
  int32_t *row = paths + n * max_len;
  int len = 0;
  if (score[n] > kNegInf) {
    for (int pass = 0; pass < 2; ++pass) {
      int cur = (int)(n % K), at = len;
      for (int t = n_steps - 1; t >= 0 && cur >= 0 && cur < K; --t) {
        const int64_t s = symbol[(int64_t)t * N + base + cur];
        if (s != pad) {
          if (pass == 0) ++len;
          else row[--at] = (int32_t)s;
        }
        cur = parent[(int64_t)t * N + base + cur];
      }
      // (a chain that leaves [0, K) early is shorter in both passes alike: `at` ends at 0)
    }
  }
  lengths[n] = len;
  for (int t = len; t < max_len; ++t) row[t] = pad;
}

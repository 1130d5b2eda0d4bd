// string_merge_kernels.h -- merge the rows of a path set by their projection onto the output tape ("crunching")
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.20.
#pragma once

// k_merge_paths: one workgroup per set, K <= 1024 rows of at most kEditMaxLen tokens, in five steps with a barrier between:
//   1 projection  a wave takes a row 64 tokens at a time: a ballot of the kept lanes and a lane's count of the kept lanes
//                 below it give the token's place in the projected row (the caller's scratch rows); the row's 64-bit hash
//                 is the XOR over its tokens of a mix of (place, token)
//   2 grouping    thread k looks for the lowest row c < k of the same projected length whose hash agrees in the bits of
//                 hash_mask and whose tokens, compared one by one, are the same: the group's leader.  The hash only spares
//                 comparisons; it never decides
//   3 weights     a leader runs over its members in ascending row order: their maximum and its first row, then the sum of
//                 exp(w - max), in float64 with sm_exp and sm_log below
//   4 ranking     a leader counts the leaders that beat it (merged weight descending, then the lower leader row)
//   5 output      rows, lengths, weights, first members and the group of every input row, the rest filled
// Everything a step hands to the next lies in LDS (40 bytes per row).  No atomics: the same bits at every launch.
constexpr int kSmThreads = 1024, kSmWaves = kSmThreads / 64, kSmMaxK = 1024;

struct SmIn {
  const int32_t *paths, *lengths;
  const double *w;
  const int32_t *n_paths;  // or null
  const uint8_t *keep;     // [vocab] or null
  int K, L, vocab, marker, pad;
  uint64_t hash_mask;
};
struct SmOut {
  int32_t *proj;  // [n_sets, K, L] scratch
  int32_t *strings, *lengths;
  double *w;
  int32_t *n_strings, *group, *first, *status;
};

// exp and log of the merged weight in IEEE operations alone -- products and sums rounded one by one, no fused
// multiply-add, no library call whose last bit differs between implementations -- so that a restatement with the same
// operations has the same bits.  sm_exp: x <= 0 (below -700: 0); sm_log: s >= 1.  Relative error ~2e-16 each.
__device__ __forceinline__ double sm_exp(double x) {
#pragma clang fp contract(off)
  if (!(x > -700.0)) return 0.0;
  const double k = rint(x * 1.4426950408889634);
  const double t = (x - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
  double p = 1.0 / 6227020800.0;
  p = p * t + 1.0 / 479001600.0;
  p = p * t + 1.0 / 39916800.0;
  p = p * t + 1.0 / 3628800.0;
  p = p * t + 1.0 / 362880.0;
  p = p * t + 1.0 / 40320.0;
  p = p * t + 1.0 / 5040.0;
  p = p * t + 1.0 / 720.0;
  p = p * t + 1.0 / 120.0;
  p = p * t + 1.0 / 24.0;
  p = p * t + 1.0 / 6.0;
  p = p * t + 0.5;
  p = p * t + 1.0;
  p = p * t + 1.0;
  return ldexp(p, (int)k);
}
__device__ __forceinline__ double sm_log(double s) {
#pragma clang fp contract(off)
  int e;
  double m = frexp(s, &e);  // [0.5, 1)
  if (m < 0.70710678118654752) {
    m = m * 2.0;
    e -= 1;
  }
  // log m = 2 atanh z, z = (m - 1) / (m + 1), |z| <= 0.1716: the odd series up to z^23 (the next term is below 1e-19)
  const double f = m - 1.0, z = f / (2.0 + f), z2 = z * z;
  double p = 1.0 / 23.0;
  p = p * z2 + 1.0 / 21.0;
  p = p * z2 + 1.0 / 19.0;
  p = p * z2 + 1.0 / 17.0;
  p = p * z2 + 1.0 / 15.0;
  p = p * z2 + 1.0 / 13.0;
  p = p * z2 + 1.0 / 11.0;
  p = p * z2 + 1.0 / 9.0;
  p = p * z2 + 1.0 / 7.0;
  p = p * z2 + 1.0 / 5.0;
  p = p * z2 + 1.0 / 3.0;
  p = p * z2 + 1.0;
  return (double)e * 0.6931471805599453 + (2.0 * z) * p;
}

__device__ __forceinline__ uint64_t sm_mix(uint64_t x) {  // the finaliser of splitmix64
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// The projection of row[0 .. len) onto the tape by one wave: the kept tokens go to out[0 ..), their number comes back
// and their hash in `hash`.  keep mode: a token is kept when keep[token] is set (a token outside the vocabulary is not).
// marker mode: token i is kept when token i - 1 is an active marker; a marker is active unless it is itself kept, so in a
// run of markers every second one is active, counted from the run's start -- a lane finds its place in its run from the
// ballot of the marker lanes (the highest lane below it that holds no marker); `carry` takes "the last token of the chunk
// is an active marker" to the next 64 tokens.  Neither: every token is kept.
__device__ __forceinline__ int sm_project(const SmIn &in, const int32_t *row, int len, int32_t *out, int lane, uint64_t &hash) {
  int base = 0;
  uint64_t h = 0, carry = 0;
  for (int c = 0; c < len; c += 64) {
    const int i = c + lane;
    const bool in_row = i < len;
    const int tok = in_row ? row[i] : 0;
    bool kept = in_row;
    if (in.keep) {
      kept = in_row && (unsigned)tok < (unsigned)in.vocab && in.keep[(unsigned)tok < (unsigned)in.vocab ? tok : 0] != 0;
    } else if (in.marker >= 0) {
      const uint64_t M = __builtin_amdgcn_ballot_w64(in_row && tok == in.marker);
      const uint64_t x = ~M & ((2ull << lane) - 1);  // the lanes up to this one without a marker
      const int off = x ? lane - (63 - __builtin_clzll(x)) - 1 : lane + (int)carry;
      const uint64_t A = __builtin_amdgcn_ballot_w64(((M >> lane) & 1) && !(off & 1));
      kept = in_row && ((((A << 1) | carry) >> lane) & 1);
      carry = A >> 63;
    }
    const uint64_t kb = __builtin_amdgcn_ballot_w64(kept);
    const int pos = base + __builtin_popcountll(kb & ((1ull << lane) - 1));
    if (kept) {
      out[pos] = tok;
      h ^= sm_mix(((uint64_t)(uint32_t)pos << 32) | (uint32_t)tok);
    }
    base += __builtin_popcountll(kb);
  }
  const KbKey r = butterfly<6>(KbKey{(uint32_t)(h >> 32), (uint32_t)h}, [](KbKey a, KbKey o) { return KbKey{a.hi ^ o.hi, a.lo ^ o.lo}; });
  hash = ((uint64_t)r.hi << 32) | r.lo;
  return base;
}

__global__ __launch_bounds__(kSmThreads) void k_merge_paths(SmIn in, SmOut o) {
  __shared__ uint64_t hash[kSmMaxK];
  __shared__ double wt[kSmMaxK], merged[kSmMaxK];
  __shared__ int plen[kSmMaxK], leader[kSmMaxK], rank[kSmMaxK], fst[kSmMaxK];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = in.K, L = in.L;
  const size_t set = (size_t)b * K;
  const int n_in = in.n_paths ? in.n_paths[b] : K;
  int32_t *proj = o.proj + set * L;
  // 1: projection (plen = -1: an invalid row)
  for (int k = wv; k < K; k += kSmWaves) {
    const double w = in.w[set + k];
    const int len = in.lengths[set + k];
    const bool len_ok = len >= 0 && len <= L;
    const bool valid = k < n_in && w > -__builtin_huge_val() && len_ok;  // (NaN compares false)
    uint64_t h = 0;
    int n = -1;
    if (valid) n = sm_project(in, in.paths + (set + k) * L, len, proj + (size_t)k * L, lane, h);
    if (lane == 0) {
      plen[k] = n;
      hash[k] = h;
      wt[k] = w;
      if (!len_ok) *o.status = NFST_ERR_LENGTH;
    }
  }
  __syncthreads();  // (the scratch rows are read by other waves)
  // 2: grouping
  const int k = tid;
  int lead = k;
  if (k < K && plen[k] >= 0) {
    const int n = plen[k];
    const uint64_t h = hash[k];
    const int32_t *mine = proj + (size_t)k * L;
    for (int c = 0; c < k; ++c) {
      if (plen[c] != n || ((hash[c] ^ h) & in.hash_mask) != 0) continue;
      const int32_t *other = proj + (size_t)c * L;
      int i = 0;
      while (i < n && other[i] == mine[i]) ++i;
      if (i == n) {
        lead = c;
        break;
      }
    }
  }
  if (k < K) leader[k] = lead;
  __syncthreads();
  // 3: weights
  const bool is_leader = k < K && plen[k] >= 0 && lead == k;
  if (is_leader) {
    double mx = wt[k];
    int f = k;
    for (int c = k + 1; c < K; ++c)
      if (plen[c] >= 0 && leader[c] == k && wt[c] > mx) {
        mx = wt[c];
        f = c;
      }
    double s = 0.0;
    for (int c = k; c < K; ++c)
      if (plen[c] >= 0 && leader[c] == k) s += sm_exp(wt[c] - mx);
    merged[k] = mx + sm_log(s);
    fst[k] = f;
  }
  const int G = __syncthreads_count(is_leader);
  // 4: ranking
  if (is_leader) {
    const double mw = merged[k];
    int r = 0;
    for (int c = 0; c < K; ++c)
      if (c != k && plen[c] >= 0 && leader[c] == c && (merged[c] > mw || (merged[c] == mw && c < k))) ++r;
    rank[k] = r;
  }
  __syncthreads();
  // 5: output
  if (k < K) {
    o.group[set + k] = plen[k] >= 0 ? rank[leader[k]] : -1;
    if (is_leader) {
      const int r = rank[k];
      o.lengths[set + r] = plen[k];
      o.w[set + r] = merged[k];
      o.first[set + r] = fst[k];
    }
    if (k >= G) {
      o.lengths[set + k] = 0;
      o.w[set + k] = -__builtin_huge_val();
      o.first[set + k] = -1;
    }
  }
  if (tid == 0) o.n_strings[b] = G;
  for (int q = wv; q < K; q += kSmWaves) {
    const bool ld = plen[q] >= 0 && leader[q] == q;  // (the same in every lane)
    if (ld) {
      int32_t *dst = o.strings + (set + rank[q]) * L;
      const int32_t *src = proj + (size_t)q * L;
      const int n = plen[q];
      for (int i = lane; i < L; i += 64) dst[i] = i < n ? src[i] : in.pad;
    }
  }
  for (int r = G + wv; r < K; r += kSmWaves) {
    int32_t *dst = o.strings + (set + r) * L;
    for (int i = lane; i < L; i += 64) dst[i] = in.pad;
  }
}

// chunk_cost.h -- the cost model and the plan search of the chunk cutter, shared by the host cutter (chunk_pack.cpp) and the
// device cutter (chunk_pack_kernels.h).  Both must make the same decisions to the bit: one copy of every expression, evaluated
// without FMA contraction (the host build has no FMA; the device compiler would otherwise fuse a * b + c).
#pragma once

#include <stdint.h>

#include "tile_format.h"  // (NFST_HD)

namespace nfst_chunk {

constexpr int kCus = 256;        // MI355X
constexpr int kMaxReach = 63;    // an entry's operand slot has 6 bits
// cost model of the chunked sweep (cycles at 2.4 GHz, MI355X, measured with profiles/tune/chunk_stamps.py: DESIGN.md
// section 4.4): pass 1 is the longest chunk at one entry per kEntry cycles (an LDS round trip per entry on a lane's chain:
// 82 ns with one wave per SIMD, 88 ns with three), or -- a bound for workgroups full of lanes -- the whole program's entries
// x F / 64 lanes x kIssue / 4 SIMDs; pass 2 is C steps of step_cycles(F); kFixed: weights, initialisation, the tail of pass 3,
// the second kernel and the empty launch of the general one
constexpr double kEntry = 205.0, kIssue = 60.0, kFixed = 25000.0;

NFST_HD inline double step_cycles(int F) {  // (234 / 250 / 322 / 445 ns at F = 2 / 3 / 8 / 16)
  return (F <= 2 ? 560.0 : F <= 4 ? 600.0 : 775.0) + 300.0 * ((F + 7) / 8 - 1);
}

NFST_HD inline int pow2_at_least(int x) { int r = 1; while (r < x) r <<= 1; return r; }

// LDS of a workgroup that runs a program with C chunks of F right-hand sides and R ring slots: the rings (one padded
// block per chunk), the frontier values of every chunk (mantissa + exponent) and the chunks' first positions
NFST_HD inline int64_t lds_need(int C, int F, int R) {
  return (int64_t)C * (R * F + F) * 8 + 64 + (int64_t)C * F * 12 + (int64_t)(2 * C + 2) * 4 + 64;
}

// Cuts for a frontier of at most Ft states, `lane_cap` lanes at most: as many chunks as the lanes, the LDS and the balance of
// pass 1 against pass 2 allow, about the same number of entries each; a cut whose frontier is wider than Ft moves to the
// nearest position where it is not (or is dropped).  n positions; pre[p] = entries of positions [1, p) (pre[0] = pre[1] = 0,
// total = pre[n]); low[a] = the smallest operand position of an arc that crosses the cut a.  emit(start) receives the first
// position of every chunk in order.  Returns false when no plan fits; else *C (chunks), *F (largest frontier) and *cycles
// (the cost model of the chunked sweep).
template <class P, class L, class Emit>
NFST_HD bool plan_cut(int Ft, int lane_cap, int n, const P *pre, const L *low, int R, int threads, int64_t lds_bytes,
                      int max_chunks, Emit &&emit, int *C_out, int *F_out, double *cycles_out) {
#pragma clang fp contract(off)
  const int64_t total = pre[n];
  const int lanes = threads < lane_cap ? threads : lane_cap;
  int C = lanes / Ft < n - 1 ? lanes / Ft : n - 1;
  {
    const int bal = (int)__builtin_ceil(__builtin_sqrt((double)total * kEntry / step_cycles(Ft)));
    const int b1 = bal > 1 ? bal : 1;
    C = C < b1 ? C : b1;
  }
  while (C > 1 && lds_need(C, Ft, R) > lds_bytes) --C;
  if (max_chunks > 0 && max_chunks < C) C = max_chunks;
  if (C < 1 || lds_need(C, Ft, R) > lds_bytes) return false;
  int last = 1, count = 1, F = 1;
  int64_t longest = 0;
  emit(1);
  if (1 - (int)low[1] > F) F = 1 - (int)low[1];
  const int slack = (n / C) / 2 > 1 ? (n / C) / 2 : 1;
  for (int c = 1; c < C; ++c) {
    const int64_t target = total * c / C;
    // (std::upper_bound over pre[1 .. n]: the first index whose entry count exceeds the target)
    int lo = 1, hi = n + 1;
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if ((int64_t)pre[mid] <= target) lo = mid + 1; else hi = mid;
    }
    int a = lo - 1;
    a = a > last + 1 ? a : last + 1;
    if (a >= n) break;
    int best = -1;
    for (int d = 0; d <= slack && best < 0; ++d)
      for (int sgn = -1; sgn <= 1 && best < 0; sgn += 2) {
        const int b = a + sgn * d;
        if (b > last && b < n && b - (int)low[b] <= Ft) best = b;
      }
    if (best > 0) {
      const int64_t cnt = (int64_t)pre[best] - (int64_t)pre[last];
      const int64_t padded = (cnt + 7) / 8 * 8;
      longest = longest > padded ? longest : padded;
      emit(best);
      if (best - (int)low[best] > F) F = best - (int)low[best];
      last = best;
      ++count;
    }
  }
  {
    const int64_t cnt = (int64_t)pre[n] - (int64_t)pre[last];
    const int64_t padded = (cnt + 7) / 8 * 8;
    longest = longest > padded ? longest : padded;
  }
  // an entry of pass 1 is an LDS round trip on its lane's chain while a SIMD holds at most two of the workgroup's waves
  // (82 .. 88 ns); with a third one the walks share its issue slots (88 .. 113 ns with nine waves, 112 .. 139 with twelve)
  const int waves = (count * F + 63) / 64, per_simd = (waves + 3) / 4;
  const double entry = kEntry + 60.0 * (per_simd - 2 > 0 ? per_simd - 2 : 0);
  const double p1 = (double)longest * entry, p1b = (double)total * F / 64.0 * kIssue / 4.0;
  *cycles_out = (p1 > p1b ? p1 : p1b) + (double)count * step_cycles(F) + kFixed;
  *C_out = count;
  *F_out = F;
  return true;
}

// the plans of one program are tried in this order: Ft = Fb .. 1, and for each a lane cap of 1024, then 512 (fewer chunks can
// be faster: two waves per SIMD); the cheapest wins, the first of equally cheap ones
NFST_HD inline int plan_ft(int Fb, int k) { return Fb - k / 2; }
NFST_HD inline int plan_lane_cap(int k) { return (k & 1) ? 512 : 1024; }

// workgroup size and LDS budget of the programs of a batch of B lattices (0 in opts = by batch size); false for bad options
inline bool resolve_opts(int B, int threads_opt, int lds_opt, int *threads, int64_t *lds_bytes) {
  const bool roomy = 2 * B <= kCus;  // every (lattice, direction) workgroup has a CU to itself
  *threads = threads_opt > 0 ? threads_opt : (roomy ? 1024 : 512);
  *lds_bytes = lds_opt > 0 ? lds_opt : (roomy ? 152 * 1024 : 64 * 1024);
  return !(*threads < 64 || *threads > 1024 || (*threads & 63) || *lds_bytes > 160 * 1024);
}

}  // namespace nfst_chunk

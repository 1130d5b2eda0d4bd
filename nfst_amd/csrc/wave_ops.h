// wave_ops.h -- cross-lane partners of a wave64 and the reductions built on them
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md section 4.11.
#pragma once

// The partner's value in stage S of the six-stage butterfly over a wave.  Stages 0 .. 3 stay inside a row of 16 lanes
// and are DPP modifiers (no LDS traffic); after them every lane of a row holds the row's result.  Stages 4 and 5 cross
// the rows (shuffles).
//   S = 0  lane ^ 1            quad_perm [1, 0, 3, 2]
//   S = 1  lane ^ 2            quad_perm [2, 3, 0, 1]
//   S = 2  half-row mirror     lane ^ 7 within 8 lanes: the other quad of the half row
//   S = 3  row mirror          lane ^ 15 within 16 lanes: the other half of the row
//   S = 4  lane ^ 16
//   S = 5  lane ^ 32
// An aggregate takes part by overloading wave_partner<S> member by member (ExpSums, KbKey).
constexpr int kStageDpp[4] = {0xB1, 0x4E, 0x141, 0x140};
template <int S>
__device__ __forceinline__ int wave_partner(int v) {
  static_assert(S >= 0 && S < 6, "a wave64 butterfly has six stages");
  if constexpr (S < 4) return __builtin_amdgcn_update_dpp(0, v, kStageDpp[S], 0xf, 0xf, false);
  else if constexpr (S == 4) return __shfl_xor(v, 16);
  else return __shfl_xor(v, 32);
}
template <int S> __device__ __forceinline__ uint32_t wave_partner(uint32_t v) { return (uint32_t)wave_partner<S>((int)v); }
template <int S>
__device__ __forceinline__ float wave_partner(float v) {
  if constexpr (S < 4) return __int_as_float(wave_partner<S>(__float_as_int(v)));
  else if constexpr (S == 4) return __shfl_xor(v, 16);
  else return __shfl_xor(v, 32);
}
template <int S>
__device__ __forceinline__ double wave_partner(double v) {
  if constexpr (S < 4) return __hiloint2double(wave_partner<S>(__double2hiint(v)), wave_partner<S>(__double2loint(v)));
  else if constexpr (S == 4) return __shfl_xor(v, 16);
  else return __shfl_xor(v, 32);
}

// Segmented all-reduce: a lane whose state owns 2^g lanes takes part in stages 0 .. g - 1, and all lanes of a state end
// with the same value.  gmax (the tile's largest g, the same in every lane, or a constant) bounds the stages executed,
// MAXS those compiled.  combine(x, o, take) folds the partner's value o into x where take is set.
template <int MAXS, class T, class F>
__device__ __forceinline__ void seg_ladder(T &x, int g, int gmax, F combine) {
  if (MAXS > 0 && gmax > 0) { const T o = wave_partner<0>(x); combine(x, o, g > 0); }
  if (MAXS > 1 && gmax > 1) { const T o = wave_partner<1>(x); combine(x, o, g > 1); }
  if (MAXS > 2 && gmax > 2) { const T o = wave_partner<2>(x); combine(x, o, g > 2); }
  if (MAXS > 3 && gmax > 3) { const T o = wave_partner<3>(x); combine(x, o, g > 3); }
  if (MAXS > 4 && gmax > 4) { const T o = wave_partner<4>(x); combine(x, o, g > 4); }
  if (MAXS > 5 && gmax > 5) { const T o = wave_partner<5>(x); combine(x, o, g > 5); }
}
// the scalar forms: op(x, o) where the lane takes part
template <int MAXS, class T, class Op>
__device__ __forceinline__ T seg_reduce(T x, int g, int gmax, Op op) {
  seg_ladder<MAXS>(x, g, gmax, [&](T &a, T o, bool take) { a = take ? op(a, o) : a; });
  return x;
}

// All-reduce over aligned groups of 2^NS lanes, every lane taking part: v = op(v, partner) stage by stage.
template <int NS, class T, class Op>
__device__ __forceinline__ T butterfly(T v, Op op) {
  if (NS > 0) v = op(v, wave_partner<0>(v));
  if (NS > 1) v = op(v, wave_partner<1>(v));
  if (NS > 2) v = op(v, wave_partner<2>(v));
  if (NS > 3) v = op(v, wave_partner<3>(v));
  if (NS > 4) v = op(v, wave_partner<4>(v));
  if (NS > 5) v = op(v, wave_partner<5>(v));
  return v;
}

__device__ __forceinline__ int read_lane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float read_lane(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ double read_lane(double v, int l) {
  return __hiloint2double(read_lane(__double2hiint(v), l), read_lane(__double2loint(v), l));
}

// The value of lane - 1, one DPP move across the whole wave (wave_shr:1, no LDS traffic); lane 0, which has no such
// neighbour, takes `first`: without bound_ctrl the move does not write a lane whose source is out of range, so lane 0
// keeps the old value of the destination, which is `first`.  The move reads the neighbour's register whatever the
// neighbour is doing: call it with every lane of the wave active (wave-uniform trip counts; mask values, not control flow).
constexpr int kDppWaveShr1 = 0x138;
__device__ __forceinline__ int wave_shr1(int v, int first) {
  return __builtin_amdgcn_update_dpp(first, v, kDppWaveShr1, 0xf, 0xf, false);
}

// The value of lane + 1, the mirror image of wave_shr1 (wave_shl:1); lane 63 takes `last`.  The same rules apply.
constexpr int kDppWaveShl1 = 0x130;
__device__ __forceinline__ int wave_shl1(int v, int last) {
  return __builtin_amdgcn_update_dpp(last, v, kDppWaveShl1, 0xf, 0xf, false);
}

// All-reduce over rows of L lanes (16, 32 or the whole wave) without LDS traffic: the four DPP stages reduce every row
// of 16 lanes, v_readlane collects the four row results, combined as op(op(a, b), op(c, d)) -- float sums keep this
// order, (a + b) + (c + d).
template <int L, class T, class Op>
__device__ __forceinline__ T row_reduce(T v, Op op) {
  static_assert(L == 16 || L == 32 || L == 64, "");
  v = butterfly<4>(v, op);
  if (L == 16) return v;  // a DPP row: every lane holds its row's result
  const T a = read_lane(v, 0), b = read_lane(v, 16), c = read_lane(v, 32), d = read_lane(v, 48);
  if (L == 64) return op(op(a, b), op(c, d));
  return (threadIdx.x & 32) ? op(c, d) : op(a, b);
}
struct OpMax {
  __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
  __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
  __device__ __forceinline__ int operator()(int a, int b) const { return max(a, b); }
};
struct OpSum {
  template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
template <int L> __device__ __forceinline__ float row_max(float v) { return row_reduce<L>(v, OpMax{}); }
template <int L> __device__ __forceinline__ float row_sum(float v) { return row_reduce<L>(v, OpSum{}); }
__device__ __forceinline__ float wave_max(float v) { return row_reduce<64>(v, OpMax{}); }
__device__ __forceinline__ int wave_max(int v) { return row_reduce<64>(v, OpMax{}); }
__device__ __forceinline__ double wave_max(double v) { return row_reduce<64>(v, OpMax{}); }
__device__ __forceinline__ float wave_sum(float v) { return row_reduce<64>(v, OpSum{}); }

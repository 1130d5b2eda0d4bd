// out_store.h -- how the kernels' outputs leave the CU: one helper, one compile-time policy
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).
//
// Posteriors, row values and label sums are written once and read by nobody inside the launch, so the form of the store
// changes no result and no visibility rule; it only decides whether the lines stay dirty in the XCD's L2 until the
// kernel boundary writes them back.  -DNFST_OUT_STORE=n picks the form for every output store of the sweep kernels:
//   0  plain            global_store
//   1  nt               global_store ... nt       (non-temporal; the default)
//   2  sc1              global_store ... sc1      (write-through)
//   3  sc0 sc1          global_store ... sc0 sc1  (write-through, system scope)
// Vector stores only.  The write-through forms are written as inline asm (hipcc has no builtin for a flat global store
// with cache bits); the statement ends in `s_nop 1` so that the next instruction cannot overwrite the data registers
// before the store has read them, and carries no memory clobber: these bytes are never read back in the kernel, and
// with a clobber the LDS gathers of the next arc group could not be scheduled above the store of this one.  hipcc does
// not count an asm store in its vmcnt bookkeeping; uncounted stores can only make a later counted wait longer.
#pragma once

#ifndef NFST_OUT_STORE
#define NFST_OUT_STORE 1
#endif
static_assert(NFST_OUT_STORE >= 0 && NFST_OUT_STORE <= 3, "NFST_OUT_STORE: 0 plain, 1 nt, 2 sc1, 3 sc0 sc1");

typedef float out_f4v __attribute__((ext_vector_type(4)));

// 16 bytes; p is 16-byte aligned
__device__ __forceinline__ void out_store16(float *p, const float4 v) {
  const out_f4v x = {v.x, v.y, v.z, v.w};
#if NFST_OUT_STORE == 0
  *reinterpret_cast<out_f4v *>(p) = x;
#elif NFST_OUT_STORE == 1
  __builtin_nontemporal_store(x, reinterpret_cast<out_f4v *>(p));
#elif NFST_OUT_STORE == 2
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(x));
#else
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" : : "v"(p), "v"(x));
#endif
}

// 4 bytes: unaligned heads and tails, a few per workgroup (a narrow write-through store costs ~6x a 16-byte one per byte)
__device__ __forceinline__ void out_store4(float *p, const float v) {
#if NFST_OUT_STORE == 0
  *p = v;
#elif NFST_OUT_STORE == 1
  __builtin_nontemporal_store(v, p);
#elif NFST_OUT_STORE == 2
  asm volatile("global_store_dword %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v));
#else
  asm volatile("global_store_dword %0, %1, off sc0 sc1\n\ts_nop 1" : : "v"(p), "v"(v));
#endif
}

// 4 bytes per lane in bulk (k_chunk_post: consecutive lanes, consecutive arcs): the policy's form only where it does not
// pay per store -- a write-through dword costs ~6x the 16-byte store per byte, so those policies keep nt here
__device__ __forceinline__ void out_store4_bulk(float *p, const float v) {
#if NFST_OUT_STORE == 0
  *p = v;
#else
  __builtin_nontemporal_store(v, p);
#endif
}

// every store of this wave has left the CU (the profiling build's last stamp; asm stores are not in hipcc's count)
__device__ __forceinline__ void out_store_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// kernels.hip -- gfx950 (MI355X) kernels of the nFST lattice engine and their
// C-ABI launchers.  Design: DESIGN.md.  One workgroup owns one lattice; alpha and
// beta of all its states live in LDS as (mantissa, exponent) pairs -- an
// extended-exponent probability semiring: exact path sums like the reference's
// probability-domain beta sweep (/root/reference/src/modules/scorers.py:692-751)
// but without its float32 overflow and without exp/log on
// the level-to-level critical path.  Arc records stream once per sweep from HBM in
// level order; per-state sums are reduced by 2^k neighbouring lanes with wave64
// shuffles.  The sweeps use no MFMA: they are sparse gather/reduce work; the neuralised
// beta sweep (neural_kernels.h) has one dense product per state and runs it on float32 MFMA.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cmath>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "nfst_hip.h"
#include "tile_format.h"

namespace {

using namespace nfst_tile;

#include "semiring.h"
#include "wave_ops.h"
#include "tile_pipeline.h"
#include "out_store.h"
#include "fb_kernels.h"
#include "path_kernels.h"
#include "neural_kernels.h"
#include "pack_kernels.h"
#include "chunk_pack_kernels.h"
#include "chunk_kernels.h"
#include "expect_kernels.h"
#include "kbest_kernels.h"
#include "beam_kernels.h"
#include "swor_kernels.h"
#include "edit_kernels.h"
#include "lattice_edit_kernels.h"
#include "string_merge_kernels.h"
#include "string_logprob_kernels.h"
#include "string_align_kernels.h"
#include "string_logprob_grad_kernels.h"
#include "string_prefix_kernels.h"
#include "string_extend_kernels.h"
#include "slack_kernels.h"
#include "intersect_kernels.h"
#include "intersect_wide_kernels.h"
#include "positional_kernels.h"
#include "positional_expect_kernels.h"
#include "positional_kbest_kernels.h"

// ------------------------------------------------------------------ host helpers
int check_batch(const nfst_batch *lat) {
  if (!lat || lat->n_lattices <= 0 || lat->vocab <= 0 || lat->max_rows <= 0) return NFST_ERR_ARG;
  if (!lat->meta || !lat->row_ptr || !lat->fwd_stream || !lat->bwd_stream) return NFST_ERR_ARG;
  if (lat->total_arcs > 0 && (!lat->arc_src || !lat->arc_dst || !lat->arc_label)) return NFST_ERR_ARG;
  if ((lat->fwd_slots > 0 && !lat->fwd_perm) || (lat->bwd_slots > 0 && !lat->bwd_perm)) return NFST_ERR_ARG;
  if (lat->weighted && !lat->arc_w) return NFST_ERR_ARG;
  if (lat->max_rows > NFST_MAX_ROWS || lat->vocab > NFST_MAX_VOCAB) return NFST_ERR_LIMIT;
  if (((uintptr_t)lat->fwd_stream | (uintptr_t)lat->bwd_stream) & 15) return NFST_ERR_ARG;
  return NFST_OK;
}
int check_scores(const nfst_batch *lat, const nfst_scores *sc) {
  if (!sc || !sc->theta) return NFST_ERR_ARG;
  if (sc->theta_stride != 0 && sc->theta_stride < lat->vocab) return NFST_ERR_ARG;
  return NFST_OK;
}
int hip_status(hipError_t e) { return e == hipSuccess ? NFST_OK : NFST_ERR_HIP; }

constexpr int64_t kMaxLds = 160 * 1024;

// Dynamic LDS above 64 KiB needs a per-kernel opt-in; it is sticky per (device, kernel), so it is
// requested once per device, kernel and size (hipFuncSetAttribute is slow and not capturable in a
// graph).  The cache is the library's only process state: keyed by the current device and guarded
// by a mutex, so several devices in one process and launches from several host threads are safe.
struct LdsSeen { int dev; const void *fn; int64_t bytes; };
std::mutex g_lds_mutex;
std::vector<LdsSeen> g_lds_seen;

template <class K>
int set_lds(K kernel, int64_t bytes) {
  if (bytes > kMaxLds) return NFST_ERR_LIMIT;
  if (bytes <= 64 * 1024) return NFST_OK;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return NFST_ERR_HIP;
  const void *fn = reinterpret_cast<const void *>(kernel);
  std::lock_guard<std::mutex> lock(g_lds_mutex);
  for (LdsSeen &e : g_lds_seen)
    if (e.dev == dev && e.fn == fn) {
      if (e.bytes >= bytes) return NFST_OK;
      int rc = hip_status(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
      if (rc == NFST_OK) e.bytes = bytes;
      return rc;
    }
  int rc = hip_status(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  if (rc == NFST_OK) g_lds_seen.push_back({dev, fn, bytes});
  return rc;
}

// Every kernel of the library is launched here: the LDS opt-in, the launch, the launch's status.
template <class K, class... A>
int launch(K kernel, dim3 grid, dim3 block, int64_t lds, hipStream_t st, A... args) {
  if (int rc = set_lds(kernel, lds)) return rc;
  hipLaunchKernelGGL(kernel, grid, block, (size_t)lds, st, args...);
  return hip_status(hipGetLastError());
}

// number of CUs of the current device (cached per device; 256 on MI355X)
int cu_count() {
  static std::mutex mu;
  static std::vector<int> per_dev;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 256;
  std::lock_guard<std::mutex> lock(mu);
  if ((int)per_dev.size() <= dev) per_dev.resize(dev + 1, 0);
  if (per_dev[dev] == 0) {
    int v = 0;
    per_dev[dev] = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
  }
  return per_dev[dev];
}

// Switches of the launchers.  The environment is read ONCE, when the first launcher runs (never on the launch path
// afterwards); nfst_tuning_set() changes a switch from the host side (tests and A/B measurements flip flavours inside
// one process).  Every switch only selects among kernels that compute the same function.
struct Tuning {
  int64_t lds_reserve = 0;  // NFST_LDS_RESERVE_KB: LDS the one-lattice-per-CU flavours leave free on every CU
  int tw = 1;               // NFST_TW=0: loader + decoder + sweep instead of tile waves
  int precise = -1;         // NFST_PRECISE: 0 never, 1 whenever it fits, unset: programs deeper than kPreciseTiles tiles
  int chunked = 1;          // NFST_CHUNKED=0: never the chunked flavour (a batch with chunked programs runs the general kernels)
};
Tuning &tuning() {
  static Tuning t = [] {
    Tuning r;
    auto num = [](const char *name, long dflt) { const char *e = getenv(name); return e && *e ? strtol(e, nullptr, 10) : dflt; };
    const long kb = num("NFST_LDS_RESERVE_KB", 0);
    r.lds_reserve = (kb > 0 && kb <= 96) ? kb * 1024 : 0;
    r.tw = num("NFST_TW", 1) != 0;
    r.precise = (int)num("NFST_PRECISE", -1);
    r.chunked = num("NFST_CHUNKED", 1) != 0;
    return r;
  }();
  return t;
}
int64_t lds_reserve() { return tuning().lds_reserve; }

// ------------------------------------------------------------------ choosing the kernel of a sweep op
template <int N>
using ic = std::integral_constant<int, N>;

// arrays of per-arc extras: 0 none, 1 one (table weights or caller scores), 2 both; 3 (forward-backward tile waves only):
// their sum staged in LDS
int extras_case(const nfst_batch *lat, const nfst_scores *sc) {
  const bool w = lat->weighted && lat->arc_w;
  return w && sc->arc_scores ? 2 : (w || sc->arc_scores) ? 1 : 0;
}
template <bool Staged = false, class F>
int with_extras(int ex, F f) {
  if constexpr (Staged) {
    if (ex == 3) return f(ic<3>());
  }
  return ex == 2 ? f(ic<2>()) : ex == 1 ? f(ic<1>()) : f(ic<0>());
}
// threads of the pipeline flavours: 256 or 512, and 1024 where Deep
template <bool Deep, class F>
int with_threads(int nt, F f) {
  if constexpr (Deep) {
    if (nt == 1024) return f(ic<1024>());
  }
  return nt == 512 ? f(ic<512>()) : f(ic<256>());
}

// the flavours of a positional sweep: per-arc extras or none, arc records staged in LDS or read from the canonical arrays
template <class F>
int with_pos_flavour(bool extra, bool staged, F f) {
  typedef std::true_type Y;
  typedef std::false_type N;
  return extra ? (staged ? f(Y(), Y()) : f(Y(), N())) : (staged ? f(N(), Y()) : f(N(), N()));
}

// the largest lattice's arc count; NFST_BATCH_MAX_ARCS_CAP: that many or more
int64_t max_lattice_arcs(const nfst_batch *lat) { return ((int64_t)lat->reserved0 >> NFST_BATCH_MAX_ARCS_SHIFT) & NFST_BATCH_MAX_ARCS_CAP; }

// ring slots per sweep beside `fixed` bytes when `reserve` bytes of the CU's LDS stay free: at most kMaxRing, a multiple
// of four (tile_sweep2 takes four tiles per trip)
int ring_slots(int64_t fixed, int64_t slot_bytes, int64_t reserve) {
  const int64_t r = (kMaxLds - reserve - fixed) / slot_bytes;
  return (int)(r > kMaxRing ? kMaxRing : r) & ~3;
}

// the precise flavour (float64 mantissas, semiring.h) runs all-compact batches whose deepest program has more than
// kPreciseTiles tiles, when at least four ring slots per sweep fit beside the 16-byte values
int precise_ring(const nfst_batch *lat, int64_t fixed, int n_rings) {
  const Tuning &tu = tuning();
  if (!(lat->reserved0 & NFST_BATCH_ALL_COMPACT) || tu.precise == 0) return 0;
  if (tu.precise != 1 && lat->max_tiles <= kPreciseTiles) return 0;
  const int R = ring_slots(fixed, (int64_t)kSlotWordsP * 4 * n_rings, lds_reserve());
  return R >= 4 ? R : 0;
}

// Ring sizes per sweep from the LDS budget of one workgroup, and which pipeline runs.
//   deep   (at most one lattice per CU): loader + decoder + sweep waves, deep staging ring;
//   shared (more lattices than CUs): the decoder loads for itself, shallow staging ring, and
//          two workgroups share a CU's 160 KiB when the lattices are small enough.
// A lattice too large for the deep rings runs the shared pipeline with the whole CU.
// NFST_LDS_RESERVE_KB (environment, read once): LDS the one-lattice-per-CU flavour leaves free on
// every CU, so that a small kernel of another stream -- RCCL's all-reduce of the loss -- finds a CU
// to run on beside a sweep workgroup instead of waiting for one to retire.  Costs ring depth only.
struct RingCfg { int R, RS; bool self; };
bool ring_config(const LdsPlan &plan, bool fb, bool deep, RingCfg *c) {
  const int n_rings = fb ? 2 : 1;
  const int64_t slot = (int64_t)kSlotWords * 4 * n_rings;
  auto fixed = [&](int RS) { return fb ? plan.fb_bytes(0, RS) : plan.bwd_bytes(0, RS); };
  auto clampr = [](int64_t r) { return (int)(r > kMaxRing ? kMaxRing : r); };
  if (deep) {
    const int64_t r = (kMaxLds - lds_reserve() - fixed(kRawSlotsDeep)) / slot;
    if (r >= kMinRing) { *c = {clampr(r), kRawSlotsDeep, false}; return true; }
  } else {
    const int64_t r = (kMaxLds / 2 - fixed(kRawSlotsShared)) / slot;
    if (r >= kMinRing + 1) { *c = {clampr(r), kRawSlotsShared, true}; return true; }
  }
  const int64_t r = (kMaxLds - fixed(kRawSlotsShared)) / slot;
  if (r < kMinRing) return false;
  *c = {clampr(r), kRawSlotsShared, true};
  return true;
}

// The kernel of a sweep op for a batch: flavour, threads, extras case, ring slots per sweep (R), staging slots or, for
// staged extras, their room in floats (RS), dynamic LDS.
//   precise:    tile waves with float64 mantissas (programs deeper than kPreciseTiles tiles);
//   tile waves: one lattice per CU, all-compact (NFST_TW=0: the pipeline instead);
//   pipeline:   loader + decoder + sweep waves (deep) or self-loading decoders + sweeps (shared; ring_config);
//   fused:      forward-backward of all-compact batches without extras, more lattices than CUs (no rings at all);
//   general:    Viterbi from global memory.
enum class Flavour { precise, tile_waves, pipeline, fused, general };
//   pre_theta (forward-backward tile waves without extras, launches that want no label sums): the helper threads gather
//   the label weights of their preloaded arcs while the sweeps run (fb_kernels.h, PTH).
struct SweepPlan { Flavour flavour; int nt, ex, R, RS; int64_t lds; bool pre_theta = false; };

int plan_backward(const nfst_batch *lat, const nfst_scores *sc, SweepPlan *p) {
  const int ex = extras_case(lat, sc);
  const LdsPlan plan(lat->max_rows, lat->vocab);
  RingCfg cfg;
  if (!ring_config(plan, false, lat->n_lattices <= cu_count(), &cfg)) return NFST_ERR_LIMIT;
  if (ex && ((uintptr_t)lat->bwd_perm & 15)) return NFST_ERR_ARG;  // the extras waves read the slot -> arc map 16 bytes at a time
  if (const int Rp = precise_ring(lat, plan.bwd_fixed_precise(), 1)) {
    *p = {Flavour::precise, 512, ex, Rp, 0, plan.bwd_fixed_precise() + (int64_t)Rp * kSlotWordsP * 4};
  } else if (!cfg.self && (lat->reserved0 & NFST_BATCH_ALL_COMPACT) && tuning().tw) {
    const int64_t fixed = plan.bwd_bytes(0, 0) + 512;  // + 64 x 8 bytes of trash for the non-leader lanes' stores
    const int R = ring_slots(fixed, (int64_t)kSlotWords2 * 4, lds_reserve());
    if (R < 4) return NFST_ERR_LIMIT;
    *p = {Flavour::tile_waves, 512, ex, R, 0, fixed + (int64_t)R * kSlotWords2 * 4};
  } else {  // 512 threads: loader + decoder + sweep (deep); 256 threads: self-loading decoder + sweep
    *p = {Flavour::pipeline, cfg.self ? 256 : 512, ex, cfg.R, cfg.RS, plan.bwd_bytes(cfg.R, cfg.RS)};
  }
  return NFST_OK;
}

int plan_forward_backward(const nfst_batch *lat, const nfst_scores *sc, bool want_grad_theta, SweepPlan *p) {
  const int ex = extras_case(lat, sc);
  if (ex && (((uintptr_t)lat->fwd_perm | (uintptr_t)lat->bwd_perm | (uintptr_t)lat->arc_w | (uintptr_t)sc->arc_scores) & 15))
    return NFST_ERR_ARG;  // (maps and extras are read 16 bytes at a time)
  const LdsPlan plan(lat->max_rows, lat->vocab);
  const int cus = cu_count();
  const bool compact = lat->reserved0 & NFST_BATCH_ALL_COMPACT;
  // deep programs: the precise flavour, whatever the number of lattices
  if (const int Rp = precise_ring(lat, plan.fb_fixed_precise(), 2)) {
    *p = {Flavour::precise, 1024, ex, Rp, 0, plan.fb_fixed_precise() + (int64_t)Rp * kSlotWordsP * 4 * 2};
    return NFST_OK;
  }
  // Measured (profiles/r02_ab_fused.txt): 227 against 164 G arcs/s at 1024 lattices, 210 against 160 at 2048,
  // equal at 512; with one lattice per CU the three-wave pipeline is 10 % faster (46.8 against 51.8 us).
  // (512 threads at most: with 1024 the 128 registers a lane may have leave hipcc 64 VGPRs beside the
  // fused sweep's 32 AGPRs, and it then spills into AGPRs -- into the ones the sweep stages tiles in)
  if (!ex && compact && lat->n_lattices > cus) {
    *p = {Flavour::fused, lat->n_lattices <= 2 * cus ? 512 : 256, 0, 0, 0, plan.fb_bytes(0, 0)};
    return NFST_OK;
  }
  RingCfg cfg;
  if (!ring_config(plan, true, lat->n_lattices <= cus, &cfg)) return NFST_ERR_LIMIT;
  if (!cfg.self && compact && tuning().tw) {  // no staging ring; ring slots of kSlotWords2 words
    const int64_t slot = (int64_t)kSlotWords2 * 4 * 2, fixed = plan.fb_bytes(0, 0);
    const int R = ring_slots(fixed, slot, lds_reserve());
    if (R < 4) return NFST_ERR_LIMIT;
    *p = {Flavour::tile_waves, 1024, ex, R, 0, fixed + (int64_t)R * slot, !ex && !want_grad_theta};
    // per-arc extras staged in LDS (the sum of both arrays, 4 bytes per arc of the largest lattice) when a ring of at least
    // eight slots per sweep still fits beside them (lattices up to ~14k arcs at 2k states); RS carries the room in floats
    const int64_t max_arcs = max_lattice_arcs(lat);
    if (ex && max_arcs > 0 && max_arcs < NFST_BATCH_MAX_ARCS_CAP) {
      const int64_t words = (max_arcs + 8 + 3) & ~(int64_t)3;
      const int Rc = ring_slots(fixed + words * 4, slot, lds_reserve());
      // (with four slots per sweep the tile waves cannot run ahead: 69 us against 50 from HBM / L2 at 256 x 20k arcs)
      if (Rc >= 8) *p = {Flavour::tile_waves, 1024, 3, Rc, (int)words, fixed + (int64_t)Rc * slot + words * 4};
    }
    return NFST_OK;
  }
  // 1024 threads: loaders + decoders + sweeps and 10 more waves for the posterior pass (deep);
  // 512 / 256 threads: self-loading decoders + sweeps, two workgroups per CU when they fit (extras waves: 512 threads)
  const int nt = !cfg.self ? 1024 : (ex || lat->n_lattices <= 2 * cus) ? 512 : 256;
  *p = {Flavour::pipeline, nt, ex, cfg.R, cfg.RS, plan.fb_bytes(cfg.R, cfg.RS)};
  return NFST_OK;
}

int plan_viterbi(const nfst_batch *lat, const nfst_scores *sc, SweepPlan *p) {
  // all-compact batches: the tile-wave kernel (NFST_TW=0: one wave reading the program from global memory)
  const int ex = extras_case(lat, sc);
  const int64_t fixed = VitLds(lat->max_rows, lat->vocab).fixed();
  const int R = ring_slots(fixed, (int64_t)kSlotWords2 * 4, 0);
  if ((lat->reserved0 & NFST_BATCH_ALL_COMPACT) && R >= 8 && tuning().tw &&  // (its trips check four tiles ahead: eight slots)
      (!ex || (((uintptr_t)lat->arc_w | (uintptr_t)sc->arc_scores) & 3) == 0) && ((uintptr_t)lat->bwd_perm & 15) == 0)
    *p = {Flavour::tile_waves, kVitTwThreads, ex, R, 0, fixed + (int64_t)R * kSlotWords2 * 4};
  else
    *p = {Flavour::general, kVitThreads, ex, 0, 0, (int64_t)lat->max_rows * 12 + (int64_t)lat->vocab * 4 + 16};
  // (the general kernel keeps 12 bytes per row and the label scores in LDS: a large lattice over a large vocabulary
  // does not fit)
  return p->lds > kMaxLds ? NFST_ERR_LIMIT : NFST_OK;
}

// the outputs of nfst_backward (n_dirs 1) and nfst_forward_backward (n_dirs 2)
struct SweepOut {
  int n_dirs;
  float *logalpha, *logbeta;
  double *logz64;
  float *logz32, *posterior, *grad_theta, *beta_me;
  double *logz_total;
  int total_slot;
};

int launch_backward(const nfst_batch *lat, const nfst_scores *sc, const SweepOut &o, hipStream_t st) {
  SweepPlan p;
  if (int rc = plan_backward(lat, sc, &p)) return rc;
  auto go = [&](auto kernel) {
    return launch(kernel, dim3(lat->n_lattices), dim3(p.nt), p.lds, st, *lat, *sc, p.R, p.RS, o.logbeta, o.logz64, o.logz32,
                  (float2 *)o.beta_me);
  };
  switch (p.flavour) {
    case Flavour::precise: return with_extras(p.ex, [&](auto EX) { return go(k_backward<512, EX, true, true>); });
    case Flavour::tile_waves: return with_extras(p.ex, [&](auto EX) { return go(k_backward<512, EX, true>); });
    default:
      return with_threads<false>(p.nt, [&](auto NT) { return with_extras(p.ex, [&](auto EX) { return go(k_backward<NT, EX>); }); });
  }
}

int launch_forward_backward(const nfst_batch *lat, const nfst_scores *sc, const SweepOut &o, hipStream_t st) {
  SweepPlan p;
  if (int rc = plan_forward_backward(lat, sc, o.grad_theta != nullptr, &p)) return rc;
  auto go = [&](auto kernel) {
    return launch(kernel, dim3(lat->n_lattices), dim3(p.nt), p.lds, st, *lat, *sc, p.R, p.RS, o.logalpha, o.logbeta, o.logz64,
                  o.logz32, o.logz_total, o.total_slot, o.posterior, o.grad_theta, (float2 *)o.beta_me);
  };
  switch (p.flavour) {
    case Flavour::precise: return with_extras(p.ex, [&](auto EX) { return go(k_forward_backward<1024, EX, false, true, true>); });
    case Flavour::tile_waves:
      if (p.pre_theta) return go(k_forward_backward<1024, 0, false, true, false, true>);
      return with_extras<true>(p.ex, [&](auto EX) { return go(k_forward_backward<1024, EX, false, true>); });
    case Flavour::fused: return with_threads<false>(p.nt, [&](auto NT) { return go(k_forward_backward<NT, 0, true>); });
    default:
      return with_threads<true>(p.nt, [&](auto NT) {
        if constexpr (NT == 256) return go(k_forward_backward<256, 0>);  // (the plan gives extras 512 threads)
        else return with_extras(p.ex, [&](auto EX) { return go(k_forward_backward<NT, EX>); });
      });
  }
}

// The sweeps of nfst_backward and nfst_forward_backward.  Deep, narrow lattices run the chunked flavour (chunk_kernels.h):
// sweeps (one workgroup per lattice and direction), then posteriors / totals; lattices whose numbers leave its range are
// flagged on the device and run by the general kernels after it (a launch that finds no flag set returns at once).
int sweeps(const nfst_batch *lat, const nfst_scores *sc, const SweepOut &o, hipStream_t st) {
  if (!lat->chunks || !tuning().chunked)
    return o.n_dirs == 2 ? launch_forward_backward(lat, sc, o, st) : launch_backward(lat, sc, o, st);
  nfst_chunks *ck = const_cast<nfst_chunks *>(lat->chunks);
  if (ck->n_lattices != lat->n_lattices || ck->total_rows != lat->total_rows || ck->total_arcs != lat->total_arcs || !ck->meta ||
      !ck->tab || !ck->stream || !ck->pos || !ck->label || !ck->ws || ck->ws_bytes < nfst_chunks_ws_bytes(ck) || ck->threads < 64 ||
      ck->threads > 1024 || (ck->threads & 63) || ck->lds_bytes <= 0 || ck->lds_bytes > kMaxLds || ((uintptr_t)ck->ws & 15))
    return NFST_ERR_ARG;
  ck->launches = ck->launches >= INT_MAX - 1 ? 1 : ck->launches + 1;
  nfst_batch rest = *lat;
  rest.chunks = nullptr;
  rest.only = chk_ws(*ck).flags;
  rest.only_tag = ck->launches;
  int rc = launch(k_chunk_sweep, dim3(lat->n_lattices * o.n_dirs), dim3(ck->threads), ck->lds_bytes, st, *lat, *sc, *ck, rest.only_tag,
                  o.n_dirs, o.logalpha, o.logbeta, o.logz64, o.logz32, o.grad_theta, (float2 *)o.beta_me);
  if (rc) return rc;
  if (o.n_dirs == 2 && (o.posterior || o.grad_theta || o.logz_total)) {
    // workgroups of 256 threads, about four arcs per thread of the largest lattice: a slice of a lattice's arcs each
    const int parts = (o.posterior || o.grad_theta) ? (int)std::max<int64_t>(1, std::min<int64_t>(64, (max_lattice_arcs(lat) + 1023) / 1024)) : 1;
    if ((rc = launch(k_chunk_post, dim3(lat->n_lattices * parts), dim3(256), o.grad_theta ? (int64_t)lat->vocab * 4 : 0, st, *lat, *sc,
                     *ck, rest.only_tag, parts, o.posterior, o.grad_theta, o.logz_total, o.total_slot)))
      return rc;
  }
  return sweeps(&rest, sc, o, st);
}

// ------------------------------------------------------------------ neural kernels and path_logprob
// Phase B of the two-phase neural kernels runs on three bfloat16 parts of Wh when hid is a multiple of 64 from 256 on
// (below 256 the split's two barriers per pass cost more than the matrix pipe gains: H = 128 1.41 against 1.39 ms); the
// parts are packed in MFMA fragment order into the workspace behind its first `ws_floats` floats.
int pack_wh(const float *wh, int hid, float *ws, int64_t ws_floats, hipStream_t st, int *packed) {
  *packed = hid % 64 == 0 && hid >= 256;
  if (!*packed) return NFST_OK;
  return launch(k_pack_mfma_b3, dim3(((hid >> 4) * (hid >> 5) * 64 + 255) / 256), dim3(256), 0, st, wh, hid,
                reinterpret_cast<uint4 *>(ws + neu_pack_off(ws_floats)));
}
// the hidden size as a template argument: the packed kernels <8 / 16 / 32> up to 32, then the two-phase kernels
// <1 / 2 / 4 / 8>.  BASELINE batch, whole op: H = 8 0.52 against 1.19 ms, 16 0.58 / 1.18, 32 1.07 / 1.19; with a whole
// wave per record (H = 64) the packed kernel has nothing to pack and loses to the two-phase one: 1.97 / 1.24
template <class S, class T>
int with_hid(int hid, S small, T two_phase) {
  if (hid <= 8) return small(ic<8>());
  if (hid <= 16) return small(ic<16>());
  if (hid <= 32) return small(ic<32>());
  if (hid <= 64) return two_phase(ic<1>());
  if (hid <= 128) return two_phase(ic<2>());
  if (hid <= 256) return two_phase(ic<4>());
  return two_phase(ic<8>());
}

// the variant of the 16-byte streaming path_logprob kernels (plp_variant) as template arguments <NV, RB, L>; 0: the
// general kernel
template <class V, class G>
int with_plp_variant(int u, V v4, G general) {
  switch (u) {
    case 0: return general();
    case 1: return v4(ic<1>(), ic<8>(), ic<16>());
    case 2: return v4(ic<2>(), ic<4>(), ic<16>());
    case 3: return v4(ic<3>(), ic<4>(), ic<16>());
    case 4: return v4(ic<4>(), ic<2>(), ic<16>());
    case 5: return v4(ic<5>(), ic<2>(), ic<16>());
    case 6: return v4(ic<6>(), ic<2>(), ic<16>());
    case 7: return v4(ic<7>(), ic<1>(), ic<16>());
    case 8: return v4(ic<8>(), ic<1>(), ic<16>());
    case 13: return v4(ic<5>(), ic<2>(), ic<32>());  // 129 .. 160 slots
    case 14: return v4(ic<6>(), ic<2>(), ic<32>());
    case 15: return v4(ic<7>(), ic<1>(), ic<32>());
    default: return v4(ic<8>(), ic<1>(), ic<32>());  // 16: up to 256 slots
  }
}

}  // namespace

extern "C" {

int nfst_device_available(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n > 0 ? 1 : 0;
}

int nfst_tuning_set(const char *name, int value) {
  if (!name) return NFST_ERR_ARG;
  Tuning &t = tuning();
  const std::string n(name);
  if (n == "tw") t.tw = value != 0;
  else if (n == "precise") t.precise = value < 0 ? -1 : (value != 0);
  else if (n == "chunked") t.chunked = value != 0;
  else if (n == "lds_reserve_kb") t.lds_reserve = (value > 0 && value <= 96) ? (int64_t)value * 1024 : 0;
  else return NFST_ERR_ARG;
  return NFST_OK;
}

// ---------------------------------------------------------------- the packer on the device
int nfst_dense_to_arcs_count(const void *emission, int emission_is_float, const int64_t *transition, int32_t n_lattices,
                             int32_t n_rows, int32_t vocab, uint8_t *reach, int32_t *row_cnt, int32_t *counts,
                             int32_t *status, void *stream) {
  if (!emission || !transition || !reach || !row_cnt || !counts || !status || n_lattices <= 0 || n_rows <= 0 || vocab <= 0) return NFST_ERR_ARG;
  if (n_rows > NFST_MAX_ROWS || vocab > NFST_MAX_VOCAB) return NFST_ERR_LIMIT;
  return launch(emission_is_float ? k_dense_reach<true> : k_dense_reach<false>, dim3(n_lattices), dim3(kPkThreads), (int64_t)n_rows * 12,
                (hipStream_t)stream, emission, transition, (int)n_rows, (int)vocab, reach, row_cnt, counts, status);
}

int nfst_dense_to_arcs_write(const void *emission, int emission_is_float, const int64_t *transition, int32_t n_lattices,
                             int32_t n_rows, int32_t vocab, const uint8_t *reach, const int32_t *row_cnt,
                             const int64_t *arc_off, int32_t *src, int32_t *label, int32_t *dst, float *arc_w, void *stream) {
  if (!emission || !transition || !reach || !row_cnt || !arc_off || !src || !label || !dst || n_lattices <= 0 || n_rows <= 0 || vocab <= 0)
    return NFST_ERR_ARG;
  if (emission_is_float && !arc_w) return NFST_ERR_ARG;
  if (n_rows > NFST_MAX_ROWS || vocab > NFST_MAX_VOCAB) return NFST_ERR_LIMIT;
  return launch(emission_is_float ? k_dense_write<true> : k_dense_write<false>, dim3(n_lattices), dim3(kPkThreads), (int64_t)n_rows * 4,
                (hipStream_t)stream, emission, transition, (int)n_rows, (int)vocab, reach, row_cnt, arc_off, src, label, dst, arc_w);
}

int64_t nfst_pack_device_ws_bytes(int32_t n_lattices, int64_t total_rows, int64_t total_arcs) {
  if (n_lattices <= 0 || total_rows < 0 || total_arcs < 0) return NFST_ERR_ARG;
  return 4 * pk_ws_words(n_lattices, total_rows, total_arcs);
}

int nfst_pack_device_limits(int64_t *lds_bytes, int32_t *max_keys, int32_t *threads) {
  if (!lds_bytes || !max_keys || !threads) return NFST_ERR_ARG;
  *lds_bytes = kPkLdsBytes; *max_keys = kPkMaxKeys; *threads = kPkThreads;
  return NFST_OK;
}

static int pack_device_args(const nfst_arcs_device *arcs, const nfst_pack_opts *opts, void *ws, int64_t ws_bytes, PkArgs *a) {
  if (!arcs || !ws || arcs->n_lattices <= 0 || arcs->vocab <= 0 || !arcs->n_rows || !arcs->row_off || !arcs->arc_off) return NFST_ERR_ARG;
  if (arcs->total_arcs > 0 && (!arcs->src || !arcs->label || !arcs->dst)) return NFST_ERR_ARG;
  if (arcs->vocab + 2 > 2048) return NFST_ERR_LIMIT;  // compact tiles only: the host packer takes wider vocabularies
  if (opts && ((opts->slots_per_lane != 0 && opts->slots_per_lane != 4) || opts->reserved1 == 1)) return NFST_ERR_LIMIT;
  if (ws_bytes < 4 * pk_ws_words(arcs->n_lattices, arcs->total_rows, arcs->total_arcs) || ((uintptr_t)ws & 15)) return NFST_ERR_ARG;
  *a = PkArgs{};
  a->n_rows = arcs->n_rows; a->row_off = arcs->row_off; a->arc_off = arcs->arc_off;
  a->src = arcs->src; a->label = arcs->label; a->dst = arcs->dst; a->w = arcs->arc_w;
  a->vocab = arcs->vocab; a->group_mode = opts ? opts->group_mode : 0;
  a->ws = (int32_t *)ws; a->total_rows = arcs->total_rows; a->total_arcs = arcs->total_arcs; a->n_lattices = arcs->n_lattices;
  return NFST_OK;
}

int nfst_pack_device_plan(const nfst_arcs_device *arcs, const nfst_pack_opts *opts, void *ws, int64_t ws_bytes, int32_t *meta,
                          int32_t *status, int32_t *scratch_rows, void *stream) {
  PkArgs a;
  int rc = pack_device_args(arcs, opts, ws, ws_bytes, &a);
  if (rc) return rc;
  if (!meta || !status || !scratch_rows) return NFST_ERR_ARG;
  a.meta = meta; a.status = status; a.scratch = scratch_rows;
  return launch(k_pack_lattice<false>, dim3(arcs->n_lattices), dim3(kPkThreads), kPkLdsBytes, (hipStream_t)stream, a);
}

int nfst_pack_device_emit(const nfst_arcs_device *arcs, const nfst_pack_opts *opts, void *ws, int64_t ws_bytes,
                          const int32_t *meta, int32_t *status, const nfst_batch *out, void *stream) {
  PkArgs a;
  int rc = pack_device_args(arcs, opts, ws, ws_bytes, &a);
  if (rc) return rc;
  if (!meta || !status || !out || out->n_lattices != arcs->n_lattices) return NFST_ERR_ARG;
  if ((rc = check_batch(out))) return rc;
  if (!out->arc_sd || !out->arc_l16 || (arcs->arc_w && !out->arc_w)) return NFST_ERR_ARG;
  if ((((uintptr_t)out->fwd_perm | (uintptr_t)out->bwd_perm) & 15)) return NFST_ERR_ARG;
  a.meta = const_cast<int32_t *>(meta); a.status = status; a.scratch = nullptr; a.out = *out;
  // the slack behind the streams and the 8 spare entries of the 6-byte arc arrays are part of the format: zero
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(const_cast<uint32_t *>(out->fwd_stream) + (out->fwd_words - kStreamSlack), 0, kStreamSlack * 4, st) != hipSuccess ||
      hipMemsetAsync(const_cast<uint32_t *>(out->bwd_stream) + (out->bwd_words - kStreamSlack), 0, kStreamSlack * 4, st) != hipSuccess ||
      hipMemsetAsync(const_cast<uint32_t *>(out->arc_sd) + out->total_arcs, 0, kArcSpare * 4, st) != hipSuccess ||
      hipMemsetAsync(const_cast<uint16_t *>(out->arc_l16) + out->total_arcs, 0, kArcSpare * 2, st) != hipSuccess)
    return NFST_ERR_HIP;
  return launch(k_pack_lattice<true>, dim3(arcs->n_lattices), dim3(kPkThreads), kPkLdsBytes, st, a);
}

int64_t nfst_pack_chunks_device_ws_bytes(int32_t n_lattices, int64_t total_rows, int64_t total_arcs) {
  if (n_lattices <= 0 || total_rows < 0 || total_arcs < 0) return NFST_ERR_ARG;
  return 4 * cp_ws_words(n_lattices, total_rows);
}

static int chunk_device_args(const nfst_arcs_device *arcs, const void *pack_ws, int64_t pack_ws_bytes, const nfst_batch *batch,
                             const void *ws, int64_t ws_bytes, CpArgs *a) {
  if (!arcs || !pack_ws || !batch || !ws || arcs->n_lattices <= 0 || !arcs->row_off || !arcs->arc_off) return NFST_ERR_ARG;
  if (batch->n_lattices != arcs->n_lattices || !batch->meta || !batch->arc_src || !batch->arc_dst || !batch->arc_label) return NFST_ERR_ARG;
  if (batch->max_rows <= 0 || batch->max_rows > NFST_MAX_ROWS) return NFST_ERR_ARG;
  if (pack_ws_bytes < 4 * pk_ws_words(arcs->n_lattices, arcs->total_rows, arcs->total_arcs) ||
      ws_bytes < 4 * cp_ws_words(arcs->n_lattices, arcs->total_rows) || ((uintptr_t)ws & 3))
    return NFST_ERR_ARG;
  *a = CpArgs{};
  a->pk_ws = (const int32_t *)pack_ws; a->row_off = arcs->row_off; a->arc_off = arcs->arc_off;
  a->in_rows = arcs->total_rows; a->in_arcs = arcs->total_arcs; a->n_lattices = arcs->n_lattices;
  a->meta = batch->meta; a->arc_src = batch->arc_src; a->arc_dst = batch->arc_dst; a->arc_label = batch->arc_label;
  a->ws = (int32_t *)const_cast<void *>(ws);
  return NFST_OK;
}

int nfst_pack_chunks_device_plan(const nfst_arcs_device *arcs, const void *pack_ws, int64_t pack_ws_bytes, const nfst_batch *batch,
                                 const nfst_chunk_opts *opts, void *ws, int64_t ws_bytes, int32_t *summary, int32_t *launched,
                                 void *stream) {
  if (!summary || !launched) return NFST_ERR_ARG;
  *launched = 0;
  CpArgs a;
  int rc = chunk_device_args(arcs, pack_ws, pack_ws_bytes, batch, ws, ws_bytes, &a);
  if (rc) return rc;
  nfst_chunk_opts o{};
  if (opts) o = *opts;
  int threads;
  int64_t lds_bytes;
  if (!nfst_chunk::resolve_opts(arcs->n_lattices, o.threads, o.lds_bytes, &threads, &lds_bytes)) return NFST_ERR_ARG;
  // (nfst_pack_chunks' quick no: up to ~160 levels the general kernels are done before this flavour's fixed costs are)
  if (!o.force && batch->max_tiles <= 160) return NFST_OK;
  a.threads = threads; a.lds_bytes = lds_bytes; a.max_chunks = o.max_chunks; a.summary = summary;
  if ((rc = launch(k_chunk_plan, dim3(2 * arcs->n_lattices), dim3(kPkThreads), cp_plan_lds(batch->max_rows), (hipStream_t)stream, a,
                   (int)batch->max_rows)))
    return rc;
  *launched = 1;
  return NFST_OK;
}

int nfst_pack_chunks_device_emit(const nfst_arcs_device *arcs, const void *pack_ws, int64_t pack_ws_bytes, const nfst_batch *batch,
                                 const nfst_chunks *chunks, const void *ws, int64_t ws_bytes, void *stream) {
  CpArgs a;
  int rc = chunk_device_args(arcs, pack_ws, pack_ws_bytes, batch, ws, ws_bytes, &a);
  if (rc) return rc;
  if (!chunks || chunks->n_lattices != arcs->n_lattices || !chunks->meta || !chunks->tab || !chunks->stream || !chunks->pos ||
      !chunks->label || chunks->n_stream < 64)
    return NFST_ERR_ARG;
  a.cmeta = chunks->meta; a.tab = const_cast<int32_t *>(chunks->tab); a.pos = const_cast<int32_t *>(chunks->pos);
  a.stream = const_cast<uint32_t *>(chunks->stream); a.label = const_cast<uint16_t *>(chunks->label);
  hipStream_t st = (hipStream_t)stream;
  // the slack behind the last program's entries is part of the format: zero
  if (hipMemsetAsync(a.stream + (chunks->n_stream - 64), 0, 64 * 4, st) != hipSuccess ||
      hipMemsetAsync(a.label + (chunks->n_stream - 64), 0, 64 * 2, st) != hipSuccess)
    return NFST_ERR_HIP;
  return launch(k_chunk_emit, dim3(2 * arcs->n_lattices), dim3(kPkThreads), 4 * (int64_t)batch->max_rows, st, a);
}

int64_t nfst_lds_bytes(const nfst_batch *lat) {
  if (!lat) return NFST_ERR_ARG;
  return LdsPlan(lat->max_rows, lat->vocab).fb_bytes(kMinRing, kRawSlotsShared);
}

int nfst_backward(const nfst_batch *lat, const nfst_scores *scores, float *logbeta, double *logz64,
                  float *logz32, float *beta_me, void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  return sweeps(lat, scores, {1, nullptr, logbeta, logz64, logz32, nullptr, nullptr, beta_me, nullptr, 0}, (hipStream_t)stream);
}

int nfst_forward_backward(const nfst_batch *lat, const nfst_scores *scores, float *logalpha,
                          float *logbeta, double *logz64, float *logz32, float *posterior,
                          float *grad_theta, float *beta_me, double *logz_total, int32_t total_slot, void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  if (posterior && ((uintptr_t)posterior & 15)) return NFST_ERR_ARG;
  if (logz_total && (total_slot < 0 || total_slot > 2)) return NFST_ERR_ARG;
  if (!lat->arc_sd || !lat->arc_l16 || ((uintptr_t)lat->arc_sd & 15) || ((uintptr_t)lat->arc_l16 & 7)) return NFST_ERR_ARG;
  return sweeps(lat, scores, {2, logalpha, logbeta, logz64, logz32, posterior, grad_theta, beta_me, logz_total, (int)total_slot},
                (hipStream_t)stream);
}

int nfst_viterbi(const nfst_batch *lat, const nfst_scores *scores, float *best, int32_t *paths,
                 int32_t *path_arcs, int32_t *lengths, int32_t max_len, int32_t pad, void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  if (!best || !paths || !lengths || max_len <= 0) return NFST_ERR_ARG;
  SweepPlan p;
  if ((rc = plan_viterbi(lat, scores, &p))) return rc;
  const hipStream_t st = (hipStream_t)stream;
  if (p.flavour == Flavour::tile_waves)
    return with_extras(p.ex, [&](auto EX) {
      return launch(k_viterbi_tw<EX>, dim3(lat->n_lattices), dim3(p.nt), p.lds, st, *lat, *scores, p.R, best, paths, path_arcs, lengths,
                    (int)max_len, (int)pad);
    });
  return launch(k_viterbi, dim3(lat->n_lattices), dim3(p.nt), p.lds, st, *lat, *scores, best, paths, path_arcs, lengths, (int)max_len,
                (int)pad);
}

int nfst_sample_paths(const nfst_batch *lat, const nfst_scores *scores, const float *beta_me,
                      const double *logz64, int32_t k, int32_t max_len, const float *uniforms,
                      uint64_t seed, int32_t pad, int32_t *paths, int32_t *path_arcs,
                      int32_t *lengths, float *logq, int32_t *status, void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  if (!beta_me || !logz64 || !paths || !lengths || !logq || !status || k <= 0 || max_len <= 0)
    return NFST_ERR_ARG;
  if (!lat->arc_sd || !lat->arc_l16) return NFST_ERR_ARG;
  const int stage_theta = (int64_t)lat->max_rows * 8 + (int64_t)lat->vocab * 4 <= 96 * 1024;
  const int64_t lds_min = (int64_t)lat->max_rows * 8 + (stage_theta ? (int64_t)((lat->vocab + 3) & ~3) * 4 : 0);
  // room for a lattice's CSR (row pointers + 6 bytes per arc; a program's slots bound its arcs): the kernel stages it
  // when it fits what it was given
  const int64_t csr = ((int64_t)lat->max_rows + 8) * 4 + ((int64_t)lat->max_tiles * 256 + 8) * 6;
  const int64_t lds = lds_min + csr <= kMaxLds ? lds_min + csr : (lds_min + 64 * 1024 <= kMaxLds ? kMaxLds : lds_min);
  // 16 walks per 256 threads; up to 64 walks (1024 threads) of a lattice in one block share its staged data
  // (with the arcs' probabilities precomputed per block -- path_arcs given and the CSR fits -- every block has 1024
  // threads for that pass, whatever k)
  const bool precdf = path_arcs && lds > lds_min;  // (the kernel decides per lattice, from its own arc count)
  const int walks = (k >= 64 || precdf) ? 64 : ((k + 15) / 16) * 16;
  return launch(k_sample, dim3(lat->n_lattices, (k + walks - 1) / walks), dim3(walks * 16), lds, (hipStream_t)stream, *lat, *scores,
                (const float2 *)beta_me, logz64, (int)k, (int)max_len, uniforms, seed, (int)pad, stage_theta, (int)lds, paths, path_arcs,
                lengths, logq, status);
}

int nfst_score_paths(const nfst_batch *lat, const nfst_scores *scores, const int32_t *marks, int32_t k,
                     int32_t max_len, float *path_score, int32_t *end_state, void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  if (!marks || !path_score || !end_state || k <= 0 || max_len <= 0) return NFST_ERR_ARG;
  return launch(k_score_paths, dim3(lat->n_lattices, (k + 63) / 64), dim3(64), 0, (hipStream_t)stream, *lat, *scores, marks, (int)k,
                (int)max_len, path_score, end_state);
}

int nfst_step(const nfst_batch *lat, const int64_t *state, const int64_t *label, int64_t *next,
              int32_t k, void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if (!state || !label || !next || k <= 0) return NFST_ERR_ARG;
  const int64_t n = (int64_t)lat->n_lattices * k;
  return launch(k_step, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *lat, state, label, next, (int)k, n);
}

int nfst_emission_mask(const nfst_batch *lat, const int64_t *state, const int64_t *inp, int32_t pad,
                       int32_t bos, int32_t eos, int32_t has_to_end, float *out, int32_t k,
                       void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if (!state || !out || k <= 0) return NFST_ERR_ARG;
  const int64_t n = (int64_t)lat->n_lattices * k;
  return launch(k_row_gather<0>, dim3((unsigned)n), dim3(64), (int64_t)lat->vocab * 4, (hipStream_t)stream, *lat, state,
                (const float *)nullptr, inp, (int)pad, (int)bos, (int)eos, (int)has_to_end, out, (int)k);
}

int nfst_beta_logits(const nfst_batch *lat, const float *values, const int64_t *state, float *out,
                     int32_t k, void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if (!values || !state || !out || k <= 0) return NFST_ERR_ARG;
  const int64_t n = (int64_t)lat->n_lattices * k;
  return launch(k_row_gather<1>, dim3((unsigned)n), dim3(64), (int64_t)lat->vocab * 4, (hipStream_t)stream, *lat, state, values,
                (const int64_t *)nullptr, 0, 0, 0, 0, out, (int)k);
}

int nfst_proposal_step(const nfst_batch *lat, const int64_t *state, const int64_t *inp, const float *scores,
                       const float *values, int32_t pad, int32_t bos, int32_t eos, int32_t has_to_end, float temperature,
                       const float *uniforms, const int64_t *forced, const nfst_step_extras *extras, int64_t *symbol,
                       float *logq, float *logz, int64_t *next_state, float *logits_out, int32_t k, void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if (!state || !scores || !symbol || !logq || !next_state || k <= 0 || !(temperature > 0.0f)) return NFST_ERR_ARG;
  if (!uniforms && !forced) return NFST_ERR_ARG;
  if (pad < 0 || pad >= lat->vocab) return NFST_ERR_ARG;
  if (lat->vocab > kStepMaxVocab) return NFST_ERR_LIMIT;
  nfst_step_extras ex = {};
  if (extras) {
    ex = *extras;
    if ((ex.accumulated || ex.vocab_use) && (ex.insertion_mark < 0 || ex.insertion_mark >= lat->vocab || ex.length < 1))
      return NFST_ERR_ARG;
  }
  const int64_t n = (int64_t)lat->n_lattices * k;
  const int64_t lds = (int64_t)kStepWaves * ((values && ex.value_state) ? 3 : 2) * lat->vocab * 4;
  if (lds > kMaxLds) return NFST_ERR_LIMIT;  // (three rows per walker with a value state: vocab <= 3413)
  return launch(k_proposal_step, dim3((unsigned)((n + kStepWaves - 1) / kStepWaves)), dim3(64 * kStepWaves), lds, (hipStream_t)stream,
                *lat, state, inp, scores, values, (int)pad, (int)bos, (int)eos, (int)has_to_end, temperature, uniforms, forced, ex, symbol,
                logq, logz, next_state, logits_out, (int)k, n);
}

int nfst_proposal_step_backward(const nfst_batch *lat, const int64_t *value_state, const float *logits,
                                const int64_t *symbol, const float *logz, const float *g_logq, const float *g_logz,
                                int32_t pad, float temperature, float *grad_scores, float *grad_values, int32_t k,
                                void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if (!logits || !symbol || !logz || !grad_scores || k <= 0 || !(temperature > 0.0f)) return NFST_ERR_ARG;
  if (grad_values && !value_state) return NFST_ERR_ARG;
  if (!g_logq && !g_logz) return NFST_ERR_ARG;
  const int64_t n = (int64_t)lat->n_lattices * k;
  return launch(k_proposal_step_bwd, dim3((unsigned)((n + kStepWaves - 1) / kStepWaves)), dim3(64 * kStepWaves), 0, (hipStream_t)stream,
                *lat, value_state, logits, symbol, logz, g_logq, g_logz, (int)pad, temperature, grad_scores, grad_values, (int)k, n);
}

int64_t nfst_neural_ws_floats(const nfst_batch *lat, int32_t hid) {
  if (!lat || hid <= 0) return NFST_ERR_ARG;
  // u and beta_hat planes, (mantissa, exponent) rows, and Wh as three bfloat16 parts in MFMA fragment order (k_pack_mfma_b3)
  return neu_pack_off(2 * (int64_t)lat->n_lattices * lat->max_rows * (hid + 1)) + 2 * (int64_t)hid * hid;  // (+ Wh: float32 or 3 x bfloat16)
}

int nfst_backward_neural(const nfst_batch *lat, const float *label_x, const float *wh, const float *w, int32_t hid,
                         float *log_beta, float *beta_hat, float *ws, void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if (!label_x || !wh || !w || !log_beta || !beta_hat || !ws || hid <= 0) return NFST_ERR_ARG;
  if (hid > kNeuMaxHid) return NFST_ERR_LIMIT;
  const int64_t lds = NeuLds(lat->max_rows, hid).bytes();
  const hipStream_t st = (hipStream_t)stream;
  int wh_packed;
  if ((rc = pack_wh(wh, hid, ws, 2 * (int64_t)lat->n_lattices * lat->max_rows * (hid + 1), st, &wh_packed))) return rc;
  const dim3 grid(lat->n_lattices), block(kNeuThreads);
  return with_hid(
      hid,
      [&](auto LPR) {
        return launch(k_backward_neural_small<LPR>, grid, block, lds, st, *lat, label_x, wh, w, (int)hid, log_beta, beta_hat, ws);
      },
      [&](auto HC) {
        return launch(k_backward_neural<HC>, grid, block, lds, st, *lat, label_x, wh, w, (int)hid, log_beta, beta_hat, ws, wh_packed);
      });
}

#ifdef NFST_PROF
extern "C" int nfst_prof_read(unsigned long long *out, int n) {  // profiling build only
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(fb_prof), sizeof(unsigned long long) * (size_t)n) == hipSuccess ? 0 : -1;
}
#endif
#ifdef NFST_PK_STAMPS
extern "C" int nfst_debug_pk_stamps(unsigned long long *out) {  // profiling build only
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(pk_stamps), sizeof(unsigned long long) * 32) == hipSuccess ? 0 : -1;
}
#endif
#ifdef NFST_NEU_STAMPS
extern "C" int nfst_debug_neu_stamps(unsigned long long *out, int reset) {  // profiling build only
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(neu_stamps), sizeof(unsigned long long) * 128) != hipSuccess) return -1;
  if (reset) { unsigned long long z[128] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(neu_stamps), z, sizeof(z)) != hipSuccess) return -1; }
  return 0;
}
#endif

int64_t nfst_neural_grad_ws_floats(const nfst_batch *lat, int32_t hid) {
  if (!lat || hid <= 0) return NFST_ERR_ARG;
  return neu_pack_off(2 * (int64_t)lat->n_lattices * lat->max_rows * hid) + 2 * (int64_t)hid * hid;  // ... + Wh^T in fragment order (float32 or 3 x bfloat16)
}

int nfst_backward_neural_grad(const nfst_batch *lat, const float *label_x, const float *wh_t, const float *w, int32_t hid,
                              const float *beta_hat, const float *ws_fwd, const float *g_log_beta, const float *g_beta_hat,
                              float *gamma, float *grad_label_x, float *grad_w, float *ws, void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if (!label_x || !wh_t || !w || !beta_hat || !ws_fwd || !g_log_beta || !gamma || !grad_label_x || !grad_w || !ws || hid <= 0)
    return NFST_ERR_ARG;
  if (hid > kNeuMaxHid) return NFST_ERR_LIMIT;
  if (lat->fwd_slots > 0 && !lat->fwd_perm) return NFST_ERR_ARG;
  const int64_t lds = NeuGradLds(lat->max_rows, hid).bytes();
  const hipStream_t st = (hipStream_t)stream;
  int wh_packed;
  if ((rc = pack_wh(wh_t, hid, ws, 2 * (int64_t)lat->n_lattices * lat->max_rows * hid, st, &wh_packed))) return rc;
  // (the packed kernel sums dL/dx per lattice in LDS when [V, hid] floats fit beside its rows and staged tiles)
  const int64_t lds_small0 = (int64_t)neu_rows_al(lat->max_rows) * 8 + (int64_t)((lat->max_rows + 3) & ~3) * 4 + 2 * kNeuGradStageWords * 4 + 16;
  // (BASELINE batch, whole gradient op: H = 8 1.34 ms with the LDS table against 1.72 with global atomics; H = 16 1.80
  // against 1.56, H = 32 3.13 against 2.56 -- the table is contended only when its rows are a few lanes wide)
  const int gx_in_lds = hid <= 8 && lds_small0 + (int64_t)lat->vocab * hid * 4 <= kMaxLds;
  const int64_t lds_small = lds_small0 + (gx_in_lds ? (int64_t)lat->vocab * hid * 4 : 0);
  const dim3 grid(lat->n_lattices), block(kNeuThreads);
  return with_hid(
      hid,
      [&](auto LPR) {
        return launch(k_backward_neural_grad_small<LPR>, grid, block, lds_small, st, *lat, label_x, wh_t, w, (int)hid, beta_hat, ws_fwd,
                      g_log_beta, g_beta_hat, gamma, grad_label_x, grad_w, ws, gx_in_lds);
      },
      [&](auto HC) {
        return launch(k_backward_neural_grad<HC>, grid, block, lds, st, *lat, label_x, wh_t, w, (int)hid, beta_hat, ws_fwd, g_log_beta,
                      g_beta_hat, gamma, grad_label_x, grad_w, ws, wh_packed);
      });
}

int nfst_gather_label_scores(const nfst_batch *lat, const nfst_scores *scores, float *out, void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  if (!out) return NFST_ERR_ARG;
  return launch(k_gather_label_scores, dim3(8, lat->n_lattices), dim3(256), 0, (hipStream_t)stream, *lat, *scores, out);
}

// consecutive parts of a caller's workspace, each 256-byte aligned; with a null base only the size adds up
struct WsCarve {
  char *base;
  int64_t size = 0;
  char *take(int64_t bytes) {
    char *p = base ? base + size : nullptr;
    size += (bytes + 255) & ~(int64_t)255;
    return p;
  }
};

// ------------------------------------------------------------------ expectation semiring (expect_kernels.h)
// workspace: slot-ordered weights (float64 mantissa, exponent) and values (float) of both programs, then (mantissa, R,
// exponent) of every row in both directions, then the per-label sums of c (float64) and p (fixed point, 64-bit)
static int64_t exp_ws_layout(const nfst_batch *lat, char *base, ExpWs *w) {
  const int64_t S = lat->fwd_slots + lat->bwd_slots, TR = lat->total_rows, BV = (int64_t)lat->n_lattices * lat->vocab;
  WsCarve c{base};
  char *wm = c.take(8 * S), *we = c.take(4 * S), *sv = c.take(4 * S), *rm = c.take(16 * TR), *rr = c.take(16 * TR), *re = c.take(8 * TR);
  char *lc = c.take(8 * BV), *lp = c.take(8 * BV);
  if (w) *w = {(double *)wm, (int *)we, (float *)sv, (double *)rm, (double *)rr, (int *)re, (double *)lc, (unsigned long long *)lp};
  return c.size;
}
static int64_t exp_lds_bytes(const nfst_batch *lat) { return (int64_t)lat->max_rows * 20 + 16; }

int64_t nfst_expectation_ws_bytes(const nfst_batch *lat) {
  const int rc = check_batch(lat);
  if (rc) return rc;
  return exp_ws_layout(lat, nullptr, nullptr);
}

int nfst_expectation(const nfst_batch *lat, const nfst_scores *scores, const float *label_values, int64_t label_values_stride,
                     const float *arc_values, float score_coef, void *ws, int64_t ws_bytes, double *logz64, double *ev64,
                     float *ev32, float *posterior, float *cov, float *label_cov, float *label_post, void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  if (!logz64 || !ev64 || !ws || ((uintptr_t)ws & 15)) return NFST_ERR_ARG;
  if (ws_bytes < exp_ws_layout(lat, nullptr, nullptr)) return NFST_ERR_ARG;
  if (label_values && label_values_stride != 0 && label_values_stride < lat->vocab) return NFST_ERR_ARG;
  if (label_values_stride < 0 || !(score_coef == score_coef)) return NFST_ERR_ARG;
  if (!lat->arc_sd || !lat->arc_l16) return NFST_ERR_ARG;
  // the general tile programs, also when the batch has chunked programs (there is no chunked flavour of this op)
  const int64_t lds = exp_lds_bytes(lat);
  if (lds > kMaxLds) return NFST_ERR_LIMIT;
  ExpWs w;
  exp_ws_layout(lat, (char *)ws, &w);
  const ExpVals x = {*scores, label_values, label_values ? label_values_stride : 0, arc_values, score_coef};
  const hipStream_t st = (hipStream_t)stream;
  const int64_t n_lab = (int64_t)lat->n_lattices * lat->vocab;
  if (label_cov && (rc = hip_status(hipMemsetAsync(w.lc, 0, (size_t)n_lab * 8, st)))) return rc;
  if (label_post && (rc = hip_status(hipMemsetAsync(w.lp, 0, (size_t)n_lab * 8, st)))) return rc;
  if ((rc = launch(k_expect_prep, dim3(lat->n_lattices, 2, kExpParts), dim3(kExpPrepThreads), 0, st, *lat, x, w)) ||
      (rc = launch(k_expect_sweep, dim3(lat->n_lattices, 2), dim3(kExpThreads), lds, st, *lat, w)) ||
      (rc = launch(k_expect_arcs, dim3(lat->n_lattices, kExpParts), dim3(kExpArcThreads), 0, st, *lat, x, w, logz64, ev64, ev32, posterior,
                   cov, label_cov != nullptr, label_post != nullptr)))
    return rc;
  if (label_cov || label_post)
    return launch(k_expect_labels, dim3((unsigned)((n_lab + 255) / 256)), dim3(256), 0, st, w, n_lab, label_cov, label_post);
  return NFST_OK;
}

// ------------------------------------------------------------------ k best paths (kbest_kernels.h)
// workspace: the k-best lists of every row, then the topological order, the level starts and the level counts
static int64_t kb_ws_layout(const nfst_batch *lat, int k, char *base, KbWs *w) {
  const int64_t TR = lat->total_rows, B = lat->n_lattices;
  WsCarve c{base};
  char *li = c.take(8 * TR * k), *od = c.take(4 * TR), *lv = c.take(4 * (TR + B)), *nl = c.take(4 * B);
  if (w) *w = {(uint2 *)li, (int *)od, (int *)lv, (int *)nl};
  return c.size;
}
static int kb_check_k(int32_t k) { return k < 1 ? NFST_ERR_ARG : (k > kKbMaxK ? NFST_ERR_LIMIT : NFST_OK); }

int64_t nfst_kbest_ws_bytes(const nfst_batch *lat, int32_t k) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = kb_check_k(k))) return rc;
  return kb_ws_layout(lat, k, nullptr, nullptr);
}

int nfst_kbest(const nfst_batch *lat, const nfst_scores *scores, int32_t k, void *ws, int64_t ws_bytes, float *best,
               int32_t *paths, int32_t *path_arcs, int32_t *lengths, int32_t *n_paths, int32_t max_len, int32_t pad,
               int32_t *status, void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  if ((rc = kb_check_k(k))) return rc;
  if (!best || !paths || !lengths || !n_paths || !status || max_len <= 0) return NFST_ERR_ARG;
  if (!ws || ((uintptr_t)ws & 15) || ws_bytes < kb_ws_layout(lat, k, nullptr, nullptr)) return NFST_ERR_ARG;
  // a payload holds (arc in lattice, rank) in 32 bits: 2^24 arcs per lattice at most (the batch records its largest
  // lattice's arc count up to a cap; beyond the cap the batch's total decides)
  if (max_lattice_arcs(lat) >= NFST_BATCH_MAX_ARCS_CAP && lat->total_arcs >= ((int64_t)1 << 24)) return NFST_ERR_LIMIT;
  const int64_t lds_lev = (int64_t)lat->max_rows * 12 + 16;
  const int64_t lds_sweep = (int64_t)kKbSweepWaves * 2 * 64 * 8 + ((int64_t)lat->max_rows * 2 + 1) * 4;
  KbWs w;
  kb_ws_layout(lat, k, (char *)ws, &w);
  const hipStream_t st = (hipStream_t)stream;
  if ((rc = launch(k_kbest_levels, dim3(lat->n_lattices), dim3(kKbLevelThreads), lds_lev, st, *lat, w)) ||
      (rc = launch(k_kbest_sweep, dim3(lat->n_lattices), dim3(kKbSweepThreads), lds_sweep, st, *lat, *scores, (int)k, w)))
    return rc;
  return launch(k_kbest_walk, dim3(lat->n_lattices), dim3(64), 0, st, *lat, (int)k, w, best, paths, path_arcs, lengths, n_paths,
                (int)max_len, (int)pad, status);
}

// ------------------------------------------------------------------ beam search (beam_kernels.h)
int32_t nfst_beam_lds_candidates(void) { return kBeamLdsCand; }

int nfst_beam_step(const nfst_batch *lat, const int64_t *state, const int64_t *inp, const float *beam_score, const float *scores,
                   const float *lookahead, int32_t pad, int32_t bos, int32_t eos, int32_t has_to_end, int32_t k, float *score,
                   int32_t *parent, int64_t *symbol, int64_t *next_state, int32_t *n_candidates, int32_t *n_open, void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if (k < 1) return NFST_ERR_ARG;
  if (k > kBeamMaxK) return NFST_ERR_LIMIT;
  if (!state || !inp || !beam_score || !scores || !score || !parent || !symbol || !next_state) return NFST_ERR_ARG;
  if (pad < 0 || pad >= lat->vocab) return NFST_ERR_ARG;
  const int64_t all = (int64_t)k * lat->vocab;  // a slot has at most one arc per label
  const int cap = (int)(all < kBeamLdsCand ? all : kBeamLdsCand);
  const BeamIn in{state, inp, beam_score, scores, lookahead, (int)pad, (int)bos, (int)eos, (int)has_to_end, (int)k};
  const BeamOut out{score, parent, symbol, next_state, n_candidates, n_open};
  return launch(k_beam_step, dim3(lat->n_lattices), dim3(kBeamThreads), (int64_t)cap * 8, (hipStream_t)stream, *lat, in, out, cap);
}

int nfst_beam_backtrack(const int32_t *parent, const int64_t *symbol, const float *score, int32_t n_steps, int32_t n_lattices,
                        int32_t k, int32_t max_len, int32_t pad, int32_t *paths, int32_t *lengths, void *stream) {
  if (k < 1 || n_lattices < 1 || n_steps < 0 || max_len < 1 || n_steps > max_len) return NFST_ERR_ARG;
  if (k > kBeamMaxK) return NFST_ERR_LIMIT;
  if (!score || !paths || !lengths || (n_steps > 0 && (!parent || !symbol))) return NFST_ERR_ARG;
  const int64_t n = (int64_t)n_lattices * k;
  return launch(k_beam_backtrack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, parent, symbol, score,
                (int)n_steps, (int)n_lattices, (int)k, (int)max_len, (int)pad, paths, lengths);
}

// ------------------------------------------------------------------ draws without replacement (swor_kernels.h)
// workspace: the back pointers of every step's slots, then room for the keys of a step that LDS does not hold
static int64_t swor_ws_layout(const nfst_batch *lat, int k, int max_len, char *base, SworWs *w) {
  const int64_t B = lat->n_lattices, all = (int64_t)k * lat->vocab;  // a slot has at most one arc per label
  WsCarve c{base};
  char *bk = c.take(8 * B * max_len * k), *sp = all > kBeamLdsCand ? c.take(8 * B * all) : nullptr;
  if (w) *w = {(int2 *)bk, (uint64_t *)sp};
  return c.size;
}
static int swor_check(int32_t k, int32_t max_len) {
  if (k < 1 || max_len < 1) return NFST_ERR_ARG;
  return k > kSworMaxK ? NFST_ERR_LIMIT : NFST_OK;
}

int64_t nfst_swor_ws_bytes(const nfst_batch *lat, int32_t k, int32_t max_len) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = swor_check(k, max_len))) return rc;
  return swor_ws_layout(lat, k, max_len, nullptr, nullptr);
}

int nfst_swor(const nfst_batch *lat, const nfst_scores *scores, const float *logbeta, const double *logz64, int32_t k, int32_t max_len,
              const float *uniforms, int32_t max_degree, uint64_t seed, int32_t pad, void *ws, int64_t ws_bytes, int32_t *paths,
              int32_t *path_arcs, int32_t *lengths, float *logp, double *gumbel, double *kappa, int32_t *n_paths, int32_t *status,
              void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  if ((rc = swor_check(k, max_len))) return rc;
  if (!logbeta || !logz64 || !paths || !lengths || !logp || !gumbel || !kappa || !n_paths || !status) return NFST_ERR_ARG;
  if (uniforms && max_degree < 1) return NFST_ERR_ARG;
  if (!ws || ((uintptr_t)ws & 15) || ws_bytes < swor_ws_layout(lat, k, max_len, nullptr, nullptr)) return NFST_ERR_ARG;
  SworWs w;
  swor_ws_layout(lat, k, max_len, (char *)ws, &w);
  const int64_t all = (int64_t)k * lat->vocab;
  const int cap = (int)(all < kBeamLdsCand ? all : kBeamLdsCand);
  const SworIn in{logbeta, logz64, uniforms, seed, (int)max_degree, (int)k, (int)max_len, (int)pad};
  const SworOut out{paths, path_arcs, lengths, logp, gumbel, kappa, n_paths, status};
  return launch(k_swor<false>, dim3(lat->n_lattices), dim3(kSworThreads), (int64_t)cap * 8, (hipStream_t)stream, *lat, *scores, in, w, out, cap);
}

// ------------------------------------------------------------------ edit distance between path sets (edit_kernels.h)
int nfst_edit_distance(const int32_t *a, const int32_t *a_len, int32_t ka, int32_t La, const int32_t *b, const int32_t *b_len, int32_t kb,
                       int32_t Lb, int32_t n_sets, int32_t symmetric, int32_t *out, int32_t *status, void *stream) {
  if (n_sets < 0 || ka < 0 || kb < 0 || La < 1 || Lb < 1) return NFST_ERR_ARG;
  if (La > kEditMaxLen || Lb > kEditMaxLen) return NFST_ERR_LIMIT;
  if (symmetric && (b != a || b_len != a_len || kb != ka || Lb != La)) return NFST_ERR_ARG;
  if (!status) return NFST_ERR_ARG;
  const int64_t n_pairs = (int64_t)n_sets * ka * kb;
  if (n_pairs == 0) return NFST_OK;
  if (!a || !a_len || !b || !b_len || !out) return NFST_ERR_ARG;
  const int64_t blocks = (n_pairs + kEditWaves - 1) / kEditWaves;
  if (blocks > INT32_MAX) return NFST_ERR_LIMIT;
  const EditIn in{a, a_len, b, b_len, n_pairs, (int)ka, (int)La, (int)kb, (int)Lb, symmetric ? 1 : 0};
  return launch(k_edit_distance, dim3((unsigned)blocks), dim3(kEditThreads), 0, (hipStream_t)stream, in, out, status);
}

// ------------------------------------------------------------------ edit distance to a whole lattice (lattice_edit_kernels.h)
// workspace: R + 1 cells of 8 bytes for every row of the batch, then the level arrays of k_kbest_levels
static int64_t le_ws_layout(const nfst_batch *lat, int R, char *base, LeWs *w) {
  const int64_t TR = lat->total_rows, B = lat->n_lattices;
  WsCarve c{base};
  char *ce = c.take(8 * TR * ((int64_t)R + 1)), *od = c.take(4 * TR), *lv = c.take(4 * (TR + B)), *nl = c.take(4 * B);
  if (w) *w = {(int2 *)ce, (int *)od, (int *)lv, (int *)nl, R + 1};
  return c.size;
}
static int le_check_R(int32_t R) { return R < 1 ? NFST_ERR_ARG : (R > kEditMaxLen ? NFST_ERR_LIMIT : NFST_OK); }

int64_t nfst_lattice_edit_ws_bytes(const nfst_batch *lat, int32_t R) {
  if (!lat) return NFST_ERR_ARG;
  int rc = le_check_R(R);
  if (rc) return rc;
  if (lat->n_lattices == 0) return 0;
  if ((rc = check_batch(lat))) return rc;
  return le_ws_layout(lat, R, nullptr, nullptr);
}

int nfst_lattice_edit(const nfst_batch *lat, const nfst_scores *scores, const int32_t *ref, const int32_t *ref_len, int32_t R, void *ws,
                      int64_t ws_bytes, int32_t *distance, float *score, int32_t *paths, int32_t *path_arcs, int32_t *align,
                      int32_t *lengths, int32_t *counts, int32_t max_len, int32_t pad, int32_t *status, void *stream) {
  if (!lat || !status || max_len < 1) return NFST_ERR_ARG;
  int rc = le_check_R(R);
  if (rc) return rc;
  if (lat->n_lattices == 0) return NFST_OK;
  if ((rc = check_batch(lat))) return rc;
  if (scores && (rc = check_scores(lat, scores))) return rc;
  if (!ref || !ref_len || !distance || !paths || !lengths) return NFST_ERR_ARG;
  if (!ws || ((uintptr_t)ws & 15) || ws_bytes < le_ws_layout(lat, R, nullptr, nullptr)) return NFST_ERR_ARG;
  const int64_t lds_lev = (int64_t)lat->max_rows * 12 + 16;
  const int64_t lds_sweep = 8 * (int64_t)kLeItems + ((int64_t)lat->max_rows * 2 + 1) * 4;
  LeWs w;
  le_ws_layout(lat, R, (char *)ws, &w);
  const KbWs lw{nullptr, w.order, w.lev, w.n_lev};  // (k_kbest_levels writes the level arrays only)
  const LeIn in{ref, ref_len, (int)R};
  const LeOut out{distance, score, paths, path_arcs, align, lengths, counts, (int)max_len, (int)pad, status};
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid(lat->n_lattices);
  if ((rc = launch(k_kbest_levels, grid, dim3(kKbLevelThreads), lds_lev, st, *lat, lw))) return rc;
  if (scores) {
    if ((rc = launch(k_lattice_edit_sweep<true>, grid, dim3(kLeThreads), lds_sweep, st, *lat, *scores, in, w, status))) return rc;
    return launch(k_lattice_edit_walk<true>, grid, dim3(64), 0, st, *lat, *scores, in, w, out);
  }
  const nfst_scores none{};
  if ((rc = launch(k_lattice_edit_sweep<false>, grid, dim3(kLeThreads), lds_sweep, st, *lat, none, in, w, status))) return rc;
  return launch(k_lattice_edit_walk<false>, grid, dim3(64), 0, st, *lat, none, in, w, out);
}

// ------------------------------------------------------------------ path sets merged by their output strings (string_merge_kernels.h)
// the tape of nfst_merge_paths and nfst_string_logprob: a keep mask, a marker, or (need_one == false) neither
static int tape_check(const uint8_t *keep, int32_t marker, int32_t vocab, bool need_one) {
  if (marker < -1 || (keep && marker >= 0) || (need_one && !keep && marker < 0)) return NFST_ERR_ARG;
  if ((keep || marker >= 0) && (vocab < 1 || marker >= vocab)) return NFST_ERR_ARG;
  return NFST_OK;
}

int nfst_merge_paths(const int32_t *paths, const int32_t *lengths, const double *log_weights, const int32_t *n_paths, int32_t n_sets,
                     int32_t K, int32_t L, const uint8_t *keep, int32_t vocab, int32_t marker, int32_t hash_bits, int32_t pad,
                     int32_t *scratch, int32_t *strings, int32_t *out_lengths, double *out_log_weights, int32_t *n_strings,
                     int32_t *group, int32_t *first, int32_t *status, void *stream) {
  if (n_sets < 0 || K < 0 || L < 1 || hash_bits < 1 || hash_bits > 64 || !status) return NFST_ERR_ARG;
  if (int rc = tape_check(keep, marker, vocab, false)) return rc;
  if (K > kSmMaxK || L > kEditMaxLen) return NFST_ERR_LIMIT;
  if ((int64_t)n_sets * K == 0) return NFST_OK;
  if (!paths || !lengths || !log_weights || !scratch || !strings || !out_lengths || !out_log_weights || !n_strings || !group || !first)
    return NFST_ERR_ARG;
  const SmIn in{paths, lengths, log_weights, n_paths, keep, (int)K, (int)L, (int)vocab, (int)marker, (int)pad,
                hash_bits == 64 ? ~0ull : ((1ull << hash_bits) - 1)};
  const SmOut out{scratch, strings, out_lengths, out_log_weights, n_strings, group, first, status};
  return launch(k_merge_paths, dim3(n_sets), dim3(kSmThreads), 0, (hipStream_t)stream, in, out);
}

// ------------------------------------------------------------------ exact string weights (string_logprob_kernels.h)
// workspace: N + 1 cells of 8 bytes per row, candidate and plane, log Z of every row, then the level arrays of k_kbest_levels
static int64_t sl_ws_layout(const nfst_batch *lat, int M, int N, int planes, char *base, SlWs *w) {
  const int64_t TR = lat->total_rows, B = lat->n_lattices, sm = (int64_t)planes * (N + 1), sr = sm * M;
  WsCarve c{base};
  char *ce = c.take(8 * TR * sr), *zz = c.take(8 * TR), *od = c.take(4 * TR), *lv = c.take(4 * (TR + B)), *nl = c.take(4 * B);
  if (w) *w = {(double *)ce, (double *)zz, (int *)od, (int *)lv, (int *)nl, sm, sr};
  return c.size;
}
static int sl_check_sizes(int32_t M, int32_t N) {
  if (M < 0 || N < 1) return NFST_ERR_ARG;
  return N > kEditMaxLen ? NFST_ERR_LIMIT : NFST_OK;
}

// the launch shape that the sum sweep and the max sweep (string_align_kernels.h) share: the LDS of the level pass and of
// the sweep, and the grid -- the candidates of a lattice are dealt to as many workgroups as fill the device about twice
// (any number gives the same bits)
struct SlPlan {
  int64_t lds_lev, lds_sweep;
  dim3 grid;
};
static SlPlan sl_plan(const nfst_batch *lat, int32_t M) {
  const int64_t want = (2 * (int64_t)cu_count() + lat->n_lattices - 1) / lat->n_lattices;
  const int Y = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(M, want), 65535));
  return {(int64_t)lat->max_rows * 12 + 16, ((int64_t)lat->max_rows * 2 + 1) * 4, dim3(lat->n_lattices, Y)};
}

int64_t nfst_string_logprob_ws_bytes(const nfst_batch *lat, int32_t M, int32_t N, int32_t marker_mode) {
  if (!lat) return NFST_ERR_ARG;
  int rc = sl_check_sizes(M, N);
  if (rc) return rc;
  if (lat->n_lattices == 0) return 0;
  if ((rc = check_batch(lat))) return rc;
  return sl_ws_layout(lat, M, N, marker_mode ? 2 : 1, nullptr, nullptr);
}

int nfst_string_logprob(const nfst_batch *lat, const nfst_scores *scores, const int32_t *strings, const int32_t *lengths, int32_t M,
                        int32_t N, const uint8_t *keep, int32_t marker, void *ws, int64_t ws_bytes, double *log_num, double *logz,
                        int32_t *status, void *stream) {
  if (!lat || !status) return NFST_ERR_ARG;
  int rc = sl_check_sizes(M, N);
  if (rc) return rc;
  if ((rc = tape_check(keep, marker, lat->vocab, true))) return rc;
  if (lat->n_lattices == 0) return NFST_OK;
  if ((rc = check_batch(lat))) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  if (!logz || (M > 0 && (!strings || !lengths || !log_num))) return NFST_ERR_ARG;
  const int planes = marker >= 0 ? 2 : 1;
  if (!ws || ((uintptr_t)ws & 15) || ws_bytes < sl_ws_layout(lat, M, N, planes, nullptr, nullptr)) return NFST_ERR_ARG;
  const SlPlan p = sl_plan(lat, M);
  if (p.lds_lev > kMaxLds || p.lds_sweep > kMaxLds) return NFST_ERR_LIMIT;
  SlWs w;
  sl_ws_layout(lat, M, N, planes, (char *)ws, &w);
  const KbWs lw{nullptr, w.order, w.lev, w.n_lev};  // (k_kbest_levels writes the level arrays only)
  const SlIn in{strings, lengths, (int)M, (int)N, keep, (int)marker};
  const hipStream_t st = (hipStream_t)stream;
  if ((rc = launch(k_kbest_levels, dim3(lat->n_lattices), dim3(kKbLevelThreads), p.lds_lev, st, *lat, lw))) return rc;
  if (marker >= 0) return launch(k_string_logprob<true>, p.grid, dim3(kSlThreads), p.lds_sweep, st, *lat, *scores, in, w, log_num, logz, status);
  return launch(k_string_logprob<false>, p.grid, dim3(kSlThreads), p.lds_sweep, st, *lat, *scores, in, w, log_num, logz, status);
}

// ------------------------------------------------------------------ alignments to given strings (string_align_kernels.h)
// both ops sweep in the workspace of nfst_string_logprob; the walk needs none of its own
int64_t nfst_string_viterbi_ws_bytes(const nfst_batch *lat, int32_t M, int32_t N, int32_t marker_mode) {
  return nfst_string_logprob_ws_bytes(lat, M, N, marker_mode);
}
int64_t nfst_string_sample_ws_bytes(const nfst_batch *lat, int32_t M, int32_t N, int32_t marker_mode) {
  return nfst_string_logprob_ws_bytes(lat, M, N, marker_mode);
}

// the host checks of both entry points, in nfst_string_logprob's order; NFST_OK with *noop set: nothing to launch
static int sa_check(const nfst_batch *lat, const nfst_scores *scores, const int32_t *strings, const int32_t *lengths, int32_t M, int32_t N,
                    const uint8_t *keep, int32_t marker, int32_t K, int32_t m0, int32_t max_len, const void *ws, int64_t ws_bytes,
                    const SaOut &o, bool sample, bool *noop) {
  *noop = true;
  if (!lat || !o.status || K < 1 || m0 < 0 || max_len < 1) return NFST_ERR_ARG;
  int rc = sl_check_sizes(M, N);
  if (rc) return rc;
  if ((rc = tape_check(keep, marker, lat->vocab, true))) return rc;
  if (lat->n_lattices == 0 || M == 0) return NFST_OK;
  if ((rc = check_batch(lat))) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  if (!strings || !lengths || !o.paths || !o.path_arcs || !o.align || !o.lengths || !o.score || (sample && !o.logq)) return NFST_ERR_ARG;
  if (!ws || ((uintptr_t)ws & 15) || ws_bytes < sl_ws_layout(lat, M, N, marker >= 0 ? 2 : 1, nullptr, nullptr)) return NFST_ERR_ARG;
  if ((int64_t)lat->n_lattices * M * K > INT32_MAX || (int64_t)m0 + M > INT32_MAX) return NFST_ERR_LIMIT;
  const SlPlan p = sl_plan(lat, M);
  if (p.lds_lev > kMaxLds || p.lds_sweep > kMaxLds) return NFST_ERR_LIMIT;
  *noop = false;
  return NFST_OK;
}

static int sa_launch_walk(const nfst_batch *lat, const nfst_scores *scores, const SlIn &in, const SlWs &w, const SaWalk &wk, const SaOut &o,
                          bool sample, hipStream_t st) {
  const int64_t walks = (int64_t)lat->n_lattices * in.M * wk.K;
  const dim3 grid((unsigned)((walks + kSaWalkWaves - 1) / kSaWalkWaves)), block(kSaWalkWaves * 64);
  if (sample) {
    if (in.marker >= 0) return launch(k_string_walk<true, true>, grid, block, 0, st, *lat, *scores, in, w, wk, o);
    return launch(k_string_walk<false, true>, grid, block, 0, st, *lat, *scores, in, w, wk, o);
  }
  if (in.marker >= 0) return launch(k_string_walk<true, false>, grid, block, 0, st, *lat, *scores, in, w, wk, o);
  return launch(k_string_walk<false, false>, grid, block, 0, st, *lat, *scores, in, w, wk, o);
}

// k_kbest_levels, the max sweep on the grid of nfst_string_logprob, then one wave per candidate
int nfst_string_viterbi(const nfst_batch *lat, const nfst_scores *scores, const int32_t *strings, const int32_t *lengths, int32_t M,
                        int32_t N, const uint8_t *keep, int32_t marker, int32_t max_len, int32_t pad, void *ws, int64_t ws_bytes,
                        double *score, int32_t *paths, int32_t *path_arcs, int32_t *align, int32_t *out_lengths, int32_t *status,
                        void *stream) {
  const SaOut o{paths, path_arcs, align, out_lengths, score, nullptr, status};
  bool noop;
  int rc = sa_check(lat, scores, strings, lengths, M, N, keep, marker, 1, 0, max_len, ws, ws_bytes, o, false, &noop);
  if (rc || noop) return rc;
  const SlPlan p = sl_plan(lat, M);  // (the grid and the LDS of nfst_string_logprob)
  SlWs w;
  sl_ws_layout(lat, M, N, marker >= 0 ? 2 : 1, (char *)ws, &w);
  const KbWs lw{nullptr, w.order, w.lev, w.n_lev};  // (k_kbest_levels writes the level arrays only)
  const SlIn in{strings, lengths, (int)M, (int)N, keep, (int)marker};
  const hipStream_t st = (hipStream_t)stream;
  if ((rc = launch(k_kbest_levels, dim3(lat->n_lattices), dim3(kKbLevelThreads), p.lds_lev, st, *lat, lw))) return rc;
  rc = marker >= 0 ? launch(k_string_viterbi_sweep<true>, p.grid, dim3(kSlThreads), p.lds_sweep, st, *lat, *scores, in, w)
                   : launch(k_string_viterbi_sweep<false>, p.grid, dim3(kSlThreads), p.lds_sweep, st, *lat, *scores, in, w);
  if (rc) return rc;
  const SaWalk wk{1, 0, nullptr, 0, (int)max_len, (int)pad};
  return sa_launch_walk(lat, scores, in, w, wk, o, false, st);
}

// nfst_string_logprob as it is (the table, log_num and logz have its bits), then one wave per draw
int nfst_string_sample(const nfst_batch *lat, const nfst_scores *scores, const int32_t *strings, const int32_t *lengths, int32_t M,
                       int32_t N, const uint8_t *keep, int32_t marker, int32_t K, int32_t m0, const float *uniforms, uint64_t seed,
                       int32_t max_len, int32_t pad, void *ws, int64_t ws_bytes, double *log_num, double *logz, double *score,
                       double *logq, int32_t *paths, int32_t *path_arcs, int32_t *align, int32_t *out_lengths, int32_t *status,
                       void *stream) {
  const SaOut o{paths, path_arcs, align, out_lengths, score, logq, status};
  bool noop;
  int rc = sa_check(lat, scores, strings, lengths, M, N, keep, marker, K, m0, max_len, ws, ws_bytes, o, true, &noop);
  if (rc || noop) return rc;
  if (!log_num || !logz) return NFST_ERR_ARG;
  if ((rc = nfst_string_logprob(lat, scores, strings, lengths, M, N, keep, marker, ws, ws_bytes, log_num, logz, status, stream))) return rc;
  SlWs w;
  sl_ws_layout(lat, M, N, marker >= 0 ? 2 : 1, (char *)ws, &w);
  const SlIn in{strings, lengths, (int)M, (int)N, keep, (int)marker};
  const SaWalk wk{(int)K, (int)m0, uniforms, seed, (int)max_len, (int)pad};
  return sa_launch_walk(lat, scores, in, w, wk, o, true, (hipStream_t)stream);
}

// ------------------------------------------------------------------ gradients of the string weights (string_logprob_grad_kernels.h)
// workspace: that of nfst_string_logprob, then the prefix table F (as large as G), az of every row, the forward's log_num
// and logz, and the in-arc lists (4 bytes per row and lattice, 8 per arc: the list and its unordered draft)
static int64_t slg_ws_layout(const nfst_batch *lat, int M, int N, int planes, char *base, SlWs *w, SlgWs *g) {
  const int64_t TR = lat->total_rows, TA = lat->total_arcs, B = lat->n_lattices, sr = (int64_t)planes * (N + 1) * M;
  const int64_t fwd = sl_ws_layout(lat, M, N, planes, base, w);
  WsCarve c{base ? base + fwd : nullptr};
  char *fc = c.take(8 * TR * sr), *az = c.take(8 * TR), *ln = c.take(8 * B * (int64_t)M), *lz = c.take(8 * B);
  char *ip = c.take(4 * (TR + B)), *il = c.take(4 * TA), *it = c.take(4 * TA);
  if (g) *g = {(double *)fc, (double *)az, (double *)ln, (double *)lz, (int *)ip, (int *)il, (int *)it};
  return fwd + c.size;
}

int64_t nfst_string_logprob_grad_ws_bytes(const nfst_batch *lat, int32_t M, int32_t N, int32_t marker_mode) {
  if (!lat) return NFST_ERR_ARG;
  int rc = sl_check_sizes(M, N);
  if (rc) return rc;
  if (lat->n_lattices == 0) return 0;
  if ((rc = check_batch(lat))) return rc;
  return slg_ws_layout(lat, M, N, marker_mode ? 2 : 1, nullptr, nullptr, nullptr);
}

int nfst_string_logprob_grad(const nfst_batch *lat, const nfst_scores *scores, const int32_t *strings, const int32_t *lengths, int32_t M,
                             int32_t N, const uint8_t *keep, int32_t marker, const double *g_num, const double *g_z,
                             int32_t accumulate, void *ws, int64_t ws_bytes, double *grad_arc, int32_t *status, void *stream) {
  if (!lat || !status) return NFST_ERR_ARG;
  int rc = sl_check_sizes(M, N);
  if (rc) return rc;
  if ((rc = tape_check(keep, marker, lat->vocab, true))) return rc;
  if (lat->n_lattices == 0) return NFST_OK;
  if ((rc = check_batch(lat))) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  if ((M > 0 && (!strings || !lengths || !g_num)) || (!accumulate && !g_z) || (lat->total_arcs > 0 && !grad_arc)) return NFST_ERR_ARG;
  const int planes = marker >= 0 ? 2 : 1;
  if (!ws || ((uintptr_t)ws & 15) || ws_bytes < slg_ws_layout(lat, M, N, planes, nullptr, nullptr, nullptr)) return NFST_ERR_ARG;
  const int64_t lds_lev = (int64_t)lat->max_rows * 12 + 16;
  const int64_t lds_sweep = ((int64_t)lat->max_rows * 2 + 1) * 4;
  const int64_t lds_index = ((int64_t)lat->max_rows * 3 + 1 + kSlgIndexThreads) * 4;
  if (lds_lev > kMaxLds || lds_sweep > kMaxLds || lds_index > kMaxLds) return NFST_ERR_LIMIT;
  if (lat->total_arcs == 0) return NFST_OK;  // (no arc, no gradient)
  SlWs w;
  SlgWs g;
  slg_ws_layout(lat, M, N, planes, (char *)ws, &w, &g);
  const KbWs lw{nullptr, w.order, w.lev, w.n_lev};  // (k_kbest_levels writes the level arrays only)
  const SlIn in{strings, lengths, (int)M, (int)N, keep, (int)marker};
  const hipStream_t st = (hipStream_t)stream;
  // the grid of nfst_string_logprob for both sweeps (any number of workgroups per lattice gives the same bits)
  const int64_t want = (2 * (int64_t)cu_count() + lat->n_lattices - 1) / lat->n_lattices;
  const int Y = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(M, want), 65535));
  const dim3 lattices(lat->n_lattices), grid(lat->n_lattices, Y);
  // the arc pass: one wave per arc of the largest lattice where the batch records that count, a share of all arcs otherwise
  int64_t per_lat = max_lattice_arcs(lat);
  if (per_lat <= 0 || per_lat >= NFST_BATCH_MAX_ARCS_CAP) per_lat = lat->total_arcs;
  const dim3 arc_grid(lat->n_lattices, (unsigned)std::min<int64_t>((per_lat + kSlgArcWaves - 1) / kSlgArcWaves, 65535));
  if ((rc = launch(k_kbest_levels, lattices, dim3(kKbLevelThreads), lds_lev, st, *lat, lw))) return rc;
  auto run = [&](auto MK) {
    constexpr bool mk = decltype(MK)::value;
    int r = launch(k_string_logprob<mk>, grid, dim3(kSlThreads), lds_sweep, st, *lat, *scores, in, w, g.log_num, g.logz, status);
    if (!r) r = launch(k_string_logprob_index, lattices, dim3(kSlgIndexThreads), lds_index, st, *lat, w, g);
    if (!r) r = launch(k_string_logprob_fwd<mk>, grid, dim3(kSlThreads), lds_sweep, st, *lat, *scores, in, w, g);
    if (!r) r = launch(k_string_logprob_arcs<mk>, arc_grid, dim3(kSlgArcThreads), 0, st, *lat, *scores, in, w, g, g_num, g_z,
                       accumulate ? 1 : 0, grad_arc);
    return r;
  };
  return marker >= 0 ? run(std::true_type{}) : run(std::false_type{});
}

// ------------------------------------------------------------------ prefix weights and next symbols (string_prefix_kernels.h)
// nfst_string_prefix sweeps H in the workspace of nfst_string_logprob.  nfst_string_next's workspace: the prefix table F
// (N + 1 cells of 8 bytes per row, candidate and plane), zn (8 bytes per row and plane), z and az of every row, the level
// arrays, the in-arc lists of k_string_logprob_index and the label lists (4 bytes per row and lattice, 12 per arc, 4
// (vocab + 1) + 8 per lattice)
static int64_t sp_ws_layout(const nfst_batch *lat, int M, int N, int planes, char *base, SlWs *w, SlWs *wz, SlgWs *g, SpWs *p) {
  const int64_t TR = lat->total_rows, TA = lat->total_arcs, B = lat->n_lattices, sm = (int64_t)planes * (N + 1), sr = sm * M;
  WsCarve c{base};
  char *fc = c.take(8 * TR * sr), *zn = c.take(8 * TR * planes), *zz = c.take(8 * TR), *az = c.take(8 * TR);
  char *od = c.take(4 * TR), *lv = c.take(4 * (TR + B)), *nl = c.take(4 * B);
  char *ip = c.take(4 * (TR + B)), *il = c.take(4 * TA), *it = c.take(4 * TA);
  char *lp = c.take(4 * B * ((int64_t)lat->vocab + 1)), *ll = c.take(4 * TA), *z0 = c.take(8 * B);
  if (w) *w = {nullptr, (double *)zz, (int *)od, (int *)lv, (int *)nl, sm, sr};  // (the forward sweep writes g->fcells)
  if (wz) *wz = {(double *)zn, (double *)zz, (int *)od, (int *)lv, (int *)nl, planes, planes};  // M = 1, N = 0
  if (g) *g = {(double *)fc, (double *)az, nullptr, nullptr, (int *)ip, (int *)il, (int *)it};
  if (p) *p = {(double *)zn, (double *)z0, (int *)lp, (int *)ll};
  return c.size;
}

int64_t nfst_string_prefix_ws_bytes(const nfst_batch *lat, int32_t M, int32_t N, int32_t marker_mode) {
  return nfst_string_logprob_ws_bytes(lat, M, N, marker_mode);
}

int nfst_string_prefix(const nfst_batch *lat, const nfst_scores *scores, const int32_t *prefixes, const int32_t *lengths, int32_t M,
                       int32_t N, const uint8_t *keep, int32_t marker, void *ws, int64_t ws_bytes, double *log_prefix, double *logz,
                       int32_t *status, void *stream) {
  if (!lat || !status) return NFST_ERR_ARG;
  int rc = sl_check_sizes(M, N);
  if (rc) return rc;
  if ((rc = tape_check(keep, marker, lat->vocab, true))) return rc;
  if (lat->n_lattices == 0) return NFST_OK;
  if ((rc = check_batch(lat))) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  if (!logz || (M > 0 && (!prefixes || !lengths || !log_prefix))) return NFST_ERR_ARG;
  const int planes = marker >= 0 ? 2 : 1;
  if (!ws || ((uintptr_t)ws & 15) || ws_bytes < sl_ws_layout(lat, M, N, planes, nullptr, nullptr)) return NFST_ERR_ARG;
  const int64_t lds_lev = (int64_t)lat->max_rows * 12 + 16;
  const int64_t lds_sweep = ((int64_t)lat->max_rows * 2 + 1) * 4;
  if (lds_lev > kMaxLds || lds_sweep > kMaxLds) return NFST_ERR_LIMIT;
  if (M == 0) return NFST_OK;
  SlWs w;
  sl_ws_layout(lat, M, N, planes, (char *)ws, &w);
  const KbWs lw{nullptr, w.order, w.lev, w.n_lev};  // (k_kbest_levels writes the level arrays only)
  const SlIn in{prefixes, lengths, (int)M, (int)N, keep, (int)marker};
  const hipStream_t st = (hipStream_t)stream;
  // the grid of nfst_string_logprob (any number of workgroups per lattice gives the same bits)
  const int64_t want = (2 * (int64_t)cu_count() + lat->n_lattices - 1) / lat->n_lattices;
  const int Y = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(M, want), 65535));
  if ((rc = launch(k_kbest_levels, dim3(lat->n_lattices), dim3(kKbLevelThreads), lds_lev, st, *lat, lw))) return rc;
  const dim3 grid(lat->n_lattices, Y);
  if (marker >= 0) return launch(k_string_prefix<true>, grid, dim3(kSlThreads), lds_sweep, st, *lat, *scores, in, w, log_prefix, logz, status);
  return launch(k_string_prefix<false>, grid, dim3(kSlThreads), lds_sweep, st, *lat, *scores, in, w, log_prefix, logz, status);
}

int64_t nfst_string_next_ws_bytes(const nfst_batch *lat, int32_t M, int32_t N, int32_t marker_mode) {
  if (!lat) return NFST_ERR_ARG;
  int rc = sl_check_sizes(M, N);
  if (rc) return rc;
  if (lat->n_lattices == 0) return 0;
  if ((rc = check_batch(lat))) return rc;
  return sp_ws_layout(lat, M, N, marker_mode ? 2 : 1, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int nfst_string_next(const nfst_batch *lat, const nfst_scores *scores, const int32_t *prefixes, const int32_t *lengths, int32_t M,
                     int32_t N, const uint8_t *keep, int32_t marker, void *ws, int64_t ws_bytes, double *next, double *eos,
                     double *log_prefix, double *logz, int32_t *status, void *stream) {
  if (!lat || !status) return NFST_ERR_ARG;
  int rc = sl_check_sizes(M, N);
  if (rc) return rc;
  if ((rc = tape_check(keep, marker, lat->vocab, true))) return rc;
  if (lat->n_lattices == 0) return NFST_OK;
  if ((rc = check_batch(lat))) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  if (!logz || (M > 0 && (!prefixes || !lengths || !next || !eos || !log_prefix))) return NFST_ERR_ARG;
  const int planes = marker >= 0 ? 2 : 1;
  if (!ws || ((uintptr_t)ws & 15) || ws_bytes < sp_ws_layout(lat, M, N, planes, nullptr, nullptr, nullptr, nullptr, nullptr))
    return NFST_ERR_ARG;
  const int64_t lds_lev = (int64_t)lat->max_rows * 12 + 16;
  const int64_t lds_sweep = ((int64_t)lat->max_rows * 2 + 1) * 4;
  const int64_t lds_index = ((int64_t)lat->max_rows * 3 + 1 + kSlgIndexThreads) * 4;
  const int64_t lds_label = ((int64_t)lat->max_rows + lat->vocab + 1 + kSpIndexThreads) * 4;
  if (lds_lev > kMaxLds || lds_sweep > kMaxLds || lds_index > kMaxLds || lds_label > kMaxLds) return NFST_ERR_LIMIT;
  if (M == 0) return NFST_OK;
  SlWs w, wz;
  SlgWs g;
  SpWs p;
  sp_ws_layout(lat, M, N, planes, (char *)ws, &w, &wz, &g, &p);
  const KbWs lw{nullptr, w.order, w.lev, w.n_lev};  // (k_kbest_levels writes the level arrays only)
  const SlIn in{prefixes, lengths, (int)M, (int)N, keep, (int)marker};
  const SlIn empty{nullptr, nullptr, 1, 0, keep, (int)marker};  // the empty prefix once per lattice: zn, z and logz
  const hipStream_t st = (hipStream_t)stream;
  const int64_t want = (2 * (int64_t)cu_count() + lat->n_lattices - 1) / lat->n_lattices;
  const int Y = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(M, want), 65535));
  const dim3 lattices(lat->n_lattices), grid(lat->n_lattices, Y), cands(lat->n_lattices, (unsigned)std::min<int64_t>(M, 65535));
  if ((rc = launch(k_kbest_levels, lattices, dim3(kKbLevelThreads), lds_lev, st, *lat, lw))) return rc;
  auto run = [&](auto MK) {
    constexpr bool mk = decltype(MK)::value;
    int r = launch(k_string_prefix<mk>, lattices, dim3(kSlThreads), lds_sweep, st, *lat, *scores, empty, wz, p.zn_lp, logz, status);
    if (!r) r = launch(k_string_logprob_index, lattices, dim3(kSlgIndexThreads), lds_index, st, *lat, w, g);
    if (!r) r = launch(k_string_label_index, lattices, dim3(kSpIndexThreads), lds_label, st, *lat, w, p);
    if (!r) r = launch(k_string_logprob_fwd<mk>, grid, dim3(kSlThreads), lds_sweep, st, *lat, *scores, in, w, g);
    if (!r) r = launch(k_string_next<mk>, cands, dim3(kSpNextThreads), 0, st, *lat, *scores, in, w, g, p, next, eos, log_prefix, status);
    return r;
  };
  return marker >= 0 ? run(std::true_type{}) : run(std::false_type{});
}

// ------------------------------------------------------------------ prefix states (string_extend_kernels.h)
// The context is nfst_string_next's workspace without a table F (M = 0): zn, z, az, the level arrays, the in-arc lists
// and the label lists.  A state is 8 bytes per row, plane and hypothesis.
static int64_t se_ctx_layout(const nfst_batch *lat, int planes, char *base, SlWs *w, SlWs *wz, SlgWs *g, SpWs *p) {
  return sp_ws_layout(lat, 0, 0, planes, base, w, wz, g, p);
}
static int64_t se_state_bytes(const nfst_batch *lat, int64_t M, int planes) {
  return (8 * planes * M * lat->total_rows + 255) & ~(int64_t)255;
}
// what the three entry points behind nfst_string_prefix_open check alike; *noop: nothing to launch
static int se_check(const nfst_batch *lat, const nfst_scores *scores, const uint8_t *keep, int32_t marker, const void *ctx,
                    int64_t ctx_bytes, const int32_t *status, bool *noop) {
  *noop = false;
  if (!lat || !status) return NFST_ERR_ARG;
  int rc = tape_check(keep, marker, lat->vocab, true);
  if (rc) return rc;
  if (lat->n_lattices == 0) {
    *noop = true;
    return NFST_OK;
  }
  if ((rc = check_batch(lat))) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  if (!ctx || ((uintptr_t)ctx & 15) || ctx_bytes < se_ctx_layout(lat, marker >= 0 ? 2 : 1, nullptr, nullptr, nullptr, nullptr, nullptr))
    return NFST_ERR_ARG;
  return NFST_OK;
}

int64_t nfst_string_prefix_open_ws_bytes(const nfst_batch *lat, int32_t marker_mode) {
  if (!lat) return NFST_ERR_ARG;
  if (lat->n_lattices == 0) return 0;
  if (int rc = check_batch(lat)) return rc;
  return se_ctx_layout(lat, marker_mode ? 2 : 1, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int nfst_string_prefix_open(const nfst_batch *lat, const nfst_scores *scores, const uint8_t *keep, int32_t marker, void *ws,
                            int64_t ws_bytes, double *logz, int32_t *status, void *stream) {
  bool noop;
  int rc = se_check(lat, scores, keep, marker, ws, ws_bytes, status, &noop);
  if (rc || noop) return rc;
  if (!logz) return NFST_ERR_ARG;
  const int64_t lds_lev = (int64_t)lat->max_rows * 12 + 16;
  const int64_t lds_sweep = ((int64_t)lat->max_rows * 2 + 1) * 4;
  const int64_t lds_index = ((int64_t)lat->max_rows * 3 + 1 + kSlgIndexThreads) * 4;
  const int64_t lds_label = ((int64_t)lat->max_rows + lat->vocab + 1 + kSpIndexThreads) * 4;
  if (lds_lev > kMaxLds || lds_sweep > kMaxLds || lds_index > kMaxLds || lds_label > kMaxLds) return NFST_ERR_LIMIT;
  SlWs w, wz;
  SlgWs g;
  SpWs p;
  se_ctx_layout(lat, marker >= 0 ? 2 : 1, (char *)ws, &w, &wz, &g, &p);
  const KbWs lw{nullptr, w.order, w.lev, w.n_lev};  // (k_kbest_levels writes the level arrays only)
  const SlIn none{nullptr, nullptr, 0, 0, keep, (int)marker};   // no candidate: az alone
  const SlIn empty{nullptr, nullptr, 1, 0, keep, (int)marker};  // the empty prefix once per lattice: zn, z and logz
  const hipStream_t st = (hipStream_t)stream;
  const dim3 lattices(lat->n_lattices);
  if ((rc = launch(k_kbest_levels, lattices, dim3(kKbLevelThreads), lds_lev, st, *lat, lw))) return rc;
  auto run = [&](auto MK) {
    constexpr bool mk = decltype(MK)::value;
    int r = launch(k_string_prefix<mk>, lattices, dim3(kSlThreads), lds_sweep, st, *lat, *scores, empty, wz, p.zn_lp, logz, status);
    if (!r) r = launch(k_string_logprob_index, lattices, dim3(kSlgIndexThreads), lds_index, st, *lat, w, g);
    if (!r) r = launch(k_string_logprob_fwd<mk>, lattices, dim3(kSlThreads), lds_sweep, st, *lat, *scores, none, w, g);
    if (!r) r = launch(k_string_label_index, lattices, dim3(kSpIndexThreads), lds_label, st, *lat, w, p);
    return r;
  };
  return marker >= 0 ? run(std::true_type{}) : run(std::false_type{});
}

int64_t nfst_string_prefix_state_bytes(const nfst_batch *lat, int32_t M, int32_t marker_mode) {
  if (!lat || M < 0) return NFST_ERR_ARG;
  if (M > kSeMaxM) return NFST_ERR_LIMIT;
  if (lat->n_lattices == 0) return 0;
  if (int rc = check_batch(lat)) return rc;
  return se_state_bytes(lat, M, marker_mode ? 2 : 1);
}

int nfst_string_prefix_extend(const nfst_batch *lat, const nfst_scores *scores, const uint8_t *keep, int32_t marker, const void *ctx_ws,
                              int64_t ctx_bytes, const double *parent_state, int64_t parent_bytes, int32_t M_in,
                              const int32_t *parent, const int32_t *symbol, double *out_state, int64_t out_bytes, int32_t M_out,
                              int32_t *status, void *stream) {
  if (M_in < 0 || M_out < 0) return NFST_ERR_ARG;
  bool noop;
  int rc = se_check(lat, scores, keep, marker, ctx_ws, ctx_bytes, status, &noop);
  if (rc) return rc;
  if (M_in > kSeMaxM || M_out > kSeMaxM) return NFST_ERR_LIMIT;
  if (noop || M_out == 0) return NFST_OK;
  const int planes = marker >= 0 ? 2 : 1;
  const int64_t need_in = M_in ? se_state_bytes(lat, M_in, planes) : 0, need_out = se_state_bytes(lat, M_out, planes);
  if (!parent || !symbol || !out_state || ((uintptr_t)out_state & 15) || out_bytes < need_out) return NFST_ERR_ARG;
  if (M_in > 0 && (!parent_state || ((uintptr_t)parent_state & 15) || parent_bytes < need_in)) return NFST_ERR_ARG;
  if (M_in > 0 && (const char *)parent_state < (const char *)out_state + need_out && (const char *)out_state < (const char *)parent_state + need_in)
    return NFST_ERR_ARG;  // (the children read their parents' cells while they are written)
  const int64_t lds_sweep = ((int64_t)lat->max_rows * 2 + 1) * 4;
  if (lds_sweep > kMaxLds) return NFST_ERR_LIMIT;
  SlWs w;
  SlgWs g;
  se_ctx_layout(lat, planes, (char *)ctx_ws, &w, nullptr, &g, nullptr);
  const SlIn in{nullptr, nullptr, 0, 0, keep, (int)marker};
  const SeIn x{M_in ? parent_state : nullptr, parent, symbol, out_state, (int)M_in, (int)M_out};
  // one wave per SIMD while a level is a few items; four when the hypotheses multiply them (the bits are the same)
  const dim3 grid(lat->n_lattices, (unsigned)((M_out + 63) / 64)), block(M_out >= 8 ? kSlThreads : 256);
  const hipStream_t st = (hipStream_t)stream;
  if (marker >= 0) return launch(k_string_extend<true>, grid, block, lds_sweep, st, *lat, *scores, in, w, g, x, status);
  return launch(k_string_extend<false>, grid, block, lds_sweep, st, *lat, *scores, in, w, g, x, status);
}

int nfst_string_prefix_state_next(const nfst_batch *lat, const nfst_scores *scores, const uint8_t *keep, int32_t marker,
                                  const void *ctx_ws, int64_t ctx_bytes, const double *state, int64_t state_bytes, int32_t M,
                                  double *next, double *eos, double *log_prefix, int32_t *status, void *stream) {
  if (M < 0) return NFST_ERR_ARG;
  bool noop;
  int rc = se_check(lat, scores, keep, marker, ctx_ws, ctx_bytes, status, &noop);
  if (rc) return rc;
  if (M > kSeMaxM) return NFST_ERR_LIMIT;
  if (noop || M == 0) return NFST_OK;
  const int planes = marker >= 0 ? 2 : 1;
  if (!state || ((uintptr_t)state & 15) || state_bytes < se_state_bytes(lat, M, planes) || !next || !eos || !log_prefix) return NFST_ERR_ARG;
  SlgWs g;
  SpWs p;
  se_ctx_layout(lat, planes, (char *)ctx_ws, nullptr, nullptr, &g, &p);
  const SlIn in{nullptr, nullptr, 0, 0, keep, (int)marker};
  const dim3 grid(lat->n_lattices, (unsigned)M), block(kSpNextThreads);
  const hipStream_t st = (hipStream_t)stream;
  if (marker >= 0) return launch(k_string_state_next<true>, grid, block, 0, st, *lat, *scores, in, g, p, state, (int)M, next, eos, log_prefix);
  return launch(k_string_state_next<false>, grid, block, 0, st, *lat, *scores, in, g, p, state, (int)M, next, eos, log_prefix);
}

// ------------------------------------------------------------------ arc slack and beam masks (slack_kernels.h)
// workspace: the gap of every canonical arc, then beta* and delta of every row (the rows only carry the values from
// launch to launch when the phases run as separate launches)
static int64_t slk_ws_layout(const nfst_batch *lat, char *base, SlkWs *w) {
  WsCarve c{base};
  char *gap = c.take(4 * lat->total_arcs), *vb = c.take(4 * lat->total_rows), *dl = c.take(4 * lat->total_rows);
  if (w) *w = {(float *)gap, (float *)vb, (float *)dl};
  return c.size;
}

int64_t nfst_arc_slack_ws_bytes(const nfst_batch *lat) {
  const int rc = check_batch(lat);
  if (rc) return rc;
  return slk_ws_layout(lat, nullptr, nullptr);
}

int nfst_arc_slack(const nfst_batch *lat, const nfst_scores *scores, const float *beam, void *ws, int64_t ws_bytes, float *best,
                   float *vbeta, float *state_slack, float *slack, uint8_t *keep, int32_t *n_kept, void *stream) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  if (!best || !slack || (beam && (!keep || !n_kept)) || (!beam && (keep || n_kept))) return NFST_ERR_ARG;
  if (!ws || ((uintptr_t)ws & 15) || ws_bytes < slk_ws_layout(lat, nullptr, nullptr)) return NFST_ERR_ARG;
  // the general tile programs, also when the batch has chunked programs (there is no chunked flavour of this op)
  const int64_t lds = ((int64_t)lat->max_rows * 2 + lat->vocab + 2 + 2) * 4;
  if (lds > kMaxLds) return NFST_ERR_LIMIT;
  SlkWs w;
  slk_ws_layout(lat, (char *)ws, &w);
  const SlkOut o = {beam, best, vbeta, state_slack, slack, keep, n_kept};
  const hipStream_t st = (hipStream_t)stream;
#ifdef NFST_SLACK_LAUNCHES  // measurement build: one launch per phase instead of barriers inside one
  for (int ph = kSlkBeta; ph <= kSlkArcs; ph <<= 1)
    if ((rc = launch(k_arc_slack, dim3(lat->n_lattices), dim3(kSlkThreads), lds, st, *lat, *scores, w, ph, o))) return rc;
  return NFST_OK;
#else
  return launch(k_arc_slack, dim3(lat->n_lattices), dim3(kSlkThreads), lds, st, *lat, *scores, w, (int)kSlkAll, o);
#endif
}

// ------------------------------------------------------------------ position-dependent scores (positional_kernels.h)
// workspace: the weights of the per-arc extras; with NFST_POS_WS_POSTERIOR the stored beta rows ((T + 1) rows of
// (float64, int32) per row of the batch), the by-destination order and the per-arc sums; with NFST_POS_WS_SAMPLE the
// stored beta rows alone; with NFST_POS_WS_VITERBI the stored max-plus rows
static int64_t pos_ws_layout(const nfst_batch *lat, int64_t T, int flags, char *base, PosWs *w) {
  const int64_t TR = lat->total_rows, A = lat->total_arcs, B = lat->n_lattices, rows = (T + 1) * TR;
  WsCarve c{base};
  PosWs r = {};
  r.ewm = (double *)c.take(8 * A);
  r.ewe = (int *)c.take(4 * A);
  if (flags & (NFST_POS_WS_POSTERIOR | NFST_POS_WS_SAMPLE)) {
    r.bm = (double *)c.take(8 * rows);
    r.be = (int *)c.take(4 * rows);
  }
  if (flags & NFST_POS_WS_POSTERIOR) {
    r.in_ptr = (int *)c.take(4 * (TR + B));
    r.in_tmp = (int *)c.take(4 * A);
    r.in_rec = (int2 *)c.take(8 * A);
    r.acc = (double *)c.take(8 * A);
  }
  if (flags & NFST_POS_WS_VITERBI) r.vb = (float *)c.take(4 * rows);
  if (w) *w = r;
  return c.size;
}
// what every positional op checks first: the batch, the scores, T and the stride of pos; then its workspace
static int pos_check(const nfst_batch *lat, const nfst_scores *scores, const float *pos, int64_t pos_stride, int32_t T) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = check_scores(lat, scores))) return rc;
  if (T < 1) return NFST_ERR_ARG;
  if (pos && pos_stride != 0 && pos_stride != (int64_t)T * lat->vocab) return NFST_ERR_ARG;
  return NFST_OK;
}
static int pos_check_ws(const void *ws, int64_t ws_bytes, int64_t need) {
  return (!ws || ((uintptr_t)ws & 15) || ws_bytes < need) ? NFST_ERR_ARG : NFST_OK;
}
static int pos_check(const nfst_batch *lat, const nfst_scores *scores, const float *pos, int64_t pos_stride, int32_t T, const void *ws,
                     int64_t ws_bytes, int flags) {
  const int rc = pos_check(lat, scores, pos, pos_stride, T);
  return rc ? rc : pos_check_ws(ws, ws_bytes, pos_ws_layout(lat, T, flags, nullptr, nullptr));
}

// LDS for the staged arc records (4 bytes per row and per arc of the largest lattice) when they fit beside `lds`
// bytes, else 0: the step loops then read the canonical arrays
static int64_t pos_staged_bytes(const nfst_batch *lat, int64_t lds) {
  const int64_t arcs = max_lattice_arcs(lat);
  if (arcs <= 0 || arcs >= NFST_BATCH_MAX_ARCS_CAP) return 0;  // (not recorded, or "unknown, large")
  const int64_t bytes = ((int64_t)lat->max_rows + 1 + arcs) * 4 + 16;
  return lds + bytes <= kMaxLds ? bytes : 0;
}

int64_t nfst_positional_ws_bytes(const nfst_batch *lat, int32_t T, int32_t flags) {
  const int rc = check_batch(lat);
  if (rc) return rc;
  if (T < 1 || (flags & ~(NFST_POS_WS_POSTERIOR | NFST_POS_WS_VITERBI | NFST_POS_WS_SAMPLE))) return NFST_ERR_ARG;
  return pos_ws_layout(lat, T, flags, nullptr, nullptr);
}

// The one place that decides what a launch of a positional sweep takes: the LDS of its kernel (`row` bytes per row of
// the largest lattice, `label` per label, `fixed`) and whether the arc records are staged beside it.  Host only (no
// device is touched): the launchers call it, and so may a caller that wants to know which flavour a batch gets.
static int pos_plan(const nfst_batch *lat, int64_t row, int64_t label, int64_t fixed, int64_t *lds_bytes, int32_t *staged) {
  const int rc = check_batch(lat);
  if (rc) return rc;
  const int64_t lds = lat->max_rows * row + lat->vocab * label + fixed;
  if (lds > kMaxLds) return NFST_ERR_LIMIT;
  const int64_t more = pos_staged_bytes(lat, lds);
  if (lds_bytes) *lds_bytes = lds + more;
  if (staged) *staged = more > 0;
  return NFST_OK;
}
int nfst_positional_plan(const nfst_batch *lat, int32_t viterbi, int64_t *lds_bytes, int32_t *staged) {
  return viterbi ? pos_plan(lat, 8, 4, 16, lds_bytes, staged) : pos_plan(lat, 24, 20, kPosThreads * 4 + 16, lds_bytes, staged);
}

// one launch of k_positional in the flavour nfst_positional_plan chose (mode: kPosModeLogz / Alpha / Rows)
static int pos_launch_sum(const nfst_batch *lat, const nfst_scores *scores, const PosIn &in, const PosWs &w, const PosOut &o, int mode,
                          hipStream_t st) {
  int64_t lds;
  int32_t staged;
  const int rc = nfst_positional_plan(lat, 0, &lds, &staged);
  if (rc) return rc;
  return with_pos_flavour(extras_case(lat, scores), staged, [&](auto EX, auto SG) {
    return launch(k_positional<EX, SG>, dim3(lat->n_lattices), dim3(kPosThreads), lds, st, *lat, in, w, o, mode);
  });
}

int nfst_positional(const nfst_batch *lat, const nfst_scores *scores, const float *pos, int64_t pos_stride, int32_t T, void *ws,
                    int64_t ws_bytes, double *logz64, float *logz32, double *len_logz, float *pos_post, float *arc_post,
                    void *stream) {
  const int need_alpha = len_logz || pos_post || arc_post;
  const int flags = need_alpha ? NFST_POS_WS_POSTERIOR : 0;
  int rc = pos_check(lat, scores, pos, pos_stride, T, ws, ws_bytes, flags);
  if (rc) return rc;
  if (!logz64) return NFST_ERR_ARG;
  PosWs w;
  pos_ws_layout(lat, T, flags, (char *)ws, &w);
  const PosIn in = {*scores, pos, pos ? pos_stride : 0, (int)T};
  const PosOut o = {logz64, logz32, len_logz, pos_post, arc_post};
  return pos_launch_sum(lat, scores, in, w, o, need_alpha ? kPosModeAlpha : kPosModeLogz, (hipStream_t)stream);
}

// the backward pass of nfst_positional alone with every beta row stored (the same kernel, the same bits, no forward
// pass), then one wave per walk over all B * K walks
int nfst_positional_sample(const nfst_batch *lat, const nfst_scores *scores, const float *pos, int64_t pos_stride, int32_t T,
                           int32_t k, const float *uniforms, uint64_t seed, int32_t pad, void *ws, int64_t ws_bytes, double *logz64,
                           float *logz32, int32_t *paths, int32_t *path_arcs, int32_t *lengths, float *logq, void *stream) {
  int rc = pos_check(lat, scores, pos, pos_stride, T, ws, ws_bytes, NFST_POS_WS_SAMPLE);
  if (rc) return rc;
  if (k < 1 || !logz64 || !paths || !lengths || !logq) return NFST_ERR_ARG;
  const int64_t walks = (int64_t)lat->n_lattices * k;
  if (walks > INT32_MAX) return NFST_ERR_LIMIT;  // (the walk is a 32-bit word of the Philox counter, as in nfst_sample_paths)
  PosWs w;
  pos_ws_layout(lat, T, NFST_POS_WS_SAMPLE, (char *)ws, &w);
  const PosIn in = {*scores, pos, pos ? pos_stride : 0, (int)T};
  const PosOut o = {logz64, logz32, nullptr, nullptr, nullptr};
  const hipStream_t st = (hipStream_t)stream;
  if ((rc = pos_launch_sum(lat, scores, in, w, o, kPosModeRows, st))) return rc;
  const PosWalkOut wo = {logz64, paths, path_arcs, lengths, logq, (int)pad};
  const dim3 grid((unsigned)((walks + kPosWalkWaves - 1) / kPosWalkWaves)), block(kPosWalkWaves * 64);
  if (extras_case(lat, scores)) return launch(k_positional_walk<true>, grid, block, 0, st, *lat, in, w, (int)k, uniforms, seed, wo);
  return launch(k_positional_walk<false>, grid, block, 0, st, *lat, in, w, (int)k, uniforms, seed, wo);
}

// workspace: the NFST_POS_WS_SAMPLE parts of nfst_positional, then the parts of nfst_swor with max_len = T
static int64_t pos_swor_ws_layout(const nfst_batch *lat, int64_t T, int k, char *base, PosWs *w, SworWs *sw) {
  const int64_t first = pos_ws_layout(lat, T, NFST_POS_WS_SAMPLE, base, w);
  return first + swor_ws_layout(lat, k, (int)T, base ? base + first : nullptr, sw);
}

int64_t nfst_positional_swor_ws_bytes(const nfst_batch *lat, int32_t T, int32_t k) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = swor_check(k, T))) return rc;
  return pos_swor_ws_layout(lat, T, k, nullptr, nullptr, nullptr);
}

// the backward pass of nfst_positional alone with every beta row stored, as nfst_positional_sample, then the search of
// nfst_swor in its positional flavour over those rows, one workgroup per lattice
int nfst_positional_swor(const nfst_batch *lat, const nfst_scores *scores, const float *pos, int64_t pos_stride, int32_t T, int32_t k,
                         const float *uniforms, int32_t max_degree, uint64_t seed, int32_t pad, void *ws, int64_t ws_bytes,
                         double *logz64, float *logz32, int32_t *paths, int32_t *path_arcs, int32_t *lengths, float *logp,
                         double *gumbel, double *kappa, int32_t *n_paths, int32_t *status, void *stream) {
  int rc = pos_check(lat, scores, pos, pos_stride, T);
  if (rc) return rc;
  if ((rc = swor_check(k, T))) return rc;
  if (!logz64 || !paths || !lengths || !logp || !gumbel || !kappa || !n_paths || !status) return NFST_ERR_ARG;
  if (uniforms && max_degree < 1) return NFST_ERR_ARG;
  if ((rc = pos_check_ws(ws, ws_bytes, pos_swor_ws_layout(lat, T, k, nullptr, nullptr, nullptr)))) return rc;
  PosWs w;
  SworWs sw;
  pos_swor_ws_layout(lat, T, k, (char *)ws, &w, &sw);
  const PosIn pin = {*scores, pos, pos ? pos_stride : 0, (int)T};
  const PosOut o = {logz64, logz32, nullptr, nullptr, nullptr};
  const hipStream_t st = (hipStream_t)stream;
  if ((rc = pos_launch_sum(lat, scores, pin, w, o, kPosModeRows, st))) return rc;
  const int64_t all = (int64_t)k * lat->vocab;
  const int cap = (int)(all < kBeamLdsCand ? all : kBeamLdsCand);
  const SworPosIn in{{nullptr, logz64, uniforms, seed, (int)max_degree, (int)k, (int)T, (int)pad}, pos, pos ? pos_stride : 0, w.bm, w.be};
  const SworOut out{paths, path_arcs, lengths, logp, gumbel, kappa, n_paths, status};
  return launch(k_swor<true>, dim3(lat->n_lattices), dim3(kSworThreads), (int64_t)cap * 8, st, *lat, *scores, in, sw, out, cap);
}

int nfst_positional_score_paths(const nfst_batch *lat, const nfst_scores *scores, const float *pos, int64_t pos_stride, int32_t T,
                                const int32_t *marks, int32_t k, float *path_score, int32_t *end_state, int32_t *lengths,
                                void *stream) {
  const int rc = pos_check(lat, scores, pos, pos_stride, T);
  if (rc) return rc;
  if (k < 1 || !marks || !path_score || !end_state || !lengths) return NFST_ERR_ARG;
  if (((int64_t)k + 63) / 64 > 65535) return NFST_ERR_LIMIT;  // (the y dimension of the grid)
  const PosIn in = {*scores, pos, pos ? pos_stride : 0, (int)T};
  return launch(k_positional_score, dim3(lat->n_lattices, (k + 63) / 64), dim3(64), 0, (hipStream_t)stream, *lat, in, marks, (int)k,
                path_score, end_state, lengths);
}

int nfst_positional_viterbi(const nfst_batch *lat, const nfst_scores *scores, const float *pos, int64_t pos_stride, int32_t T,
                            void *ws, int64_t ws_bytes, float *best, int32_t *paths, int32_t *path_arcs, int32_t *lengths,
                            int32_t pad, void *stream) {
  int rc = pos_check(lat, scores, pos, pos_stride, T, ws, ws_bytes, NFST_POS_WS_VITERBI);
  if (rc) return rc;
  if (!best || !paths || !lengths) return NFST_ERR_ARG;
  int64_t lds;
  int32_t staged;
  if ((rc = nfst_positional_plan(lat, 1, &lds, &staged))) return rc;
  PosWs w;
  pos_ws_layout(lat, T, NFST_POS_WS_VITERBI, (char *)ws, &w);
  const PosIn in = {*scores, pos, pos ? pos_stride : 0, (int)T};
  const PosVitOut o = {best, paths, path_arcs, lengths, (int)pad};
  return with_pos_flavour(false, staged, [&](auto, auto SG) {
    return launch(k_positional_viterbi<SG>, dim3(lat->n_lattices), dim3(kPosThreads), lds, (hipStream_t)stream, *lat, in, w, o);
  });
}

// ------------------------------------------------------------------ expectations under positional scores (positional_expect_kernels.h)
// workspace: the NFST_POS_WS_POSTERIOR parts of nfst_positional, then R_t(s) beside every stored beta row, the
// position-independent value of every arc and the per-arc sums of c
static int64_t pos_exp_ws_layout(const nfst_batch *lat, int64_t T, char *base, PosWs *w, PosExpWs *xw) {
  const int64_t first = pos_ws_layout(lat, T, NFST_POS_WS_POSTERIOR, base, w);
  WsCarve c{base ? base + first : nullptr};
  char *br = c.take(8 * (T + 1) * lat->total_rows), *av = c.take(8 * lat->total_arcs), *a2 = c.take(8 * lat->total_arcs);
  if (xw) *xw = {(double *)br, (double *)av, (double *)a2};
  return first + c.size;
}

int64_t nfst_positional_expectation_ws_bytes(const nfst_batch *lat, int32_t T) {
  const int rc = check_batch(lat);
  if (rc) return rc;
  if (T < 1) return NFST_ERR_ARG;
  return pos_exp_ws_layout(lat, T, nullptr, nullptr, nullptr);
}

// what a launch of nfst_positional_expectation takes, as nfst_positional_plan (host only; the launcher calls it)
int nfst_positional_expectation_plan(const nfst_batch *lat, int64_t *lds_bytes, int32_t *staged) {
  return pos_plan(lat, 40, 36, kPosThreads * 4 + 16, lds_bytes, staged);
}

int nfst_positional_expectation(const nfst_batch *lat, const nfst_scores *scores, const float *pos, int64_t pos_stride, int32_t T,
                                const float *pos_values, int64_t pos_values_stride, const float *label_values,
                                int64_t label_values_stride, const float *arc_values, float score_coef, void *ws, int64_t ws_bytes,
                                double *logz64, float *logz32, double *ev64, float *ev32, float *pos_post, float *arc_post,
                                float *pos_cov, float *arc_cov, void *stream) {
  int rc = pos_check(lat, scores, pos, pos_stride, T);
  if (rc) return rc;
  if (!logz64 || !ev64) return NFST_ERR_ARG;
  if (pos_values && pos_values_stride != 0 && pos_values_stride != (int64_t)T * lat->vocab) return NFST_ERR_ARG;
  if (label_values && label_values_stride != 0 && label_values_stride != lat->vocab) return NFST_ERR_ARG;
  if (!(score_coef - score_coef == 0.0f)) return NFST_ERR_ARG;  // NaN or an infinity
  if ((rc = pos_check_ws(ws, ws_bytes, pos_exp_ws_layout(lat, T, nullptr, nullptr, nullptr)))) return rc;
  int64_t lds;
  int32_t staged;
  if ((rc = nfst_positional_expectation_plan(lat, &lds, &staged))) return rc;
  PosWs w;
  PosExpWs xw;
  pos_exp_ws_layout(lat, T, (char *)ws, &w, &xw);
  const PosIn in = {*scores, pos, pos ? pos_stride : 0, (int)T};
  const PosExpVals x = {pos_values, pos_values ? pos_values_stride : 0, label_values, label_values ? label_values_stride : 0,
                        arc_values, (double)score_coef};
  const PosExpOut o = {logz64, logz32, ev64, ev32, pos_post, arc_post, pos_cov, arc_cov};
  return with_pos_flavour(extras_case(lat, scores), staged, [&](auto EX, auto SG) {
    return launch(k_positional_expect<EX, SG>, dim3(lat->n_lattices), dim3(kPosThreads), lds, (hipStream_t)stream, *lat, in, x, w, xw, o);
  });
}

// ------------------------------------------------------------------ k best paths under positional scores (positional_kbest_kernels.h)
// workspace: the k-best lists of every (position, row), 8 (T + 1) total_rows k bytes, then one byte per (position, row):
// reached from state 0 in exactly that many arcs
static int64_t pkb_ws_layout(const nfst_batch *lat, int64_t T, int64_t k, char *base, PkbWs *w) {
  const int64_t pairs = (T + 1) * lat->total_rows;
  WsCarve c{base};
  char *li = c.take(8 * pairs * k), *re = c.take(pairs);
  if (w) *w = {(uint2 *)li, (uint8_t *)re};
  return c.size;
}

int64_t nfst_positional_kbest_ws_bytes(const nfst_batch *lat, int32_t T, int32_t k) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if (T < 1) return NFST_ERR_ARG;
  if ((rc = kb_check_k(k))) return rc;
  return pkb_ws_layout(lat, T, k, nullptr, nullptr);
}

int nfst_positional_kbest(const nfst_batch *lat, const nfst_scores *scores, const float *pos, int64_t pos_stride, int32_t T, int32_t k,
                          void *ws, int64_t ws_bytes, float *best, int32_t *paths, int32_t *path_arcs, int32_t *lengths,
                          int32_t *n_paths, int32_t pad, void *stream) {
  int rc = pos_check(lat, scores, pos, pos_stride, T);
  if (rc) return rc;
  if ((rc = kb_check_k(k))) return rc;
  if (!best || !paths || !lengths || !n_paths) return NFST_ERR_ARG;
  if ((rc = pos_check_ws(ws, ws_bytes, pkb_ws_layout(lat, T, k, nullptr, nullptr)))) return rc;
  // nfst_kbest's payload: (arc in lattice, rank) in 32 bits
  if (max_lattice_arcs(lat) >= NFST_BATCH_MAX_ARCS_CAP && lat->total_arcs >= ((int64_t)1 << 24)) return NFST_ERR_LIMIT;
  const int64_t lds = (int64_t)kKbSweepWaves * 2 * 64 * 8 + ((int64_t)lat->max_rows + 2 + lat->vocab) * 4;
  if (lds > kMaxLds) return NFST_ERR_LIMIT;
  PkbWs w;
  pkb_ws_layout(lat, T, k, (char *)ws, &w);
  const PosIn in = {*scores, pos, pos ? pos_stride : 0, (int)T};
  const hipStream_t st = (hipStream_t)stream;
  if ((rc = launch(k_positional_kbest_sweep, dim3(lat->n_lattices), dim3(kKbSweepThreads), lds, st, *lat, in, (int)k, w))) return rc;
  return launch(k_positional_kbest_walk, dim3(lat->n_lattices), dim3(64), 0, st, *lat, (int)T, (int)k, w, best, paths, path_arcs, lengths,
                n_paths, (int)pad);
}

// ------------------------------------------------------------------ product with a label automaton (intersect_kernels.h)
// workspace: the level order of k_kbest_levels, then live and the first product row of every lattice state, then the
// pair and the first arc of every product row (NFST_MAX_ROWS per lattice) and the product rows per lattice
static int64_t is_ws_layout(const nfst_batch *lat, char *base, IsWs *w) {
  const int64_t TR = lat->total_rows, B = lat->n_lattices;
  WsCarve c{base};
  char *od = c.take(4 * TR), *lv = c.take(4 * (TR + B)), *nl = c.take(4 * B), *li = c.take(8 * TR), *fi = c.take(4 * TR);
  char *pa = c.take(4 * B * NFST_MAX_ROWS), *ao = c.take(4 * B * NFST_MAX_ROWS), *no = c.take(4 * B);
  if (w) *w = {(int *)od, (int *)lv, (int *)nl, (is_mask *)li, (int *)fi, (int *)pa, (int *)ao, (int *)no};
  return c.size;
}
static int is_check_q(int32_t n_q) { return n_q < 1 ? NFST_ERR_ARG : (n_q > 64 ? NFST_ERR_LIMIT : NFST_OK); }
static int is_check(const nfst_batch *lat, const int8_t *delta, int64_t delta_stride, int32_t n_q, const void *ws, int64_t ws_bytes) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = is_check_q(n_q))) return rc;
  if (!delta || (delta_stride != 0 && delta_stride < (int64_t)lat->vocab * 64)) return NFST_ERR_ARG;
  if (!ws || ((uintptr_t)ws & 15) || ws_bytes < is_ws_layout(lat, nullptr, nullptr)) return NFST_ERR_ARG;
  return NFST_OK;
}

int64_t nfst_intersect_ws_bytes(const nfst_batch *lat, int32_t n_q) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = is_check_q(n_q))) return rc;
  return is_ws_layout(lat, nullptr, nullptr);
}

int nfst_intersect_count(const nfst_batch *lat, const int8_t *delta, int64_t delta_stride, const uint64_t *final_mask,
                         int64_t final_stride, int32_t n_q, void *ws, int64_t ws_bytes, int32_t *counts, int32_t *status,
                         void *stream) {
  int rc = is_check(lat, delta, delta_stride, n_q, ws, ws_bytes);
  if (rc) return rc;
  if (!final_mask || final_stride < 0 || !counts || !status) return NFST_ERR_ARG;
  const int64_t lds_lev = (int64_t)lat->max_rows * 12 + 16, lds = (int64_t)lat->max_rows * 16 + 256;
  if (lds > kMaxLds) return NFST_ERR_LIMIT;  // (never: max_rows <= NFST_MAX_ROWS)
  IsWs w;
  is_ws_layout(lat, (char *)ws, &w);
  const KbWs kw = {nullptr, w.order, w.lev, w.n_lev};
  const IsDfa d = {delta, delta_stride, (const is_mask *)final_mask, final_stride};
  const hipStream_t st = (hipStream_t)stream;
  if ((rc = launch(k_kbest_levels, dim3(lat->n_lattices), dim3(kKbLevelThreads), lds_lev, st, *lat, kw))) return rc;
  return launch(k_intersect_count, dim3(lat->n_lattices), dim3(kIsThreads), lds, st, *lat, d, w, counts, status);
}

int nfst_intersect_write(const nfst_batch *lat, const int8_t *delta, int64_t delta_stride, int32_t n_q, void *ws,
                         int64_t ws_bytes, const int64_t *out_row_off, const int64_t *out_arc_off, int32_t *src, int32_t *label,
                         int32_t *dst, int64_t *arc_map, int32_t *arc_q, int32_t *row_state, int32_t *row_q, void *stream) {
  const int rc = is_check(lat, delta, delta_stride, n_q, ws, ws_bytes);
  if (rc) return rc;
  if (!out_row_off || !out_arc_off || !src || !label || !dst || !arc_map || !arc_q || !row_state || !row_q) return NFST_ERR_ARG;
  IsWs w;
  is_ws_layout(lat, (char *)ws, &w);
  const IsDfa d = {delta, delta_stride, nullptr, 0};
  const IsOut o = {out_row_off, out_arc_off, src, label, dst, arc_map, arc_q, row_state, row_q};
  return launch(k_intersect_write, dim3(lat->n_lattices), dim3(kIsThreads), 0, (hipStream_t)stream, *lat, d, w, o);
}

// ------------------------------------------------------------------ product with a sparse automaton of up to 4096 states (intersect_wide_kernels.h)
// workspace: as is_ws_layout, with fwd and live as W = ceil(max_q / 64) words per row of the batch
static int64_t iw_ws_layout(const nfst_batch *lat, int32_t max_q, char *base, IwWs *w) {
  const int64_t TR = lat->total_rows, B = lat->n_lattices, W = (max_q + 63) / 64;
  WsCarve c{base};
  char *od = c.take(4 * TR), *lv = c.take(4 * (TR + B)), *nl = c.take(4 * B), *fw = c.take(8 * W * TR), *li = c.take(8 * W * TR);
  char *fi = c.take(4 * TR), *pa = c.take(4 * B * NFST_MAX_ROWS), *ao = c.take(4 * B * NFST_MAX_ROWS), *no = c.take(4 * B);
  if (w) *w = {(int *)od, (int *)lv, (int *)nl, (is_mask *)fw, (is_mask *)li, (int *)fi, (int *)pa, (int *)ao, (int *)no, (int)W};
  return c.size;
}
static int iw_check_q(int32_t max_q) { return max_q < 1 ? NFST_ERR_ARG : (max_q > kIwMaxQ ? NFST_ERR_LIMIT : NFST_OK); }
static int iw_check(const nfst_batch *lat, const int32_t *q_off, const int32_t *dflt, const int32_t *exc_off, const int32_t *exc_label,
                    const int32_t *exc_dst, const uint8_t *final, int32_t n_dfa, int32_t max_q, const void *ws, int64_t ws_bytes) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = iw_check_q(max_q))) return rc;
  if (!q_off || !dflt || !exc_off || !exc_label || !exc_dst || !final || (n_dfa != 1 && n_dfa != lat->n_lattices)) return NFST_ERR_ARG;
  if (!ws || ((uintptr_t)ws & 15) || ws_bytes < iw_ws_layout(lat, max_q, nullptr, nullptr)) return NFST_ERR_ARG;
  return NFST_OK;
}

int64_t nfst_intersect_wide_ws_bytes(const nfst_batch *lat, int32_t max_q) {
  int rc = check_batch(lat);
  if (rc) return rc;
  if ((rc = iw_check_q(max_q))) return rc;
  return iw_ws_layout(lat, max_q, nullptr, nullptr);
}

int nfst_intersect_wide_count(const nfst_batch *lat, const int32_t *q_off, const int32_t *dflt, const int32_t *exc_off,
                              const int32_t *exc_label, const int32_t *exc_dst, const uint8_t *final, int32_t n_dfa, int32_t max_q,
                              void *ws, int64_t ws_bytes, int32_t *counts, int32_t *status, void *stream) {
  int rc = iw_check(lat, q_off, dflt, exc_off, exc_label, exc_dst, final, n_dfa, max_q, ws, ws_bytes);
  if (rc) return rc;
  if (!counts || !status) return NFST_ERR_ARG;
  const int64_t lds_lev = (int64_t)lat->max_rows * 12 + 16;
  IwWs w;
  iw_ws_layout(lat, max_q, (char *)ws, &w);
  const KbWs kw = {nullptr, w.order, w.lev, w.n_lev};
  const IwDfa d = {q_off, dflt, exc_off, exc_label, exc_dst, final, n_dfa == 1 ? 0 : 1};
  const hipStream_t st = (hipStream_t)stream;
  if ((rc = launch(k_kbest_levels, dim3(lat->n_lattices), dim3(kKbLevelThreads), lds_lev, st, *lat, kw))) return rc;
  return launch(k_intersect_wide_count, dim3(lat->n_lattices), dim3(kIwThreads), 0, st, *lat, d, w, counts, status);
}

int nfst_intersect_wide_write(const nfst_batch *lat, const int32_t *q_off, const int32_t *dflt, const int32_t *exc_off,
                              const int32_t *exc_label, const int32_t *exc_dst, const uint8_t *final, int32_t n_dfa, int32_t max_q,
                              void *ws, int64_t ws_bytes, const int64_t *out_row_off, const int64_t *out_arc_off, int32_t *src,
                              int32_t *label, int32_t *dst, int64_t *arc_map, int32_t *arc_q, int32_t *row_state, int32_t *row_q,
                              void *stream) {
  const int rc = iw_check(lat, q_off, dflt, exc_off, exc_label, exc_dst, final, n_dfa, max_q, ws, ws_bytes);
  if (rc) return rc;
  if (!out_row_off || !out_arc_off || !src || !label || !dst || !arc_map || !arc_q || !row_state || !row_q) return NFST_ERR_ARG;
  IwWs w;
  iw_ws_layout(lat, max_q, (char *)ws, &w);
  const IwDfa d = {q_off, dflt, exc_off, exc_label, exc_dst, final, n_dfa == 1 ? 0 : 1};
  const IsOut o = {out_row_off, out_arc_off, src, label, dst, arc_map, arc_q, row_state, row_q};
  return launch(k_intersect_wide_write, dim3(lat->n_lattices), dim3(kIwThreads), 0, (hipStream_t)stream, *lat, d, w, o);
}

// shared argument checks and the variant table of the 16-byte streaming kernels: a row lies on a
// quarter wave (up to 128 slots of 16 bytes, 8 per lane) or a half wave, four or two rows side by
// side: the per-row instructions (two reductions, masks) are shared by the rows of a wave, and the
// slots a row wastes are at most 15 / 31.
static int plp_check(const void *scores, const void *marks, int64_t n, int32_t t, int32_t vocab, float temp,
                     float smoothing, int32_t mask_mode) {
  if (!scores || !marks || n <= 0 || t <= 0 || vocab <= 0 || !(temp > 0.0f)) return NFST_ERR_ARG;
  if (!(smoothing >= 0.0f && smoothing < 1.0f)) return NFST_ERR_ARG;  // scorers.py:1514
  if (mask_mode != NFST_MASK_STATICRNN && mask_mode != NFST_MASK_GPT2) return NFST_ERR_ARG;
  if (n > 0x7fffffffll) return NFST_ERR_LIMIT;
  return NFST_OK;
}
static int plp_variant(const void *p0, const void *p1, int32_t vocab) {
  const bool v4 = vocab % 4 == 0 && (((uintptr_t)p0 | (uintptr_t)p1) & 15) == 0 && vocab <= 1024;
  if (!v4) return 0;
  const int f4 = vocab / 4;
  return f4 <= 128 ? (f4 + 15) / 16 : 8 + (f4 + 31) / 32;
}
int nfst_path_logprob(const float *scores, const int64_t *marks, int64_t n, int32_t t, int32_t vocab,
                      int32_t pad, int32_t bos, int32_t eos, int32_t max_length, float temp,
                      int32_t normalize, float smoothing, int32_t mask_mode, float *out, void *stream) {
  int rc = plp_check(scores, marks, n, t, vocab, temp, smoothing, mask_mode);
  if (rc) return rc;
  if (!out) return NFST_ERR_ARG;
  auto go = [&](auto kernel) {
    return launch(kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, scores, marks, (int)t, (int)vocab, (int)pad, (int)bos,
                  (int)eos, (int)max_length, temp, (int)normalize, smoothing, (int)mask_mode, out);
  };
  return with_plp_variant(plp_variant(scores, nullptr, vocab), [&](auto NV, auto RB, auto L) { return go(k_path_logprob_v4<NV, RB, L>); },
                          [&] { return go(k_path_logprob); });
}

int nfst_path_logprob_backward(const float *scores, const int64_t *marks, const float *grad_out, int64_t n, int32_t t,
                               int32_t vocab, int32_t pad, int32_t bos, int32_t eos, int32_t max_length, float temp,
                               int32_t normalize, float smoothing, int32_t mask_mode, float *grad_scores, void *stream) {
  int rc = plp_check(scores, marks, n, t, vocab, temp, smoothing, mask_mode);
  if (rc) return rc;
  if (!grad_out || !grad_scores) return NFST_ERR_ARG;
  auto go = [&](auto kernel) {
    return launch(kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, scores, marks, grad_out, (int)t, (int)vocab, (int)pad,
                  (int)bos, (int)eos, (int)max_length, temp, (int)normalize, smoothing, (int)mask_mode, grad_scores);
  };
  return with_plp_variant(plp_variant(scores, grad_scores, vocab),
                          [&](auto NV, auto RB, auto L) { return go(k_path_logprob_bwd_v4<NV, RB, L>); },
                          [&] { return go(k_path_logprob_bwd); });
}

int nfst_iwae(const float *log_p, const float *log_q, int32_t b, int32_t k, float *log_w,
              float *log_marginal, void *stream) {
  if (!log_p || !log_q || !log_w || !log_marginal || b <= 0 || k <= 0) return NFST_ERR_ARG;
  return launch(k_iwae, dim3((b + 127) / 128), dim3(128), 0, (hipStream_t)stream, log_p, log_q, (int)b, (int)k, log_w, log_marginal);
}

}  // extern "C"

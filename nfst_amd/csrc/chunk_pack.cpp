// Host side of the chunked flavour for deep, narrow lattices (include/nfst_hip.h, "Chunked programs"): puts the states
// of a lattice in topological order per direction, cuts the positions into chunks and writes one entry per arc in the
// order a chunk's lanes walk them.  The kernels are in chunk_kernels.h; the same cuts made on the device, from the device
// packer's workspace, are in chunk_pack_kernels.h (the cost model and the plan search of both: chunk_cost.h).
//
// Reference shape this serves: the SNIPS tagging machines (/root/reference/src/main_snips.py, conf/train/lstm_snips.yaml:2
// max_length 750; decode/decoder.py:77-79 walks them state by state): a few tag states per token position.
#include "../../include/nfst_hip.h"
#include "chunk_cost.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

struct nfst_chunks_host {
  nfst_chunks view{};
  std::vector<int32_t> meta, tab, pos;
  std::vector<uint32_t> stream;
  std::vector<uint16_t> label;
};

namespace {

using nfst_chunk::kCus;
using nfst_chunk::kMaxReach;
using nfst_chunk::lds_need;
using nfst_chunk::pow2_at_least;

struct Prog {
  int C = 0, F = 0, R = 0, npos = 0;
  std::vector<int32_t> tab, pos;
  std::vector<uint32_t> stream;
  double cycles = 0.0;           // cost model of the chunked sweep
};

template <class Fn>
void parallel_for(int n, int n_threads, Fn f) {
  if (n_threads <= 0) n_threads = (int)std::thread::hardware_concurrency();
  n_threads = std::max(1, std::min(n_threads, n));
  if (n_threads == 1) { for (int i = 0; i < n; ++i) f(i); return; }
  std::atomic<int> next(0);
  std::vector<std::thread> th;
  for (int t = 0; t < n_threads; ++t)
    th.emplace_back([&] { for (int i; (i = next.fetch_add(1)) < n;) f(i); });
  for (auto &x : th) x.join();
}

// One direction of one lattice.  level[s]: longest path from the start (alpha) / to the sink (beta); operands of a
// state: the sources of its in-arcs (alpha) / the destinations of its out-arcs (beta), as lists of canonical arcs.
bool cut(int n_rows, const std::vector<int32_t> &level, const std::vector<uint8_t> &reach, const std::vector<int32_t> &ptr,
         const std::vector<int32_t> &list, const int32_t *operand_of_arc, int threads, int64_t lds_bytes, int max_chunks, Prog &out) {
  std::vector<int32_t> order;
  for (int s = 0; s < n_rows; ++s)
    if (reach[s]) order.push_back(s);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return level[a] < level[b]; });
  const int n = (int)order.size();
  if (n < 2) return false;
  std::vector<int32_t> posof(n_rows, -1);
  for (int p = 0; p < n; ++p) posof[order[p]] = p;
  // the longest reach of an arc, and per cut a (a chunk starting at position a) the deepest operand below it
  int W = 0;
  std::vector<int32_t> low(n + 1);
  for (int a = 0; a <= n; ++a) low[a] = a;  // low[a] = smallest operand position of an arc that crosses the cut
  std::vector<int64_t> pre(n + 1, 0);       // entries of positions [1, p)
  for (int p = 1; p < n; ++p) {
    const int s = order[p];
    const int cnt = ptr[s + 1] - ptr[s];
    pre[p + 1] = pre[p] + std::max(cnt, 1);
    for (int j = ptr[s]; j < ptr[s + 1]; ++j) {
      const int q = posof[operand_of_arc[list[j]]];
      if (q < 0 || q >= p) return false;  // (not a topological order: cannot happen for a packed batch)
      W = std::max(W, p - q);
      if (p - q > kMaxReach) return false;
      for (int a = q + 1; a <= p; ++a) low[a] = std::min(low[a], q);
    }
  }
  pre[1] = 0;
  const int R = std::max(4, pow2_at_least(W + 1));
  auto reach_of = [&](int a) { return a - low[a]; };  // frontier of a chunk that starts at a
  int Fb = 1;
  for (int a = 1; a < n; ++a) Fb = std::max(Fb, reach_of(a));
  // the cheapest plan over all frontier limits by the cost model wins (nfst_chunk::plan_cut)
  int best_k = -1;
  double best_cycles = 0.0;
  for (int k = 0; k < 2 * Fb; ++k) {
    int pc, pf;
    double cyc;
    if (!nfst_chunk::plan_cut(nfst_chunk::plan_ft(Fb, k), nfst_chunk::plan_lane_cap(k), n, pre.data(), low.data(), R, threads,
                              lds_bytes, max_chunks, [](int) {}, &pc, &pf, &cyc))
      continue;
    if (best_k < 0 || cyc < best_cycles) { best_k = k; best_cycles = cyc; }
  }
  if (best_k < 0) return false;
  std::vector<int32_t> starts;
  int C, F;
  double cycles;
  nfst_chunk::plan_cut(nfst_chunk::plan_ft(Fb, best_k), nfst_chunk::plan_lane_cap(best_k), n, pre.data(), low.data(), R, threads,
                       lds_bytes, max_chunks, [&](int a) { starts.push_back(a); }, &C, &F, &cycles);
  if (C * F > threads || lds_need(C, F, R) > lds_bytes || F > R) return false;
  out.C = C; out.F = F; out.R = R; out.npos = n;
  out.pos.assign(order.begin(), order.end());
  out.tab.clear(); out.stream.clear();
  for (int c = 0; c < C; ++c) {
    const int a = starts[c], b = c + 1 < C ? starts[c + 1] : n;
    const int64_t begin = (int64_t)out.stream.size();
    for (int p = a; p < b; ++p) {
      const int s = order[p];
      const int cnt = ptr[s + 1] - ptr[s];
      if (cnt == 0) out.stream.push_back(NFST_CHK_LAST | NFST_CHK_ZERO);
      for (int j = 0; j < cnt; ++j) {
        const int arc = list[j + ptr[s]];
        const int q = posof[operand_of_arc[arc]];
        out.stream.push_back((uint32_t)(q & (R - 1)) | (j + 1 == cnt ? NFST_CHK_LAST : 0u) | ((uint32_t)arc << 8));
      }
    }
    // (a chunk's entries are walked eight at a time without a bounds test: padded with zero-weight entries)
    while ((out.stream.size() - begin) % 8) out.stream.push_back(NFST_CHK_ZERO);
    const int64_t count = (int64_t)out.stream.size() - begin;
    out.tab.push_back(a); out.tab.push_back((int32_t)begin); out.tab.push_back((int32_t)count); out.tab.push_back(0);
  }
  out.cycles = cycles;
  return true;
}

// what the layout of a batch's programs needs to know about one of them
struct ProgSize {
  int C = 0, F = 0, R = 0, npos = 0;
  int64_t entries = 0;           // stream entries, chunks padded to multiples of eight
  double cycles = 0.0;
};

// The programs of a batch one behind the other (direction 0 and 1 of lattice 0, then of lattice 1, ...) and the choice of the
// flavour: cmeta [B * 2 * NFST_CHK_META_WORDS] and the sizes of v (pointers untouched).  False = no programs for this batch:
// an offset beyond int32, or -- unless forced -- a chunked sweep the cost model does not find faster than the general one.
bool lay_out(const int32_t *batch_meta, int B, const ProgSize *ps, int threads, bool force, int32_t *cmeta, nfst_chunks &v) {
  const bool roomy = 2 * B <= kCus;
  int64_t t_units = 0, n_tab = 0, n_stream = 0, n_pos = 0, lds_used = 0;
  double cycles_chunked = 0.0, cycles_general = 0.0;
  for (int b = 0; b < B; ++b) {
    const int32_t *m = batch_meta + (size_t)b * NFST_META_WORDS;
    for (int dir = 0; dir < 2; ++dir) {
      const ProgSize &p = ps[2 * b + dir];
      int32_t *cm = cmeta + ((size_t)b * 2 + dir) * NFST_CHK_META_WORDS;
      cm[NFST_CHK_C] = p.C; cm[NFST_CHK_F] = p.F; cm[NFST_CHK_R] = p.R; cm[NFST_CHK_NPOS] = p.npos;
      cm[NFST_CHK_TAB_OFF] = (int32_t)n_tab;
      cm[NFST_CHK_STREAM_OFF] = (int32_t)n_stream;
      cm[NFST_CHK_POS_OFF] = (int32_t)n_pos;
      cm[NFST_CHK_T_OFF] = (int32_t)t_units;
      t_units += ((int64_t)p.npos * p.F + 63) / 64;
      if (t_units > INT32_MAX || n_stream + p.entries > (int64_t)INT32_MAX) return false;
      n_tab += p.C; n_stream += p.entries; n_pos += p.npos;
      lds_used = std::max(lds_used, lds_need(p.C, p.F, p.R));
      cycles_chunked = std::max(cycles_chunked, p.cycles * (roomy ? 1.0 : 2.0 * B / kCus));
    }
    // the general flavour: a chain of tiles (precise flavour beyond 192 tiles), one lattice per CU
    const int tiles = std::max(m[NFST_META_FWD_TILES], m[NFST_META_BWD_TILES]);
    cycles_general = std::max(cycles_general, tiles * (tiles > 192 ? 500.0 : 400.0) * std::max(1.0, (double)B / kCus) + 12000.0);
  }
  if (!force && cycles_chunked > 0.9 * cycles_general) return false;  // (profiles/tune/chunk_auto.py: the choice against measurements)
  v.n_lattices = B; v.threads = threads; v.lds_bytes = (int32_t)((lds_used + 255) & ~(int64_t)255); v.launches = 0;
  v.n_tab = n_tab; v.n_stream = n_stream + 64;  // (slack: a lane of pass 1 reads up to 24 entries ahead)
  v.n_pos = n_pos; v.t_units = t_units;
  return true;
}

}  // namespace

extern "C" int nfst_pack_chunks(const nfst_batch *hb, const nfst_chunk_opts *opts, nfst_chunks_host **out) {
  if (!hb || !out) return NFST_ERR_ARG;
  *out = nullptr;
  if (hb->n_lattices <= 0 || !hb->meta || !hb->arc_src || !hb->arc_dst || !hb->arc_label) return NFST_ERR_ARG;
  nfst_chunk_opts o{};
  if (opts) o = *opts;
  const int B = hb->n_lattices;
  int threads;
  int64_t lds_bytes;
  if (!nfst_chunk::resolve_opts(B, o.threads, o.lds_bytes, &threads, &lds_bytes)) return NFST_ERR_ARG;
  // a quick no: up to ~160 levels the general kernels are done before the fixed costs of this flavour are (the BASELINE shape:
  // 130 .. 150 tiles)
  if (!o.force && hb->max_tiles <= 160) return NFST_OK;
  nfst_chunks_host *h = new (std::nothrow) nfst_chunks_host();
  if (!h) return NFST_ERR_NOMEM;
  h->meta.assign((size_t)B * 2 * NFST_CHK_META_WORDS, 0);
  // per lattice, on host threads: both programs (or "cannot be cut"), then the programs are laid out one behind the other
  struct One { int err = NFST_OK; bool ok = false; Prog p[2]; };
  std::vector<One> ones(B);
  parallel_for(B, o.n_threads, [&](int b) {
    One &one = ones[b];
    const int32_t *m = hb->meta + (size_t)b * NFST_META_WORDS;
    const int n = m[NFST_META_N_ROWS], A = m[NFST_META_N_ARCS];
    const int32_t *src = hb->arc_src + m[NFST_META_ARC_OFF], *dst = hb->arc_dst + m[NFST_META_ARC_OFF];
    if (A >= (1 << 24)) return;
    std::vector<uint8_t> reach(n, 0);
    reach[0] = 1;
    std::vector<int32_t> in_ptr(n + 1, 0), out_ptr(n + 1, 0);
    for (int a = 0; a < A; ++a) {
      if (src[a] < 0 || src[a] >= n || dst[a] < 0 || dst[a] >= n) { one.err = NFST_ERR_INDEX; return; }
      reach[src[a]] = 1; reach[dst[a]] = 1;
      if (src[a] != dst[a]) { in_ptr[dst[a] + 1]++; out_ptr[src[a] + 1]++; }
    }
    for (int s = 0; s < n; ++s) { in_ptr[s + 1] += in_ptr[s]; out_ptr[s + 1] += out_ptr[s]; }
    std::vector<int32_t> in_list(in_ptr[n]), out_list(out_ptr[n]);
    {
      std::vector<int32_t> ip(in_ptr.begin(), in_ptr.end() - 1), op(out_ptr.begin(), out_ptr.end() - 1);
      for (int a = 0; a < A; ++a)
        if (src[a] != dst[a]) { in_list[ip[dst[a]]++] = a; out_list[op[src[a]]++] = a; }
    }
    // longest path from the start / to the sink (Kahn; the packer has already refused cycles)
    std::vector<int32_t> depth(n, 0), height(n, 0), rem(n), order;
    for (int s = 0; s < n; ++s) rem[s] = in_ptr[s + 1] - in_ptr[s];
    order.push_back(0);
    for (size_t i = 0; i < order.size(); ++i) {
      const int s = order[i];
      for (int j = out_ptr[s]; j < out_ptr[s + 1]; ++j) {
        const int d = dst[out_list[j]];
        depth[d] = std::max(depth[d], depth[s] + 1);
        if (--rem[d] == 0) order.push_back(d);
      }
    }
    int n_reach = 0;
    for (int s = 0; s < n; ++s) n_reach += reach[s];
    if ((int)order.size() != n_reach) { one.err = NFST_ERR_CYCLE; return; }
    for (int i = n_reach - 1; i >= 0; --i) {
      const int s = order[i];
      for (int j = out_ptr[s]; j < out_ptr[s + 1]; ++j) height[s] = std::max(height[s], height[dst[out_list[j]]] + 1);
    }
    for (int dir = 0; dir < 2; ++dir) {
      Prog &p = one.p[dir];
      const bool ok = dir == 0 ? cut(n, depth, reach, in_ptr, in_list, src, threads, lds_bytes, o.max_chunks, p)
                               : cut(n, height, reach, out_ptr, out_list, dst, threads, lds_bytes, o.max_chunks, p);
      // position 0 must be the start (alpha) / the sink (beta)
      if (!ok || p.pos[0] != (dir == 0 ? 0 : m[NFST_META_SINK])) return;
    }
    one.ok = true;
  });
  for (int b = 0; b < B; ++b) {
    if (ones[b].err != NFST_OK) { const int err = ones[b].err; delete h; return err; }
    if (!ones[b].ok) { delete h; return NFST_OK; }
  }
  std::vector<ProgSize> ps((size_t)B * 2);
  for (int b = 0; b < B; ++b)
    for (int dir = 0; dir < 2; ++dir) {
      const Prog &p = ones[b].p[dir];
      ps[2 * b + dir] = ProgSize{p.C, p.F, p.R, p.npos, (int64_t)p.stream.size(), p.cycles};
    }
  nfst_chunks &v = h->view;
  if (!lay_out(hb->meta, B, ps.data(), threads, o.force != 0, h->meta.data(), v)) { delete h; return NFST_OK; }
  for (int b = 0; b < B; ++b)
    for (int dir = 0; dir < 2; ++dir) {
      const Prog &p = ones[b].p[dir];
      h->tab.insert(h->tab.end(), p.tab.begin(), p.tab.end());
      h->stream.insert(h->stream.end(), p.stream.begin(), p.stream.end());
      h->pos.insert(h->pos.end(), p.pos.begin(), p.pos.end());
    }
  h->stream.resize(v.n_stream, 0);
  // the label of every entry's arc, beside the entry
  h->label.assign(h->stream.size(), 0);
  for (int b = 0; b < B; ++b) {
    const int32_t *m = hb->meta + (size_t)b * NFST_META_WORDS;
    for (int dir = 0; dir < 2; ++dir) {
      const int32_t *cm = h->meta.data() + ((size_t)b * 2 + dir) * NFST_CHK_META_WORDS;
      const int32_t *tb = h->tab.data() + (size_t)cm[NFST_CHK_TAB_OFF] * 4;
      const int64_t n_e = tb[(cm[NFST_CHK_C] - 1) * 4 + 1] + tb[(cm[NFST_CHK_C] - 1) * 4 + 2];
      for (int64_t k = 0; k < n_e; ++k) {
        const uint32_t e = h->stream[cm[NFST_CHK_STREAM_OFF] + k];
        if (!(e & NFST_CHK_ZERO)) h->label[cm[NFST_CHK_STREAM_OFF] + k] = (uint16_t)hb->arc_label[m[NFST_META_ARC_OFF] + (e >> 8)];
      }
    }
  }
  v.total_rows = hb->total_rows; v.total_arcs = hb->total_arcs;
  v.meta = h->meta.data(); v.tab = h->tab.data(); v.stream = h->stream.data(); v.pos = h->pos.data(); v.label = h->label.data();
  v.ws = nullptr; v.ws_bytes = 0;
  *out = h;
  return NFST_OK;
}

extern "C" int nfst_chunks_view(const nfst_chunks_host *c, nfst_chunks *view) {
  if (!c || !view) return NFST_ERR_ARG;
  *view = c->view;
  return NFST_OK;
}

extern "C" void nfst_chunks_free(nfst_chunks_host *c) { delete c; }

// scratch: the entries with their weights (16 B each), T, the (mantissa, exponent) values of every row per direction,
// Z per lattice, the flags
extern "C" int64_t nfst_chunks_ws_bytes(const nfst_chunks *c) {
  if (!c) return NFST_ERR_ARG;
  return c->n_stream * 16 + c->t_units * 64 * 8 + c->total_rows * 2 * 16 + (int64_t)c->n_lattices * 16 + (int64_t)c->n_lattices * 4 + 1024;
}

// The layout step of the device cutter (chunk_pack_kernels.h): the same routine as nfst_pack_chunks', on the summaries the
// planning pass read back.
extern "C" int nfst_pack_chunks_device_layout(const int32_t *summary, const int32_t *batch_meta, const nfst_batch *header,
                                              const nfst_chunk_opts *opts, int32_t *chunk_meta, nfst_chunks *out, int32_t *cut) {
  if (!summary || !batch_meta || !header || !chunk_meta || !out || !cut || header->n_lattices <= 0) return NFST_ERR_ARG;
  *cut = 0;
  nfst_chunk_opts o{};
  if (opts) o = *opts;
  const int B = header->n_lattices;
  int threads;
  int64_t lds_bytes;
  if (!nfst_chunk::resolve_opts(B, o.threads, o.lds_bytes, &threads, &lds_bytes)) return NFST_ERR_ARG;
  if (!o.force && header->max_tiles <= 160) return NFST_OK;  // (the planning pass launched nothing: nfst_pack_chunks' quick no)
  std::vector<ProgSize> ps((size_t)B * 2);
  for (int i = 0; i < 2 * B; ++i) {
    const int32_t *sm = summary + (size_t)i * NFST_CHK_SUM_WORDS;
    if (sm[NFST_CHK_SUM_OK] != 1) return NFST_OK;  // a program that cannot be cut: no programs for the batch
    ProgSize &p = ps[i];
    p.C = sm[NFST_CHK_SUM_C]; p.F = sm[NFST_CHK_SUM_F]; p.R = sm[NFST_CHK_SUM_R]; p.npos = sm[NFST_CHK_SUM_NPOS];
    p.entries = sm[NFST_CHK_SUM_ENTRIES];
    std::memcpy(&p.cycles, sm + NFST_CHK_SUM_CYCLES, sizeof(double));
  }
  nfst_chunks v{};
  std::memset(chunk_meta, 0, sizeof(int32_t) * (size_t)B * 2 * NFST_CHK_META_WORDS);
  if (!lay_out(batch_meta, B, ps.data(), threads, o.force != 0, chunk_meta, v)) return NFST_OK;
  v.total_rows = header->total_rows; v.total_arcs = header->total_arcs;
  *out = v;
  *cut = 1;
  return NFST_OK;
}

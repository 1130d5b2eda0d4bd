// positional_kbest_kernels.h -- exact k best paths under position-dependent scores and a length budget
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.12.
#pragma once

// The paths, positions and scores of positional_kernels.h with the k-best lists of kbest_kernels.h: for every position
// t in [0, T] and state s a list v(t, s, .) of at most k entries (float score, uint32 payload), payload =
// arc_in_lattice << 6 | rank in the list of (t + 1, dst).  The sink's list is the one entry (0.0f, kKbSinkPay) at every
// t; every other list is empty at t = T; a list shorter than k ends with an entry of score -inf.  A state is reached at
// many path lengths, so there is no level schedule: the states advance one position per step, as in
// k_positional_viterbi, one workgroup per lattice, on the canonical arrays only.
//   k_positional_kbest_sweep  T steps from T - 1 down to 0; per step the row theta[l] + pos[t, l] is staged in LDS and
//                             every state reached at t merges the lists of (t + 1, successors) into its own
//                             (kb_merge_state, one wave per state at a time)
//   k_positional_kbest_walk   k lanes follow (arc, rank) forwards from the list of (0, state 0)
// Only the pairs (t, s) that state 0 reaches in exactly t arcs are swept: no other list is read on the way to (0, state 0).
// A forward pass marks them (one byte per pair), and every step compacts its marked states into LDS, so that the 16
// waves share them evenly.  The workspace is the lists and the marks: lattice b owns the list entries from
// (T + 1) * row_off * k on, list (t, s) begins at (t * n_rows + s) * k (64-bit indices: (T + 1) * total_rows * k passes
// 2^31 on ordinary batches), and the marks from (T + 1) * row_off on, pair (t, s) at t * n_rows + s.
static_assert(kKbSweepThreads == kPosThreads, "pos_fill_table strides by kPosThreads");
struct PkbWs {
  uint2 *lists;    // [(T + 1) * total_rows, k]
  uint8_t *reach;  // [(T + 1) * total_rows]
};

// LDS: two k-entry buffers per wave (16 KiB), the states of the step (4 bytes per row), their two counters and the label
// row of the step (4 bytes per label).
__global__ __launch_bounds__(kKbSweepThreads) void k_positional_kbest_sweep(nfst_batch lat, PosIn in, int k, PkbWs w) {
  extern __shared__ int kb_lds[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Meta m = load_meta(lat.meta, b);
  const int n = m.n_rows, V = lat.vocab, T = in.T;
  uint2 *bufs = (uint2 *)kb_lds;  // [kKbSweepWaves][2][64]
  int *todo = (int *)(bufs + kKbSweepWaves * 2 * 64), *n_todo = todo + lat.max_rows;  // n_todo[2]: steps alternate
  float *tab = (float *)(n_todo + 2);
  const PosMax::Rows row = {tab};
  const int32_t *rp = lat.row_ptr + m.row_off + b;
  const int a_lo = m.arc_off, a_hi = m.arc_off + m.n_arcs;
  const float *theta = in.sc.theta + (size_t)in.sc.theta_stride * b;
  const float *pos_b = in.pos ? in.pos + (size_t)in.pos_stride * b : nullptr;
  const Extra ex = {lat.weighted ? lat.arc_w : nullptr, in.sc.arc_scores};
  const size_t per_pos = (size_t)n * k;
  uint2 *lists = w.lists + (size_t)(T + 1) * m.row_off * k;
  uint8_t *reach = w.reach + (size_t)(T + 1) * m.row_off;
  const uint2 kNone = make_uint2(__float_as_uint(kNegInf), 0u), kSink = make_uint2(__float_as_uint(0.0f), kKbSinkPay);
  uint2 *buf0 = bufs + wv * 128;
  // forwards in time: the states reached by exactly t arcs (several threads may store the same 1)
  for (size_t i = tid; i < (size_t)(T + 1) * n; i += kKbSweepThreads) reach[i] = i == 0;
  if (tid < 2) n_todo[tid] = 0;
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const uint8_t *cur = reach + (size_t)t * n;
    uint8_t *nxt = reach + (size_t)(t + 1) * n;
    for (int s = tid; s < n; s += kKbSweepThreads) {
      if (!cur[s] || s == m.sink) continue;
      const int a0 = max(rp[s], a_lo), a1 = min(rp[s + 1], a_hi);
      for (int a = a0; a < a1; ++a) {
        const int d = lat.arc_dst[a];
        if (d != s) nxt[d] = 1;
      }
    }
    __syncthreads();  // (the marks of position t + 1 are visible to the threads that read them)
  }
  // position T: nothing but the sink has a path of zero arcs (every list of this position: the marks decide who reads)
  for (size_t i = tid; i < per_pos; i += kKbSweepThreads) lists[(size_t)T * per_pos + i] = i == (size_t)m.sink * k ? kSink : kNone;
  if (!pos_b) pos_fill_table<PosMax>(row, theta, nullptr, V);
  for (int t = T - 1; t >= 0; --t) {
    if (pos_b) pos_fill_table<PosMax>(row, theta, pos_b + (size_t)t * V, V);
    int *cnt = n_todo + (t & 1);
    for (int s = tid; s < n; s += kKbSweepThreads)
      if (reach[(size_t)t * n + s]) todo[atomicAdd(cnt, 1)] = s;  // (any order: a list does not depend on who merges it when)
    __syncthreads();  // the label row, the states of this step and the lists of position t + 1 are complete (and visible: as k_kbest_sweep's levels)
    const uint2 *nxt = lists + (size_t)(t + 1) * per_pos;
    uint2 *cur = lists + (size_t)t * per_pos;
    const int n_cur = *cnt;
    if (tid == 0) n_todo[(t + 1) & 1] = 0;  // the next step's counter (last read before the barrier that ended step t + 1)
    for (int i = wv; i < n_cur; i += kKbSweepWaves) {
      const int s = todo[i];
      uint2 *out = cur + (size_t)s * k;
      if (s == m.sink) {
        if (lane < k) out[lane] = lane == 0 ? kSink : kNone;
        continue;
      }
      const int a0 = max(rp[s], a_lo), a1 = min(rp[s + 1], a_hi);
      kb_merge_state(lat, m, ex, [&](int l) { return tab[l]; }, nxt, k, s, a0, max(a1 - a0, 0), buf0, lane, out);
    }
    __syncthreads();  // (the next step overwrites the label row and the states)
  }
}

// Lane j < k follows entry j of the list of (0, state 0) for at most T arcs and writes every element of its outputs.
__global__ __launch_bounds__(64) void k_positional_kbest_walk(nfst_batch lat, int T, int k, PkbWs w, float *best, int32_t *paths,
                                                              int32_t *path_arcs, int32_t *lengths, int32_t *n_paths, int pad) {
  const int b = blockIdx.x, j = threadIdx.x;
  const Meta m = load_meta(lat.meta, b);
  const size_t per_pos = (size_t)m.n_rows * k;
  const uint2 *lists = w.lists + (size_t)(T + 1) * m.row_off * k;
  uint2 e = make_uint2(__float_as_uint(kNegInf), 0u);
  if (j < k) e = lists[j];
  const float sc = __uint_as_float(e.x);
  const bool found = j < k && sc > kNegInf;
  const int np = __popcll(__builtin_amdgcn_ballot_w64(found));
  if (j == 0) n_paths[b] = np;
  if (j >= k) return;
  const size_t out_row = (size_t)b * k + j;
  best[out_row] = found ? sc : kNegInf;
  int32_t *po = paths + out_row * T;
  int32_t *ao = path_arcs ? path_arcs + out_row * T : nullptr;
  int len = 0;
  if (found) {
    uint32_t pay = e.y;
    for (int t = 0; t < T && pay != kKbSinkPay; ++t) {
      if ((pay >> 6) >= (uint32_t)m.n_arcs || (pay & 63u) >= (uint32_t)k) break;  // (never on a valid batch)
      const int a = m.arc_off + (int)(pay >> 6);
      po[len] = lat.arc_label[a];
      if (ao) ao[len] = a;
      ++len;
      pay = lists[(size_t)(t + 1) * per_pos + (size_t)lat.arc_dst[a] * k + (pay & 63u)].y;
    }
  }
  lengths[out_row] = len;
  for (int t = len; t < T; ++t) {
    po[t] = pad;
    if (ao) ao[t] = -1;
  }
}

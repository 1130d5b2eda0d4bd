/*
 * nfst_hip.h -- C ABI of the MI355X (gfx950) lattice engine for nFST.
 *
 * Drop-in boundary for the reference's lattice hot path.
 * The reference (steventan0110/nFST) is pure Python and has no FFI; the entry
 * points below are what a ctypes binding for that path binds, one per Python
 * call site it replaces (file:line into /root/reference/src):
 *
 *   nfst_pack_dense / nfst_pack_arcs   FSAGRUScorer.set_masks + set_k
 *                                      (modules/scorers.py:877-918), table format
 *                                      of get_state_mask_pynini (995-1035) and of
 *                                      the .npz files (preprocess/tr.py:182-190)
 *   nfst_backward                      FSAGRUScorer.compute_beta
 *                                      (scorers.py:692-751, 753-875)
 *   nfst_forward_backward              exact log-Z / alpha / arc posteriors: the
 *                                      quantity Estimators.iwae estimates
 *                                      (modules/estimatros.py:33-44), cf.
 *                                      JointProb.log_marginalize
 *                                      (modules/lightning.py:408-440)
 *   nfst_viterbi                       best_sample of JointProb.forward
 *                                      (lightning.py:474-479)
 *   nfst_sample_paths                  Sampler.sample / stateful_sample
 *                                      (modules/samplers.py:137-335)
 *   nfst_score_paths                   forced scoring (samplers.py:208-218)
 *   nfst_step                          FSAGRUScorer.update_fsa_state
 *                                      (scorers.py:683-690)
 *   nfst_emission_mask                 FSAGRUScorer.mask_out_invalid
 *                                      (scorers.py:1037-1054)
 *   nfst_beta_logits                   beta-logit gather (scorers.py:581-593)
 *   nfst_proposal_step (+ _backward)   one step of Sampler.stateful_sample on the lattice
 *                                      side (samplers.py:243-297; scorers.py:340-366, 630-690)
 *   nfst_backward_neural               compute_beta with Wh != 0 (scorers.py:692-856)
 *   nfst_backward_neural_grad          its gradient (tune_proposal, lightning.py:339-406)
 *   nfst_gather_label_scores           WFSTScorer (scorers.py:1671-1687)
 *   nfst_path_logprob (+ _backward)    StaticRNNScorer.evaluate_seq_with_temp
 *                                      gather (scorers.py:1564-1611) and its gradient
 *                                      (lightning.py:511-516 trains through it),
 *                                      GPT2Wrapper.forward (transformer.py:45-52)
 *   nfst_iwae                          Estimators.iwae (estimatros.py:11-44)
 *   nfst_expectation                   exact E_p[additive path value] and its covariance with
 *                                      every arc: the entropy / KL terms that
 *                                      Estimators.estimate_offset_kl_q_p estimates from
 *                                      samples (estimatros.py:236-285), second derivatives of log Z
 *   nfst_kbest                         the k best paths of every lattice: the n-best list that
 *                                      evaluate/rerank.py reranks (read from an outside system
 *                                      there) and the exact form of JointProb.forward's "best of
 *                                      K samples" (lightning.py:474-479)
 *   nfst_beam_step, nfst_beam_backtrack  lattice-constrained beam search for path-dependent scorers: the
 *                                      deterministic twin of the proposal sampler's step
 *   nfst_swor                          k distinct paths per lattice drawn without replacement from the exact
 *                                      posterior (stochastic beam search): the draws Estimators.iwae and
 *                                      tune_proposal average over, without the copies of the best path
 *   nfst_positional, nfst_positional_viterbi  exact sweeps under scores that depend on the position of an arc on the
 *                                      path ([B, T, V] logits) and under a length budget: what the sampler side only
 *                                      truncates (emission_mask(has_to_end = length > max_length), NFST_ERR_LENGTH)
 *   nfst_positional_sample, nfst_positional_score_paths  exact draws from that distribution (no draw overruns the
 *                                      budget) with their log-probabilities, and forced scores of given marks
 *   nfst_positional_kbest              the k best paths under those scores and that budget: the reranker's n-best
 *                                      list for a tagger's or encoder's per-position logits
 *   nfst_positional_swor               k distinct paths drawn without replacement under those scores and that budget:
 *                                      the weighted path set a sequence-level loss (F1, exact match, edit distance) needs
 *   nfst_edit_distance                 that loss: the edit distance of every path of a set to a gold row, or between the
 *                                      paths of a set (the k x k table of minimum-Bayes-risk selection from an n-best
 *                                      list), in one launch instead of one host-side dynamic program per pair
 *   nfst_lattice_edit                  the distance between a gold row and a whole lattice with the path that attains
 *                                      it: the oracle error rate of a lattice and the closest reachable string
 *   nfst_merge_paths                   the rows of a path set merged by the output string they spell, weights summed:
 *                                      an n-best list of alignments becomes an n-best list of strings
 *   nfst_string_logprob                exact log p(y | x) of candidate strings from the lattice alone: the reranker's
 *                                      score of its hypotheses, without one product lattice per hypothesis
 *   nfst_string_logprob_grad           its exact gradient in every arc's score: maximum likelihood and risk on strings,
 *                                      and the arc posteriors given a string
 *   nfst_string_prefix / _next         the exact weight of all strings that start with a prefix, and of its extensions
 *                                      by every next symbol: prefix beam search with a bound on every completion
 *   nfst_string_viterbi / _sample      the alignments of given strings: the best path that spells y with the arc that
 *                                      emitted every symbol (forced alignment), and exact draws from p(path | x, y)
 *
 * Conventions
 *   - plain C: pointers and sizes only, no C++/torch types.
 *   - "device" pointers are HIP device memory owned by the caller (the Python
 *     host side passes torch tensors' data_ptr()); "host" pointers are ordinary
 *     memory.  The library allocates device memory nowhere; every launch goes to
 *     the hipStream_t passed as `stream` (void*) on the calling thread's current
 *     device.  Its only process state is a mutex-guarded cache, keyed by device,
 *     of the kernels' dynamic-LDS opt-ins and of the CU count: several devices in
 *     one process and launches from several host threads are safe.
 *   - every function returns NFST_OK (0) or a negative error code; the message
 *     is available from nfst_strerror().  Kernels are never launched on invalid
 *     shapes: all operands are validated on the host first.
 *   - state, arc and label indices are int32 and bit-exact with the reference's
 *     int64 tables; floating point is float32 unless stated (log Z also float64).
 */
#ifndef NFST_HIP_H
#define NFST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFST_ABI_VERSION 7

/* error codes */
#define NFST_OK 0
#define NFST_ERR_ARG -1        /* null pointer / bad size */
#define NFST_ERR_INDEX -2      /* state or label index out of range */
#define NFST_ERR_CYCLE -3      /* lattice is not acyclic */
#define NFST_ERR_SINK -4       /* not exactly one final (sink) state */
#define NFST_ERR_DETERMINISM -5/* two arcs with the same (state, label) */
#define NFST_ERR_LIMIT -6      /* lattice exceeds the engine's limits */
#define NFST_ERR_HIP -7        /* HIP runtime error */
#define NFST_ERR_NOMEM -8
#define NFST_ERR_LENGTH -9     /* "ran out of length budget" (samplers.py:299-302) */

/* limits of the LDS-resident kernels */
#define NFST_MAX_ROWS 8192     /* states per lattice incl. sink (alpha+beta live in LDS) */
#define NFST_MAX_VOCAB 32767   /* labels + the null label are packed in 16 bits of an arc record */

/* per-lattice metadata: NFST_META_WORDS int32 each, see DESIGN.md */
#define NFST_META_WORDS 16
#define NFST_META_ROW_OFF 0    /* first row of this lattice in row-indexed arrays */
#define NFST_META_N_ROWS 1     /* rows of this lattice (S+1; padded rows included) */
#define NFST_META_ARC_OFF 2    /* first canonical arc */
#define NFST_META_N_ARCS 3     /* canonical arcs (incl. self loops) */
#define NFST_META_FWD_OFF 4    /* word offset of the alpha (by-destination) tile program */
#define NFST_META_FWD_TILES 5
#define NFST_META_BWD_OFF 6    /* word offset of the beta (by-source) tile program */
#define NFST_META_BWD_TILES 7
#define NFST_META_SINK 8       /* sink state id */
#define NFST_META_N_REACH 9    /* states reachable from 0 */
#define NFST_META_DEPTH 10     /* longest path, in arcs */
#define NFST_META_N_DP 11      /* non-self-loop arcs */
#define NFST_META_FWD_U 12     /* alpha program format: bits [0:8) 1, 2 or 4 arc slots per lane in 32-bit records,
                                  or 8 = four 24-bit records per lane; bit 8 = wide groups (up to 64 lanes) */
#define NFST_META_BWD_U 13
#define NFST_META_FWD_SLOT_OFF 14 /* first slot of this lattice in fwd_perm */
#define NFST_META_BWD_SLOT_OFF 15

/*
 * A packed batch of lattices.  All pointers are host memory when returned by
 * the packer and device memory when handed to a kernel entry point (the host
 * side copies the arrays once; K samples per lattice share them, K is a launch
 * parameter -- scorers.py:887-918 materialises K copies instead).
 *
 * Canonical arrays (user-facing): arcs of the states
 * reachable from state 0 in (state asc, label asc) order; values bit-exact with
 * nonzero(emission) / transition.  The sink's pad self loop is included.
 * Tile programs (engine-private): the level-scheduled sweeps, DESIGN.md section 3.
 *
 * What structure a lattice may have ("Lattice structure"; tests/structure_cases.py holds every
 * statement).  Rows that state 0 does not reach may sit anywhere, below, between and above the reachable ones; the
 * packers drop their arcs, so canonical arc ids are positions in the list of the REACHABLE states' arcs, not in the
 * caller's list.  The sink (NFST_META_SINK) is the one reachable state without an out-arc other than self loops,
 * whatever its row id: every entry point compares against it, none against n_rows - 1.  Self loops may sit at any
 * reachable state, state 0 included; for every path-side entry point (all but the walkers nfst_step,
 * nfst_emission_mask, nfst_beta_logits, nfst_proposal_step and nfst_beam_step) a self loop lies on no path: its
 * posterior, covariance and gradient are exactly 0, its label is not counted, no best path, draw or oracle path takes
 * it, and its slack is its state's.  Row outputs (log alpha, log beta, vbeta, state slack) hold -inf / +inf at rows
 * that state 0 does not reach.
 * A lattice whose state 0 is the sink (one row, or rows and no reachable arc) has exactly one path, the empty one:
 * length 0, no arc, score 0.0f.  Viterbi, k best, the samplers and the draws without replacement return it (n_paths 1,
 * labels all pad, arcs all -1; the perturbed score of the one draw is the root's, +inf, and kappa -inf); log Z is 0
 * within the entry point's tolerance (the sweeps take the logarithm of a (mantissa, exponent) pair), log q and log p
 * of the empty path likewise; the positional sums give log Z_T = 0 exactly and len_logz entry 0 = 0, every other entry
 * -inf; E[V], the entropy and every per-label sum are 0; nfst_lattice_edit gives distance n, counts (0, 0, n), length 0
 * and score 0.0f for a reference of n tokens; nfst_arc_slack gives best 0.0f and keeps nothing, and
 * LatticeBatch.restrict leaves such a member as it is; the product with an automaton is one row without arcs if state
 * 0 of the automaton is final, else empty.  The forced walks (nfst_score_paths, nfst_positional_score_paths) follow
 * marks: on the empty path's marks, all pad, they look for a pad arc at state 0 and, as for any mark without an arc,
 * return -inf and end state 0.  Such members may stand anywhere in a batch, and a batch may consist of them alone
 * (total_arcs = 0); an entry point then still wants non-null pointers for its required per-arc outputs.
 */
/* nfst_batch.reserved0 bit: every tile program of the batch is in the compact format (code 8): the
 * fused sweep kernels apply (set by the packer; LatticeBatch.concat keeps it if all parts have it) */
#define NFST_BATCH_ALL_COMPACT 1
/* nfst_batch.reserved0 bits 8 .. 30: the largest number of canonical arcs of one lattice of the batch (capped: the cap
 * means "unknown, large"); the launchers size LDS-resident per-arc data with it */
#define NFST_BATCH_MAX_ARCS_SHIFT 8
#define NFST_BATCH_MAX_ARCS_CAP 0x7fffff

typedef struct nfst_batch {
  int32_t n_lattices;
  int32_t vocab;
  int32_t max_rows;        /* max over the batch of the LDS rows a lattice needs: n_rows + scratch rows of its tile programs */
  int32_t max_tiles;       /* max tiles of one program over the batch */
  int32_t weighted;        /* arc_w holds the table's float weights */
  int32_t reserved0;       /* NFST_BATCH_ALL_COMPACT | largest arc count of one lattice << NFST_BATCH_MAX_ARCS_SHIFT */
  int64_t total_rows;
  int64_t total_arcs;
  int64_t total_dp_arcs;
  int64_t fwd_words;
  int64_t bwd_words;
  int64_t fwd_slots;
  int64_t bwd_slots;
  const int32_t *meta;       /* [n_lattices * NFST_META_WORDS] */
  const int32_t *row_ptr;    /* [total_rows + n_lattices] absolute arc indices */
  const int32_t *arc_src;    /* [total_arcs] */
  const int32_t *arc_dst;    /* [total_arcs] */
  const int32_t *arc_label;  /* [total_arcs] */
  const float *arc_w;        /* [total_arcs] or NULL */
  const uint32_t *fwd_stream;/* [fwd_words] */
  const uint32_t *bwd_stream;/* [bwd_words] */
  const int32_t *fwd_perm;   /* [fwd_slots] tile slot -> canonical arc, -1 = empty slot */
  const int32_t *bwd_perm;   /* [bwd_slots] */
  const uint32_t *arc_sd;    /* [total_arcs + 8] src | dst << 16: the canonical arcs in 6 B/arc */
  const uint16_t *arc_l16;   /* [total_arcs + 8] label            for the posterior pass        */
  /* ABI 7 */
  const struct nfst_chunks *chunks; /* HOST pointer or NULL: the chunked programs of a batch of deep, narrow lattices
                                       (nfst_pack_chunks) with their device arrays and scratch; nfst_backward and
                                       nfst_forward_backward run the chunked flavour when it is there */
  const int32_t *only;       /* launcher-internal, callers pass NULL: device [n_lattices]; a sweep kernel skips lattice b */
  int32_t only_tag;          /*   unless only[b] == only_tag (the chunked flavour hands lattices whose numbers leave   */
  int32_t reserved2;         /*   its range back to the general kernels this way)                                      */
} nfst_batch;

/*
 * Chunked programs for deep, narrow lattices (SNIPS-shaped tagging machines, main_snips.py / lstm_snips.yaml:2
 * max_length 750: hundreds of levels of a few states each, where a level-by-level sweep is a chain of ~200 ns steps
 * with most of a wave idle).  Per lattice and direction the states are put in topological order ("positions":
 * by longest path from the start for alpha, to the sink for beta) and the positions are cut into C chunks.  A chunk's
 * values depend on at most F positions before it (its frontier; arcs reach at most R - 1 positions back), so
 *   pass 1  every chunk is swept at the same time with F right-hand sides (unit vectors on its frontier), one lane per
 *           (chunk, right-hand side): T[p][f] = total weight of the paths from frontier state f to position p inside the chunk;
 *   pass 2  the frontier values are chained through the chunks (C steps of an F x F product);
 *   pass 3  value[p] = sum_f T[p][f] * frontier[f] for every position, all at once.
 * Depth L becomes L / C + C.  Pass 1 computes in plain float64 (a chunk's products stay within 2^+-480 for any
 * sane scores); passes 2 and 3 in (float64 mantissa, int32 exponent).  A lattice whose numbers leave that range
 * (a weight or a partial sum beyond 2^+-480) is flagged on the device and run by the general kernels in the same call.
 * Results: the same function as the general kernels (<= 1e-9 from the float64 oracle on log Z).
 * (A launch captured into a HIP graph replays with the tag it was captured with: a lattice flagged in one replay stays
 * with the general kernels in the following ones -- same results, their speed.)
 */
#define NFST_CHK_META_WORDS 8
#define NFST_CHK_C 0          /* chunks */
#define NFST_CHK_F 1          /* right-hand sides per chunk (largest frontier) */
#define NFST_CHK_R 2          /* ring slots (power of two > the longest reach of an arc, in positions; >= F) */
#define NFST_CHK_NPOS 3       /* positions = reachable states; position 0 is the start (alpha) / the sink (beta) */
#define NFST_CHK_TAB_OFF 4    /* first chunk of this program in tab (4 int32 per chunk) */
#define NFST_CHK_STREAM_OFF 5 /* first entry of this program in stream */
#define NFST_CHK_POS_OFF 6    /* first position of this program in pos */
#define NFST_CHK_T_OFF 7      /* first row of this program's T matrix, in units of 64 doubles */
/* stream entry: operand ring slot (bits 0..5) | last entry of its state (bit 6) | weight zero (bit 7: the entry
 * of a state without arcs, and the entries that pad a chunk to a multiple of eight) | canonical arc, relative to the lattice (bits 8..31) */
#define NFST_CHK_LAST 0x40u
#define NFST_CHK_ZERO 0x80u

typedef struct nfst_chunks {
  int32_t n_lattices;
  int32_t threads;         /* workgroup size the programs were cut for: C * F <= threads for every program */
  int32_t lds_bytes;       /* dynamic LDS of the sweep kernel */
  int32_t launches;        /* launcher-internal: counts the launches (tags the device flags) */
  int64_t n_tab;           /* chunks over all programs */
  int64_t n_stream;        /* stream entries over all programs */
  int64_t n_pos;           /* positions over all programs */
  int64_t t_units;         /* T rows over all programs, in units of 64 doubles */
  int64_t total_rows;      /* of the batch the programs were cut from */
  int64_t total_arcs;
  const int32_t *meta;     /* [n_lattices * 2 * NFST_CHK_META_WORDS]: direction 0 = alpha, 1 = beta */
  const int32_t *tab;      /* [n_tab * 4]: first position, first entry (relative to the program), entries, 0 */
  const uint32_t *stream;  /* [n_stream] */
  const int32_t *pos;      /* [n_pos] position -> state */
  const uint16_t *label;   /* [n_stream] the label of every entry's arc (saves the sweep kernel a dependent load) */
  void *ws;                /* device scratch of nfst_chunks_ws_bytes() bytes, owned by the caller and zeroed by it once (when
                              `launches` is zero), used by every launch on this batch (one launch at a time per batch) */
  int64_t ws_bytes;
} nfst_chunks;

typedef struct nfst_chunk_opts {
  int32_t threads;         /* 0 = by batch size: 1024 when every program gets a CU to itself, else 512 */
  int32_t lds_bytes;       /* 0 = by batch size: 152 KiB / 64 KiB */
  int32_t force;           /* 1 = cut every batch that can be cut (testing); 0 = only when the cost model of the
                              two flavours says the chunked one is faster */
  int32_t max_chunks;      /* 0 = no limit beside threads / LDS (testing: small values) */
  int32_t n_threads;       /* host threads over lattices (0 = hardware) */
  int32_t reserved;
} nfst_chunk_opts;

typedef struct nfst_chunks_host nfst_chunks_host; /* opaque, owns host arrays */
/* Cut the chunked programs of a packed batch (host arrays, as nfst_packed_view returns them).  *out = NULL (and
 * NFST_OK) when the batch is not one for this flavour: an arc that reaches more than 63 positions back, a frontier
 * too wide for the workgroup, or no gain by the cost model. */
int nfst_pack_chunks(const nfst_batch *host_batch, const nfst_chunk_opts *opts, nfst_chunks_host **out);
int nfst_chunks_view(const nfst_chunks_host *c, nfst_chunks *view); /* host pointers; ws = NULL */
void nfst_chunks_free(nfst_chunks_host *c);
int64_t nfst_chunks_ws_bytes(const nfst_chunks *c);

const char *nfst_strerror(int code);
int nfst_abi_version(void);
/* sizeof the named struct of this header ("nfst_batch", "nfst_scores", "nfst_chunks", "nfst_chunk_opts", "nfst_pack_opts",
 * "nfst_step_extras", "nfst_arcs_device") as the library was compiled, -1 for another name: a binding checks its own
 * declarations against it (the entry points copy whole structs) */
int nfst_sizeof(const char *struct_name);
/* 1 when a HIP device is usable, 0 otherwise (never an error) */
int nfst_device_available(void);

/*
 * Launcher switches (tests and A/B measurements; every switch only selects among kernels that compute the same
 * function).  The environment variables of the same meaning -- NFST_TW, NFST_PRECISE, NFST_CHUNKED, NFST_LDS_RESERVE_KB -- are
 * read once, when the first launcher runs, never on the launch path.  name: "tw", "chunked" (0 / 1), "precise" (0 never,
 * 1 whenever it fits, -1 by program depth: the default), "lds_reserve_kb" (0 .. 96); any other name: NFST_ERR_ARG.  Not
 * thread-safe against concurrent launches.
 */
int nfst_tuning_set(const char *name, int value);

/* ---------------------------------------------------------------- packing (host) */
typedef struct nfst_packed nfst_packed; /* opaque, owns host arrays */

/* pack options; zero-initialise for defaults */
typedef struct nfst_pack_opts {
  int32_t n_threads;       /* host threads over lattices (0 = hardware) */
  int32_t slots_per_lane;  /* arc slots per lane of a tile: 1, 2 or 4 (0 = per lattice and direction, cheapest) */
  int32_t group_mode;      /* largest lane group of a state: 1 = narrow (8 lanes, more tiles for high-degree
                              states), 2 = wide (64 lanes), 0 = per lattice and direction, cheapest */
  int32_t reserved1;       /* 1 = never use the compact (24-bit record) tile format (testing) */
} nfst_pack_opts;

/*
 * Dense tables of the reference (scorers.py:995-1035; collated batches as in
 * util/dataset_reader.py:175-186): emission [B, n_rows, V] as uint8 bool
 * (emission_is_float = 0) or float32 log weight with -inf for "no arc"
 * (emission_is_float = 1); transition [B, n_rows, V] int64.  Rows that cannot be
 * reached from state 0 (collate padding, the machine's old final state) are
 * ignored.  Host pointers.  On success *out owns the packed batch.
 * err_lattice (may be NULL) receives the index of the offending lattice.
 */
int nfst_pack_dense(const void *emission, int emission_is_float, const int64_t *transition,
                    int32_t n_lattices, int32_t n_rows, int32_t vocab,
                    const nfst_pack_opts *opts, nfst_packed **out, int32_t *err_lattice);

/*
 * Arc lists (a CSR/COO sidecar of the same lattices): lattice b owns arcs
 * [arc_off[b], arc_off[b+1]) sorted by (src, label); n_rows[b] rows each.
 * arc_w may be NULL.  Host pointers.
 */
int nfst_pack_arcs(const int32_t *n_rows, const int64_t *arc_off, const int32_t *src,
                   const int32_t *label, const int32_t *dst, const float *arc_w,
                   int32_t n_lattices, int32_t vocab, const nfst_pack_opts *opts,
                   nfst_packed **out, int32_t *err_lattice);

/*
 * Packed batches on the host (sidecar files, DataLoader workers).
 *
 * nfst_validate_batch: everything a kernel turns into an address without looking -- offsets and counts of the meta
 * records, row pointers, the state / label / arc ids of the canonical arrays, of every tile's control words and records
 * and of the slot -> arc maps -- is inside the batch's arrays and inside the LDS rows the launchers size from max_rows
 * and vocab.  Host pointers, O(words of the batch).  A batch read back from a file is checked with this before it is
 * ever handed to a kernel (LatticeBatch.load); err_lattice (may be NULL) receives the offending lattice.
 *
 * nfst_crc32c: CRC-32C of a byte range (the checksum stored per array in sidecar files); chain calls through `seed`
 * (0 for the first).
 *
 * nfst_concat_sizes / nfst_concat_packed: one batch from already packed ones without running the packer again -- the
 * collate step of a loader that packs every example once (util/dataset_reader.py:175-186 pads and stacks dense tables
 * instead).  concat_sizes fills the scalar fields of *total; the caller allocates the arrays (ordinary or page-locked
 * host memory), stores their addresses in *total and calls concat_packed, which writes through those pointers:
 * memcpy + offset fix-ups, n_threads host threads over the parts (0 = hardware).  The parts must agree in vocabulary
 * and in being weighted; the result is bit-identical to packing the lattices as one batch.
 */
int nfst_validate_batch(const nfst_batch *lat, int32_t *err_lattice);
uint32_t nfst_crc32c(const void *data, int64_t n_bytes, uint32_t seed);
int nfst_concat_sizes(const nfst_batch *parts, int32_t n_parts, nfst_batch *total);
int nfst_concat_packed(const nfst_batch *parts, int32_t n_parts, const nfst_batch *out, int32_t n_threads);

/*
 * The packer on the device (SURVEY.md section 2 "K1", section 7 step 4).  The reference's trainer hands set_masks
 * tables that already live on the GPU (modules/lightning.py:417 -> scorers.py:877-885); these entry points pack them
 * there, and pack compact arc lists (12 bytes per arc) uploaded by a loader.  Output: the arrays of an nfst_batch in
 * device memory, BIT-IDENTICAL to nfst_pack_dense / nfst_pack_arcs on the same lattices.  Supported: vocab + 2 <= 2048
 * (compact tiles, four slots per lane), nfst_pack_opts.group_mode; slots_per_lane must be 0 or 4.  A lattice beyond
 * the device packer's limits (more than 16384 reachable states or pieces of one sweep direction) gets NFST_ERR_LIMIT in
 * its status word: pack that batch on the host.
 *
 * Dense tables -> arc lists, two launches around one small read-back:
 *   nfst_dense_to_arcs_count  reach [B, n_rows] bytes, row_cnt [B, n_rows], counts [B] = arcs of the rows reachable
 *                             from state 0 (collate padding rows never become arcs), status [B] (NFST_ERR_INDEX)
 *   (host: arc_off = prefix sums of counts; allocate src / label / dst (/ arc_w) of arc_off[B] entries)
 *   nfst_dense_to_arcs_write  the arcs of lattice b at arc_off[b] in (state, label) order
 * Arc lists -> packed batch, two launches around one small read-back:
 *   nfst_pack_device_plan     meta [B, 16] counts (rows, arcs, tiles, sink, depth, formats), status [B], scratch_rows [B]
 *   nfst_pack_device_layout   (host) offsets into *meta, sizes and flags into *header: allocate the arrays, store their
 *                             device addresses in the header, upload meta (it is the batch's meta array)
 *   nfst_pack_device_emit     writes every array of the batch
 * ws: device workspace of nfst_pack_device_ws_bytes() bytes.  The emitting pass reads what the planning pass of the same
 * batch left there: the same workspace, untouched in between; free afterwards.
 */
typedef struct nfst_arcs_device {
  const int32_t *n_rows;   /* [B] device */
  const int64_t *row_off;  /* [B + 1] device: prefix sums of n_rows */
  const int64_t *arc_off;  /* [B + 1] device */
  const int32_t *src;      /* [total_arcs] device, sorted by (src, label) inside a lattice */
  const int32_t *label;
  const int32_t *dst;
  const float *arc_w;      /* or NULL */
  int64_t total_rows;      /* = row_off[B] */
  int64_t total_arcs;      /* = arc_off[B] */
  int32_t n_lattices;
  int32_t vocab;
} nfst_arcs_device;

int nfst_dense_to_arcs_count(const void *emission, int emission_is_float, const int64_t *transition, int32_t n_lattices,
                             int32_t n_rows, int32_t vocab, uint8_t *reach, int32_t *row_cnt, int32_t *counts,
                             int32_t *status, void *stream);
int nfst_dense_to_arcs_write(const void *emission, int emission_is_float, const int64_t *transition, int32_t n_lattices,
                             int32_t n_rows, int32_t vocab, const uint8_t *reach, const int32_t *row_cnt,
                             const int64_t *arc_off, int32_t *src, int32_t *label, int32_t *dst, float *arc_w, void *stream);
int64_t nfst_pack_device_ws_bytes(int32_t n_lattices, int64_t total_rows, int64_t total_arcs);
/* (host) the sizes at which the packing kernel changes its path: *lds_bytes = dynamic LDS of a workgroup (what does not
 * fit beside the depths and heights lives in global memory), *max_keys = 64-bit sort keys that fit it (pieces of one sweep
 * direction beyond that: NFST_ERR_LIMIT), *threads = threads of a workgroup.  For tests that must reach every path. */
int nfst_pack_device_limits(int64_t *lds_bytes, int32_t *max_keys, int32_t *threads);
int nfst_pack_device_plan(const nfst_arcs_device *arcs, const nfst_pack_opts *opts, void *ws, int64_t ws_bytes, int32_t *meta,
                          int32_t *status, int32_t *scratch_rows, void *stream);
int nfst_pack_device_layout(int32_t *meta, const int32_t *status, const int32_t *scratch_rows, int32_t n_lattices,
                            int32_t vocab, int32_t weighted, nfst_batch *header, int32_t *err_lattice);
int nfst_pack_device_emit(const nfst_arcs_device *arcs, const nfst_pack_opts *opts, void *ws, int64_t ws_bytes,
                          const int32_t *meta, int32_t *status, const nfst_batch *out, void *stream);

/*
 * The same programs cut on the device, for a batch the device packer has just emitted (nfst_pack_device_emit) while its
 * workspace is still untouched: the cutter reads the depths, heights and arc lists the packer left there.  BIT-IDENTICAL to
 * nfst_pack_chunks on the same batch (the decision, the header and every array).  opts as for nfst_pack_chunks (n_threads is
 * ignored).  Two launches around one small read-back, on the packer's stream:
 *   nfst_pack_chunks_device_plan    one workgroup per (lattice, direction): the cheapest plan of every program; summary
 *                                   [B * 2 * NFST_CHK_SUM_WORDS] (device).  *launched = 0 (and nothing is written) for a batch
 *                                   nfst_pack_chunks would decline without looking at it
 *   nfst_pack_chunks_device_layout  (host) summary read back + the batch's meta (host) -> chunk_meta [B * 2 *
 *                                   NFST_CHK_META_WORDS] and the sizes of *out (pointers untouched); *cut = 0: no programs.
 *                                   Allocate the arrays (n_tab * 4, n_stream, n_pos, n_stream), store their device addresses
 *                                   and a device copy of chunk_meta in *out
 *   nfst_pack_chunks_device_emit    writes tab, stream (with its zero slack), pos and label
 * pack_ws: the device packer's workspace of the same batch; ws: nfst_pack_chunks_device_ws_bytes() bytes, from the planning
 * pass to the emitting one.  batch: device arrays (host struct), as nfst_pack_device_emit wrote them.
 */
#define NFST_CHK_SUM_WORDS 8
#define NFST_CHK_SUM_OK 0      /* 1 = the program could be cut */
#define NFST_CHK_SUM_C 1
#define NFST_CHK_SUM_F 2
#define NFST_CHK_SUM_R 3
#define NFST_CHK_SUM_NPOS 4
#define NFST_CHK_SUM_ENTRIES 5 /* stream entries, chunks padded to multiples of eight */
#define NFST_CHK_SUM_CYCLES 6  /* two words: the bits of the plan's modelled cycles (a double) */
int64_t nfst_pack_chunks_device_ws_bytes(int32_t n_lattices, int64_t total_rows, int64_t total_arcs);
int nfst_pack_chunks_device_plan(const nfst_arcs_device *arcs, const void *pack_ws, int64_t pack_ws_bytes, const nfst_batch *batch,
                                 const nfst_chunk_opts *opts, void *ws, int64_t ws_bytes, int32_t *summary, int32_t *launched,
                                 void *stream);
int nfst_pack_chunks_device_layout(const int32_t *summary, const int32_t *batch_meta, const nfst_batch *header,
                                   const nfst_chunk_opts *opts, int32_t *chunk_meta, nfst_chunks *out, int32_t *cut);
int nfst_pack_chunks_device_emit(const nfst_arcs_device *arcs, const void *pack_ws, int64_t pack_ws_bytes, const nfst_batch *batch,
                                 const nfst_chunks *chunks, const void *ws, int64_t ws_bytes, void *stream);

/* view of the arrays owned by a packed batch (host pointers, valid until free) */
int nfst_packed_view(const nfst_packed *p, nfst_batch *view);
void nfst_packed_free(nfst_packed *p);

/* ---------------------------------------------------------------- kernels (device) */

/* bytes of dynamic LDS the sweep kernels need for this batch (informational) */
int64_t nfst_lds_bytes(const nfst_batch *lat);

/*
 * Arc scores.  The log weight of canonical arc a of lattice b is
 *     theta[(theta_stride * b) + label[a]]  (+ arc_w[a] if the batch is weighted)
 *                                          (+ arc_scores[a] if arc_scores != NULL)
 * theta: device float32 [V] (theta_stride = 0, one table for the batch, the
 * WFSTScorer case) or [B, V] (theta_stride = V).  arc_scores: device float32
 * [total_arcs] in canonical order, or NULL.
 */
typedef struct nfst_scores {
  const float *theta;
  int64_t theta_stride;
  const float *arc_scores;
  float *reserved_ws;      /* unused since ABI 5 (was a workspace for slot-ordered extras: the sweeps now gather
                              per-arc extras inside the kernel, on otherwise idle waves); pass NULL */
  int64_t reserved_flag;   /* unused, pass 0 */
} nfst_scores;

/*
 * Backward (beta) sweep: log beta[row] for every row (float32, -inf for rows
 * unreachable from 0), log Z = log beta[start] per lattice.  Any output may be
 * NULL.  beta_me (optional) receives the raw (mantissa, exponent) pairs, 2
 * float32 words per row, consumed by nfst_sample_paths.
 * Replaces FSAGRUScorer.compute_beta (scorers.py:858-875); semantics follow
 * compute_beta_per_sample (692-751) with Wh = 0.
 */
int nfst_backward(const nfst_batch *lat, const nfst_scores *scores, float *logbeta,
                  double *logz64, float *logz32, float *beta_me, void *stream);
/* (lat->chunks != NULL: the chunked flavour, see nfst_chunks) */

/*
 * Full forward-backward: alpha and beta sweeps, log Z and arc posteriors
 * posterior[a] = exp(alpha[src] + score + beta[dst] - log Z) in canonical arc
 * order (= d log Z / d score[a]); grad_theta (optional, [B, V] float32) receives the
 * posteriors summed per label (d log Z / d theta[b, l]).
 * logz_total (optional, 3 doubles, zero-initialised once by the caller): the launch adds every
 * lattice's log Z to logz_total[total_slot] (atomic adds: the summation order is not fixed) and
 * clears logz_total[(total_slot + 1) % 3] for the next launch -- the loss of a training step
 * without a reduction kernel; use total_slot = step % 3.
 * Environment: NFST_LDS_RESERVE_KB=<0..96> (read once per process) makes nfst_backward and
 * nfst_forward_backward leave that much LDS free on every CU when they run one lattice per CU,
 * so that a small kernel of another stream (RCCL's all-reduce of the loss) can run beside them.
 */
int nfst_forward_backward(const nfst_batch *lat, const nfst_scores *scores, float *logalpha,
                          float *logbeta, double *logz64, float *logz32, float *posterior,
                          float *grad_theta, float *beta_me, double *logz_total, int32_t total_slot, void *stream);

/*
 * Expectations of an additive path function (the first-order expectation semiring; DESIGN.md sections 2 and 4.5).
 * A path pi from state 0 to the sink has score S(pi) = sum of the log weights s_a of its arcs (nfst_scores) and
 * probability exp(S(pi) - log Z).  Every arc carries a value
 *     v_a = label_values[label_values_stride * b + label[a]]   (if label_values != NULL; stride 0: one [V] table)
 *         + arc_values[a]                                      (if arc_values != NULL; [total_arcs], canonical order)
 *         + score_coef * s_a
 * (rounded to float32 per arc), and V(pi) = sum of v_a over the path.  Per lattice:
 *     logz64[b] = log Z,  ev64[b] (and ev32[b], optional) = E[V]
 * and, each optional, per canonical arc
 *     posterior[a] = p_a (the arc posterior),  cov[a] = c_a = p_a (E[V | a on pi] - E[V]) = Cov(1_a, V)
 * and per lattice and label ([B, V] float32)
 *     label_cov[b, l] = sum of c_a over the arcs with label l (float64 atomic sums: their order is not fixed),
 *     label_post[b, l] = sum of p_a over them (exact sums of p_a rounded to 2^-44: independent of the order).
 * For values that do not depend on the scores c_a = dE[V]/ds_a = sum_b' d2 log Z / ds_a ds_b' v_b' (a Hessian-vector
 * product of log Z); with score_coef = 1 and no other values, H(p) = log Z - E[V] and dH/ds_a = -c_a.
 * Self loops (the sink's pad loop) and arcs of weight zero have p_a = c_a = 0.  An arc of weight zero (a label or an
 * arc score at -inf) has no value: its label_values / arc_values entries are not read into any output (they may be
 * infinite or NaN) and score_coef * s_a is left out.  A lattice without a path of finite score gets
 *     logz64[b] = -inf,  ev64[b] = ev32[b] = 0,  posterior = cov = 0 on its arcs,  label_cov[b, :] = label_post[b, :] = 0
 * (never a NaN; H = log Z - E[V] is then -inf) and does not disturb the other lattices of the batch.  Everything but
 * label_cov is bit-identical from launch to launch.
 * ws: device workspace of nfst_expectation_ws_bytes(lat) bytes (16-byte aligned), overwritten.  logz64 and ev64 are
 * required.  The sweeps run the general tile programs (also when lat->chunks is set: this op has no chunked flavour)
 * with the path mass as (float64 mantissa, int32 exponent) and E[value | row] in float64 for every program, 20 bytes
 * of LDS per row: a batch whose max_rows exceeds 8191 (20 max_rows + 16 > 160 KiB) returns NFST_ERR_LIMIT.  Bad
 * strides, null required pointers or a short workspace return NFST_ERR_ARG.
 */
int64_t nfst_expectation_ws_bytes(const nfst_batch *lat);
int nfst_expectation(const nfst_batch *lat, const nfst_scores *scores, const float *label_values, int64_t label_values_stride,
                     const float *arc_values, float score_coef, void *ws, int64_t ws_bytes, double *logz64, double *ev64,
                     float *ev32, float *posterior, float *cov, float *label_cov, float *label_post, void *stream);

/*
 * The k best paths of every lattice.  A path runs from state 0 to the sink; self loops (the
 * sink's pad loop) are on no path.  Lattices are deterministic: distinct paths are distinct label sequences.
 * Score: a float32 sum built from the sink backwards with the adds of nfst_viterbi's general kernel: the sink holds
 * the single entry 0.0f, and arc a from state s to d extends entry r of d's list to
 *     c = e_a + (theta[label_a] + v(d, r)),   e_a = 0.0f (+ arc_w[a] if weighted) (+ arc_scores[a] if given).
 * Order: a state's list is the top k of its candidates (a, r) with c > -inf (a over its out-arcs without self loops,
 * r over the entries of d's list), by (c desc, canonical arc asc, r asc): on exactly tied scores the smaller first
 * label wins (arcs of a state are in label order).  Entry 0 is therefore nfst_viterbi's path (score, labels, arcs,
 * length) bit for bit whenever the general Viterbi kernel runs (its tile-wave flavour for all-compact batches adds
 * per-arc extras in another order: v + (theta + e_a); without arc_w and arc_scores both are the same).
 * Outputs (device): best [B, k] float32; paths [B, k, max_len] labels (bos .. eos) padded with `pad`; path_arcs
 * (optional) [B, k, max_len] canonical arc ids padded with -1; lengths [B, k] arcs per path; n_paths [B] =
 * min(k, paths of score > -inf).  Entries j >= n_paths[b] have score -inf, length 0, labels pad and arcs -1.  A path
 * longer than max_len is cut there and sets *status = NFST_ERR_LENGTH (status: device, one word, zeroed by the
 * caller).
 * Reads the canonical arrays only (row_ptr, arc_src, arc_dst, arc_label, arc_w): any batch, compact or not, with or
 * without chunked programs, with the same bits.  ws: device workspace of nfst_kbest_ws_bytes(lat, k) bytes (16-byte
 * aligned, overwritten): total_rows * k * 8 bytes of lists plus 12 bytes per row.  Limits: 1 <= k <= 64 (k < 1:
 * NFST_ERR_ARG, k > 64: NFST_ERR_LIMIT); a back pointer holds (arc in lattice, rank) in 32 bits, so a batch that may
 * hold a lattice of 2^24 arcs or more returns NFST_ERR_LIMIT.  All checks run on the host before any launch.
 */
int64_t nfst_kbest_ws_bytes(const nfst_batch *lat, int32_t k);
int nfst_kbest(const nfst_batch *lat, const nfst_scores *scores, int32_t k, void *ws, int64_t ws_bytes, float *best,
               int32_t *paths, int32_t *path_arcs, int32_t *lengths, int32_t *n_paths, int32_t max_len, int32_t pad,
               int32_t *status, void *stream);

/*
 * One step of lattice-constrained beam search (DESIGN.md sections 2 and 4.9) for N = n_lattices * k slots: slot n
 * belongs to lattice n / k and has rank n % k in its beam, 1 <= k <= 64.  Reads the canonical arrays only (row_ptr,
 * arc_label, arc_dst, arc_w): any batch, compact or not, with or without chunked programs, with the same bits.
 * Inputs (device): state [N] int64, the state after inp was consumed; inp [N] int64, the previous mark; beam_score [N]
 * float32, -inf marks a dead slot; scores [N, vocab] float32, the network's outputs for this step as the caller
 * normalised them; lookahead [total_rows] float32 (optional), row-indexed.
 * A candidate is (j, a): a live slot j (beam_score > -inf, state in range) and a canonical arc a out of its state with
 * label l, legal under the rules of nfst_proposal_step: l != bos; l == pad exactly when inp[j] is eos or pad; with
 * has_to_end a slot that has not ended takes eos only.  All arithmetic is float32, in this order:
 *     c = beam_score[j] + (x + w_a),   x = scores[j, l] (0.0f for l == pad: the pad entry is never read),
 *                                      w_a = arc_w[a] if weighted, else 0.0f
 *     r = c + lookahead[row_off + dst_a]   (r = c without lookahead)
 * and the candidate is dropped unless c > -inf and r > -inf (NaN is dropped too).  Candidates are ordered by (r desc,
 * j asc, l asc), -0.0 and +0.0 alike; lattices are deterministic, so the order is total and the result is determined.
 * Outputs (device), rank i < min(k, candidates) of every lattice: score = c (not r), parent = j (int32, the rank in the
 * lattice's beam), symbol = l, next_state = dst_a; the remaining ranks get -inf, -1, pad, 0.  n_candidates [B]
 * (optional): the candidates before truncation.  n_open (optional, one device word, zeroed by the caller) receives the
 * number of output slots that are live with a symbol other than pad: zero means every hypothesis has ended or died.
 * The outputs may be the inputs' buffers.  A lattice's candidates (at most k * its largest out-degree) are kept in LDS
 * up to nfst_beam_lds_candidates() of them and computed again in every pass of the selection beyond that.
 * k < 1, null required pointers or a pad outside the vocabulary: NFST_ERR_ARG; k > 64: NFST_ERR_LIMIT; all on the host
 * before any launch.
 */
int32_t nfst_beam_lds_candidates(void);
int nfst_beam_step(const nfst_batch *lat, const int64_t *state, const int64_t *inp, const float *beam_score, const float *scores,
                   const float *lookahead, int32_t pad, int32_t bos, int32_t eos, int32_t has_to_end, int32_t k, float *score,
                   int32_t *parent, int64_t *symbol, int64_t *next_state, int32_t *n_candidates, int32_t *n_open, void *stream);

/*
 * The paths of a finished beam search: parent and symbol [T, N] (rows of N = n_lattices * k, as nfst_beam_step wrote
 * them step by step), score [N] the scores of the last step, n_steps <= max_len the steps to follow.  Slot n follows
 * its parents from step n_steps - 1 back to step 0; paths [n_lattices, k, max_len] int32 receives its marks other than
 * pad, in order, right-padded with pad, lengths [n_lattices, k] their number.  A slot whose score is -inf gets length 0.
 * k < 1, n_steps > max_len or null pointers: NFST_ERR_ARG; k > 64: NFST_ERR_LIMIT.
 */
int nfst_beam_backtrack(const int32_t *parent, const int64_t *symbol, const float *score, int32_t n_steps, int32_t n_lattices,
                        int32_t k, int32_t max_len, int32_t pad, int32_t *paths, int32_t *lengths, void *stream);

/*
 * k distinct paths per lattice, drawn without replacement from p(path) = exp S(path) / Z by stochastic beam search
 * (Gumbel top-k; Kool, van Hoof and Welling 2019; DESIGN.md sections 2 and 4.15), the whole search in one launch.
 * logbeta [total_rows] and logz64 [B] are what nfst_backward wrote for the same scores.  1 <= k <= 64.  Reads the
 * canonical arrays only (row_ptr, arc_label, arc_dst, arc_w): any batch, any packing, the same bits.
 * Per lattice b, all in float64, Z = logz64[b].  If Z is not finite the lattice is empty: n_paths = 0 and every entry
 * has length 0, marks `pad`, arcs -1, logp = gumbel = -inf; kappa = -inf.
 * A lattice keeps at most k slots (state s, score S of the prefix, perturbed score G) and starts with one: state 0,
 * S = 0, G = +inf ("not conditioned").  Step t = 0, 1, ... while some slot is off the sink: the candidates in flat order
 * are slot j ascending, then the slot's out-arcs in canonical order without self loops; a slot at the sink is one
 * candidate, itself, unchanged (same S, same G, no noise).  For slot j at state s and arc a of rank r = a - row_ptr[s]:
 *     e_a = the arc's float32 score: theta[label_a] (+ arc_w[a] if weighted) (+ arc_scores[a] if given), added in this order
 *     S' = S_j + e_a,   phi = S' + logbeta[dst_a] - Z;   a candidate whose phi is not > -inf (NaN included) is dropped
 *     g = phi - log(-log x),   x = (double)u + 2^-25
 *     u = uniforms[b, t, j, r] (uniforms [B, max_len, k, max_degree] float32 in [0, 1); a rank r >= max_degree sets
 *         *status = NFST_ERR_ARG and drops the candidate), or without uniforms word 0 of the Philox4x32-10 block keyed by
 *         `seed` with the counter (b, t, j, r) (the block function of nfst_sample_paths)
 * With M_j the largest g of slot j's kept candidates: G~ = g if G_j = +inf; otherwise the first candidate of the slot
 * (in flat order) with g = M_j gets G~ = G_j, and every other one
 *     v = G_j - g + log(1 - exp(g - M_j))   (evaluated as log(-expm1(g - M_j))),
 *     G~ = G_j - max(v, 0) - log1p(exp(-|v|)).
 * The k candidates with the largest G~ are kept (-0.0 and +0.0 alike, equal values to the earlier flat index) and take
 * the new slots in flat order, not ranked: slot order is the lexicographic order of the prefixes.  kappa[b] is the
 * largest G~ ever dropped, -inf if nothing was.  Every step stores (parent slot, arc) per slot in ws.
 * If max_len steps pass and some slot is still off the sink, *status = NFST_ERR_LENGTH (status: device, one word,
 * zeroed by the caller) and the lattice's outputs are those of an empty one.  Otherwise the slots are ranked by
 * (G desc, slot asc) and entry i < n_paths[b] receives paths [B, k, max_len] marks padded with `pad`, path_arcs
 * (optional) [B, k, max_len] canonical arc ids padded with -1, lengths [B, k], logp [B, k] = (float)(S - Z) and gumbel
 * [B, k] = G (float64); entries from n_paths[b] on look like those of an empty lattice.
 * ws: device workspace of nfst_swor_ws_bytes(lat, k, max_len) bytes (16-byte aligned, overwritten): 8 bytes per
 * (lattice, step, slot) and, when k * vocab exceeds nfst_beam_lds_candidates(), 8 k vocab bytes per lattice for the keys
 * of a step that LDS does not hold; both parts rounded up to 256 bytes.  No atomics: the same bits from launch to
 * launch and, with uniforms, wherever the lattice sits in the batch.
 * Null required pointers, max_len < 1, k < 1, uniforms with max_degree < 1 or a short workspace: NFST_ERR_ARG; k > 64:
 * NFST_ERR_LIMIT; all on the host before any launch.
 */
int64_t nfst_swor_ws_bytes(const nfst_batch *lat, int32_t k, int32_t max_len);
int nfst_swor(const nfst_batch *lat, const nfst_scores *scores, const float *logbeta, const double *logz64, int32_t k, int32_t max_len,
              const float *uniforms, int32_t max_degree, uint64_t seed, int32_t pad, void *ws, int64_t ws_bytes, int32_t *paths,
              int32_t *path_arcs, int32_t *lengths, float *logp, double *gumbel, double *kappa, int32_t *n_paths, int32_t *status,
              void *stream);

/*
 * Unit-cost edit distance (Levenshtein: insertion, deletion and substitution cost 1 each) between the rows of two path
 * sets, the sequence-level loss the draws above exist for and the k x k table minimum-Bayes-risk selection needs
 * (DESIGN.md sections 2 and 4.17).  All pointers are device memory:
 *   a [n_sets, ka, La], b [n_sets, kb, Lb]   contiguous int32 token rows (the paths of nfst_kbest, nfst_swor, ...)
 *   a_len [n_sets, ka], b_len [n_sets, kb]   the rows' lengths
 *   out [n_sets, ka, kb]                     out[s, i, j] = distance of a[s, i, :a_len[s, i]] and b[s, j, :b_len[s, j]]
 *   status                                   one word, zeroed by the caller
 * Tokens are compared as plain integers and nothing beyond a row's length is read: the pad labels and -1 fills behind
 * a path do not matter.  A length outside [0, La] (or [0, Lb]) is found on the device: *status = NFST_ERR_LENGTH, every
 * pair of that row gets -1, no token of the pair is read, and every other pair of the launch is computed as usual.
 * symmetric != 0 is the pairwise table of one set: it requires b == a, b_len == a_len, kb == ka and Lb == La
 * (NFST_ERR_ARG otherwise), computes only i < j, writes both [i, j] and [j, i] and 0 on the diagonal, and gives the
 * bits of the general mode called with b = a.
 * La and Lb are at most NFST_EDIT_MAX_LEN: a longer row returns NFST_ERR_LIMIT, as do more than 4 (2^31 - 1) pairs.
 * Null pointers, negative n_sets, ka or kb, La < 1 or Lb < 1 return NFST_ERR_ARG; all on the host before any launch.
 * n_sets * ka * kb == 0 is a successful no-op (the data pointers may then be null).  One wave64 per pair, integer
 * arithmetic only and no atomics: the same bits at every launch.
 */
#define NFST_EDIT_MAX_LEN 1024
int nfst_edit_distance(const int32_t *a, const int32_t *a_len, int32_t ka, int32_t La, const int32_t *b, const int32_t *b_len,
                       int32_t kb, int32_t Lb, int32_t n_sets, int32_t symmetric, int32_t *out, int32_t *status, void *stream);

/*
 * The edit distance between a reference string and a whole lattice, with the path that attains it: the oracle path
 * (DESIGN.md sections 2 and 4.18).  For lattice b the reference is r = ref[b * R .. b * R + n), n = ref_len[b], int32
 * tokens compared as plain integers; nothing beyond n is read.  A path runs from state 0 to the sink (self loops are on
 * no path), its string is the labels of its arcs, bos to eos, as nfst_kbest writes them.  d(path) is the unit-cost
 * Levenshtein distance of that string and r (nfst_edit_distance's).  The path score is nfst_kbest's float32 sum: the
 * sink holds 0.0f and arc a extends value v to c = e_a + (theta[label_a] + v), e_a = 0.0f (+ arc_w[a] if weighted)
 * (+ arc_scores[a] if given); a path of score -inf or NaN is no candidate.  scores == NULL: every term is 0.0f (arc_w
 * is not read either) and every path counts.
 * Result: the lexicographic optimum, least distance, then greatest score (scores are ordered by their bits, so +0.0
 * ranks above -0.0), from cells E[s][j] = (dist, score), j tokens of r consumed:
 *     E[sink][j] = (n - j, 0.0f)
 *     E[s][j]    = the best of, over the out-arcs a: s -> d, d != s, label l:
 *                      insertion           (E[d][j].dist + 1, c(E[d][j].score))
 *                      match/substitution  (E[d][j + 1].dist + [l != r[j]], c(E[d][j + 1].score))      for j < n
 *                  and then of the deletion (E[s][j + 1].dist + 1, E[s][j + 1].score), j from n - 1 down to 0.
 * The answer is E[0][0].  The walk from (0, 0) takes at every cell the first candidate whose (dist, score bits) equal
 * the cell's: arcs in canonical order, per arc match/substitution before insertion, the deletion last; at the sink the
 * remaining tokens of r are deletions.
 * Outputs (device): distance [B]; score [B] (optional); paths [B, max_len] labels padded with `pad`; path_arcs
 * (optional) [B, max_len] canonical arc ids padded with -1; align (optional) [B, max_len]: for every arc of the path the
 * index in r of the token it was matched or substituted with, -1 for an insertion, padded with -1; lengths [B]; counts
 * (optional) [B, 3] = (substitutions, insertions, deletions), which sum to distance[b].  A lattice without a candidate
 * path gets distance -1, score -inf, length 0, pads and counts 0.
 * A ref_len[b] outside [0, R] is found on the device: *status = NFST_ERR_LENGTH (status: device, one word, zeroed by the
 * caller), that lattice gets the outputs of one without a path and none of its tokens is read; the other lattices are
 * computed as usual.  An oracle path longer than max_len is cut there (length max_len; distance, score and counts are
 * those of the whole path) and sets *status = NFST_ERR_LENGTH.
 * ws: device workspace of nfst_lattice_edit_ws_bytes(lat, R) bytes (16-byte aligned, overwritten): (R + 1) cells of 8
 * bytes per row of the batch plus 12 bytes per row.  Reads the canonical arrays only: any batch, any packing, the same
 * bits; no atomics on values: the same bits at every launch.
 * Null required pointers, R < 1, max_len < 1 or a short workspace: NFST_ERR_ARG; R > NFST_EDIT_MAX_LEN: NFST_ERR_LIMIT;
 * all on the host before any launch.  n_lattices == 0 is a successful no-op (nfst_lattice_edit_ws_bytes: 0).
 */
int64_t nfst_lattice_edit_ws_bytes(const nfst_batch *lat, int32_t R);
int nfst_lattice_edit(const nfst_batch *lat, const nfst_scores *scores /* or NULL */, const int32_t *ref, const int32_t *ref_len,
                      int32_t R /* row stride of ref */, void *ws, int64_t ws_bytes, int32_t *distance /* [B] */,
                      float *score /* [B] or NULL */, int32_t *paths, int32_t *path_arcs /* or NULL */, int32_t *align /* or NULL */,
                      int32_t *lengths /* [B] */, int32_t *counts /* [B,3] or NULL */, int32_t max_len, int32_t pad,
                      int32_t *status, void *stream);

/*
 * Output strings (DESIGN.md sections 2, 4.20 and 4.21).  The path-side ops answer in mark paths; the string of a path
 * is its projection onto the output tape, given in one of two ways (device pointer, host integer):
 *   keep [vocab] uint8    the labels of the path whose entry is non-zero, in order (WideDFA.projected_sequence's meaning)
 *   marker                the labels that directly follow an arc labelled marker (marked_sequence's meaning): a label
 *                         that follows the marker is a symbol even if it is the marker itself, and it does not then act
 *                         as a marker; a marker with nothing behind it yields no symbol
 * keep == NULL means "no mask" and marker == -1 "no marker".  Both given, a marker below -1 or not below vocab:
 * NFST_ERR_ARG.  Neither given: NFST_ERR_ARG for nfst_string_logprob; the identity for nfst_merge_paths.
 *
 * nfst_merge_paths merges the rows of path sets that spell the same string ("crunching" an n-best list).  All pointers
 * but keep's meaning above are device memory:
 *   paths [n_sets, K, L] int32, lengths [n_sets, K], log_weights [n_sets, K] float64, n_paths [n_sets] or NULL
 * Row k of set b is valid when k < n_paths[b] (always without n_paths) and its weight is neither -inf nor NaN (a
 * weight of +inf is not supported).  Only paths[b, k, :lengths[b, k]] is read, and projected; a token outside
 * [0, vocab) is on no keep mask.  Outputs, one entry per distinct projected string of the valid rows:
 *   strings [n_sets, K, L]     the strings, every row filled up with `pad`; rows beyond n_strings[b] all pad
 *   out_lengths [n_sets, K]    their lengths; 0 beyond n_strings[b]
 *   out_log_weights            float64: max + log(sum_k exp(w_k - max)) over the members k in ascending row order, max
 *                              their greatest weight; -inf beyond n_strings[b].  exp and log are evaluated in IEEE
 *                              products, sums and one division, none of them fused (string_merge_kernels.h: exp by
 *                              ln 2 reduction and the Taylor series to degree 13, log by 2 atanh((m - 1) / (m + 1)) to
 *                              z^23), so the bits do not depend on a math library and a restatement reproduces them
 *   n_strings [n_sets]
 *   group [n_sets, K]          the entry input row k went to; -1 for an invalid row
 *   first [n_sets, K]          per entry the lowest input row among its members of greatest weight; -1 beyond n_strings
 * Entries are ordered by merged weight, descending; equal weights by their lowest member row.  Rows are equal when their
 * projected lengths are, a 64-bit hash of the projected rows agrees in its low hash_bits bits (1 .. 64) and a comparison
 * token by token confirms it: hash_bits changes the work, never the outputs.  scratch [n_sets, K, L] int32 is
 * overwritten (the projected rows).  One workgroup per set, no atomics: the same bits at every launch.
 * A length outside [0, L] is found on the device: *status = NFST_ERR_LENGTH (status: device, one word, zeroed by the
 * caller), the row counts as invalid, none of its tokens is read and the rest is computed as usual.
 * K > 1024 or L > NFST_EDIT_MAX_LEN: NFST_ERR_LIMIT.  Negative n_sets or K, L < 1, hash_bits outside 1 .. 64, a bad
 * tape, a null status or (when n_sets * K > 0) any other null required pointer: NFST_ERR_ARG; all on the host before
 * any launch.  n_sets * K == 0 is a successful no-op (the data pointers may then be null).
 */
int nfst_merge_paths(const int32_t *paths, const int32_t *lengths, const double *log_weights, const int32_t *n_paths /* or NULL */,
                     int32_t n_sets, int32_t K, int32_t L, const uint8_t *keep /* [vocab] or NULL */, int32_t vocab,
                     int32_t marker /* -1: none */, int32_t hash_bits, int32_t pad, int32_t *scratch, int32_t *strings,
                     int32_t *out_lengths, double *out_log_weights, int32_t *n_strings, int32_t *group, int32_t *first,
                     int32_t *status, void *stream);

/*
 * nfst_string_logprob: for lattice b and candidate m, y = strings[b, m, :lengths[b, m]] (strings [B, M, N] int32,
 * lengths [B, M]; nothing beyond a length is read),
 *   log_num [B, M] float64   the log of the sum of exp(path score) over the paths whose projection onto the tape is y;
 *                            -inf (never NaN, and no error) when no path spells y
 *   logz [B] float64         the same sum over all paths of the lattice, from the same sweep
 * so that log_num - logz is log p(y | x) exactly, for any number of paths and without a product lattice.  A path runs
 * from state 0 to the sink, self loops are on no path, and an arc contributes theta[label] + arc_w[a] (if weighted) +
 * arc_scores[a] (if given), each taken as float64 and added in this order.  Acceptance is that of
 * WideDFA.projected_sequence(vocab, keep, y) or WideDFA.marked_sequence(vocab, marker, y): a path that ends on a marker
 * with nothing behind it spells no string (in marker mode the strings' probabilities add up to 1 less those paths'
 * share).  Cells are float64 log weights, n = len(y), j tokens of y spelled so far:
 *   keep:    G[sink][j] = [j == n];  G[s][j] = sum over the out-arcs a: s -> d, d != s, label l of
 *                w_a (l not kept ? G[d][j] : (j < n and y[j] == l) ? G[d][j + 1] : 0)
 *   marker:  two rows per state, G0 (the arc into s was no active marker) and G1 (it was one): under G1 the label must
 *            equal y[j] and leads to G0[d][j + 1]; under G0 a marker arc leads to G1[d][j], any other to G0[d][j];
 *            G0[sink][j] = [j == n], G1[sink][j] = 0
 * and the answer is G[0][0] (G0).  A state's sum runs over its arcs in canonical order as a running log-sum around the
 * greatest term so far; only the canonical arrays are read and there are no atomics: the same bits at every launch and
 * under every packing.  A lattice whose state 0 is the sink gives 0 for the empty string, -inf otherwise, and logz 0.
 * A lengths[b, m] outside [0, N] is found on the device: *status = NFST_ERR_LENGTH (status: device, one word, zeroed by
 * the caller), that candidate gets -inf and none of its tokens is read; the others are computed as usual.
 * ws: device workspace of nfst_string_logprob_ws_bytes(lat, M, N, marker >= 0) bytes (16-byte aligned, overwritten):
 * 8 (N + 1) M bytes per row of the batch, twice that in marker mode, plus 20 bytes per row; every part rounded up to
 * 256.  LDS: 12 max_rows + 16 bytes (the level pass); more than 160 KiB returns NFST_ERR_LIMIT.
 * M < 0, N < 1, a bad tape, null required pointers (strings, lengths and log_num may be null when M == 0: logz alone is
 * computed) or a short workspace: NFST_ERR_ARG; N > NFST_EDIT_MAX_LEN: NFST_ERR_LIMIT; all on the host before any
 * launch.  n_lattices == 0 is a successful no-op (nfst_string_logprob_ws_bytes: 0).
 */
int64_t nfst_string_logprob_ws_bytes(const nfst_batch *lat, int32_t M, int32_t N, int32_t marker_mode);
int nfst_string_logprob(const nfst_batch *lat, const nfst_scores *scores, const int32_t *strings, const int32_t *lengths, int32_t M,
                        int32_t N /* row stride of strings */, const uint8_t *keep /* [vocab] or NULL */, int32_t marker /* -1: none */,
                        void *ws, int64_t ws_bytes, double *log_num /* [B,M] */, double *logz /* [B] */, int32_t *status,
                        void *stream);

/*
 * nfst_string_logprob_grad: the derivative of sum_{b,m} g_num[b, m] log_num[b, m] + sum_b g_z[b] logz[b] in every arc's
 * score, the one float64 value theta[label] + arc_w + arc_scores that nfst_string_logprob forms.
 * Inputs as nfst_string_logprob's, plus g_num [B, M] and g_z [B] float64 (device) and the host integer accumulate;
 * output grad_arc [total_arcs] float64 in canonical arc order.  The entry point recomputes G, G0, G1 and z (the sweep of
 * nfst_string_logprob, bit for bit) and sweeps the matching prefix tables in ascending level order: F[s][j], the log
 * weight of the path prefixes from state 0 to s that have spelled y[:j], and az[s], that of all prefixes; w_a is the score
 * of arc a: s -> d with label l, s != d:
 *   keep:    F[0][j] = [j == 0];  a non-kept arc carries F[s][j] to F[d][j], a kept one F[s][j] to F[d][j + 1] when
 *            j < n and y[j] == l
 *            post_m(a) = sum_j exp(F[s][j] + w_a + G[d][j] - log_num)                         (l not kept)
 *                        sum_{j < n, y[j] == l} exp(F[s][j] + w_a + G[d][j + 1] - log_num)    (l kept)
 *   marker:  F0[0][j] = [j == 0], F1[0][j] = 0;  from F0[s][j] a marker arc goes to F1[d][j], any other to F0[d][j];
 *            from F1[s][j] every arc goes to F0[d][j + 1] when j < n and y[j] == l
 *            post_m(a) = sum_j (exp(F0[s][j] + w_a + (l == marker ? G1 : G0)[d][j] - log_num)
 *                               + [j < n and y[j] == l] exp(F1[s][j] + w_a + G0[d][j + 1] - log_num))
 *   log Z:   az[0] = 0;  post_z(a) = exp(az[s] + w_a + z[d] - z[0])
 *   grad_arc[a] = (((start + t_0) + t_1) + ...) + t_{M-1},  t_m = g_num[b, m] post_m(a), added in ascending m;
 *            start = g_z[b] post_z(a) with accumulate == 0; with accumulate != 0 start is the value already in
 *            grad_arc[a] and the g_z term is not added again (g_z may then be NULL), so that a caller who slices the
 *            candidates -- the first slice with accumulate == 0, the others in ascending order with accumulate != 0 --
 *            gets the bits of one launch.
 * Order of the sums (float64, none fused across terms): a cell of F is a running log-sum around the greatest term so far
 * (as G's) over the in-arcs of its state in ascending canonical arc id, a term being w_a + F[s][.]; in marker mode an
 * in-arc adds to F0[d][j] first its F0 term, then its F1 term.  An exponent of post is evaluated as ((F + w_a) + G) -
 * log_num.  Inside t_m the columns j are taken in strips of 64, j = 64 p + lane; lane j's term of a strip is 0 outside
 * the row and in marker mode the F0 term plus the F1 term in this order; the 64 terms of a strip are added in the tree
 * x_i += x_(i^1), x_(i^2), x_(i^7), x_(i^15) (four stages inside every 16 lanes), then (r_0 + r_16) + (r_32 + r_48); the
 * strips' sums are added to 0.0 in ascending p; t_m is g_num[b, m] times that sum.
 * Exactly 0 (never NaN, and no error): a self loop, an arc whose source state 0 does not reach or that reaches no sink,
 * a candidate whose log_num is -inf, a candidate with g_num[b, m] == 0, a candidate with a length outside [0, N]
 * (*status = NFST_ERR_LENGTH as in nfst_string_logprob, none of its tokens is read), a lattice whose state 0 is the sink.
 * Only the canonical arrays are read and there are no atomics on values: the same bits at every launch, for every grid,
 * under every packing and for every such slicing.
 * ws: device workspace of nfst_string_logprob_grad_ws_bytes(lat, M, N, marker >= 0) bytes (16-byte aligned, overwritten):
 * that of nfst_string_logprob, a second cell table of the same size, 8 bytes per row, 8 (M + 1) per lattice, and the
 * in-arc lists (4 bytes per row and lattice, 8 per arc); every part rounded up to 256.  LDS: 12 max_rows + 4100 bytes.
 * Checks and their codes are those of nfst_string_logprob (g_num may be null when M == 0: the log Z term alone; a null
 * g_z without accumulate, a null grad_arc with arcs: NFST_ERR_ARG), all on the host before any launch, outputs untouched.
 * n_lattices == 0 is a successful no-op (nfst_string_logprob_grad_ws_bytes: 0).
 */
int64_t nfst_string_logprob_grad_ws_bytes(const nfst_batch *lat, int32_t M, int32_t N, int32_t marker_mode);
int nfst_string_logprob_grad(const nfst_batch *lat, const nfst_scores *scores, const int32_t *strings, const int32_t *lengths, int32_t M,
                             int32_t N /* row stride of strings */, const uint8_t *keep /* [vocab] or NULL */,
                             int32_t marker /* -1: none */, const double *g_num /* [B,M] */, const double *g_z /* [B] */,
                             int32_t accumulate, void *ws, int64_t ws_bytes, double *grad_arc /* [total_arcs] */, int32_t *status,
                             void *stream);

/*
 * Prefix weights and next symbols (DESIGN.md sections 2 and 4.23).  Tape, scores, paths and the canonical order of the
 * arcs are nfst_string_logprob's; for lattice b and prefix y = prefixes[b, m, :lengths[b, m]] (prefixes [B, M, N] int32,
 * lengths [B, M]; nothing beyond a length is read), n = len(y), all outputs float64 log weights on the device:
 *   log_prefix [B, M]      the sum of exp(path score) over the paths whose string starts with y; a path that ends on a
 *                          marker with nothing behind it spells no string and counts nowhere.  The empty prefix gives
 *                          log Z in keep mode and log Z less those paths' share in marker mode
 *   eos [B, M]             the same over the paths that spell exactly y (nfst_string_logprob's log_num)
 *   next [B, M, vocab]     log_prefix of y followed by the label v, for every v; -inf for a label that is never on the
 *                          tape (keep mode: v not kept)
 *   logz [B]               nfst_string_logprob's logz, bit for bit (the same items in the same order)
 * so that exp(log_prefix) = exp(eos) + sum_v exp(next[v]) as real numbers.  A prefix that no path spells gives -inf
 * everywhere, never NaN, and no error.
 *
 * nfst_string_prefix (log_prefix and logz) sweeps H, which is G of nfst_string_logprob with "anything may follow" at
 * column n, in descending level order; columns j < n follow G's recurrence, and at j = n
 *   keep:    H[sink][n] = 1;  every out-arc a: s -> d, d != s, kept or not, carries w_a H[d][n]
 *   marker:  H0[sink][n] = 1, H1[sink][n] = 0;  H0[s][n] = sum_a w_a (l == marker ? H1 : H0)[d][n];
 *            H1[s][n] = sum_a w_a H0[d][n]
 * and log_prefix = H0[0][0].  A cell is a running log-sum around the greatest term so far over the out-arcs of its
 * state in ascending canonical arc id, as G's.
 *
 * nfst_string_next (all four outputs) sweeps no H over the candidates.  It runs nfst_string_prefix's sweep once per
 * lattice on the empty prefix (one column), which leaves z[s] (log Z of the rest of the lattice behind s) and zn0[s],
 * zn1[s] (the same without the paths that end on a marker, the arc into s being no active marker / one), then the
 * prefix tables F, F0, F1 and az of nfst_string_logprob_grad (same kernels, same order), and forms
 *   keep:    next[v] = sum over the arcs a: s -> d, d != s, of label v (v kept) of exp((F[s][n] + w_a) + z[d])
 *   marker:  next[v] = sum over the arcs of label v of exp((F1[s][n] + w_a) + zn0[d])
 *   eos = F0[sink][n];  log_prefix = the sum of eos and next[0 .. vocab - 1]
 * Order of these sums (float64, none fused across terms): the terms of a sum are numbered i = 0, 1, ... -- for next[v]
 * the arcs of label v whose source state 0 reaches in ascending canonical arc id, for log_prefix eos first and then
 * next[v] in ascending v.  The greatest term t* is found first (exact in any order).  Term i belongs to strip i / 64 and
 * lane i mod 64; the 64 values exp(t_i - t*) of a strip (0 beyond the last term and for a term of -inf) are added in
 * the tree of nfst_string_logprob_grad (x_i += x_(i^1), x_(i^2), x_(i^7), x_(i^15), then (r_0 + r_16) + (r_32 + r_48));
 * the strips' sums are added to 0.0 in ascending order, and the result is t* + log(sum), or -inf without a term above
 * -inf.  Only the canonical arrays are read and there are no atomics on values: the same bits at every launch, for every
 * grid, under every packing and for every slicing of the candidates.
 * A lattice whose state 0 is the sink gives log_prefix = eos = 0 for the empty prefix, -inf otherwise, and next = -inf.
 * A lengths[b, m] outside [0, N] is found on the device: *status = NFST_ERR_LENGTH (status: device, one word, zeroed by
 * the caller), every output of that candidate is -inf and none of its tokens is read; the others are computed as usual.
 * ws: device workspace (16-byte aligned, overwritten), every part rounded up to 256.  nfst_string_prefix_ws_bytes is
 * nfst_string_logprob_ws_bytes.  nfst_string_next_ws_bytes(lat, M, N, marker >= 0): 8 (N + 1) M bytes per row of the
 * batch (F), twice that in marker mode, 8 (planes + 2) + 12 bytes per row, 12 bytes per arc and 4 vocab + 24 bytes per
 * lattice.  LDS: 12 max_rows + 4100 bytes (the in-arc lists), and for nfst_string_next 4 (max_rows + vocab) + 4100 bytes
 * (the label lists); more than 160 KiB returns NFST_ERR_LIMIT.
 * M < 0, N < 1, a bad tape, null required pointers (all but lat, scores, ws, logz and status may be null when M == 0)
 * or a short workspace: NFST_ERR_ARG; N > NFST_EDIT_MAX_LEN: NFST_ERR_LIMIT; all on the host before any launch, outputs
 * untouched.  n_lattices == 0 and M == 0 are successful no-ops (n_lattices == 0: the ws_bytes queries return 0).
 */
int64_t nfst_string_prefix_ws_bytes(const nfst_batch *lat, int32_t M, int32_t N, int32_t marker_mode);
int nfst_string_prefix(const nfst_batch *lat, const nfst_scores *scores, const int32_t *prefixes, const int32_t *lengths, int32_t M,
                       int32_t N /* row stride of prefixes */, const uint8_t *keep /* [vocab] or NULL */, int32_t marker /* -1: none */,
                       void *ws, int64_t ws_bytes, double *log_prefix /* [B,M] */, double *logz /* [B] */, int32_t *status,
                       void *stream);
int64_t nfst_string_next_ws_bytes(const nfst_batch *lat, int32_t M, int32_t N, int32_t marker_mode);
int nfst_string_next(const nfst_batch *lat, const nfst_scores *scores, const int32_t *prefixes, const int32_t *lengths, int32_t M,
                     int32_t N /* row stride of prefixes */, const uint8_t *keep /* [vocab] or NULL */, int32_t marker /* -1: none */,
                     void *ws, int64_t ws_bytes, double *next /* [B,M,vocab] */, double *eos /* [B,M] */,
                     double *log_prefix /* [B,M] */, double *logz /* [B] */, int32_t *status, void *stream);

/*
 * Prefix states (DESIGN.md sections 2 and 4.25): nfst_string_next's answers for prefixes that grow by one symbol per call,
 * at the cost of one column of F per symbol instead of the whole table.  Tape, scores, paths and the canonical order of
 * the arcs are nfst_string_logprob's.
 *
 * nfst_string_prefix_open does once what depends on the lattice and the scores but on no prefix, with the kernels of
 * nfst_string_next in this order: the level pass, nfst_string_prefix's sweep on the empty prefix (z, zn0 / zn1 and
 * logz [B], which has nfst_string_logprob's bits), the in-arc lists, az (the prefix sweep without a candidate), the label
 * lists.  Its workspace is the context that the other calls read (with the same lattice, scores and tape; it must be
 * opened again when any of them changes): nfst_string_prefix_open_ws_bytes(lat, marker >= 0) is nfst_string_next_ws_bytes
 * without the table F -- 8 (planes + 2) + 12 bytes per row, 12 bytes per arc and 4 vocab + 24 bytes per lattice, every part
 * rounded up to 256.  LDS: nfst_string_next's; more than 160 KiB returns NFST_ERR_LIMIT.
 *
 * A state holds one column of F (marker mode: of F0 and F1) for M hypotheses of every lattice, float64: the cell of row r
 * of lattice b (row_off[b] + r in the batch), plane p and hypothesis m lies at ((row_off[b] + r) planes + p) M + m, so
 * the hypotheses of one state are adjacent.  nfst_string_prefix_state_bytes(lat, M, marker >= 0) = 8 planes M total_rows
 * rounded up to 256 (planes = 2 in marker mode, else 1).  Rows that state 0 does not reach are never written and never
 * read.  A state is opaque to the caller, 16-byte aligned, and belongs to the context it was made with.
 *
 * nfst_string_prefix_extend forms, for lattice b and child slot m < M_out, the column of the prefix that is one symbol,
 * symbol[b, m], longer than the prefix of slot parent[b, m] of parent_state (M_in slots):
 *   parent == -2   the empty prefix (column 0: F0[state 0] = 0, F1 = -inf, and the arcs that are not on the tape / no
 *                  markers carry it forward); the symbol is not read.  With no parent >= 0 anywhere parent_state may be
 *                  null and M_in 0
 *   parent == -1   a dead slot: every cell is -inf
 * The recurrence and the order of every cell's sum are those of nfst_string_logprob_grad's table F at column n + 1: a
 * running log-sum around the greatest term so far over the in-arcs of the state (source reached from state 0, no self
 * loop) in ascending canonical arc id, one term per in-arc, in marker mode the F0 term before the F1 term into F0.  A
 * child's column therefore has the bits of column n + 1 of that table for the same prefix.  Children are independent of
 * one another and several may share a parent; the bits do not depend on M_in, M_out, the slots or the launch.  A parent
 * outside [-2, M_in), or a symbol outside [0, vocab) in a slot with parent >= 0, is found on the device: *status =
 * NFST_ERR_INDEX (status: device, one word, zeroed by the caller), that slot is dead and the others are computed as usual.
 * A symbol that is off the tape, or that no path spells after the parent, gives -inf cells, never NaN, and no error.
 * LDS: 8 max_rows + 4 bytes.
 *
 * nfst_string_prefix_state_next gives next [B, M, vocab], eos [B, M] and log_prefix [B, M] of nfst_string_next, formed
 * from the state's column in place of F[.][n] with the same terms in the same order: bit for bit nfst_string_next's
 * outputs for the same prefixes.  A dead slot gives -inf everywhere.  logz is nfst_string_prefix_open's.
 *
 * On the host before any launch, outputs untouched: a bad tape, null required pointers (parent_state only when M_in == 0),
 * a context, a state or an output state shorter than its _bytes query says, a misaligned buffer, a negative M, or an
 * out_state that overlaps parent_state: NFST_ERR_ARG; M, M_in or M_out above 1024 or more than 160 KiB of LDS:
 * NFST_ERR_LIMIT.  n_lattices == 0, M_out == 0 and M == 0 are successful no-ops (n_lattices == 0: the _bytes queries
 * return 0).
 */
int64_t nfst_string_prefix_open_ws_bytes(const nfst_batch *lat, int32_t marker_mode);
int nfst_string_prefix_open(const nfst_batch *lat, const nfst_scores *scores, const uint8_t *keep /* [vocab] or NULL */,
                            int32_t marker /* -1: none */, void *ws, int64_t ws_bytes, double *logz /* [B] */, int32_t *status,
                            void *stream);
int64_t nfst_string_prefix_state_bytes(const nfst_batch *lat, int32_t M, int32_t marker_mode);
int nfst_string_prefix_extend(const nfst_batch *lat, const nfst_scores *scores, const uint8_t *keep, int32_t marker, const void *ctx_ws,
                              int64_t ctx_bytes, const double *parent_state, int64_t parent_bytes, int32_t M_in,
                              const int32_t *parent /* [B,M_out] */, const int32_t *symbol /* [B,M_out] */, double *out_state,
                              int64_t out_bytes, int32_t M_out, int32_t *status, void *stream);
int nfst_string_prefix_state_next(const nfst_batch *lat, const nfst_scores *scores, const uint8_t *keep, int32_t marker,
                                  const void *ctx_ws, int64_t ctx_bytes, const double *state, int64_t state_bytes, int32_t M,
                                  double *next /* [B,M,vocab] */, double *eos /* [B,M] */, double *log_prefix /* [B,M] */,
                                  int32_t *status, void *stream);

/*
 * Alignments to given strings (DESIGN.md sections 2 and 4.24).  Tape, scores, paths, candidates (strings [B, M, N],
 * lengths [B, M]), the canonical order of the arcs and the workspace are nfst_string_logprob's.  A walk is in a state
 * (s, j, f): lattice state, tokens of y already spelled, and (marker mode) "the arc into s was an active marker"; it
 * starts at (0, 0, 0) and an out-arc a: s -> d, d != s, label l leads to the cell its term of G reads:
 *   keep:    l not kept: (d, j);  l kept, j < n and y[j] == l: (d, j + 1), the arc emits position j;  otherwise nowhere
 *   marker:  f == 0: (d, j, l == marker);  f == 1, j < n and y[j] == l: (d, j + 1, 0), the arc emits position j;
 *            f == 1 otherwise nowhere
 * and it ends at the sink, where the table leaves only j == n, f == 0.
 *
 * nfst_string_viterbi: V is G with max for the sum, V[sink][n] = 0, V[s][j] = max over the arcs of fl(w_a + V[cell of
 * a]), float64, -inf without an arc.  score [B, M] is V0[0][0], -inf where no path of finite score spells y.  From every
 * state the walk takes the first arc in canonical order whose term equals the state's cell.  Every output is a pure
 * function of the inputs: the same bits as any restatement that forms w_a as nfst_string_logprob does.
 *
 * nfst_string_sample: K draws per (lattice, candidate) from p(path | x, y) = exp(score(path) - log_num) over the paths
 * that spell y, behind the sweep of nfst_string_logprob as it is (log_num [B, M] and logz [B] have its bits).  At
 * (s, j, f) arc a has the weight p_a = exp((w_a + G[cell of a]) - G_f[s][j]); the walk takes the first arc of positive
 * weight whose running sum in canonical order exceeds u, and if rounding leaves none the last arc of positive weight
 * (the rule of nfst_positional_sample; the running sum is an inclusive scan over 64 arcs at a time carried from chunk
 * to chunk, so that a draw whose u lies within rounding of a boundary may differ from another order of summation).
 * u is float32: step t of walk (b, m, k) reads uniforms[b, m, k, t] (uniforms [B, M, K, max_len], device), or without
 * uniforms word t mod 4 of the Philox4x32-10 block keyed by seed at the counter (b, t / 4, m0 + m, k); m0 is the place
 * of this call's first candidate among the caller's, so that a caller who slices the candidates gets the draws of one
 * call.  score [B, M, K] is the float64 sum of the path's arc scores in path order, logq [B, M, K] = score - log_num.
 *
 * Both write per walk (one per candidate, or K): paths [.., max_len] int32 labels, pad-terminated; path_arcs the
 * canonical arc ids, -1 padded; align the position of y that each arc emitted, -1 for none and beyond the path;
 * out_lengths the arcs of the path.  A candidate that no path spells: length 0, pad, -1, score -inf, logq 0.  A lattice
 * whose state 0 is the sink: the empty path of score 0 for the empty string, nothing for any other.
 * A lengths[b, m] outside [0, N] is found on the device: *status = NFST_ERR_LENGTH (status: device, one word, zeroed by
 * the caller), that candidate gets the empty answer and none of its tokens is read.  A path longer than max_len: the
 * same status, the path is cut at max_len (a draw's score and logq still cover the whole path).
 * ws: nfst_string_viterbi_ws_bytes and nfst_string_sample_ws_bytes are nfst_string_logprob_ws_bytes; the walks need no
 * workspace.  LDS as nfst_string_logprob.
 * M < 0, N < 1, K < 1, m0 < 0, max_len < 1, a bad tape, a null required pointer (every output is required) or a short
 * workspace: NFST_ERR_ARG; N > NFST_EDIT_MAX_LEN or more than 2^31 - 1 walks: NFST_ERR_LIMIT; all on the host before
 * any launch, outputs untouched.  n_lattices == 0 and M == 0 are successful no-ops that launch nothing and write nothing:
 * with M == 0 nfst_string_sample leaves logz untouched too, unlike nfst_string_logprob, which computes log Z without
 * candidates -- call that one for log Z alone.  nfst_string_viterbi has no K, m0, uniforms or seed: it walks once per
 * candidate and reads no uniform.
 */
int64_t nfst_string_viterbi_ws_bytes(const nfst_batch *lat, int32_t M, int32_t N, int32_t marker_mode);
int nfst_string_viterbi(const nfst_batch *lat, const nfst_scores *scores, const int32_t *strings, const int32_t *lengths, int32_t M,
                        int32_t N /* row stride of strings */, const uint8_t *keep /* [vocab] or NULL */, int32_t marker /* -1: none */,
                        int32_t max_len, int32_t pad, void *ws, int64_t ws_bytes, double *score /* [B,M] */,
                        int32_t *paths /* [B,M,max_len] */, int32_t *path_arcs, int32_t *align, int32_t *out_lengths /* [B,M] */,
                        int32_t *status, void *stream);
int64_t nfst_string_sample_ws_bytes(const nfst_batch *lat, int32_t M, int32_t N, int32_t marker_mode);
int nfst_string_sample(const nfst_batch *lat, const nfst_scores *scores, const int32_t *strings, const int32_t *lengths, int32_t M,
                       int32_t N /* row stride of strings */, const uint8_t *keep /* [vocab] or NULL */, int32_t marker /* -1: none */,
                       int32_t K, int32_t m0, const float *uniforms /* [B,M,K,max_len] or NULL */, uint64_t seed, int32_t max_len,
                       int32_t pad, void *ws, int64_t ws_bytes, double *log_num /* [B,M] */, double *logz /* [B] */,
                       double *score /* [B,M,K] */, double *logq /* [B,M,K] */, int32_t *paths /* [B,M,K,max_len] */,
                       int32_t *path_arcs, int32_t *align, int32_t *out_lengths /* [B,M,K] */, int32_t *status, void *stream);

/*
 * Arc slack, the max-plus counterpart of the arc posteriors, and beam masks (DESIGN.md sections 2 and 4.7).  A path
 * runs from state 0 to the sink; self loops (the sink's pad loop) are on no path.  All arithmetic is float32, in this order:
 *     c_a = e_a + (theta[label_a] + vbeta(dst_a)),  e_a = 0.0f (+ arc_w[a] if weighted) (+ arc_scores[a] if given)
 *     vbeta(sink) = 0,  vbeta(s) = max of c_a over the out-arcs of s without self loops (-inf without one)
 *     best[b] = vbeta(0): the bits of nfst_kbest's entry 0 (and of nfst_viterbi's best without per-arc extras)
 *     gap_a = vbeta(src_a) - c_a where c_a > -inf: >= 0, and exactly 0 on the arc that attains the maximum
 *     delta(0) = 0 if best > -inf, else +inf;  slack_a = delta(src_a) + gap_a (+inf where c_a = -inf or delta = +inf)
 *     delta(d) = min of slack_a over the in-arcs of d without self loops (+inf without one);  a self loop at s: delta(s)
 * slack_a is how far the best path through arc a falls short of the best path: >= 0, exactly 0 on every arc of
 * nfst_kbest's entry 0, +inf on arcs that lie on no path of finite score; best[b] - slack_a is the arc's max-marginal
 * (one more rounding).  With beam ([B], device, each >= 0 or +inf): keep[a] = slack_a <= beam[b] and slack_a < +inf
 * (uint8 0 / 1; an arc on no path of finite score is never kept, also under beam +inf) and n_kept[b] = the kept arcs.  The kept arcs are trim: every kept arc lies on a path of kept arcs from state
 * 0 to the sink, and the sink's pad loop is kept whenever best > -inf.  The beam is not read on the host: the caller
 * validates it (the Python wrapper raises for a negative or NaN beam); under such a beam a lattice keeps no arc.
 * Outputs (device): best [B]; slack [total_arcs]; keep [total_arcs] and n_kept [B] (both required with beam, both
 * NULL without); optional vbeta and state_slack [total_rows]: vbeta(s) and delta(s) of the rows that lie on a path of
 * finite score, -inf and +inf for every other row.  A lattice without a path of finite score gets best = -inf, slack
 * +inf everywhere and n_kept = 0.  Every output is written exactly once: bit-identical from launch to launch, and for
 * every packing of the same lattices (max and min are exact, the programs only order them), with or without chunked
 * programs (this op has no chunked flavour).
 * ws: device workspace of nfst_arc_slack_ws_bytes(lat) bytes (16-byte aligned, overwritten): 4 bytes per arc and 8 per
 * row.  LDS: 8 bytes per row and 4 per label: 8 max_rows + 4 vocab + 16 > 160 KiB returns NFST_ERR_LIMIT.  Null
 * required pointers, keep / n_kept without beam (or beam without them) or a short workspace return NFST_ERR_ARG.
 */
int64_t nfst_arc_slack_ws_bytes(const nfst_batch *lat);
int nfst_arc_slack(const nfst_batch *lat, const nfst_scores *scores, const float *beam, void *ws, int64_t ws_bytes, float *best,
                   float *vbeta, float *state_slack, float *slack, uint8_t *keep, int32_t *n_kept, void *stream);

/*
 * The product of every lattice with a deterministic automaton over the labels (DESIGN.md sections 2 and 4.8): sorted
 * arc lists that both packers take, whose paths are exactly the paths of the lattice that the automaton accepts.  A
 * path runs from state 0 to the sink over canonical arcs; self loops (the sink's pad loop) are on no path.
 * Automaton: n_q states, 1 <= n_q <= 64, start state 0; delta[q][l] in {-1, 0 .. n_q - 1} for every label l < vocab
 * (-1: no transition); final states.  It reads the label of every arc of a path, bos and eos included, never the label
 * of a self loop; a path is accepted when every step has a transition and the run ends in a final state.  On the device
 * the table is label-major: delta_t [vocab, 64] int8, -1 padded (delta_t[l * 64 + q] = delta[q][l]) and final_mask is one
 * 64-bit word (bit q = final[q]); delta_stride / final_stride = 0: one automaton for the batch, else the distance in
 * elements between the automata of consecutive lattices (delta_stride >= vocab * 64, final_stride >= 1).
 * Product, per lattice (fwd, bwd, live: sets of automaton states, 64-bit masks):
 *     fwd(0) = {0};  fwd(d) = union over the in-arcs (s, l, d) without self loops of { delta[q][l] >= 0 : q in fwd(s) }
 *     bwd(sink) = the final states;  bwd(s) = union over the out-arcs (s, l, d) without self loops of
 *                 { q : delta[q][l] in bwd(d) }
 *     live(s) = fwd(s) & bwd(s) for the states that state 0 reaches, empty for every other row; the product is empty
 *               iff 0 is not in live(0)
 * Rows: the pairs (s, q), q in live(s), in (s ascending, q ascending) order; all pairs of the sink are ONE row, at the
 * position of the first of them.  A row's id is its rank in that order (row 0 = (0, 0)); row_state = s, row_q = q (the
 * sink row: its smallest live q).
 * Arcs: for every row (s, q) in row order, for every canonical arc a = (s, l, d) of s in canonical order: a self loop
 * gives (row, l, row), once per row; any other arc with t = delta[q][l] >= 0 and t in live(d) gives
 * (row(s, q), l, row(d, t)); nothing else.  arc_map = a's position among the batch's canonical arcs (int64), arc_q = q
 * (0 on a self loop of the sink row).  The list is sorted by (src, label), deterministic, acyclic apart from self loops,
 * trim, and has exactly one sink; row and state ids are relative to the lattice, as nfst_arcs_device takes them.
 * Every output is an integer written once at a position fixed by prefix sums: bit-identical from launch to launch and
 * for every packing of the input, with or without chunked programs (only the canonical arrays are read).
 *   nfst_intersect_count  counts [B, 2] = (rows, arcs) of every product, status [B]: a product of more than
 *                         NFST_MAX_ROWS rows gets NFST_ERR_LIMIT (counts = (rows, 0)); an empty product has counts (0, 0)
 *                         and status 0.  Leaves the masks and the offsets in ws.
 *   nfst_intersect_write  after one read-back of counts and status: out_row_off / out_arc_off [B] int64 (device) = the
 *                         exclusive prefix sums of the rows / arcs of count (0 rows and arcs for a lattice over the
 *                         limit); src, label, dst, arc_q [sum of arcs] int32, arc_map [sum of arcs] int64, row_state,
 *                         row_q [sum of rows] int32.  Same lat, delta_t, n_q and ws as the count call.
 * ws: device workspace of nfst_intersect_ws_bytes(lat, n_q) bytes (16-byte aligned, overwritten): 24 bytes per row of
 * the batch and 8 * NFST_MAX_ROWS + 8 per lattice.  LDS: 16 bytes per row of the largest lattice.  Any lattice the
 * engine packs is taken.  n_q > 64: NFST_ERR_LIMIT; n_q < 1, null required pointers, bad strides or a short workspace:
 * NFST_ERR_ARG; all on the host before any launch.  The entries of delta_t are not read on the host: the caller
 * validates them (the Python wrapper does).
 */
int64_t nfst_intersect_ws_bytes(const nfst_batch *lat, int32_t n_q);
int nfst_intersect_count(const nfst_batch *lat, const int8_t *delta_t, int64_t delta_stride, const uint64_t *final_mask,
                         int64_t final_stride, int32_t n_q, void *ws, int64_t ws_bytes, int32_t *counts, int32_t *status,
                         void *stream);
int nfst_intersect_write(const nfst_batch *lat, const int8_t *delta_t, int64_t delta_stride, int32_t n_q, void *ws,
                         int64_t ws_bytes, const int64_t *out_row_off, const int64_t *out_arc_off, int32_t *src, int32_t *label,
                         int32_t *dst, int64_t *arc_map, int32_t *arc_q, int32_t *row_state, int32_t *row_q, void *stream);

/*
 * The same product with a sparse automaton of up to 4096 states (DESIGN.md sections 2 and 4.19): the wide route beside
 * the trio above, which stays as it is.  Semantics, rows, arcs and outputs are exactly those described above with 64
 * replaced by 4096: reading rules, fwd / bwd / live, row order (s ascending, q ascending), the sink's pairs as one row
 * carrying its smallest live q, arcs in canonical order per row, self loops once per row, a trim product, arc_q = 0 on
 * the sink row's loop, and the same determinism: integers written once at positions fixed by prefix sums, from the
 * canonical arrays only.
 * Automata: n_dfa = 1 (one for the batch) or n_dfa = n_lattices (one per lattice, ragged), concatenated, device memory:
 *     q_off     [n_dfa + 1] int32  first state of every automaton in dflt / exc_off / final; Q_i = q_off[i+1] - q_off[i],
 *                                  1 <= Q_i <= max_q <= 4096; start state 0
 *     dflt      [sum Q]     int32  default target of every state
 *     exc_off   [sum Q + 1] int32  first exception of every state in exc_label / exc_dst (one ascending array over all
 *                                  automata)
 *     exc_label [E]         int32  strictly ascending inside a state, < vocab
 *     exc_dst   [E]         int32
 *     final     [sum Q]     uint8  non-zero: final
 * delta(q, l) = exc_dst[k] if some k in [exc_off[q], exc_off[q + 1]) has exc_label[k] == l, else dflt[q].  A target is
 * relative to its own automaton; -1 (in either place) = no transition.  exc_label and exc_dst must be valid pointers
 * even when E = 0.
 *   nfst_intersect_wide_count / _write  as nfst_intersect_count / _write: counts [B, 2], status [B] (a product of more
 *                         than NFST_MAX_ROWS rows: NFST_ERR_LIMIT with counts (rows, 0); an empty product: counts (0, 0),
 *                         status 0), one read-back, then the write call with the prefix sums and the same lat, automata,
 *                         max_q and ws.  arc_q, row_q, row_state, src, label, dst int32; arc_map int64.
 * ws: device workspace of nfst_intersect_wide_ws_bytes(lat, max_q) bytes (16-byte aligned, overwritten): with
 * W = ceil(max_q / 64), 16 W + 12 bytes per row of the batch and 8 * NFST_MAX_ROWS + 12 per lattice, every array rounded
 * up to 256 bytes.  No LDS beyond 256 bytes.  max_q > 4096: NFST_ERR_LIMIT; max_q < 1, a null pointer, n_dfa other than 1
 * or n_lattices, or a short workspace: NFST_ERR_ARG; all on the host before any launch.  The automaton's entries are not
 * read on the host: the caller validates them (offsets ascending and inside the arrays, targets in -1 .. Q_i - 1,
 * labels ascending and < vocab, Q_i <= max_q; the Python wrapper does).  As a last line of defence the kernels treat a
 * target outside 0 .. Q_i - 1 as "no transition" and give a lattice whose Q_i lies outside 1 .. 64 W the status
 * NFST_ERR_ARG with counts (0, 0).
 */
int64_t nfst_intersect_wide_ws_bytes(const nfst_batch *lat, int32_t max_q);
int nfst_intersect_wide_count(const nfst_batch *lat, const int32_t *q_off, const int32_t *dflt, const int32_t *exc_off,
                              const int32_t *exc_label, const int32_t *exc_dst, const uint8_t *final, int32_t n_dfa, int32_t max_q,
                              void *ws, int64_t ws_bytes, int32_t *counts, int32_t *status, void *stream);
int nfst_intersect_wide_write(const nfst_batch *lat, const int32_t *q_off, const int32_t *dflt, const int32_t *exc_off,
                              const int32_t *exc_label, const int32_t *exc_dst, const uint8_t *final, int32_t n_dfa, int32_t max_q,
                              void *ws, int64_t ws_bytes, const int64_t *out_row_off, const int64_t *out_arc_off, int32_t *src,
                              int32_t *label, int32_t *dst, int64_t *arc_map, int32_t *arc_q, int32_t *row_state, int32_t *row_q,
                              void *stream);

/*
 * Position-dependent scores: time-synchronous sweeps (DESIGN.md sections 2 and 4.10).  A path pi = a_0 .. a_{L-1} runs
 * from state 0 to the sink over canonical arcs; self loops (the sink's pad loop) are on no path.  Arc a_t is "at
 * position t": the bos arc at position 0, the eos arc at L - 1.  The caller gives T >= 1 positions and optionally pos
 * (device float32): one [T, V] table (pos_stride = 0) or [B, T, V] (pos_stride = T * V).  With s_a the arc log weight of
 * nfst_scores,
 *     S_T(pi) = sum_t ( s_{a_t} + pos[b, t, label(a_t)] ),     Z_T = sum over the paths with L <= T of exp S_T(pi).
 * Paths of more than T arcs are not counted.  pos = NULL: the term is absent (no add happens, it is not "zeros").  An
 * entry of pos may be -inf: the arc has weight zero at that position (how a caller forces or forbids a mark at a
 * position).  Every label of a path is read, bos and eos included; the pad label lies on no path, so pos[.., pad] enters
 * no output (it may hold anything).  NaN or +inf in pos is the caller's business: nothing scans for it.
 *
 * nfst_positional (sum-product).  Outputs on the device, optional unless stated, every element written exactly once
 * (no zeroing by the caller):
 *     logz64 [B] (required), logz32 [B]   log Z_T
 *     len_logz [B, T + 1] float64         entry L = log of the total weight of the paths of exactly L arcs; entry 0 = -inf
 *                                         (0.0 for a lattice whose state 0 is the sink: its one path is the empty one);
 *                                         logsumexp over L = logz64, len_logz - logz64 = the length distribution under
 *                                         truncation at T
 *     pos_post [B, T, V] float32          sum over the arcs with label l of P(that arc is at position t)
 *                                         = d log Z_T / d pos[b, t, l]; zeros at positions no path reaches.  Summed as
 *                                         integers in units of 2^-44 (label_post of nfst_expectation): independent of
 *                                         the order, bit-identical from launch to launch
 *     arc_post [total_arcs] float32       sum_t P(arc a is at position t); 0 on self loops
 * Identities: sum_l pos_post[b, t, l] = P(L > t); pos_post[b, 0, bos] = 1; sum_t pos_post[b, t, l] = the sum of arc_post
 * over the arcs with label l; with pos = NULL and T >= the lattice's NFST_META_DEPTH logz64 and arc_post are
 * nfst_forward_backward's log Z and posterior.  A lattice without a path of finite score and L <= T gets logz = -inf,
 * len_logz = -inf and zero posteriors (never a NaN) and does not disturb the other lattices (nfst_expectation's rule).
 * Arithmetic: (float64 mantissa, int32 exponent) throughout, for every T (float32 mantissas repeat one rounding error
 * per label at every position); fixed summation order, no float atomics: every output is bit-identical from launch to
 * launch and for every packing of the same lattices.
 *
 * nfst_positional_viterbi (max-plus).  Plain float32 in a fixed order, from position T backwards:
 *     vb_T(sink) = 0, vb_T(s) = -inf for every other s;  vb_t(sink) = 0 for every t
 *     vb_t(s) = max over the out-arcs of s without self loops of  c = e_a + ((theta[l] + pos[b, t, l]) + vb_{t+1}(dst_a)),
 *     e_a as in nfst_kbest; without pos the inner add is absent: c = e_a + (theta[l] + vb_{t+1}(dst_a))
 *     best[b] = vb_0(0)
 * The path is read forwards from state 0: at position t the out-arc that attains vb_t(state), the smallest canonical arc
 * on exact ties (nfst_kbest's rule).  paths [B, T] int32 labels padded with `pad`, path_arcs (optional) [B, T] padded
 * with -1, lengths [B]; best = -inf gives length 0.  Without pos and with T >= depth: nfst_kbest's entry 0 bit for bit.
 *
 * Both read the canonical arrays only (row_ptr, arc_src, arc_dst, arc_label, arc_w): any batch, compact or not, with or
 * without chunked programs.  One workgroup per lattice advances all its states one position per step, T steps per
 * direction.
 * ws: device workspace of nfst_positional_ws_bytes(lat, T, flags) bytes (16-byte aligned, overwritten); every part is
 * rounded up to 256 bytes.  flags = 0 (log Z only): 12 bytes per arc.  NFST_POS_WS_POSTERIOR (any of len_logz, pos_post,
 * arc_post): + 12 * (T + 1) * total_rows -- EVERY beta row of every position is stored, (T + 1) * rows values per
 * lattice: this is the cost of the op -- + 20 bytes per arc + 4 per row.  NFST_POS_WS_VITERBI: 12 per arc +
 * 4 * (T + 1) * total_rows.
 * LDS: nfst_positional 24 max_rows + 20 vocab + 4112 bytes, nfst_positional_viterbi 8 max_rows + 4 vocab + 16 bytes; more
 * than 160 KiB returns NFST_ERR_LIMIT.  When 4 (max_rows + 1 + arcs of the largest lattice) + 16 more bytes fit, the arc
 * records are staged in LDS; otherwise the step loops read the canonical arrays (the same bits, slower steps).  Null required pointers, T < 1, a stride that is neither 0 nor T * vocab or a
 * short workspace return NFST_ERR_ARG.  All checks run on the host before any launch.
 *
 * nfst_positional_plan(lat, viterbi, lds_bytes, staged) is that decision, asked on the host (it touches no device and
 * takes a host-packed batch): for nfst_positional (viterbi = 0) or nfst_positional_viterbi (viterbi != 0) it writes the
 * dynamic LDS of the launch, arc records included, to *lds_bytes and 1 or 0 to *staged (either may be null) and returns
 * NFST_OK, or returns NFST_ERR_LIMIT exactly when the op itself would.  Both launchers call it: there is no second copy
 * of the rule.
 *
 * nfst_positional_sample (draws).  K exact draws per lattice from p_T(pi) = exp(S_T(pi)) / Z_T over the paths of at most
 * T arcs; paths, positions, pos, pos_stride, T and -inf entries are exactly those of nfst_positional.  The launch runs
 * the backward pass of nfst_positional with every beta row stored and NO forward pass (the same kernel: logz64 / logz32
 * are the bits nfst_positional writes for the same inputs), then one wave per walk, the grid over all B * K walks.
 * Walk (b, k) starts in state 0.  At position t in state s != sink it looks at the out-arcs of s without self loops, in
 * canonical order; arc a has
 *     p_a = w_t(a) beta_{t+1}(dst_a) / beta_t(s),     w_t(a) = exp(s_a + pos[b, t, label_a]),
 * in the arithmetic of the backward pass ((float64 mantissa, int32 exponent), exp_split64).  With u = uniforms[b, k, t]
 * (device float32 in [0, 1), shape [B, K, T]) the walk takes the FIRST arc whose running sum of w beta_{t+1} exceeds
 * u beta_t(s) -- compared without a division.  An arc of weight zero is never taken; if rounding leaves no arc above the
 * target, the last arc of positive weight is.  The walk ends at the sink.  beta_T(s) = 0 off the sink, so a walk never
 * needs more than T arcs: there is no status word and no NFST_ERR_LENGTH (nfst_sample_paths truncates; this does not).
 * uniforms = NULL: Philox4x32-10 exactly as nfst_sample_paths uses it (key = seed, counter = (walk, step / 4),
 * walk = b K + k, one block for four steps).  Outputs, every element written exactly once:
 *     paths [B, K, T] int32 labels padded with `pad`; path_arcs (optional) [B, K, T] canonical arc ids padded with -1;
 *     lengths [B, K];  logq [B, K] float32 = S_T(pi) - log Z_T, S summed in float64 from the float32 inputs and rounded
 *     once;  logz64 [B] (required), logz32 [B] (optional).
 * A lattice with log Z_T = -inf gets length 0, labels `pad`, arcs -1 and logq = 0 (so log p - log q stays -inf, never a
 * NaN) and does not disturb its neighbours.  The op reads the canonical arrays only and shares nothing between walks: the
 * same bits for every packing (staged or not, with or without chunked programs) and at every launch; walk (b, k) depends
 * on nothing but its own uniforms (not on K).
 * ws: nfst_positional_ws_bytes(lat, T, NFST_POS_WS_SAMPLE) = 12 bytes per arc + 12 * (T + 1) * total_rows: EVERY beta row
 * of every position, as NFST_POS_WS_POSTERIOR stores them (no checkpointing).  LDS and NFST_ERR_LIMIT: nfst_positional's,
 * through nfst_positional_plan; more than 2^31 - 1 walks (B * K; the walk is a 32-bit word of the Philox counter) also
 * return NFST_ERR_LIMIT.  k < 1, T < 1, a bad stride, null required pointers or a short workspace return NFST_ERR_ARG.
 * All checks run on the host before any launch.
 *
 * nfst_positional_score_paths (forced scores).  The forced walk of marks [B, K, T] (device int32, pad-terminated) from
 * state 0 under the same scores: the mark at position t takes the arc of the current state with that label and scores
 * s_a + pos[b, t, label].  The sink's pad loop scores nothing.
 *     path_score [B, K] float32   the float64 sum rounded once; -inf if a mark has no arc or an entry is -inf
 *     end_state [B, K]            the state reached; 0 if the walk fell off the lattice (nfst_score_paths' rule)
 *     lengths [B, K]              the marks before the first pad
 * With pos = NULL it is nfst_score_paths up to float32 rounding (that op adds an arc's terms in float32 first).
 * k < 1, T < 1, a bad stride or null pointers return NFST_ERR_ARG, k above 64 * 65535 NFST_ERR_LIMIT; on the host.
 *
 * nfst_positional_kbest (the k best paths).  Paths, positions, pos, pos_stride, T, -inf entries and e_a are exactly those
 * of nfst_positional_viterbi.  For every position t in [0, T] and state s a list of at most k float32 scores
 * v(t, s, r), r = 0, 1, ..:
 *     the sink holds the single entry 0.0f at every t; every other state has an empty list at t = T;
 *     for s != sink and t < T the list is the top k of the candidates (a, r), a over the out-arcs of s without self
 *     loops, r over the entries of the list of (t + 1, dst_a), with
 *         c = e_a + ((theta[l] + pos[b, t, l]) + v(t + 1, dst_a, r))      (without pos: c = e_a + (theta[l] + v))
 *     Only candidates with c > -inf count; the order is (c descending, canonical arc ascending, r ascending): the
 *     arithmetic of nfst_positional_viterbi and the rule of nfst_kbest.
 * The result is the list of (0, state 0); path j is read forwards from there by following (arc, rank).  Outputs on the
 * device, every element written exactly once:
 *     best [B, k] float32 path scores, best first;  paths [B, k, T] int32 labels padded with `pad`;  path_arcs (optional)
 *     [B, k, T] canonical arc ids padded with -1;  lengths [B, k] arcs per path;  n_paths [B] the number of real entries.
 * Entries j >= n_paths[b] have score -inf, length 0, labels `pad` and arcs -1.  No path exceeds T arcs: there is no
 * max_len and no status word.  A lattice without a path of finite score and L <= T has n_paths = 0 and does not disturb
 * its neighbours.  float32 addition is monotone, so the top k of a state depends only on the top k of its successors:
 * entry 0 is nfst_positional_viterbi's best, labels, arcs and length bit for bit; with pos = NULL and T >= the batch's
 * depth every output is nfst_kbest's bit for bit (the padded width aside); with pos = NULL and T below the depth the
 * result is nfst_kbest's list without the paths longer than T, in the same order and bits, as long as neither list is
 * truncated.  The op reads the canonical arrays only: the same bits for every packing, with or without chunked programs,
 * at every launch.  One workgroup per lattice, T barrier-separated steps; there is one launch flavour.  Only the pairs
 * (t, s) that state 0 reaches in exactly t arcs are swept (a forward pass marks them): no other list is ever read.
 * ws: device workspace of nfst_positional_kbest_ws_bytes(lat, T, k) bytes (16-byte aligned, overwritten, need not be
 * zeroed) = 8 * (T + 1) * total_rows * k (the lists) + (T + 1) * total_rows (the marks), each part rounded up to 256:
 * EVERY list of every position (no checkpointing, no lazy enumeration) -- 0.58 GB * k for the 516 236 rows of the
 * 256-lattice benchmark batch at T = 140.  LDS: 16 392 + 4 max_rows + 4 vocab bytes.
 * 1 <= k <= 64: k < 1 returns NFST_ERR_ARG, k > 64 NFST_ERR_LIMIT.  T < 1, a bad stride, null required pointers or a
 * short workspace return NFST_ERR_ARG; 2^24 or more arcs in one lattice (nfst_kbest's payload limit) or more than
 * 160 KiB of LDS return NFST_ERR_LIMIT.  All checks run on the host before any launch.
 *
 * nfst_positional_expectation (the first-order expectation semiring on the same sweeps).  Paths, positions, pos,
 * pos_stride, T and -inf entries are exactly those of nfst_positional; p_T(pi) = exp(S_T(pi) - log Z_T).  The arc at
 * position t of a path carries the value
 *     v_t(a) = pos_values[b, t, label_a]        (optional; [T, V] with stride 0 or [B, T, V] with stride T * vocab, as pos)
 *            + label_values[b, label_a]          (optional; [V] with stride 0 or [B, V] with stride vocab)
 *            + arc_values[a]                     (optional; [total_arcs])
 *            + score_coef * (s_a + pos[b, t, label_a])
 * summed in float64 from the float32 inputs, and V(pi) is the sum of v_t(a_t) over the path.  A term of weight zero (a
 * label, arc score or pos entry at -inf) has no value: its value entries are never multiplied in and may be +-inf or
 * NaN, and score_coef * s is left out for it.  Outputs on the device, every element written exactly once; logz64 and
 * ev64 are required, the rest optional:
 *     logz64 [B], logz32 [B], pos_post [B, T, V], arc_post [total_arcs]: the bits nfst_positional writes for the same
 *         inputs (the same sums in the same order; the expectation numerators ride beside the path mass under its
 *         exponent and never enter it)
 *     ev64 [B], ev32 [B]          E_{p_T}[V]
 *     pos_cov [B, T, V] float32   the sum over the arcs with label l of c_{a,t} = P(a at t) (E[V | a at t] - E[V])
 *     arc_cov [total_arcs] float32  the sum over t of c_{a,t}; 0 on self loops
 * sum pos_cov = sum arc_cov = Cov(L, V).  With score_coef = 1 alone H(p_T) = log Z_T - E[V] and dH/d(score) = -c; for
 * values that do not depend on the scores pos_cov = d E[V] / d pos = (Hessian of log Z_T) v.  With pos = pos_values =
 * NULL and T >= the batch's depth, log Z, E[V], arc_post and arc_cov are nfst_expectation's logz64, ev64, posterior
 * and cov up to rounding.  A lattice without a path of finite score and L <= T gets log Z = -inf, E[V] = 0 and zeros
 * everywhere (never a NaN) and does not disturb its neighbours.
 * pos_cov is accumulated per label with float64 LDS atomics: the order of its adds is NOT fixed (as label_cov of
 * nfst_expectation), so its last bits may differ from launch to launch.  Every other output is bit-identical from
 * launch to launch and for every packing; only the canonical arrays are read.
 * ws: nfst_positional_expectation_ws_bytes(lat, T) bytes (16-byte aligned, overwritten), every part rounded up to 256:
 * 20 * (T + 1) * total_rows -- EVERY (beta, R) row of every position, (float64, int32, float64): the cost of the op, no
 * checkpointing -- + 48 bytes per arc + 4 per row.
 * LDS: 40 max_rows + 36 vocab + 4112 bytes; more than 160 KiB returns NFST_ERR_LIMIT.  When 4 (max_rows + 1 + arcs of
 * the largest lattice) + 16 more bytes fit, the arc records are staged in LDS, otherwise the step loops read the
 * canonical arrays (the same bits, slower steps).  nfst_positional_expectation_plan(lat, lds_bytes, staged) is that
 * decision, asked on the host as nfst_positional_plan; the launcher calls it.  Null required pointers, T < 1, a stride
 * that is neither 0 nor the full one, a non-finite score_coef or a short workspace return NFST_ERR_ARG.  All checks run
 * on the host before any launch.
 *
 * nfst_positional_swor (draws without replacement).  k distinct paths per lattice drawn without replacement from
 * p_T(pi) = exp(S_T(pi) - log Z_T) over the paths of at most T arcs; paths, positions, pos, pos_stride, T, -inf entries
 * and pos = NULL are exactly those of nfst_positional.  The launch runs the backward pass of nfst_positional with every
 * beta row stored, as nfst_positional_sample does (logz64 / logz32 are the bits nfst_positional writes), then the search
 * of nfst_swor on the caller's stream, one workgroup per lattice: the same kernel in a second flavour.  Every rule of
 * nfst_swor holds as written there -- at most k slots in flat order, the conditioning on the parent's perturbed score
 * with the first-holder rule, ties to the earlier flat index, kappa the largest G~ ever dropped, the final ranking by
 * (G desc, slot asc), x = u + 2^-25, all arithmetic in float64 -- with max_len = T (uniforms [B, T, k, max_degree], or
 * Philox with the counter (b, t, j, r)) and two differences.  For slot j at state s and arc a at step t:
 *     S' = (S_j + (double)e_a) + (double)pos[b, t, label_a]      (e_a: nfst_swor's float32 arc score; without pos: S_j + e_a)
 *     phi = S' + log beta_{t+1}(dst_a) - Z
 * where beta_{t+1} is the (float64 mantissa m, int32 exponent e) row the backward pass stored, read as log(m) + e ln 2
 * (-inf at m = 0), and Z = logz64[b] as the same launch wrote it.  The budget needs no rule of its own: beta_T is 0 off
 * the sink, so a candidate that cannot finish within T arcs has phi = -inf and is dropped; the search ends within T
 * steps and there is no NFST_ERR_LENGTH.  *status (device, one word, zeroed by the caller) only reports uniforms narrower
 * than an out-degree (NFST_ERR_ARG, the candidate is dropped).  Outputs: paths and path_arcs (optional) [B, k, T], lengths,
 * logp = (float)(S - Z), gumbel [B, k], kappa, n_paths [B], as nfst_swor; a lattice with log Z_T = -inf looks like
 * nfst_swor's empty lattice and does not disturb its neighbours.  The op reads the canonical arrays only and uses no
 * atomics: the same bits at every launch, for every packing and, with given uniforms, wherever the lattice sits in the batch.
 * ws: nfst_positional_swor_ws_bytes(lat, T, k) bytes (16-byte aligned, overwritten): the NFST_POS_WS_SAMPLE parts of
 * nfst_positional_ws_bytes, then the parts of nfst_swor_ws_bytes(lat, k, T) (back pointers [B, T, k], the key spill when
 * k * vocab exceeds nfst_beam_lds_candidates()), every part rounded up to 256.  LDS and NFST_ERR_LIMIT: nfst_positional's,
 * through nfst_positional_plan; k > 64 also returns NFST_ERR_LIMIT.  k < 1, T < 1, a bad stride, uniforms with
 * max_degree < 1, null required pointers (logz32 and path_arcs are optional) or a short workspace return NFST_ERR_ARG.
 * All checks run on the host before any launch.
 */
#define NFST_POS_WS_POSTERIOR 1
#define NFST_POS_WS_VITERBI 2
#define NFST_POS_WS_SAMPLE 8 /* 12 bytes per arc + 12 (T + 1) total_rows: every beta row of every position */
int64_t nfst_positional_ws_bytes(const nfst_batch *lat, int32_t T, int32_t flags);
int nfst_positional_sample(const nfst_batch *lat, const nfst_scores *scores, const float *pos, int64_t pos_stride, int32_t T,
                           int32_t k, const float *uniforms, uint64_t seed, int32_t pad, void *ws, int64_t ws_bytes, double *logz64,
                           float *logz32, int32_t *paths, int32_t *path_arcs, int32_t *lengths, float *logq, void *stream);
int nfst_positional_score_paths(const nfst_batch *lat, const nfst_scores *scores, const float *pos, int64_t pos_stride, int32_t T,
                                const int32_t *marks, int32_t k, float *path_score, int32_t *end_state, int32_t *lengths,
                                void *stream);
int64_t nfst_positional_swor_ws_bytes(const nfst_batch *lat, int32_t T, int32_t k);
int nfst_positional_swor(const nfst_batch *lat, const nfst_scores *scores, const float *pos, int64_t pos_stride, int32_t T, int32_t k,
                         const float *uniforms, int32_t max_degree, uint64_t seed, int32_t pad, void *ws, int64_t ws_bytes,
                         double *logz64, float *logz32, int32_t *paths, int32_t *path_arcs, int32_t *lengths, float *logp,
                         double *gumbel, double *kappa, int32_t *n_paths, int32_t *status, void *stream);
int nfst_positional_plan(const nfst_batch *lat, int32_t viterbi, int64_t *lds_bytes, int32_t *staged);
int nfst_positional(const nfst_batch *lat, const nfst_scores *scores, const float *pos, int64_t pos_stride, int32_t T, void *ws,
                    int64_t ws_bytes, double *logz64, float *logz32, double *len_logz, float *pos_post, float *arc_post,
                    void *stream);
int nfst_positional_viterbi(const nfst_batch *lat, const nfst_scores *scores, const float *pos, int64_t pos_stride, int32_t T,
                            void *ws, int64_t ws_bytes, float *best, int32_t *paths, int32_t *path_arcs, int32_t *lengths,
                            int32_t pad, void *stream);
int64_t nfst_positional_expectation_ws_bytes(const nfst_batch *lat, int32_t T);
int nfst_positional_expectation_plan(const nfst_batch *lat, int64_t *lds_bytes, int32_t *staged);
int nfst_positional_expectation(const nfst_batch *lat, const nfst_scores *scores, const float *pos, int64_t pos_stride, int32_t T,
                                const float *pos_values, int64_t pos_values_stride, const float *label_values,
                                int64_t label_values_stride, const float *arc_values, float score_coef, void *ws, int64_t ws_bytes,
                                double *logz64, float *logz32, double *ev64, float *ev32, float *pos_post, float *arc_post,
                                float *pos_cov, float *arc_cov, void *stream);
int64_t nfst_positional_kbest_ws_bytes(const nfst_batch *lat, int32_t T, int32_t k);
int nfst_positional_kbest(const nfst_batch *lat, const nfst_scores *scores, const float *pos, int64_t pos_stride, int32_t T, int32_t k,
                          void *ws, int64_t ws_bytes, float *best, int32_t *paths, int32_t *path_arcs, int32_t *lengths,
                          int32_t *n_paths, int32_t pad, void *stream);

/*
 * Viterbi: best[b] = max path score (float32), paths [B, max_len] int32 labels
 * of the best path (bos .. eos) padded with `pad`, lengths [B]; path_arcs
 * (optional) canonical arc ids, -1 padded.  Ties keep the smallest label.
 * The score is a float32 sum built from the sink (0.0f) backwards; arc a from s to d gives the candidate
 *     general kernel:    c = e_a + (theta[label_a] + v(d)),  e_a = 0.0f (+ arc_w[a] if weighted) (+ arc_scores[a] if given)
 *     tile-wave kernel:  c = v(d) + (theta[label_a] + e_a),  e_a = arc_w[a] + arc_scores[a], arc_w[a] or arc_scores[a]
 * (all-compact batches run the tile-wave kernel; without arc_w and arc_scores both are theta[label_a] + v(d)), and
 * v(s) is the largest candidate of s, the smaller canonical arc on exactly tied candidates.  Self loops are on no path.
 * A lattice without a path of finite score (labels at -inf on every path) gets best = -inf, length 0, labels all
 * `pad` and arcs all -1: entry 0 of nfst_kbest for such a lattice.  A path longer than max_len gets length -1.
 * The general kernel keeps 12 bytes per row and 4 per label in LDS: a batch it has to run (not all-compact, or too
 * large for the tile-wave ring) with 12 max_rows + 4 vocab + 16 > 160 KiB returns NFST_ERR_LIMIT before any launch.
 */
int nfst_viterbi(const nfst_batch *lat, const nfst_scores *scores, float *best, int32_t *paths,
                 int32_t *path_arcs, int32_t *lengths, int32_t max_len, int32_t pad,
                 void *stream);

/*
 * Exact posterior path sampling: K walks per lattice from state 0; at state s
 * arc a is taken with probability exp(score[a] + beta[dst] - beta[s]), chosen by
 * inverse CDF over the state's arcs in label order from uniforms [B, K, max_len]
 * (device float32 in [0,1)); if uniforms is NULL a Philox4x32-10 stream is used
 * (key = seed, counter = (walk, step / 4): one output word per step).  paths [B, K, max_len] labels padded with `pad`,
 * path_arcs (optional) canonical arc ids, lengths [B, K], logq [B, K] =
 * path score - log Z.  status (device int32, one word, zeroed by the caller)
 * becomes NFST_ERR_LENGTH if a walk does not reach the sink within max_len.
 */
int nfst_sample_paths(const nfst_batch *lat, const nfst_scores *scores, const float *beta_me,
                      const double *logz64, int32_t k, int32_t max_len, const float *uniforms,
                      uint64_t seed, int32_t pad, int32_t *paths, int32_t *path_arcs,
                      int32_t *lengths, float *logq, int32_t *status, void *stream);

/*
 * Forced walk of marks [B, K, max_len] (pad-terminated) from state 0:
 * path_score [B, K] = sum of arc scores (-inf if a mark has no arc),
 * end_state [B, K] (0 if the walk fell off the lattice, like the dense gather).
 */
int nfst_score_paths(const nfst_batch *lat, const nfst_scores *scores, const int32_t *marks,
                     int32_t k, int32_t max_len, float *path_score, int32_t *end_state,
                     void *stream);

/* state' = transition[state, label] for N = B*K walkers (walker n belongs to
 * lattice n / k); 0 where the arc does not exist.  int64 in/out like the
 * reference's LongTensors. */
int nfst_step(const nfst_batch *lat, const int64_t *state, const int64_t *label, int64_t *next,
              int32_t k, void *stream);

/* out [B*K, V] float32: 0 (or the table's weight) where the walker's state has
 * an arc with that label, -inf elsewhere.  If inp != NULL (the previously
 * emitted mark per walker) the legality masks of LeftToRightScorer.mask_out_invalid
 * (scorers.py:59-83, 314-338) are added in the same pass: bos never, pad only
 * after eos/pad, and -- when has_to_end -- only eos for walkers that have not
 * ended: the whole of FSAGRUScorer.mask_out_invalid in one kernel. */
int nfst_emission_mask(const nfst_batch *lat, const int64_t *state, const int64_t *inp,
                       int32_t pad, int32_t bos, int32_t eos, int32_t has_to_end, float *out,
                       int32_t k, void *stream);

/* out [B*K, V] = values[row_off(b) + transition[state, label]] with values a
 * row-indexed float32 array (beta in the probability domain in the reference,
 * any row-indexed array here); labels without an arc read row 0 like the dense
 * gather does. */
int nfst_beta_logits(const nfst_batch *lat, const float *values, const int64_t *state,
                     float *out, int32_t k, void *stream);

/*
 * Optional operands of nfst_proposal_step (zero-initialise; NULL pointers switch a part off).
 *   value_state [N]: the state whose transition row the `values` gather reads.  The reference gathers
 *     its beta "logits" from the state BEFORE the previous symbol was consumed (scorers.py:584-590 run
 *     inside super().actual_left_to_right_score, the advance is line 679) while the masks use the state
 *     after it: pass the previous step's `state` here to reproduce that (pinned by
 *     tests/golden/sampler_beta.npz); NULL = gather from `state`.
 *   accumulated [N] int64, vocab_use [N, V] float32 (in/out, zeroed by the caller before the first
 *     step): the counters of scorers.py:654-661, updated with the previous symbol `inp` first; then
 *       scores[:, insertion_mark] -= insert_penalty * (length - insert_threshold)
 *           where accumulated > insert_threshold             (if insert_threshold > 0; 663-669)
 *       scores -= vocab_use * length_penalty                  (if 0 < length_threshold < length; 671-677)
 *     `length` is the step's metadata["length"] (1 at the first step).
 *   not_pad: device int32 word (zeroed by the caller): the launch adds the number of walkers whose symbol is
 *     not `pad` -- zero means "every walker has ended" (Sampler.all_reached_eos, samplers.py:288-290) without a
 *     reduction kernel; a sampling loop reads it every few steps instead of synchronising with the device at
 *     every step.
 */
typedef struct nfst_step_extras {
  const int64_t *value_state;
  int64_t *accumulated;
  float *vocab_use;
  int32_t insertion_mark;
  int32_t insert_threshold;
  float insert_penalty;
  int32_t length_threshold;
  float length_penalty;
  int32_t length;
  int32_t *not_pad;
} nfst_step_extras;

/*
 * Fused lattice side of one proposal-sampler step (Sampler.stateful_sample, samplers.py:243-297;
 * left_to_right_score, scorers.py:340-366; mask_out_invalid, 1037-1054 + 59-83; beta-logit gather,
 * 581-593; penalties, 654-677; update_fsa_state, 683-690): for every walker n (lattice n / k)
 *   logits = (pad_masking(scores[n, :] [+ values[next state]] [- penalties]) + emission row + legality masks) / temperature
 *   symbol = forced[n], or the first mark (in id order) whose CDF exceeds uniforms[n]
 *   logq = logits[symbol] - logsumexp(logits), logz = that logsumexp (optional), next_state as nfst_step.
 * `state` is the state after the previous symbol `inp` was consumed.  inp may be NULL: no bos / pad /
 * eos legality masks and no counters then.  values is row-indexed [total_rows] (e.g. beta in the domain
 * the caller's scorer expects) or NULL.  extras may be NULL.  logits_out (optional, [N, V]) receives the
 * masked, scaled logits: what nfst_proposal_step_backward needs.  vocab <= 4096 (<= 3413 with
 * values and extras->value_state: four walkers x three rows of vocab words must fit 160 KiB of LDS); a larger
 * vocabulary returns NFST_ERR_LIMIT before any launch.
 */
int nfst_proposal_step(const nfst_batch *lat, const int64_t *state, const int64_t *inp, const float *scores,
                       const float *values, int32_t pad, int32_t bos, int32_t eos, int32_t has_to_end, float temperature,
                       const float *uniforms, const int64_t *forced, const nfst_step_extras *extras, int64_t *symbol,
                       float *logq, float *logz, int64_t *next_state, float *logits_out, int32_t k, void *stream);

/*
 * Backward of nfst_proposal_step: the reference's Categorical.log_prob is differentiable in the
 * proposal's logits (samplers.py:256-273; tune_proposal, lightning.py:339-406).  From the logits the
 * forward pass wrote: grad_scores [N, V] = (g_logq * (onehot(symbol) - softmax) + g_logz * softmax) /
 * temperature for legal marks other than pad, 0 elsewhere (g_logq, g_logz [N]; either may be NULL).
 * grad_values (optional, [total_rows], zeroed by the caller) accumulates the same numbers through the
 * next-state gather out of value_state (float atomics: the summation order is not fixed).
 */
int nfst_proposal_step_backward(const nfst_batch *lat, const int64_t *value_state, const float *logits,
                                const int64_t *symbol, const float *logz, const float *g_logq, const float *g_logz,
                                int32_t pad, float temperature, float *grad_scores, float *grad_values, int32_t k,
                                void *stream);

/*
 * Neuralised beta: FSAGRUScorer.compute_beta_per_sample with Wh != 0
 * (modules/scorers.py:692-751; compute_beta_parallel, 753-856, is the same
 * recurrence).  For every arc (s, l, s') with s' != s
 *     t   = tanh(label_x[l] + Wh . beta_hat(s')),  label_x[l] = Wx . e(l) + bias
 *     msg = exp(w . t (+ arc_w)) * beta(s')
 *     beta(s) = sum msg,  beta_hat(s) = sum (msg / beta(s)) t;  beta(sink) = 1, beta_hat(sink) = 0.
 * label_x: device float32 [vocab, hid]; wh: Wh as the reference holds it, [hid (out),
 * hid (in)] row-major; w: [hid]; hid <= 512.  Outputs: log_beta [total_rows] (natural log;
 * the reference returns exp of it), beta_hat [total_rows, hid].  ws: device
 * workspace of nfst_neural_ws_floats() floats, contents irrelevant.
 * LDS: 8 bytes per row (max_rows rounded up to even), two staged tiles, 32 rows of beta_hat and three bfloat16 planes of
 * 16 rows: with S = ((hid + 15) & ~15) + 4,  8 max_rows + 5152 + 128 S + 96 (hid + 8) bytes (the part in front of the
 * planes rounded up to 16), whatever kernel hid selects.  More than 160 KiB returns NFST_ERR_LIMIT before any launch
 * but the packing of Wh (hid a multiple of 64 from 256 on): max_rows <= 5340 at hid = 512, 7132 at 448; up to
 * hid = 402 every batch (8191 rows) fits.
 */
int64_t nfst_neural_ws_floats(const nfst_batch *lat, int32_t hid);
int nfst_backward_neural(const nfst_batch *lat, const float *label_x, const float *wh, const float *w,
                         int32_t hid, float *log_beta, float *beta_hat, float *ws, void *stream);

/*
 * Gradient of nfst_backward_neural: tune_proposal differentiates log q through compute_beta()
 * (modules/lightning.py:339-406) w.r.t. Wh, Wx, W, beta_bias and the embeddings
 * (scorers.py:954-970).  Inputs: the forward call's label_x, w, beta_hat and workspace (ws_fwd,
 * untouched since), wh_t = Wh transposed ([hid (in), hid (out)] row-major), g_log_beta
 * [total_rows] = dL / d log_beta, g_beta_hat [total_rows, hid] = dL / d beta_hat or NULL.
 * Outputs: grad_label_x [vocab, hid] and grad_w [hid] ACCUMULATE (float atomics: the caller zeroes
 * them, the summation order is not fixed); gamma [total_rows, hid] (zeroed by the caller) receives
 * dL / d (Wh . beta_hat(s)) per state, so that dL/dWh = gamma^T . beta_hat is one library GEMM on
 * the caller's side.  dL/dWx, dL/dbias and dL/d embeddings follow from grad_label_x through
 * label_x = emb . Wx^T + bias.  ws: nfst_neural_grad_ws_floats() floats, contents irrelevant.
 * LDS, hid > 32: the forward call's rows and planes, 4 more bytes per row (max_rows rounded up to a multiple of 4) and
 * wider staged tiles:  8 max_rows + 4 max_rows + 7216 + 128 S + 96 (hid + 8) bytes.  hid <= 32:  8 max_rows +
 * 4 max_rows + 7216 bytes, and for hid <= 8 a [vocab, hid] float table of dL/dx beside them while it fits (global
 * atomics otherwise).  More than 160 KiB returns NFST_ERR_LIMIT before any launch but the packing of wh_t.  The limit
 * is lower than the forward call's -- max_rows <= 3388 against 5340 at hid = 512, 5776 at 384, every batch only up
 * to hid = 252 -- so a batch between the two runs nfst_backward_neural and is refused here.
 */
int64_t nfst_neural_grad_ws_floats(const nfst_batch *lat, int32_t hid);
int nfst_backward_neural_grad(const nfst_batch *lat, const float *label_x, const float *wh_t, const float *w,
                              int32_t hid, const float *beta_hat, const float *ws_fwd, const float *g_log_beta,
                              const float *g_beta_hat, float *gamma, float *grad_label_x, float *grad_w,
                              float *ws, void *stream);

/* out[a] = theta[(theta_stride * b) + label[a]] (+ arc_w[a]) (+ arc_scores[a]) */
int nfst_gather_label_scores(const nfst_batch *lat, const nfst_scores *scores, float *out,
                             void *stream);

/*
 * Fused log_softmax + gather + mask-sum over sequences: scores [N, T, V] float32,
 * marks [N, T] int64, out [N] float32.
 * mask_mode NFST_MASK_STATICRNN -- StaticRNNScorer.evaluate_seq_with_temp (scorers.py:1564-1611):
 * masks as in scorers.py:89-134: bos/pad illegal, after eos/pad only pad, beyond
 * max_length only eos (max_length < 0 disables); the pad column of scores is
 * zeroed (pad_masking_3d, scorers.py:189-192); positions holding pad contribute
 * 0.  normalize = 0 skips the log_softmax (self_normalized = False).
 * smoothing in [0,1): 0 = evaluation (gather of the realised mark); > 0 = the
 * training branch (scorers.py:1502-1528, 1584-1592): weight 1 - smoothing on the
 * realised mark, smoothing / (legal marks - 1) on the other legal marks, values
 * clamped to +-1e9.
 * mask_mode NFST_MASK_GPT2 -- GPT2Wrapper.forward (modules/transformer.py:45-52): scores are
 * the language model's logits for the bos-shifted input, marks is gold_x (the sequence with one
 * trailing pad); the pad logit is replaced by -1e8, there are no legality masks, positions
 * holding pad contribute 0 (bos, eos, max_length are ignored; temp = 1, normalize = 1 there).
 */
#define NFST_MASK_STATICRNN 0
#define NFST_MASK_GPT2 1
int nfst_path_logprob(const float *scores, const int64_t *marks, int64_t n, int32_t t,
                      int32_t vocab, int32_t pad, int32_t bos, int32_t eos, int32_t max_length,
                      float temp, int32_t normalize, float smoothing, int32_t mask_mode, float *out,
                      void *stream);

/*
 * Backward of nfst_path_logprob: grad_scores [N, T, V] = grad_out[n] * d out[n] / d scores[n, t, v]
 * (every element is written).  The reference trains p~ straight through this op:
 * p_loss = -(num_prob - denom_prob).mean() (modules/lightning.py:511-516) back-propagates through
 * evaluate_seq_with_temp.  Per row: (target - softmax * sum(target)) / temp with the one-hot or
 * label-smoothed target; the pad column and rows whose mark is pad get 0.  The row is recomputed
 * from scores (nothing is saved by the forward pass): N T V 4 bytes read, as many written.
 */
int nfst_path_logprob_backward(const float *scores, const int64_t *marks, const float *grad_out, int64_t n,
                               int32_t t, int32_t vocab, int32_t pad, int32_t bos, int32_t eos,
                               int32_t max_length, float temp, int32_t normalize, float smoothing,
                               int32_t mask_mode, float *grad_scores, void *stream);

/* log_w [B,K] = log_p - log_q ; log_marginal [B] = logsumexp_k(log_w) - log K (-inf for a row whose log_w are all -inf) */
int nfst_iwae(const float *log_p, const float *log_q, int32_t b, int32_t k, float *log_w,
              float *log_marginal, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NFST_HIP_H */

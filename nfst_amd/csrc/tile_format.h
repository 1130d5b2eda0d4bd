// tile_format.h -- the tile-program format, defined once for the host packer (pack.cpp), the device
// packer (pack_kernels.h), the batch checks and concatenation (pack.cpp) and every kernel that reads a program.  Plain
// constants and inline functions, host + device: both packers must lay out the same bytes.
//
// A sweep direction of a lattice is a "tile program": a sequence of fixed-size tiles, each one wave-wide unit of work --
// 64 control words and 64*U arc records (U = 1, 2 or 4 slots per lane).  A state with d arcs takes 2^g lanes,
// g = ceil(log2(ceil(d/U))), at a lane offset that is a multiple of 2^g; lane r of the group owns records [r*U, r*U+U).
// Tiles never mix levels, so every record's operand was produced by an earlier tile.
//
// A state whose arcs do not fit the largest group (2^max_g lanes) is cut into pieces that go into successive tiles: every
// continuation piece starts with a CARRY record (operand = the state itself, label = vocab + 1, weight one), so its sum
// includes what the earlier pieces stored and the piece simply overwrites the state's value.  Its leader lane also carries
// the "accumulate" flag (the max-plus kernel keeps the earlier back pointer when the carry wins).  max_g = 3 ("narrow":
// groups of up to 8 lanes, the sweep needs no cross-row reduction stage) or 6 ("wide": up to the whole wave).  In a narrow
// program a state with more than two groups' worth of arcs is summed as a tree instead of a chain: its arcs are spread over
// PARTIAL groups that write scratch rows (ids from n_rows up, reused from level to level) -- up to eight of them side by
// side in one tile -- and a chain of COMBINE pieces in later tiles adds the scratch rows up with unit-label records.
//
// control word: [0:16) 8 x state id (the byte offset of its value in the alpha / beta array)
//               [20:23) g: the state's lanes are the 2^g-aligned group of 2^g lanes
//               [23:26) largest g in this tile (same in every lane)
//               [26] the tile holds a continuation piece (same in every lane)
//               [30] continuation piece (its first record is the carry)  [31] leader lane
//               (stores the state's sum)
// record:       [0:16) 8 x operand state | [16:32) label (vocab = the null label: weight 0,
//               vocab + 1 = the unit label of a carry or combine record: weight 1)
// compact tile (format code 8): U = 4 and labels < 2048; 16 bytes per lane = control word + four 24-bit records
//               (state 13 bits | label 11 bits) packed into three words -- one 16-byte LDS-DMA per lane and tile
// meta format word (NFST_META_FWD_U / _BWD_U): format code (1, 2, 4: slots per lane with 32-bit records after a block of
//               64 control words; 8: compact) | 1 << 8 when the program has groups wider than 8 lanes
#pragma once

#include <stdint.h>

#if defined(__HIP__)
#define NFST_HD __attribute__((host)) __attribute__((device))
#else
#define NFST_HD
#endif

namespace nfst_tile {

constexpr int64_t kStreamSlack = 512;  // zero words behind each stream: an empty last lattice still owns valid memory
constexpr int kArcSpare = 8;           // zero entries behind arc_sd and arc_l16
constexpr int kNarrowG = 3, kWideG = 6;  // largest group of a narrow / wide program: 8 / 64 lanes
constexpr int kFmtCompact = 8;         // format code of the compact tile
constexpr int kCompactLabels = 2048;   // the compact tile holds vocab + 2 labels (null and unit label included) up to this
constexpr int64_t kMaxOffset = 0x7ffff000;  // largest element count of every array of a batch (offsets are int32)

// ---- format code, meta format word
NFST_HD constexpr int fmt_u(int F) { return F == kFmtCompact ? 4 : F; }                       // slots per lane
NFST_HD constexpr int fmt_words(int F) { return F == kFmtCompact ? 256 : 64 * (1 + F); }     // words per tile
NFST_HD constexpr int32_t meta_fmt(bool compact, int U, bool wide) { return (compact ? kFmtCompact : U) | ((wide ? 1 : 0) << 8); }
NFST_HD constexpr int meta_code(int32_t w) { return w & 0xff; }
NFST_HD constexpr int meta_wide(int32_t w) { return (w >> 8) & 1; }

// ---- control word
NFST_HD constexpr uint32_t ctl_word(uint32_t state, uint32_t g, bool leader, bool accum) {
  return (state << 3) | (g << 20) | (leader ? (1u << 31) | (accum ? (1u << 30) : 0u) : 0u);
}
NFST_HD constexpr uint32_t ctl_tile_bits(uint32_t gmax, bool any_accum) { return (gmax << 23) | (any_accum ? (1u << 26) : 0u); }
NFST_HD constexpr uint32_t ctl_state(uint32_t c) { return (c & 0xffffu) >> 3; }
NFST_HD constexpr uint32_t ctl_g(uint32_t c) { return (c >> 20) & 7u; }
NFST_HD constexpr uint32_t ctl_gmax(uint32_t c) { return (c >> 23) & 7u; }
NFST_HD constexpr bool ctl_accum(uint32_t c) { return ((c >> 30) & 1u) != 0; }
NFST_HD constexpr bool ctl_leader(uint32_t c) { return (c >> 31) != 0; }

// ---- records: 32-bit, compact 24-bit, and a compact lane's three record words
NFST_HD constexpr uint32_t rec32(uint32_t state, uint32_t label) { return (state << 3) | (label << 16); }
NFST_HD constexpr uint32_t rec32_state(uint32_t r) { return (r & 0xffffu) >> 3; }
NFST_HD constexpr uint32_t rec32_label(uint32_t r) { return r >> 16; }
NFST_HD constexpr uint32_t rec24(uint32_t state, uint32_t label) { return state | (label << 13); }
NFST_HD constexpr uint32_t rec24_state(uint32_t r) { return r & 0x1fffu; }  // (bits above 24 are ignored)
NFST_HD constexpr uint32_t rec24_label(uint32_t r) { return (r >> 13) & 0x7ffu; }
NFST_HD constexpr uint32_t rec24_to_32(uint32_t r) { return rec32(rec24_state(r), rec24_label(r)); }
// the decoders' forms: 8 x state (the byte offset of its value in the alpha / beta array), 8 x label
NFST_HD constexpr uint32_t ctl_off8(uint32_t c) { return c & 0xffffu; }
NFST_HD constexpr uint32_t rec32_off8(uint32_t r) { return r & 0xffffu; }
NFST_HD constexpr uint32_t rec32_label8(uint32_t r) { return (r >> 16) << 3; }
NFST_HD constexpr uint32_t rec24_off8(uint32_t r) { return (r << 3) & 0xfff8u; }
NFST_HD constexpr uint32_t rec24_label8(uint32_t r) { return (r >> 10) & 0x3ff8u; }
NFST_HD inline void pack24(const uint32_t (&r)[4], uint32_t &w1, uint32_t &w2, uint32_t &w3) {
  w1 = r[0] | (r[1] << 24);
  w2 = (r[1] >> 8) | (r[2] << 16);
  w3 = (r[2] >> 16) | (r[3] << 8);
}
// r[0 .. 2] keep the bits of the next record above bit 24: the decoders above mask them
NFST_HD inline void unpack24(uint32_t w1, uint32_t w2, uint32_t w3, uint32_t (&r)[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
  r[0] = w1; r[1] = __builtin_amdgcn_alignbit(w2, w1, 24); r[2] = __builtin_amdgcn_alignbit(w3, w2, 16); r[3] = w3 >> 8;
#else
  r[0] = w1; r[1] = (w1 >> 24) | (w2 << 8); r[2] = (w2 >> 16) | (w3 << 16); r[3] = w3 >> 8;
#endif
}
// state and label of a compact lane's four records, one bit-field extract each: only record 1's state and record 2's label
// straddle a word.  (Device: the extracts are opaque to the compiler, which otherwise folds the shift that follows -- times
// 8 or 16, plus an array's base: one shift-and-add -- into a shift, a mask and an add.)
NFST_HD inline void unpack24_fields(uint32_t w1, uint32_t w2, uint32_t w3, uint32_t (&state)[4], uint32_t (&label)[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
#define NFST_BFE(D, X, OFF, W) asm("v_bfe_u32 %0, %1, %2, %3" : "=v"(D) : "v"(X), "n"(OFF), "n"(W))
  const uint32_t r1 = __builtin_amdgcn_alignbit(w2, w1, 24), r2 = __builtin_amdgcn_alignbit(w3, w2, 16);
  NFST_BFE(state[0], w1, 0, 13);  NFST_BFE(label[0], w1, 13, 11);
  NFST_BFE(state[1], r1, 0, 13);  NFST_BFE(label[1], w2, 5, 11);
  NFST_BFE(state[2], w2, 16, 13); NFST_BFE(label[2], r2, 13, 11);
  NFST_BFE(state[3], w3, 8, 13);  NFST_BFE(label[3], w3, 21, 11);
#undef NFST_BFE
#else
  uint32_t r[4];
  unpack24(w1, w2, w3, r);
  for (int j = 0; j < 4; ++j) { state[j] = rec24_state(r[j]); label[j] = rec24_label(r[j]); }
#endif
}

// ---- pieces of a state.  cap = records of the largest group; a chain's first piece takes cap records, every
// continuation piece one less (its carry).  Pass k of a level holds the k-th piece of every state of the level: a chain's
// pieces are passes 0, 1, ...; a tree's partial groups are pass 0 and its combine chain passes 1, 2, ...
NFST_HD inline int ceil_log2(int x) { return x <= 1 ? 0 : 32 - __builtin_clz(x - 1); }
NFST_HD inline int group_cap(int max_g, int U) { return (1 << max_g) * U; }
struct Shape {
  int row, b0, e0;  // the state; arcs [b0, e0) of its list
  int n_part;       // partial groups of a tree (0: a chain)
  int first;        // scratch row of its first partial group
};
NFST_HD inline int tree_parts(int deg, int max_g, int cap) { return (max_g == kNarrowG && deg > 2 * cap) ? (deg + cap - 1) / cap : 0; }
NFST_HD inline int chain_pieces(int len, int cap) { return len <= cap ? 1 : 1 + (len - 2) / (cap - 1); }
NFST_HD inline int state_passes(const Shape &st, int cap) { return st.n_part ? 1 + chain_pieces(st.n_part, cap) : chain_pieces(st.e0 - st.b0, cap); }
NFST_HD inline int state_pieces(const Shape &st, int cap) { return st.n_part ? st.n_part + chain_pieces(st.n_part, cap) : chain_pieces(st.e0 - st.b0, cap); }
NFST_HD inline int pass_pieces(const Shape &st, int pass) { return st.n_part && pass == 0 ? st.n_part : 1; }

struct Piece {
  int row;         // receives the sum (a scratch row for a partial group)
  int begin, end;  // records [begin, end) of the state's arc list, or scratch rows [begin, end) for a combine piece
  int accum;       // continuation piece: starts with the carry record
  int units;       // combine piece: unit-label records of scratch rows
  int g;           // the piece's group has 2^g lanes
};
// the c-th piece of a chain over [b, e)
NFST_HD inline void chain_piece(int b, int e, int c, int cap, int &pb, int &pe) {
  pb = c == 0 ? b : b + cap + (c - 1) * (cap - 1);
  pe = pb + (c == 0 ? cap : cap - 1);
  pe = e < pe ? e : pe;
}
// the piece of pass `pass` of a state (`sub`: the partial group, in pass 0 of a tree)
NFST_HD inline Piece piece(const Shape &st, int pass, int sub, int cap, int U) {
  Piece p;
  if (st.n_part && pass == 0) {
    p.row = st.first + sub; p.begin = st.b0 + sub * cap; p.end = p.begin + cap; p.end = st.e0 < p.end ? st.e0 : p.end;
    p.accum = 0; p.units = 0;
  } else if (st.n_part) {
    chain_piece(st.first, st.first + st.n_part, pass - 1, cap, p.begin, p.end);
    p.row = st.row; p.accum = pass > 1; p.units = 1;
  } else {
    chain_piece(st.b0, st.e0, pass, cap, p.begin, p.end);
    p.row = st.row; p.accum = pass > 0; p.units = 0;
  }
  const int lanes = (p.end - p.begin + p.accum + U - 1) / U;
  p.g = ceil_log2(lanes > 1 ? lanes : 1);
  return p;
}
// record q of a piece (q = r * U + j: slot j of the group's lane r): *state and *label of a null, carry or combine record
// and -1, or the position in the state's arc list of an arc record (the caller looks the arc up)
NFST_HD inline int piece_slot(const Piece &p, int q, uint32_t vocab, uint32_t *state, uint32_t *label) {
  *state = 0; *label = vocab;
  if (q >= p.end - p.begin + p.accum) return -1;
  if (p.accum && q == 0) { *state = (uint32_t)p.row; *label = vocab + 1; return -1; }
  if (p.units) { *state = (uint32_t)(p.begin + q - p.accum); *label = vocab + 1; return -1; }
  return p.begin + q - p.accum;
}

// ---- program order: by level, pass, group size (largest first), position of the state in its level, partial index.
// Sizes in a (level, pass) segment are powers of two in falling order, so a piece never straddles a tile: next fit is the
// running sum, the segment takes ceil(sum of sizes / 64) tiles, and its tiles with a group wider than 8 lanes (those come
// first) ceil(sum of those sizes / 64).  Sort key: level 13 | pass 14 | 7 - g 3 | position 20 | partial index 13 bits.
NFST_HD inline unsigned long long piece_key(int level, int pass, int g, int pos, int sub) {
  return ((unsigned long long)level << 50) | ((unsigned long long)pass << 36) | ((unsigned long long)(7 - g) << 33) |
         ((unsigned long long)pos << 13) | (unsigned long long)sub;
}
NFST_HD inline int key_level(unsigned long long k) { return (int)(k >> 50); }
NFST_HD inline int key_pass(unsigned long long k) { return (int)((k >> 36) & 0x3fffull); }
NFST_HD inline unsigned long long key_segment(unsigned long long k) { return k >> 36; }  // (level, pass)
NFST_HD inline int key_g(unsigned long long k) { return 7 - (int)((k >> 33) & 7ull); }
NFST_HD inline int key_pos(unsigned long long k) { return (int)((k >> 13) & 0xfffffull); }
NFST_HD inline int key_sub(unsigned long long k) { return (int)(k & 0x1fffull); }
NFST_HD inline int seg_tiles(int lanes) { return (lanes + 63) >> 6; }

// ---- cost model of a program, cycles of the sweep kernel as measured on MI355X (one wave): ~330 +
// 55 U per tile, 60 more per tile in a program with wide tiles (the per-tile test for them), 450 more per wide tile (the
// general path).  The packers try U ascending, narrow before wide, and keep the first of equally cheap programs.
NFST_HD inline int64_t program_cycles(int64_t tiles, int64_t wide_tiles, int U, bool wide) {
  return tiles * (330 + 55 * U + (wide ? 60 : 0)) + 450 * wide_tiles;
}

}  // namespace nfst_tile

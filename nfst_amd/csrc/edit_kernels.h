// edit_kernels.h -- unit-cost edit distance (Levenshtein) between the rows of two path sets
// Part of the single translation unit kernels.hip (device code in an anonymous namespace).  DESIGN.md sections 2 and 4.17.
#pragma once

// k_edit_distance: one wave64 per pair (set, i, j), kEditWaves pairs per workgroup, the whole table of a pair in one
// launch.  The shorter row of the pair lies on the lanes (the distance is symmetric in its arguments and an integer, so
// the choice cannot show in the result): its C tokens are the columns of the table, in strips of 64, lane l of strip p
// holding column j = 64 p + l + 1 and the token col[j - 1] for the whole strip.  The R tokens of the longer row are the
// rows of the table.  A strip is swept as a skewed wavefront: at step s lane l computes the cell of row i = s - l + 1,
//     D[i][j] = min(min(D[i][j - 1], D[i - 1][j]) + 1, D[i - 1][j - 1] + (row[i - 1] != col[j - 1]))
// where D[i - 1][j] is the lane's own last value, D[i][j - 1] the value lane l - 1 computed at step s - 1 (one lane
// shift, wave_shr1) and D[i - 1][j - 1] what that shift brought one step earlier.  The row token a lane needs travels
// with the wavefront by the same shift.  Lane 0 takes what enters the strip from the left: the row token row[s] and
// D[s + 1][64 p], which every lane loads 64 steps at a time (lane q the values of step s0 + q) and lane 0 receives by
// v_readlane.  D[.][64 p] is i for the first strip; for the next ones it is the right boundary column of the strip
// before, which lane 63 stores in the wave's own LDS array (4 R bytes; entry i - 1 is read at step 64 floor((i - 1) / 64)
// of a strip and overwritten at step i + 62 of the same strip: always after it was read.  The LDS accesses of one wave
// execute in order).  A strip of n lanes costs R + n - 1 steps of two lane shifts, two v_readlane and a handful of integer
// instructions; only strips beyond the first touch LDS.  The cell of an idle lane (a column beyond C, a row outside
// [1, R]) is computed and discarded: trip counts are the same in every lane of a wave and every cross-lane move
// executes with all 64 lanes active.  The waves of a workgroup never wait for each other (no barrier).
//
// Nothing beyond a row's length is read.  A length outside [0, L] sets *status = NFST_ERR_LENGTH and gives the pair -1
// without reading a token.  In symmetric mode (b == a) the waves of i > j leave at once, the wave of i == j writes 0 (-1
// under a bad length, as the general mode does) and the wave of i < j writes [i, j] and [j, i].  Integers only, no
// atomics: the same bits at every launch.
constexpr int kEditMaxLen = NFST_EDIT_MAX_LEN;
constexpr int kEditWaves = 4, kEditThreads = 64 * kEditWaves;

struct EditIn {
  const int32_t *a, *a_len, *b, *b_len;
  int64_t n_pairs;  // n_sets * ka * kb
  int ka, La, kb, Lb, symmetric;
};

// D[R][C] of the rows `row` (R tokens) and `col` (C tokens), C <= R <= kEditMaxLen, in every lane; bnd: R words of LDS
// of this wave alone.  Every lane of the wave calls it with the same arguments.
__device__ __forceinline__ int edit_pair(const int32_t *row, int R, const int32_t *col, int C, int32_t *bnd, int lane) {
  if (C == 0) return R;
  const int strips = (C + 63) >> 6;
  int cur = 0;
  for (int p = 0; p < strips; ++p) {
    const int j = 64 * p + lane + 1;
    const bool col_ok = j <= C;
    const int ctok = col_ok ? col[j - 1] : 0;
    const int n_lanes = C - 64 * p < 64 ? C - 64 * p : 64;
    const int steps = R + n_lanes - 1;
    const bool more = p + 1 < strips;
    cur = j;           // D[0][j]
    int diag = j - 1;  // D[0][j - 1]
    int rtok = 0;
    asm volatile("" ::: "memory");  // (the boundary column of the strip before is in LDS)
    for (int s0 = 0; s0 < steps; s0 += 64) {
      const int idx = s0 + lane;  // lane q: what lane 0 takes at step s0 + q
      const int rin = idx < R ? row[idx] : 0;
      const int bin = p == 0 ? idx + 1 : (idx < R ? bnd[idx] : 0);
      asm volatile("" ::: "memory");
      const int n = steps - s0 < 64 ? steps - s0 : 64;
      for (int q = 0; q < n; ++q) {
        const int left = wave_shr1(cur, read_lane(bin, q));
        rtok = wave_shr1(rtok, read_lane(rin, q));
        const int i = s0 + q - lane + 1;
        const int sub = diag + (rtok != ctok ? 1 : 0), ins = (left < cur ? left : cur) + 1;
        const bool ok = col_ok && i >= 1 && i <= R;
        cur = ok ? (sub < ins ? sub : ins) : cur;
        diag = left;
        if (more && lane == 63 && ok) bnd[i - 1] = cur;
      }
    }
  }
  return read_lane(cur, (C - 1) & 63);
}

__global__ __launch_bounds__(kEditThreads) void k_edit_distance(EditIn in, int32_t *out, int32_t *status) {
  __shared__ int32_t bnd[kEditWaves][kEditMaxLen];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t pair = (int64_t)blockIdx.x * kEditWaves + wv;  // (set * ka + i) * kb + j: the same in every lane
  if (pair >= in.n_pairs) return;
  const int64_t ai = pair / in.kb, set = ai / in.ka;
  const int j = (int)(pair - ai * in.kb), i = (int)(ai - set * in.ka);
  if (in.symmetric && i > j) return;
  const int64_t bj = set * in.kb + j;
  const int la = in.a_len[ai], lb = in.b_len[bj];
  int d = 0;
  if (la < 0 || la > in.La || lb < 0 || lb > in.Lb) {
    d = -1;
    if (lane == 0) *status = NFST_ERR_LENGTH;
  } else if (!in.symmetric || i < j) {
    const int32_t *ra = in.a + ai * in.La, *rb = in.b + bj * in.Lb;
    const bool a_rows = la >= lb;  // the longer row gives the table's rows
    d = edit_pair(a_rows ? ra : rb, a_rows ? la : lb, a_rows ? rb : ra, a_rows ? lb : la, bnd[wv], lane);
  }
  if (lane == 0) {
    out[pair] = d;
    if (in.symmetric && i < j) out[(set * in.ka + j) * in.kb + i] = d;
  }
}

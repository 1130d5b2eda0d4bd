"""The yardstick of the edit-distance op and of MBR selection: a NumPy Wagner-Fischer for one pair, the tables built
from it, and the float64 restatement of ``decoders.mbr_select``.  The project's own code; no test module."""
import numpy as np


def levenshtein(x, y) -> int:
    """The unit-cost edit distance of two integer sequences, the full (len(x) + 1) x (len(y) + 1) table."""
    x, y = np.asarray(x, dtype=np.int64).reshape(-1), np.asarray(y, dtype=np.int64).reshape(-1)
    n, m = len(x), len(y)
    D = np.zeros((n + 1, m + 1), dtype=np.int64)
    D[:, 0] = np.arange(n + 1)
    D[0, :] = np.arange(m + 1)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            D[i, j] = min(D[i - 1, j] + 1, D[i, j - 1] + 1, D[i - 1, j - 1] + (0 if x[i - 1] == y[j - 1] else 1))
    return int(D[n, m])


def levenshtein_fast(x, y) -> int:
    """The same number by a row sweep (vectorised over the columns: t = min(up + 1, diagonal + neq), then
    d[j] = min_{j' <= j} (t[j'] - j') + j for the insertions), for the large cases; held to ``levenshtein`` in
    test_edit_cpu.py."""
    x, y = np.asarray(x, dtype=np.int64).reshape(-1), np.asarray(y, dtype=np.int64).reshape(-1)
    m = len(y)
    col = np.arange(m + 1, dtype=np.int64)
    prev = col.copy()
    for i in range(1, len(x) + 1):
        t = np.empty(m + 1, dtype=np.int64)
        t[0] = i
        t[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (y != x[i - 1]))
        prev = np.minimum.accumulate(t - col) + col
    return int(prev[m])


def _set_table(x, xl, y, yl) -> np.ndarray:
    """[Ka, Kb] of one set: the row sweep of ``levenshtein_fast`` on every pair at once (tables [Ka, Kb, m + 1] of int16:
    no distance exceeds the longer row; a pair whose x row has ended keeps its last row, and the answer is read at the
    y row's own length)."""
    m = int(yl.max()) if yl.size else 0
    n = int(xl.max()) if xl.size else 0
    assert max(m, n) < 2 ** 14
    col = np.arange(m + 1, dtype=np.int16)
    prev = np.broadcast_to(col, (len(x), len(y), m + 1)).copy()
    t = np.empty_like(prev)
    yy = y[None, :, :m]
    for i in range(1, n + 1):
        live = i <= xl
        t[..., 0] = i
        np.minimum(prev[..., 1:] + np.int16(1), prev[..., :-1] + (yy != x[:, None, i - 1, None]).astype(np.int16), out=t[..., 1:])
        t -= col
        np.minimum.accumulate(t, axis=-1, out=t)
        t += col
        if live.all():
            prev, t = t, prev
        else:
            prev[live] = t[live]
    return np.take_along_axis(prev, np.broadcast_to(yl[None, :, None], (len(x), len(y), 1)).astype(np.int64), axis=-1)[..., 0]


def distance_table(a, a_len, b, b_len, fn=None) -> np.ndarray:
    """int32 [B, Ka, Kb]: the distance of ``a[s, i, :a_len[s, i]]`` and ``b[s, j, :b_len[s, j]]``.  With ``fn`` (one of
    the two functions above) pair by pair, equal pairs of rows once; without, set by set (``_set_table``, for the large
    tables; held to the pair-by-pair form in test_edit_cpu.py).  Lengths must lie inside their rows."""
    a, b = np.asarray(a), np.asarray(b)
    a_len, b_len = np.asarray(a_len), np.asarray(b_len)
    B, Ka, Kb = a.shape[0], a.shape[1], b.shape[1]
    assert a_len.shape == (B, Ka) and b_len.shape == (B, Kb)
    assert np.all((a_len >= 0) & (a_len <= a.shape[2])) and np.all((b_len >= 0) & (b_len <= b.shape[2]))
    if fn is None:
        return np.stack([_set_table(a[s], a_len[s], b[s], b_len[s]) for s in range(B)]).astype(np.int32) if B else \
            np.zeros((0, Ka, Kb), np.int32)
    out = np.zeros((B, Ka, Kb), dtype=np.int32)
    memo = {}
    for s in range(B):
        for i in range(Ka):
            x = a[s, i, :a_len[s, i]]
            for j in range(Kb):
                y = b[s, j, :b_len[s, j]]
                key = (x.tobytes(), y.tobytes())
                if key not in memo:
                    memo[key] = memo[(key[1], key[0])] = fn(x, y)
                out[s, i, j] = memo[key]
    return out


def mbr_select(distances, log_weights, n_paths=None):
    """``(index [B] int64, risk [B, K] float64)``: risk[b, i] = sum_j w[b, j] D[b, i, j] with w the float64 softmax of
    ``log_weights`` over the valid entries (j < n_paths[b]; without n_paths: a finite weight), +inf for an invalid i;
    index = the first valid argmin, -1 where nothing is valid.  Plain loops."""
    D = np.asarray(distances, dtype=np.float64)
    lw = np.asarray(log_weights, dtype=np.float64)
    B, K = lw.shape
    index = np.full(B, -1, dtype=np.int64)
    risk = np.full((B, K), np.inf, dtype=np.float64)
    for b in range(B):
        valid = [j for j in range(K) if (j < int(n_paths[b]) if n_paths is not None else np.isfinite(lw[b, j]))]
        if not valid or max(lw[b, j] for j in valid) == -np.inf:  # (no entry, or none with any mass)
            continue
        top = max(lw[b, j] for j in valid)
        w = {j: np.exp(lw[b, j] - top) for j in valid}
        tot = sum(w.values())
        best = None
        for i in valid:
            risk[b, i] = sum(w[j] / tot * D[b, i, j] for j in valid)
            if best is None or risk[b, i] < best:
                best, index[b] = risk[b, i], i
    return index, risk

"""Float32 NumPy reference of the k-best recursion of ``nfst_kbest`` on one lattice (test helper, not a test module),
a float64 brute-force path enumerator for small lattices and a counter of the paths of finite score.

A path runs from state 0 to the sink; self loops lie on no path.  Arc a from s to d extends entry r of d's list to
    c = e_a + (theta[label_a] + v(d, r))          (float32, in this order; e_a = 0 + arc_w[a] + arc_scores[a])
The sink's list is the single entry 0.0.  A state's list is the top k of its candidates (a, r) with c > -inf by
(c desc, canonical arc asc, r asc).  States are swept by decreasing level (longest distance from state 0).
"""
from __future__ import annotations

import numpy as np

from tests.expectation_ref import levels

F32 = np.float32


def arc_terms(l, theta_b, arc_scores=None):
    """(th, e): float32 theta[label_a] and e_a = (0 + arc_w[a]) + arc_scores[a] (each term only if present), in the
    engine's rounding."""
    th = np.asarray(theta_b, F32)[l.label]
    e = np.zeros(l.n_arcs, F32)
    if l.weight is not None:
        e = e + np.asarray(l.weight, F32)
    if arc_scores is not None:
        e = e + np.asarray(arc_scores, F32)
    return th.astype(F32), e.astype(F32)


def k_best(n_rows: int, src, dst, th, e, k: int, sink: int) -> dict:
    """{"best": float32 [k] (-inf padded), "arcs": list of arc lists (relative to the lattice), "n_paths"}."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    th, e = np.asarray(th, F32), np.asarray(e, F32)
    depth = levels(n_rows, src, dst)
    out = [[] for _ in range(n_rows)]
    for a in range(len(src)):
        if src[a] != dst[a]:
            out[int(src[a])].append(a)
    # per state: (scores float32, arc, rank) of its list
    lists = {}
    for s in sorted((r for r in range(n_rows) if depth[r] >= 0), key=lambda r: -depth[r]):
        if s == sink:
            lists[s] = (np.zeros(1, F32), np.full(1, -1, np.int64), np.zeros(1, np.int64))
            continue
        cs, aa, rr = [], [], []
        for a in out[s]:
            v = lists[int(dst[a])][0]
            c = e[a] + (th[a] + v)  # (float32 arrays: float32 adds)
            cs.append(c)
            aa.append(np.full(len(v), a, np.int64))
            rr.append(np.arange(len(v), dtype=np.int64))
        if cs:
            c, a_, r_ = np.concatenate(cs), np.concatenate(aa), np.concatenate(rr)
            keep = c > -np.inf
            c, a_, r_ = c[keep], a_[keep], r_[keep]
            o = np.lexsort((r_, a_, -c))[:k]
            lists[s] = (c[o].astype(F32), a_[o], r_[o])
        else:
            lists[s] = (np.zeros(0, F32), np.zeros(0, np.int64), np.zeros(0, np.int64))
    c0 = lists[0][0]
    n = len(c0)
    best = np.full(k, -np.inf, F32)
    best[:n] = c0
    paths = []
    for j in range(n):
        s, r, arcs = 0, j, []
        while s != sink:
            a = int(lists[s][1][r])
            arcs.append(a)
            s, r = int(dst[a]), int(lists[s][2][r])
        paths.append(arcs)
    return {"best": best, "arcs": paths, "n_paths": n}


def enumerate_paths(n_rows: int, src, dst, score, sink: int):
    """Every path from state 0 to ``sink`` with its float64 score (sum of ``score`` over its arcs), score > -inf only,
    best first: a list of (score, arcs)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    score = np.asarray(score, np.float64)
    out = {r: [] for r in range(n_rows)}
    for a in range(len(src)):
        if src[a] != dst[a]:
            out[int(src[a])].append(a)
    paths = []

    def walk(r, arcs):
        if r == sink:
            paths.append(list(arcs))
            return
        for a in out[r]:
            walk(int(dst[a]), arcs + [a])

    walk(0, [])
    scored = [(float(score[p].sum()), p) for p in paths]
    scored = [x for x in scored if x[0] > -np.inf]
    scored.sort(key=lambda x: -x[0])
    return scored


def count_finite_paths(n_rows: int, src, dst, score, sink: int) -> int:
    """Paths from state 0 to the sink whose arcs all have a score > -inf (exact, Python integers)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    score = np.asarray(score, np.float64)
    depth = levels(n_rows, src, dst)
    out = {r: [] for r in range(n_rows)}
    for a in np.nonzero((src != dst) & (score > -np.inf))[0]:
        out[int(src[a])].append(int(dst[a]))
    cnt = [0] * n_rows
    cnt[sink] = 1
    for s in sorted((r for r in range(n_rows) if depth[r] >= 0 and r != sink), key=lambda r: -depth[r]):
        cnt[s] = sum(cnt[d] for d in out[s])
    return cnt[0]

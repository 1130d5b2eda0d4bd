"""Float32 NumPy restatement of ``nfst_positional_kbest`` on one lattice (test helper, not a test module).

Paths, positions and scores are those of tests/positional_ref.py (``max_plus``); the lists are those of tests/kbest_ref.py
with a position index.  For every position t in [0, T] and state s a list of at most k float32 scores v(t, s, r):
the sink holds the single entry 0.0 at every t, every other state has an empty list at t = T, and for s != sink, t < T
the list is the top k, by ``lexsort((r, a, -c))``, of the candidates (a, r) with
    c = e_a + ((theta[l] + pos[t, l]) + v(t + 1, dst_a, r))        (float32, in this nesting; no pos: e_a + (theta[l] + v))
and c > -inf, a over the out-arcs of s without self loops, r over the list of (t + 1, dst_a).  The result is the list of
(0, state 0); path j follows (arc, rank) forwards from there.
"""
from __future__ import annotations

import numpy as np

from tests import kbest_ref as K
from tests.expectation_ref import sink_of

F32 = np.float32
NEG = -np.inf


def _out_arcs(l):
    out = [[] for _ in range(l.n_rows)]
    for a in np.nonzero(l.src != l.dst)[0]:
        out[int(l.src[a])].append(int(a))
    return [np.asarray(x, np.int64) for x in out]


def reached(l, T: int) -> np.ndarray:
    """[T + 1, n] bool: state s is reached from state 0 by exactly t arcs (without self loops)."""
    keep = l.src != l.dst
    s, d = l.src[keep].astype(np.int64), l.dst[keep].astype(np.int64)
    r = np.zeros((T + 1, l.n_rows), bool)
    r[0, 0] = True
    for t in range(T):
        r[t + 1, d[r[t, s]]] = True
    return r


def k_best(l, theta_b, pos, T: int, k: int, arc_scores=None, every_list: bool = False) -> dict:
    """{"best": float32 [k] (-inf padded), "arcs": list of arc lists (relative to the lattice), "labels", "lengths",
    "n_paths"}.  ``pos`` [T, V] or None.  Only the lists of the (t, s) that state 0 reaches in exactly t arcs are
    computed -- no other list is ever read on the way to (0, state 0) -- unless ``every_list`` is set
    (tests/test_positional_kbest_cpu.py: the result is the same)."""
    n, sink = l.n_rows, sink_of(l.n_rows, l.src, l.dst)
    need = np.ones((T + 1, n), bool) if every_list else reached(l, T)
    th, e = K.arc_terms(l, theta_b, arc_scores)
    P = None if pos is None else np.asarray(pos, F32)
    out = _out_arcs(l)
    dst = l.dst.astype(np.int64)
    val = np.full((T + 1, n, k), NEG, F32)
    arc = np.full((T + 1, n, k), -1, np.int32)
    rank = np.zeros((T + 1, n, k), np.int32)
    cnt = np.zeros((T + 1, n), np.int64)
    val[:, sink, 0] = 0.0
    cnt[:, sink] = 1
    ranks = np.arange(k, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):  # (+inf + -inf, NaN in the pad column: no candidate)
        for t in range(T - 1, -1, -1):
            x = th if P is None else (th + P[t, l.label]).astype(F32)
            for s in np.nonzero(need[t])[0]:
                A = out[s]
                if s == sink or not len(A) or not cnt[t + 1, dst[A]].any():
                    continue
                d = dst[A]
                c = (e[A][:, None] + (x[A][:, None] + val[t + 1, d]).astype(F32)).astype(F32)  # [arcs, k]
                keep = (ranks[None, :] < cnt[t + 1, d][:, None]) & (c > NEG)
                ai, ri = np.nonzero(keep)
                cc, aa = c[ai, ri], A[ai]
                o = np.lexsort((ri, aa, -cc))[:k]
                m = len(o)
                val[t, s, :m], arc[t, s, :m], rank[t, s, :m], cnt[t, s] = cc[o], aa[o], ri[o], m
    m = int(cnt[0, 0])
    best = np.full(k, NEG, F32)
    best[:m] = val[0, 0, :m]
    paths = []
    for j in range(m):
        s, r, arcs = 0, j, []
        for t in range(T + 1):
            if s == sink:
                break
            a = int(arc[t, s, r])
            arcs.append(a)
            s, r = int(dst[a]), int(rank[t, s, r])
        assert s == sink
        paths.append(arcs)
    return {"best": best, "arcs": paths, "labels": [[int(l.label[a]) for a in p] for p in paths],
            "lengths": [len(p) for p in paths], "n_paths": m}


def path_score32(l, theta_b, pos, arcs, arc_scores=None) -> np.float32:
    """The right-nested float32 score of one path: v_L = 0, v_t = e_a + ((theta[l] + pos[t, l]) + v_{t+1})."""
    th, e = K.arc_terms(l, theta_b, arc_scores)
    P = None if pos is None else np.asarray(pos, F32)
    v = F32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(len(arcs) - 1, -1, -1):
            a = arcs[t]
            x = th[a] if P is None else F32(th[a] + P[t, l.label[a]])
            v = F32(e[a] + F32(x + v))
    return v


def path_terms64(l, theta_b, pos, arcs, arc_scores=None):
    """(float64 sum of the path's terms, sum of their absolute values M, number of terms)."""
    th = np.asarray(theta_b, F32).astype(np.float64)
    terms = []
    for t, a in enumerate(arcs):
        terms.append(th[l.label[a]])
        if pos is not None:
            terms.append(float(pos[t, l.label[a]]))
        if l.weight is not None:
            terms.append(float(l.weight[a]))
        if arc_scores is not None:
            terms.append(float(arc_scores[a]))
    terms = np.asarray(terms, np.float64)
    return float(terms.sum()), float(np.abs(terms).sum()), len(terms)

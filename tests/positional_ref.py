"""NumPy restatement of the time-synchronous sweeps of ``nfst_positional`` / ``nfst_positional_viterbi`` on one lattice
(test helper, not a test module).

A path a_0 .. a_{L-1} runs from state 0 to the sink over the arcs without self loops; arc a_t is at position t and scores
    score[a_t] + pos[t, label(a_t)]                (pos optional: None means the term is absent)
Only paths with L <= T count.

``sum_product``  float64, log domain: alpha_t / beta_t over positions, log Z_T, len_logz, pos_post, arc_post
``max_plus``     float32 in the engine's add order  c = e_a + ((theta[l] + pos[t, l]) + vb_{t+1}(dst)),  ties to the
                 smaller canonical arc
``enumerate``    every path of a small lattice, one by one (capped)
"""
from __future__ import annotations

import numpy as np

from tests.expectation_ref import sink_of

F32 = np.float32
NEG = -np.inf


def arc_score64(l, theta_b, arc_scores=None) -> np.ndarray:
    """float64 log weight of every arc: theta[label] (+ weight) (+ arc_scores), from the float32 inputs."""
    s = np.asarray(theta_b, F32).astype(np.float64)[l.label]
    if l.weight is not None:
        s = s + np.asarray(l.weight, F32).astype(np.float64)
    if arc_scores is not None:
        s = s + np.asarray(arc_scores, F32).astype(np.float64)
    return s


def min_max_len(l):
    """(shortest, longest) path from state 0 to the sink, in arcs."""
    sink = sink_of(l.n_rows, l.src, l.dst)
    if sink == 0:  # state 0 is the sink: the one path is the empty one
        return 0, 0
    keep = l.src != l.dst
    s, d = l.src[keep].astype(np.int64), l.dst[keep].astype(np.int64)
    reach = np.zeros(l.n_rows, bool)
    reach[0] = True
    lens = []
    for t in range(1, l.n_rows + 1):
        nxt = np.zeros(l.n_rows, bool)
        nxt[d[reach[s]]] = True
        if nxt[sink]:
            lens.append(t)
        nxt[sink] = False
        reach = nxt
        if not reach.any():
            break
    return min(lens), max(lens)


def sum_product(l, score, pos, T: int) -> dict:
    """{"logz", "len_logz" [T + 1], "pos_post" [T, V], "arc_post" [A]} in float64.  ``score`` [A] float64, ``pos`` [T, V]
    or None."""
    n, sink, V = l.n_rows, sink_of(l.n_rows, l.src, l.dst), l.vocab
    live = np.nonzero(l.src != l.dst)[0]
    s, d, lab = l.src[live].astype(np.int64), l.dst[live].astype(np.int64), l.label[live].astype(np.int64)
    sc = np.asarray(score, np.float64)[live]
    P = None if pos is None else np.asarray(pos, np.float64)

    def w(t):
        return sc if P is None else sc + P[t, lab]

    with np.errstate(invalid="ignore", over="ignore"):
        beta = np.full((T + 1, n), NEG)
        beta[:, sink] = 0.0  # a path that has ended stays ended: L <= T
        for t in range(T - 1, -1, -1):
            term = w(t) + beta[t + 1, d]
            row = np.full(n, NEG)
            np.logaddexp.at(row, s, np.where(np.isnan(term), NEG, term))
            row[sink] = 0.0
            beta[t] = row
        logz = float(beta[0, 0])
        alpha = np.full(n, NEG)
        alpha[0] = 0.0
        len_logz = np.full(T + 1, NEG)
        if sink == 0:  # the empty path
            len_logz[0] = 0.0
        pos_post = np.zeros((T, V))
        arc_post = np.zeros(l.n_arcs)
        for t in range(T):
            term = alpha[s] + w(t)
            term = np.where(np.isnan(term), NEG, term)
            if np.isfinite(logz):
                p = np.exp(term + beta[t + 1, d] - logz)
                p = np.where(np.isfinite(p), p, 0.0)
                np.add.at(pos_post[t], lab, p)
                np.add.at(arc_post, live, p)
            nxt = np.full(n, NEG)
            np.logaddexp.at(nxt, d, term)
            len_logz[t + 1] = nxt[sink]
            nxt[sink] = NEG  # nothing leaves the sink
            alpha = nxt
    return {"logz": logz, "len_logz": len_logz, "pos_post": pos_post, "arc_post": arc_post}


def max_plus(l, theta_b, pos, T: int, arc_scores=None) -> dict:
    """{"best" float32, "arcs" list (relative to the lattice), "labels", "vb" [T + 1, n] float32, "ties"}: plain float32
    in the engine's order, from position T backwards; the walk takes the smallest canonical arc whose candidate has the
    bits of vb_t(state).  ``ties[t]`` is the number of live arcs of the walked state that attain it at step t."""
    n, sink = l.n_rows, sink_of(l.n_rows, l.src, l.dst)
    th = np.asarray(theta_b, F32)
    e = np.zeros(l.n_arcs, F32)
    if l.weight is not None:
        e = e + np.asarray(l.weight, F32)
    if arc_scores is not None:
        e = e + np.asarray(arc_scores, F32)
    e = e.astype(F32)
    live = np.nonzero(l.src != l.dst)[0]
    s, d, lab = l.src[live].astype(np.int64), l.dst[live].astype(np.int64), l.label[live].astype(np.int64)
    P = None if pos is None else np.asarray(pos, F32)

    def cand(t, vb_next):
        with np.errstate(invalid="ignore", over="ignore"):
            x = th[lab] if P is None else (th[lab] + P[t, lab]).astype(F32)
            return (e[live] + (x + vb_next[d]).astype(F32)).astype(F32)

    vb = np.full((T + 1, n), NEG, F32)
    vb[:, sink] = 0.0
    cs = [None] * T
    for t in range(T - 1, -1, -1):
        c = cand(t, vb[t + 1])
        cs[t] = c
        row = np.full(n, NEG, F32)
        np.maximum.at(row, s, np.where(np.isnan(c), F32(NEG), c))
        row[sink] = 0.0
        vb[t] = row
    best = vb[0, 0]
    arcs, ties = [], []
    if best > NEG:
        st = 0
        for t in range(T):
            if st == sink:
                break
            k = np.nonzero((s == st) & (cs[t] == vb[t, st]))[0]
            a = int(live[k[0]])  # (live is ascending: the smallest canonical arc)
            arcs.append(a)
            ties.append(len(k))
            st = int(l.dst[a])
    return {"best": F32(best), "arcs": arcs, "labels": [int(l.label[a]) for a in arcs], "vb": vb, "ties": ties}


POS_THREADS = 1024  # kPosThreads of csrc/positional_kernels.h


def pos_group(n_dp: int, n_reach: int, n_rows: int) -> int:
    """Restatement of ``pos_group`` (csrc/positional_kernels.h) from the meta words the kernel reads: the lanes that share
    a state's arcs -- the largest power of two <= the mean out-degree (n_dp / n_reach, integer division as in C), doubled
    while it is below that mean and twice as many lanes per state still fit the workgroup."""
    avg = int(n_dp) // max(int(n_reach), 1)
    g = 1
    while g < 64 and g * 2 <= avg:
        g <<= 1
    while g < 64 and g < avg and int(n_rows) * g * 2 <= POS_THREADS:
        g <<= 1
    return g


def batch_groups(lat) -> list:
    """``pos_group`` of every lattice of a packed batch, from its meta words."""
    from nfst_amd import _lib

    m = lat.meta_host
    return [pos_group(r[_lib.META_N_DP], r[_lib.META_N_REACH], r[_lib.META_N_ROWS]) for r in m]


def enumerate_paths(l, cap: int = 10000):
    """Every path from state 0 to the sink as a list of arcs; asserts that there are at most ``cap``."""
    sink = sink_of(l.n_rows, l.src, l.dst)
    out = {r: [] for r in range(l.n_rows)}
    for a in range(l.n_arcs):
        if l.src[a] != l.dst[a]:
            out[int(l.src[a])].append(a)
    paths = []

    def walk(r, arcs):
        if r == sink:
            paths.append(arcs)
            assert len(paths) <= cap, "more paths than the enumeration's cap"
            return
        for a in out[r]:
            walk(int(l.dst[a]), arcs + [a])

    walk(0, [])
    return paths


def brute_force(l, score, pos, T: int, paths=None) -> dict:
    """The quantities of ``sum_product`` and the best path, path by path in float64."""
    paths = enumerate_paths(l) if paths is None else paths
    score = np.asarray(score, np.float64)
    P = None if pos is None else np.asarray(pos, np.float64)
    fit = [p for p in paths if len(p) <= T]
    S = []
    for p in fit:
        x = score[p].sum()
        if P is not None:
            x = x + sum(P[t, l.label[a]] for t, a in enumerate(p))
        S.append(x)
    S = np.asarray(S, np.float64)
    len_logz = np.full(T + 1, NEG)
    pos_post = np.zeros((T, l.vocab))
    arc_post = np.zeros(l.n_arcs)
    ok = np.isfinite(S)
    if not ok.any():
        return {"logz": NEG, "len_logz": len_logz, "pos_post": pos_post, "arc_post": arc_post, "best": NEG, "best_arcs": [],
                "runner_up": NEG, "n_paths": len(paths), "lengths": sorted({len(p) for p in paths})}
    logz = float(np.logaddexp.reduce(S[ok]))
    for p, x in zip(fit, S):
        if not np.isfinite(x):
            continue
        len_logz[len(p)] = np.logaddexp(len_logz[len(p)], x)
        w = np.exp(x - logz)
        for t, a in enumerate(p):
            pos_post[t, l.label[a]] += w
            arc_post[a] += w
    j = int(np.argmax(np.where(ok, S, NEG)))
    top = np.sort(S[ok])[::-1]
    return {"logz": logz, "len_logz": len_logz, "pos_post": pos_post, "arc_post": arc_post, "best": float(S[j]),
            "best_arcs": list(fit[j]), "runner_up": float(top[1]) if len(top) > 1 else NEG, "n_paths": len(paths),
            "lengths": sorted({len(p) for p in paths})}


def logsumexp(x) -> float:
    x = np.asarray(x, np.float64)
    x = x[np.isfinite(x)]
    return float(np.logaddexp.reduce(x)) if len(x) else NEG

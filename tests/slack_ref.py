"""Float32 NumPy restatement of the arc slack semantics of ``nfst_arc_slack`` on one lattice (test helper, not a test
module; DESIGN.md section 2, "Arc slack and beam pruning"), the trim check of a kept set, and a float64 max-marginal by
path enumeration for small lattices.

A path runs from state 0 to the sink; self loops lie on no path.  All adds are float32, in the engine's order:
    c_a = e_a + (theta[label_a] + vbeta(dst_a))        e_a = 0 + arc_w[a] + arc_scores[a]  (kbest_ref.arc_terms)
    vbeta(sink) = 0, vbeta(s) = max c_a over the out-arcs;  gap_a = vbeta(src_a) - c_a  (c_a > -inf, else +inf)
    delta(0) = 0 (best > -inf), slack_a = delta(src_a) + gap_a, delta(d) = min slack_a over the in-arcs
    a self loop at s: slack = delta(s);  keep_a = slack_a <= beam and slack_a < +inf
"""
from __future__ import annotations

import numpy as np

from tests.expectation_ref import levels, sink_of
from tests.kbest_ref import arc_terms, enumerate_paths

F32 = np.float32
INF = F32(np.inf)


def arc_slack(l, theta_b, arc_scores=None, beam=None) -> dict:
    """{"best", "vbeta" [n_rows], "state_slack" [n_rows], "slack" [A], "keep", "n_kept" (with a beam), "depth"}; vbeta
    and state_slack are -inf / +inf for the rows that lie on no path of finite score."""
    th, e = arc_terms(l, theta_b, arc_scores)
    n, sink = l.n_rows, sink_of(l.n_rows, l.src, l.dst)
    src, dst = np.asarray(l.src, np.int64), np.asarray(l.dst, np.int64)
    depth = levels(n, src, dst)
    loop = src == dst
    out_arcs = [[] for _ in range(n)]
    in_arcs = [[] for _ in range(n)]
    for a in np.nonzero(~loop)[0]:
        out_arcs[src[a]].append(a)
        in_arcs[dst[a]].append(a)
    reach = [r for r in range(n) if depth[r] >= 0]
    vb = np.full(n, -INF, F32)
    vb[sink] = 0.0
    with np.errstate(invalid="ignore"):
        for s in sorted(reach, key=lambda r: -depth[r]):
            if s == sink or not out_arcs[s]:
                continue
            a = np.asarray(out_arcs[s])
            vb[s] = np.max(e[a] + (th[a] + vb[dst[a]]))  # (float32 arrays: float32 adds)
        c = (e + (th + vb[dst])).astype(F32)
        gap = np.where(loop, F32(0.0), np.where(c > -INF, vb[src] - c, INF)).astype(F32)
        dl = np.full(n, INF, F32)
        if vb[0] > -INF:
            dl[0] = 0.0
        for d in sorted(reach, key=lambda r: depth[r]):
            if d == 0 or not in_arcs[d]:
                continue
            a = np.asarray(in_arcs[d])
            dl[d] = np.min(dl[src[a]] + gap[a])
        slack = (dl[src] + gap).astype(F32)
    res = {"best": vb[0], "vbeta": np.where(dl < INF, vb, -INF).astype(F32), "state_slack": dl, "slack": slack,
           "depth": int(depth.max())}
    if beam is not None:
        res["keep"] = (slack <= F32(beam)) & (slack < INF)  # (an arc on no path of finite score is never kept)
        res["n_kept"] = int(res["keep"].sum())
    return res


def is_trim(l, keep) -> bool:
    """Every kept arc without a self loop starts at state 0 or at a state with a kept in-arc, and ends at the sink or
    at a state with a kept out-arc (self loops do not count as in- or out-arcs)."""
    src, dst = np.asarray(l.src, np.int64), np.asarray(l.dst, np.int64)
    k = np.asarray(keep, bool) & (src != dst)
    has_in = np.zeros(l.n_rows, bool)
    has_out = np.zeros(l.n_rows, bool)
    has_in[dst[k]] = True
    has_out[src[k]] = True
    has_in[0] = True
    has_out[sink_of(l.n_rows, l.src, l.dst)] = True
    return bool(np.all(has_in[src[k]]) and np.all(has_out[dst[k]]))


def max_marginals64(l, theta_b, arc_scores=None) -> np.ndarray:
    """float64 [A]: the best score of a path through every arc, by enumeration of all paths (small lattices); -inf
    for arcs on no path of finite score (self loops included)."""
    th, e = arc_terms(l, theta_b, arc_scores)
    score = th.astype(np.float64) + e.astype(np.float64)
    mm = np.full(l.n_arcs, -np.inf)
    for s, p in enumerate_paths(l.n_rows, l.src, l.dst, score, sink_of(l.n_rows, l.src, l.dst)):
        mm[p] = np.maximum(mm[p], s)
    return mm

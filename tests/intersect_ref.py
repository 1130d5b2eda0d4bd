"""Pure-Python restatement of the product of one lattice with a constraint automaton (test helper, not a test module):
the semantics of ``nfst_intersect_count`` / ``_write`` (include/nfst_hip.h) on one ``SynthLattice``,
with Python integers as the masks of automaton states.

A path runs from state 0 to the sink (``expectation_ref.sink_of``) over canonical arcs; self loops lie on no path and the automaton
never reads them.  ``delta`` is ``[Q, V]`` (-1: no transition), ``final`` ``[Q]``.
"""
from __future__ import annotations

import numpy as np

from tests.expectation_ref import levels, sink_of


def _bits(m: int):
    q = 0
    while m:
        if m & 1:
            yield q
        m >>= 1
        q += 1


def masks(l, delta, final):
    """(fwd, bwd, live): one Python-int mask per row."""
    delta = np.asarray(delta, np.int64)
    n, sink = l.n_rows, sink_of(l.n_rows, l.src, l.dst)
    depth = levels(n, l.src, l.dst)
    order = sorted((s for s in range(n) if depth[s] >= 0), key=lambda s: depth[s])
    out = [[] for _ in range(n)]
    for a in range(l.n_arcs):
        if l.src[a] != l.dst[a]:
            out[int(l.src[a])].append(a)
    fwd = [0] * n
    fwd[0] = 1
    for s in order:  # (every in-arc of a state comes from an earlier level)
        for a in out[s]:
            for q in _bits(fwd[s]):
                t = int(delta[q, l.label[a]])
                if t >= 0:
                    fwd[int(l.dst[a])] |= 1 << t
    bwd = [0] * n
    bwd[sink] = sum(1 << q for q in range(delta.shape[0]) if final[q])
    for s in reversed(order):
        for a in out[s]:
            tgt = bwd[int(l.dst[a])]
            for q in range(delta.shape[0]):
                t = int(delta[q, l.label[a]])
                if t >= 0 and (tgt >> t) & 1:
                    bwd[s] |= 1 << q
    live = [fwd[s] & bwd[s] if depth[s] >= 0 else 0 for s in range(n)]
    return fwd, bwd, live


def intersect(l, delta, final) -> dict:
    """{"n_rows", "n_arcs", "src", "label", "dst", "arc_map" (positions among the lattice's arcs), "arc_q", "row_state",
    "row_q"}; an empty product has n_rows = n_arcs = 0."""
    delta = np.asarray(delta, np.int64)
    n, sink = l.n_rows, sink_of(l.n_rows, l.src, l.dst)
    _, _, live = masks(l, delta, final)
    row_state, row_q, row_of = [], [], {}
    for s in range(n):
        for q in _bits(live[s]):
            if s == sink and (s, -1) in row_of:  # all pairs of the sink are one row
                row_of[(s, q)] = row_of[(s, -1)]
                continue
            row_of[(s, q)] = len(row_state)
            if s == sink:
                row_of[(s, -1)] = len(row_state)
            row_state.append(s)
            row_q.append(q)
    first_arc = np.searchsorted(l.src, np.arange(n + 1))
    src, label, dst, arc_map, arc_q = [], [], [], [], []
    for r, (s, q) in enumerate(zip(row_state, row_q)):
        for a in range(int(first_arc[s]), int(first_arc[s + 1])):
            lab, d = int(l.label[a]), int(l.dst[a])
            if d == s:
                src.append(r), label.append(lab), dst.append(r), arc_map.append(a), arc_q.append(0 if s == sink else q)
                continue
            t = int(delta[q, lab])
            if t >= 0 and (live[d] >> t) & 1:
                src.append(r), label.append(lab), dst.append(row_of[(d, t)]), arc_map.append(a), arc_q.append(q)
    if not (live[0] & 1):
        assert not row_state and not src
    i32 = lambda x: np.asarray(x, np.int32)
    return {"n_rows": len(row_state), "n_arcs": len(src), "src": i32(src), "label": i32(label), "dst": i32(dst),
            "arc_map": np.asarray(arc_map, np.int64), "arc_q": i32(arc_q), "row_state": i32(row_state), "row_q": i32(row_q)}


def run(delta, final, labels) -> bool:
    """Does the automaton accept the label sequence?"""
    q = 0
    for lab in labels:
        q = int(delta[q][int(lab)])
        if q < 0:
            return False
    return bool(final[q])


def product_paths(p: dict):
    """Every path of a reference product from row 0 to its sink as (label tuple, arc_map tuple)."""
    if p["n_rows"] == 0:
        return []
    out = [[] for _ in range(p["n_rows"])]
    has_out = np.zeros(p["n_rows"], bool)
    for k in range(p["n_arcs"]):
        if p["src"][k] != p["dst"][k]:
            out[int(p["src"][k])].append(k)
            has_out[p["src"][k]] = True
    sinks = np.nonzero(~has_out)[0]
    assert len(sinks) == 1
    res = []

    def walk(r, arcs):
        if r == sinks[0]:
            res.append((tuple(int(p["label"][k]) for k in arcs), tuple(int(p["arc_map"][k]) for k in arcs)))
            return
        for k in out[r]:
            walk(int(p["dst"][k]), arcs + [k])

    walk(0, [])
    return res

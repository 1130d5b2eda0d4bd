"""Vectorised NumPy restatement of the product of one lattice with an automaton of any number of states (test helper, not
a test module): the semantics of ``tests/intersect_ref.intersect`` with boolean ``[rows, Q]`` arrays as the sets of
automaton states and one NumPy operation over the states per arc, where the pure-Python one iterates Q times per arc.
``tests/test_intersect_wide_cpu.py`` holds it to ``intersect_ref.intersect`` on the small cases.

``delta`` is ``[Q, V]`` (-1: no transition), ``final`` ``[Q]``: what ``WideDFA.to_dense()`` returns.
"""
from __future__ import annotations

import numpy as np

from tests.expectation_ref import levels, sink_of


def edit_denominator(x, symbols, max_out: int, vocab: int, input_mark: int = 3, output_mark: int = 4, insertion_mark: int = 5):
    """The denominator lattice x o T of ``synth.edit_lattice``'s transducer: the edit grid of ``x`` that emits ANY of
    ``symbols`` after the output mark, at most ``max_out`` of them.  Node (i, j) has consumed x[:i] and produced j symbols;
    the edits and their marks are ``synth.edit_lattice``'s, the symbol after an output mark is a fan of one arc per symbol
    out of the edit's last private state, so the machine is deterministic; every node (len(x), j) has the eos arc.  The
    paths whose symbols after the output marks spell y are, label sequence for label sequence, the paths of
    ``synth.edit_lattice(x, y)``."""
    from nfst_amd import synth

    n = len(x)
    src, lab, dst = [], [], []
    nxt = [1]

    def new_state():
        nxt[0] += 1
        return nxt[0] - 1

    node = {(i, j): new_state() for i in range(n + 1) for j in range(max_out + 1)}

    def chain(a, marks):  # the marks one after the other through private states; returns the last of them
        cur = a
        for mk in marks:
            nx = new_state()
            src.append(cur), lab.append(int(mk)), dst.append(nx)
            cur = nx
        return cur

    def arc(a, l, b):
        src.append(a), lab.append(int(l)), dst.append(b)

    arc(0, synth.BOS, node[(0, 0)])
    for i in range(n + 1):
        for j in range(max_out + 1):
            a = node[(i, j)]
            if j < max_out:
                u = chain(a, [output_mark])
                for c in symbols:
                    arc(u, c, node[(i, j + 1)])
            if i < n:
                u = chain(a, [input_mark])
                arc(u, x[i], node[(i + 1, j)])
            if i < n and j < max_out:
                u = chain(a, [insertion_mark, input_mark, x[i], output_mark])
                for c in symbols:
                    arc(u, c, node[(i + 1, j + 1)])
    sink = nxt[0]
    for j in range(max_out + 1):
        arc(node[(n, j)], synth.EOS, sink)
    return synth._finish(sink + 1, vocab, src, lab, dst)


def live_sets(l, delta, final) -> np.ndarray:
    """bool ``[rows, Q]``: the pairs (s, q) that lie on an accepted path."""
    delta = np.asarray(delta, np.int64)
    Q = delta.shape[0]
    n, sink = l.n_rows, sink_of(l.n_rows, l.src, l.dst)
    depth = levels(n, l.src, l.dst)
    order = sorted((s for s in range(n) if depth[s] >= 0), key=lambda s: depth[s])
    first_arc = np.searchsorted(l.src, np.arange(n + 1))
    fwd = np.zeros((n, Q), bool)
    fwd[0, 0] = True
    for s in order:  # (every in-arc of a state comes from an earlier level)
        qs = np.nonzero(fwd[s])[0]
        if not qs.size:
            continue
        for a in range(int(first_arc[s]), int(first_arc[s + 1])):
            d = int(l.dst[a])
            if d == s:
                continue
            t = delta[qs, int(l.label[a])]
            fwd[d, t[t >= 0]] = True
    live = np.zeros((n, Q), bool)
    if depth[sink] >= 0:
        live[sink] = fwd[sink] & (np.asarray(final) != 0)
    for s in reversed(order):
        if s == sink:
            continue
        qs = np.nonzero(fwd[s])[0]
        for a in range(int(first_arc[s]), int(first_arc[s + 1])):
            d = int(l.dst[a])
            if d == s or not qs.size:
                continue
            t = delta[qs, int(l.label[a])]
            ok = t >= 0
            ok[ok] = live[d, t[ok]]
            live[s, qs[ok]] = True
    return live


def intersect(l, delta, final) -> dict:
    """The dictionary of ``intersect_ref.intersect``."""
    delta = np.asarray(delta, np.int64)
    n, sink = l.n_rows, sink_of(l.n_rows, l.src, l.dst)
    live = live_sets(l, delta, final)
    i32 = lambda x: np.asarray(x, np.int32)
    if not live[0, 0]:
        assert not live.any()
        e = np.zeros(0, np.int32)
        return {"n_rows": 0, "n_arcs": 0, "src": e, "label": e, "dst": e, "arc_map": np.zeros(0, np.int64), "arc_q": e,
                "row_state": e, "row_q": e}
    live_rows = live.copy()
    if live[sink].any():  # all pairs of the sink are one row, at its smallest q
        live_rows[sink] = False
        live_rows[sink, int(np.argmax(live[sink]))] = True
    row_state, row_q = np.nonzero(live_rows)  # (s ascending, q ascending)
    row_of = np.full(live.shape, -1, np.int64)
    row_of[row_state, row_q] = np.arange(row_state.size)
    row_of[sink, live[sink]] = row_of[sink, row_q[row_state == sink][0]] if live[sink].any() else -1
    first_arc = np.searchsorted(l.src, np.arange(n + 1))
    src, arc, dst, arc_q = [], [], [], []
    for s in np.unique(row_state):
        qs = np.nonzero(live_rows[s])[0]
        rows = row_of[s, qs]
        for a in range(int(first_arc[s]), int(first_arc[s + 1])):
            d = int(l.dst[a])
            if d == s:
                src.append(rows), arc.append(np.full(rows.size, a)), dst.append(rows)
                arc_q.append(np.zeros(rows.size, np.int64) if s == sink else qs)
                continue
            t = delta[qs, int(l.label[a])]
            ok = t >= 0
            ok[ok] = live[d, t[ok]]
            src.append(rows[ok]), arc.append(np.full(int(ok.sum()), a)), dst.append(row_of[d, t[ok]]), arc_q.append(qs[ok])
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)
    src, arc, dst, arc_q = cat(src), cat(arc), cat(dst), cat(arc_q)
    o = np.lexsort((arc, src))  # rows in order, a row's arcs in canonical order
    src, arc, dst, arc_q = src[o], arc[o], dst[o], arc_q[o]
    return {"n_rows": int(row_state.size), "n_arcs": int(src.size), "src": i32(src), "label": i32(np.asarray(l.label)[arc]),
            "dst": i32(dst), "arc_map": arc.astype(np.int64), "arc_q": i32(arc_q), "row_state": i32(row_state), "row_q": i32(row_q)}

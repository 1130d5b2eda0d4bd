"""NumPy float64 restatement of ``nfst_string_prefix``, ``nfst_string_next`` and ``decoders.prefix_search`` (test helper,
not a test module), on one lattice in the engine's numbering with one float64 score per arc (``edge_cases.score64``):
the suffix table H (G of tests/strings_ref.py with "anything may follow" at column n), the prefix tables F, F0, F1 of
include/nfst_hip.h, the reduction by label and the search in its two phases.  Sums are ``_lse_rows`` (around the
maximum), not the kernels' order: the results agree with the kernels' to round-off, not bit for bit.
tests/test_strings_prefix_cpu.py holds it to brute force over every path.
"""
from __future__ import annotations

import numpy as np

from tests.expectation_ref import levels, sink_of
from tests.strings_ref import F64, NEG, _lse_rows


def _lse(xs) -> float:
    xs = np.asarray(list(xs), F64).reshape(-1)
    return float(_lse_rows(xs[:, None])[0]) if xs.size else NEG


def _graph(l):
    src, dst, label = np.asarray(l.src, np.int64), np.asarray(l.dst, np.int64), np.asarray(l.label, np.int64)
    depth = levels(l.n_rows, src, dst)
    arcs = [a for a in range(len(src)) if src[a] != dst[a] and depth[src[a]] >= 0]  # canonical order, on some path from state 0
    by_depth = sorted((r for r in range(l.n_rows) if depth[r] >= 0), key=lambda r: depth[r])
    return src, dst, label, sink_of(l.n_rows, src, dst), arcs, by_depth


def suffix_tables(l, score, y, keep=None, marker=None) -> tuple:
    """``(H0, H1, Z)``: per state reachable from state 0 the rows H0[s][0 .. n] and H1[s][0 .. n] (keep mode: H1 is all
    -inf) and log Z of the rest of the lattice behind s."""
    assert (keep is None) != (marker is None)
    src, dst, label, sink, arcs, by_depth = _graph(l)
    score = np.asarray(score, F64)
    y = np.asarray(y, np.int64).reshape(-1)
    n = len(y)
    kept = None if keep is None else set(int(x) for x in keep)
    none = np.full(n + 1, NEG)
    out = {}
    for a in arcs:
        out.setdefault(int(src[a]), []).append(a)
    H0, H1, Z = {}, {}, {}

    def shifted(row, lab, open_row):  # j < n: (y[j] == lab) ? row[j + 1] : -inf;  j == n: the open column
        r = none.copy()
        r[:n] = np.where(y == lab, row[1:], NEG)
        r[n] = open_row[n]
        return r

    for s in reversed(by_depth):
        if s == sink:
            H0[s] = np.where(np.arange(n + 1) == n, 0.0, NEG)
            H1[s] = none.copy()
            Z[s] = 0.0
            continue
        t0, t1, tz = [none], [none], [np.array(NEG)]
        for a in out.get(s, []):
            d, lab, w = int(dst[a]), int(label[a]), score[a]
            tz.append(np.array(w + Z[d]))
            if kept is not None:
                t0.append(w + (shifted(H0[d], lab, H0[d]) if lab in kept else H0[d]))
            else:
                t0.append(w + (H1[d] if lab == marker else H0[d]))
                t1.append(w + shifted(H0[d], lab, H0[d]))
        H0[s], H1[s], Z[s] = _lse_rows(t0), _lse_rows(t1), float(_lse_rows(tz))
    return H0, H1, Z


def prefix_log_prob(l, score, y, keep=None, marker=None) -> tuple:
    """``(log_prefix, logz)`` of the prefix ``y``: H0[state 0][0] and Z[state 0]"""
    H0, _, Z = suffix_tables(l, score, y, keep, marker)
    return float(H0[0][0]), float(Z[0])


def prefix_tables(l, score, y, keep=None, marker=None) -> tuple:
    """``(F0, F1)``: per state reachable from state 0 the log weight of the path prefixes from state 0 that have spelled
    y[:j], the arc into the state being no active marker (F0) or one (F1; keep mode: all -inf)."""
    src, dst, label, sink, arcs, by_depth = _graph(l)
    score = np.asarray(score, F64)
    y = np.asarray(y, np.int64).reshape(-1)
    n = len(y)
    kept = None if keep is None else set(int(x) for x in keep)
    none = np.full(n + 1, NEG)
    into = {}
    for a in arcs:
        into.setdefault(int(dst[a]), []).append(a)

    def shifted(row, lab):  # j >= 1 and y[j - 1] == lab ? row[j - 1] : -inf
        r = none.copy()
        r[1:] = np.where(y == lab, row[:n], NEG)
        return r

    F0, F1 = {}, {}
    for s in by_depth:
        if s == 0:
            F0[s] = np.where(np.arange(n + 1) == 0, 0.0, NEG)
            F1[s] = none.copy()
            continue
        t0, t1 = [none], [none]
        for a in into.get(s, []):
            u, lab, w = int(src[a]), int(label[a]), score[a]
            if kept is not None:
                t0.append(w + (shifted(F0[u], lab) if lab in kept else F0[u]))
            else:
                (t1 if lab == marker else t0).append(w + F0[u])
                t0.append(w + shifted(F1[u], lab))
        F0[s], F1[s] = _lse_rows(t0), _lse_rows(t1)
    return F0, F1


def next_log_probs(l, score, y, keep=None, marker=None) -> tuple:
    """``(next [vocab], eos, log_prefix, logz)`` of the prefix ``y`` as ``nfst_string_next`` forms them: F at column n, the
    arcs by label, and the continuation weights of the empty prefix."""
    src, dst, label, sink, arcs, _ = _graph(l)
    score = np.asarray(score, F64)
    n = len(np.asarray(y).reshape(-1))
    F0, F1 = prefix_tables(l, score, y, keep, marker)
    Zn0, _, Z = suffix_tables(l, score, [], keep, marker)
    kept = None if keep is None else set(int(x) for x in keep)
    terms = [[] for _ in range(l.vocab)]
    for a in arcs:
        s, d, v = int(src[a]), int(dst[a]), int(label[a])
        if kept is not None:
            if v in kept:
                terms[v].append((F0[s][n] + score[a]) + Z[d])
        else:
            terms[v].append((F1[s][n] + score[a]) + Zn0[d][0])
    nxt = np.array([_lse(t) for t in terms], F64)
    eos = float(F0[sink][n]) if sink in F0 else NEG
    return nxt, eos, _lse([eos] + list(nxt)), float(Z[0])


def prefix_search(l, score, k=8, max_len=None, keep=None, marker=None, reserve=64, refine_steps=32) -> dict:
    """``decoders.prefix_search`` on one lattice: strings (tuples, best first), log_prob, bound, exact and the steps taken.
    Step t of the length-synchronous phase holds at most k open prefixes of length t; their eos enter the list of the k
    best complete strings (ties: the earlier entry, then the lower slot); the k V extensions are ranked by next (ties:
    lower slot, then lower label), the k heaviest stay open and the rest is set aside in the reserve, which keeps its
    ``reserve`` heaviest entries (ties: the older entry) -- the heaviest one it drops raises the bound; a prefix of
    max_len symbols is not extended, its mass beyond its eos raises the bound; the phase stops when no open prefix
    outweighs the k-th complete string.  The second phase takes the k heaviest prefixes of the reserve per step, whatever
    their lengths, and sets all their extensions aside, until the reserve holds nothing heavier than the first complete
    string or ``refine_steps`` steps have passed.  What is left in the reserve joins the bound."""
    if max_len is None:
        max_len = int(max(levels(l.n_rows, np.asarray(l.src), np.asarray(l.dst))))
    V = l.vocab
    st = dict(complete=[], bound=NEG, reserve=[], logz=None)

    def expand(open_):
        """eos of the open prefixes into the complete list; their extensions (mass, slot, label) in (slot, label) order"""
        cands = []
        for slot, (y, _) in enumerate(open_):
            nxt, eos, _, st["logz"] = next_log_probs(l, score, list(y), keep, marker)
            if eos > NEG:
                st["complete"].append((eos, y))
            live = [(float(nxt[v]), slot, v) for v in range(V) if nxt[v] > NEG]
            if len(y) >= max_len:
                if live:
                    st["bound"] = max(st["bound"], _lse(m for m, _, _ in live))
            else:
                cands += live
        st["complete"] = sorted(st["complete"], key=lambda e: -e[0])[:k]  # (stable: the earlier entry first)
        return cands

    def set_aside(entries):
        both = sorted(st["reserve"] + entries, key=lambda e: -e[0])  # (stable: the reserve's entries first, then in the order given)
        if len(both) > reserve:
            st["bound"] = max(st["bound"], both[reserve][0])
        st["reserve"] = both[:reserve]

    open_, open_at_stop, steps = [((), 0.0)], NEG, 0  # (prefix, mass): the empty prefix's mass is not needed
    for t in range(max_len + 1):
        steps += 1
        cands = sorted(expand(open_), key=lambda c: (-c[0], c[1], c[2]))
        set_aside([(m, open_[slot][0] + (v,)) for m, slot, v in cands[k:]])
        open_ = [(open_[slot][0] + (v,), m) for m, slot, v in cands[:k]]
        kth = st["complete"][k - 1][0] if len(st["complete"]) >= k else NEG
        if not any(m > kth for _, m in open_):
            open_at_stop = max([NEG] + [m for _, m in open_])
            break
    for _ in range(refine_steps):
        first = st["complete"][0][0] if st["complete"] else NEG
        if not st["reserve"] or not st["reserve"][0][0] > first:
            break
        steps += 1
        open_, st["reserve"] = [(y, m) for m, y in st["reserve"][:k]], st["reserve"][k:]
        set_aside([(m, open_[slot][0] + (v,)) for m, slot, v in expand(open_)])
    complete, logz = st["complete"], st["logz"]
    bound = max([st["bound"]] + [m for m, _ in st["reserve"][:1]])
    first = complete[0][0] if complete else NEG
    return dict(strings=[y for _, y in complete], log_prob=np.array([w - logz for w, _ in complete], F64),
                bound=bound - logz if bound > NEG else NEG, exact=bool(complete) and first >= bound and first >= open_at_stop,
                steps=steps)

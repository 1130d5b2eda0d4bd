"""NumPy float64 restatement of the prefix states (``nfst_string_prefix_extend``, ``nfst_string_prefix_state_next``) and of
``decoders.prefix_search(incremental=True)`` (test helper, not a test module), on one lattice in the engine's numbering
with one float64 score per arc (``edge_cases.score64``): a column of the prefix tables F0, F1 of include/nfst_hip.h per
prefix, the step from the column of a prefix to that of the prefix one symbol longer, and ``next`` from a column.  Sums
are ``_lse_rows`` (around the maximum), not the kernels' order: the results agree with the kernels' to round-off, not bit
for bit.  tests/test_strings_extend_cpu.py holds it to tests/strings_prefix_ref.py, which is held to brute force.
"""
from __future__ import annotations

import numpy as np

from tests import strings_prefix_ref as PR
from tests.strings_ref import F64, NEG


class Context:
    """What depends on the lattice, the scores and the tape but on no prefix"""

    def __init__(self, l, score, keep=None, marker=None):
        assert (keep is None) != (marker is None)
        self.l, self.score, self.keep, self.marker = l, np.asarray(score, F64), keep, marker
        self.kept = None if keep is None else set(int(x) for x in keep)
        self.src, self.dst, self.label, self.sink, self.arcs, self.by_depth = PR._graph(l)
        self.into = {}
        for a in self.arcs:
            self.into.setdefault(int(self.dst[a]), []).append(a)
        self.Zn0, _, self.Z = PR.suffix_tables(l, self.score, [], keep, marker)
        self.logz = float(self.Z[0])

    def dead(self) -> tuple:
        n = self.l.n_rows
        return np.full(n, NEG), np.full(n, NEG)

    def root(self) -> tuple:
        """Column 0: the empty prefix"""
        return self._sweep(None, None)

    def extend(self, col, symbol: int) -> tuple:
        """The column of the prefix of ``col`` followed by ``symbol``"""
        return self._sweep(col, int(symbol))

    def _sweep(self, parent, symbol) -> tuple:
        c0, c1 = self.dead()
        for s in self.by_depth:
            if s == 0:
                c0[s] = 0.0 if parent is None else NEG
                continue
            t0, t1 = [NEG], [NEG]
            for a in self.into.get(s, []):
                u, lab, w = int(self.src[a]), int(self.label[a]), self.score[a]
                match = parent is not None and lab == symbol
                if self.kept is not None:
                    if lab not in self.kept:
                        t0.append(w + c0[u])
                    elif match:
                        t0.append(w + parent[0][u])
                else:
                    (t1 if lab == self.marker else t0).append(w + c0[u])
                    if match:
                        t0.append(w + parent[1][u])
            c0[s], c1[s] = PR._lse(t0), PR._lse(t1)
        return c0, c1

    def next(self, col) -> tuple:
        """``(next [vocab], eos, log_prefix)`` of the prefix of ``col``, as ``strings_prefix_ref.next_log_probs`` forms them"""
        terms = [[] for _ in range(self.l.vocab)]
        for a in self.arcs:
            s, d, v = int(self.src[a]), int(self.dst[a]), int(self.label[a])
            if self.kept is not None:
                if v in self.kept:
                    terms[v].append((col[0][s] + self.score[a]) + self.Z[d])
            else:
                terms[v].append((col[1][s] + self.score[a]) + self.Zn0[d][0])
        nxt = np.array([PR._lse(t) for t in terms], F64)
        eos = float(col[0][self.sink])
        return nxt, eos, PR._lse([eos] + list(nxt))

    def state_of(self, y) -> tuple:
        col = self.root()
        for v in y:
            col = self.extend(col, v)
        return col


def prefix_search(l, score, k=8, max_len=None, keep=None, marker=None, reserve=64, refine_steps=32) -> dict:
    """``strings_prefix_ref.prefix_search`` with the first phase on columns: an open prefix carries its column, a pick
    extends its parent's column by its label; the second phase scores its prefixes from scratch.  Same result dict."""
    if max_len is None:
        max_len = int(max(PR.levels(l.n_rows, np.asarray(l.src), np.asarray(l.dst))))
    V = l.vocab
    ctx = Context(l, score, keep, marker)
    st = dict(complete=[], bound=NEG, reserve=[], logz=ctx.logz)

    def expand(open_, cols=None):
        cands = []
        for slot, (y, _) in enumerate(open_):
            if cols is not None:
                nxt, eos, _ = ctx.next(cols[slot])
            else:
                nxt, eos, _, _ = PR.next_log_probs(l, score, list(y), keep, marker)
            if eos > NEG:
                st["complete"].append((eos, y))
            live = [(float(nxt[v]), slot, v) for v in range(V) if nxt[v] > NEG]
            if len(y) >= max_len:
                if live:
                    st["bound"] = max(st["bound"], PR._lse(m for m, _, _ in live))
            else:
                cands += live
        st["complete"] = sorted(st["complete"], key=lambda e: -e[0])[:k]
        return cands

    def set_aside(entries):
        both = sorted(st["reserve"] + entries, key=lambda e: -e[0])
        if len(both) > reserve:
            st["bound"] = max(st["bound"], both[reserve][0])
        st["reserve"] = both[:reserve]

    open_, cols, open_at_stop, steps = [((), 0.0)], [ctx.root()], NEG, 0
    for t in range(max_len + 1):
        steps += 1
        cands = sorted(expand(open_, cols), key=lambda c: (-c[0], c[1], c[2]))
        set_aside([(m, open_[slot][0] + (v,)) for m, slot, v in cands[k:]])
        open_, cols = ([(open_[slot][0] + (v,), m) for m, slot, v in cands[:k]], [ctx.extend(cols[slot], v) for _, slot, v in cands[:k]])
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

"""NumPy float64 restatement of ``nfst_string_viterbi`` and ``nfst_string_sample`` on one lattice (test helper, not a test
module): the suffix table G of ``strings_ref.string_log_prob`` (the same terms in the same order, so G0[0][0] has its
bits) and its max-plus sibling V, both returned in full, and the two walks of include/nfst_hip.h over them.

A walk is in (s, j, f): state, symbols of y spelled, "the arc into s was an active marker".  ``Aligner.arcs_at`` lists
the out-arcs of s without self loops in canonical order with the cell each leads to.  The best alignment takes the first
arc whose term score + V[cell] equals V of the state; a draw takes the first arc of positive weight p_a = exp((score +
G[cell]) - G_f[s][j]) whose running sum exceeds u, and the last arc of positive weight if rounding leaves none.
``margin`` of a draw is that of ``positional_sample_ref``: the least distance over its steps between u and either
boundary of the chosen arc's interval (+inf where one arc alone has positive weight).

Also the inputs that tests/test_strings_align_cpu.py and tests/test_gpu_strings_align.py share (``sample_cases``), so
that the CPU file can hold the GPU file's cases to the cap on the undecided walks on the reference alone.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import strings_ref as SR
from tests.expectation_ref import levels, sink_of
from tests.positional_sample_ref import CAP, DECIDED  # noqa: F401  (the constants and the rule of the positional draws)

F64 = np.float64
NEG = -np.inf


class Aligner:
    """The tables and walks of one (lattice, float64 arc scores, string y, tape)."""

    def __init__(self, l, score, y, keep=None, marker=None):
        assert (keep is None) != (marker is None)
        self.l = l
        self.src, self.dst, self.label = (np.asarray(x, np.int64) for x in (l.src, l.dst, l.label))
        self.score = np.asarray(score, F64)
        self.y = np.asarray(y, np.int64).reshape(-1)
        self.n = n = len(self.y)
        self.kept = None if keep is None else set(int(x) for x in keep)
        self.marker = marker
        self.sink = sink = sink_of(l.n_rows, self.src, self.dst)
        depth = levels(l.n_rows, self.src, self.dst)
        self.out = [[] for _ in range(l.n_rows)]
        for a in range(len(self.src)):
            if self.src[a] != self.dst[a]:
                self.out[int(self.src[a])].append(a)
        self.out = [np.asarray(o, np.int64) for o in self.out]
        none = np.full(n + 1, NEG)
        y = self.y

        def shifted(row, lab):  # (j < n and y[j] == lab) ? row[j + 1] : -inf
            r = none.copy()
            r[:n] = np.where(y == lab, row[1:], NEG)
            return r

        # [plane, state, column]; rows of states that state 0 does not reach stay -inf
        self.G = np.full((2, l.n_rows, n + 1), NEG)
        self.V = np.full((2, l.n_rows, n + 1), NEG)
        for s in sorted((r for r in range(l.n_rows) if depth[r] >= 0), key=lambda r: -depth[r]):
            if s == sink:
                self.G[0, s] = self.V[0, s] = np.where(np.arange(n + 1) == n, 0.0, NEG)
                continue
            for T, fold in ((self.G, SR._lse_rows), (self.V, lambda t: np.max(np.asarray(t, F64), axis=0))):
                t0, t1 = [none], [none]
                for a in self.out[s]:
                    d, lab, w = int(self.dst[a]), int(self.label[a]), self.score[a]
                    with np.errstate(invalid="ignore"):
                        if self.kept is not None:
                            t0.append(w + (shifted(T[0, d], lab) if lab in self.kept else T[0, d]))
                        else:
                            t0.append(w + (T[1, d] if lab == marker else T[0, d]))
                            t1.append(w + shifted(T[0, d], lab))
                T[0, s], T[1, s] = fold(t0), fold(t1)
        self.log_num = float(self.G[0, 0, 0])
        self._steps = {}
        self.best = float(self.V[0, 0, 0])

    def arcs_at(self, s: int, j: int, f: int) -> tuple:
        """(arcs, column, plane, ok) of the out-arcs of s in canonical order: the cell (dst, column, plane) each leads
        to from (s, j, f); an arc that is off the string is not ok.  An arc emits position j when its column is j + 1."""
        arcs = self.out[s]
        lab = self.label[arcs]
        tok = int(self.y[j]) if j < self.n else -1
        hit = lab == tok if j < self.n else np.zeros(len(arcs), bool)
        if self.kept is not None:
            on = np.array([int(x) in self.kept for x in lab], bool)
            return arcs, np.where(on, j + 1, j), np.zeros(len(arcs), np.int64), ~on | hit
        if f:
            return arcs, np.full(len(arcs), j + 1), np.zeros(len(arcs), np.int64), hit
        return arcs, np.full(len(arcs), j), (lab == self.marker).astype(np.int64), np.ones(len(arcs), bool)

    def terms(self, T, s: int, j: int, f: int) -> tuple:
        arcs, col, plane, ok = self.arcs_at(s, j, f)
        with np.errstate(invalid="ignore"):
            t = self.score[arcs] + T[plane, self.dst[arcs], np.minimum(col, self.n)]
        return arcs, col, plane, np.where(ok, t, NEG)

    def _result(self, arcs, align, **more) -> dict:
        return dict(arcs=arcs, labels=[int(self.label[a]) for a in arcs], align=align, length=len(arcs), **more)

    def viterbi(self) -> dict:
        """{"arcs", "labels", "align", "length", "score"} of the best path that spells y (empty, -inf: none does)"""
        if not self.best > NEG:
            return self._result([], [], score=NEG)
        s, j, f, arcs, align = 0, 0, 0, [], []
        while s != self.sink:
            out, col, plane, t = self.terms(self.V, s, j, f)
            i = int(np.nonzero(t == self.V[f, s, j])[0][0])
            arcs.append(int(out[i]))
            align.append(j if col[i] > j else -1)
            s, j, f = int(self.dst[out[i]]), int(col[i]), int(plane[i])
        assert (j, f) == (self.n, 0)
        return self._result(arcs, align, score=self.best)

    def step_probs(self, s: int, j: int, f: int) -> tuple:
        """(arcs, column, plane, p, running sums of p, the indices of positive p) at (s, j, f); kept per state"""
        if (s, j, f) not in self._steps:
            out, col, plane, x = self.terms(self.G, s, j, f)
            with np.errstate(invalid="ignore", over="ignore"):
                p = np.exp(np.where(np.isnan(x), NEG, x) - self.G[f, s, j])
            self._steps[(s, j, f)] = (out, col, plane, p, np.cumsum(p), np.nonzero(p > 0.0)[0])
        return self._steps[(s, j, f)]

    def walk(self, u) -> dict:
        """{"arcs", "labels", "align", "length", "score", "logq", "margin"} of the draw that reads the uniforms u"""
        if not self.log_num > NEG:
            return self._result([], [], score=NEG, logq=0.0, margin=np.inf)
        s, j, f, arcs, align, S, margin = 0, 0, 0, [], [], 0.0, np.inf
        t = 0
        while s != self.sink:
            out, col, plane, p, cdf, ok = self.step_probs(s, j, f)
            hit = ok[cdf[ok] > float(u[t])]
            i = int(hit[0]) if len(hit) else int(ok[-1])
            if len(ok) > 1:
                margin = min(margin, abs(float(u[t]) - (cdf[i] - p[i])), abs(cdf[i] - float(u[t])))
            arcs.append(int(out[i]))
            align.append(j if col[i] > j else -1)
            S += float(self.score[out[i]])
            s, j, f = int(self.dst[out[i]]), int(col[i]), int(plane[i])
            t += 1
        assert (j, f) == (self.n, 0)
        return self._result(arcs, align, score=S, logq=S - self.log_num, margin=margin)

    def path_logq(self, arcs) -> float:
        """log of the product of the walk's step probabilities along a path that spells y"""
        s, j, f, lp = 0, 0, 0, 0.0
        for a in arcs:
            out, col, plane, x = self.terms(self.G, s, j, f)
            i = int(np.nonzero(out == a)[0][0])
            lp += float(x[i] - self.G[f, s, j])
            s, j, f = int(self.dst[a]), int(col[i]), int(plane[i])
        return lp


def uniforms(seed: int, shape) -> np.ndarray:
    """float32 in [0, 1): float64 draws cast to float32 (a cast that rounds up to 1 is pulled back)"""
    u = np.random.default_rng(seed).random(tuple(shape)).astype(np.float32)
    return np.minimum(u, np.nextafter(np.float32(1.0), np.float32(0.0)))


def longest(lats) -> int:
    """``ops._max_len`` of a batch: the longest path + 1"""
    return max(int(levels(l.n_rows, l.src, l.dst).max()) for l in lats) + 1


def rows(cands, N=None, tail=8) -> tuple:
    """(strings [B, M, N] int32 with ``tail`` behind every string, lengths [B, M])"""
    n = np.array([[len(y) for y in row] for row in cands], np.int32).reshape(len(cands), len(cands[0]))
    out = np.full((len(cands), len(cands[0]), max(1, int(n.max()) if N is None else N)), tail, np.int32)
    for b, row in enumerate(cands):
        for m, y in enumerate(row):
            out[b, m, :len(y)] = y
    return out, n


def aligners(case) -> list:
    """[b][m] -> Aligner of a case"""
    from tests.edge_cases import score64

    out, a0 = [], 0
    for b, l in enumerate(case["lats"]):
        th = case["theta"][b] if np.ndim(case["theta"]) == 2 else case["theta"]
        s64 = score64(l, th, None if case["asc"] is None else case["asc"][a0:a0 + l.n_arcs])
        a0 += l.n_arcs
        out.append([Aligner(l, s64, y, **case["tape"]) for y in case["cands"][b]])
    return out


def first_path_labels(l) -> list:
    """the labels along the first arc out of every state that is no self loop"""
    first = np.searchsorted(l.src, np.arange(l.n_rows + 1))
    s, sink, labs = 0, sink_of(l.n_rows, l.src, l.dst), []
    while s != sink:
        a = next(a for a in range(int(first[s]), int(first[s + 1])) if l.dst[a] != s)
        labs.append(int(l.label[a]))
        s = int(l.dst[a])
    return labs


def random_path_labels(l, seed: int) -> list:
    """the labels of a path that ``default_rng(seed)`` walks, uniform over each state's out-arcs that are not self loops"""
    rng = np.random.default_rng(seed)
    first = np.searchsorted(l.src, np.arange(l.n_rows + 1))
    s, sink, labs = 0, sink_of(l.n_rows, l.src, l.dst), []
    while s != sink:
        arcs = [a for a in range(int(first[s]), int(first[s + 1])) if l.dst[a] != s]
        a = arcs[int(rng.integers(len(arcs)))]
        labs.append(int(l.label[a]))
        s = int(l.dst[a])
    return labs


def _case(lats, theta, tape, cands, K, seed, asc=None, N=None, tail=8) -> dict:
    L = longest(lats)
    return dict(lats=lats, theta=theta, asc=asc, tape=tape, cands=cands, K=K, N=N, tail=tail, L=L,
                uniforms=uniforms(seed, (len(lats), len(cands[0]), K, L)))


@functools.lru_cache(maxsize=None)
def sample_cases() -> dict:
    """The cases of the GPU file's draws with given uniforms, and of its best alignments: name -> {lats, theta ([V] or
    [B, V]), asc, tape, cands [b][m], K, N (row stride or None), tail, L (max_len), uniforms [B, M, K, L]}."""
    from nfst_amd import synth
    from tests import edge_cases as E
    from tests import intersect_wide_ref as IW

    out = {}
    # the marker tape's corners: every string the lattice spells, a symbol equal to the marker among them, the empty
    # string, one no path spells, one symbol more and one less than a path spells
    l = SR.tape_lattice()
    theta = synth.label_scores(3, l.vocab, mean=-1.0, std=0.5)
    by, _, _ = SR.brute_force(l, E.score64(l, theta), marker=SR.MARK)
    ys = sorted(by, key=lambda y: -by[y])
    out["tape"] = _case([l], theta, dict(marker=SR.MARK), [[list(y) for y in ys] + [[], [9, 9], list(ys[0]) + [8], list(ys[0])[:-1]]], 64, 1)
    # 200 live arcs in four chunks; and one live arc per string, in chunks 0, 1 and 3
    star = E.star()
    th_star = synth.label_scores(5, star.vocab, mean=-1.0, std=0.5)
    out["star keep 5"] = _case([star], th_star, dict(keep={5}), [[[5]]], 65, 2)
    every = set(range(star.vocab))
    out["star keep all"] = _case([star], th_star, dict(keep=every), [[[E.BOS, 3 + i, 5, E.EOS] for i in (0, 70, 199)]], 1, 3)
    df = E.double_funnel()
    out["double funnel"] = _case([df], synth.label_scores(6, df.vocab, mean=-1.0, std=0.5), dict(keep={5, 6}), [[[5, 6], [5], [6, 5]]], 64, 4)
    # per-lattice theta, per-arc scores and the tables' weights in one launch
    wb = E.weighted_batch()
    Vw = wb[0].vocab
    rng = np.random.default_rng(7)
    th = rng.normal(-1.0, 0.6, size=(len(wb), Vw)).astype(np.float32)
    asc = rng.normal(0.0, 0.4, size=sum(l.n_arcs for l in wb)).astype(np.float32)
    keep = set(range(3, Vw, 3))
    cands = []
    for b, l in enumerate(wb):
        y = list(SR.project(random_path_labels(l, 10 + b), keep=keep))
        cands.append([y, list(SR.project(first_path_labels(l), keep=keep)), y[:-1] + [Vw - 1]])
    out["mixed"] = _case(wb, th, dict(keep=keep), cands, 3, 5, asc=asc)
    cands = []
    for b, l in enumerate(wb):
        y = list(SR.project(random_path_labels(l, 20 + b), marker=5))
        cands.append([y, list(SR.project(first_path_labels(l), marker=5)), []])
    out["mixed marker"] = _case(wb, th, dict(marker=5), cands, 3, 6, asc=asc)
    # strips of 64 columns: N + 1 in {1, 2, 64, 65, 66, 129}, one candidate each with nothing behind it
    grid = IW.edit_denominator([6], [8, 9], 129, vocab=12)
    th_grid = synth.label_scores(4, 12, mean=-1.0, std=0.5)
    rng = np.random.default_rng(2)
    pool = {n: [int(t) for t in rng.integers(8, 10, size=n)] for n in (0, 1, 63, 64, 65, 128)}
    for n, y in pool.items():
        for name, tape in (("marker", dict(marker=SR.MARK)), ("keep", dict(keep={8, 9}))):
            out[f"strip {n} {name}"] = _case([grid], th_grid, tape, [[y]], 2, 100 + n, N=max(n, 1))
    # candidates of different lengths in one launch, with a tail behind each that must not be read: M in {3, 65}
    for M in (3, 65):
        lens = [65, 0, 63] if M == 3 else [int(x) for x in np.random.default_rng(3).integers(0, 20, size=65)]
        cands = [[[int(t) for t in np.random.default_rng(50 + i).integers(8, 10, size=n)] for i, n in enumerate(lens)]]
        out[f"mixed lengths {M}"] = _case([grid], th_grid, dict(marker=SR.MARK), cands, 1 if M == 65 else 2, 200 + M, N=130)
    # the 1200-state lattice whose product with the string's automaton does not fit
    l, keep, y = SR.layered_case()
    out["layered"] = _case([l], synth.label_scores(2, 12), dict(keep=keep), [[y, y[:-1], y + [3]]], 4, 8)
    return out

"""NumPy restatement of ``nfst_positional_sample`` / ``nfst_positional_score_paths`` on one lattice (test helper, not a
test module): the beta rows of ``positional_ref.sum_product`` in float64, then the walk of include/nfst_hip.h.

At position t in state s the out-arcs of s without self loops, in canonical order, have
    p_a = exp(score[a] + pos[t, label(a)] + beta_{t+1}(dst_a) - beta_t(s))
and the walk takes the first arc of positive weight whose running sum exceeds u; if rounding leaves none, the last arc
of positive weight.  ``margin`` of a walk is the smallest distance, over its steps, between u and either boundary of the
chosen arc's interval of the CDF (+inf where the chosen arc is the only one of positive weight): a walk whose margin is
above the engine's error is decided, whatever the rounding.

Also the inputs the CPU and the GPU tests share (``small_uniforms``, ``DECIDED``, ``undecided_cap``), so that the CPU
file can hold the GPU file's cases to the cap on the reference alone.
"""
from __future__ import annotations

import numpy as np

from tests.expectation_ref import sink_of
from tests.positional_ref import NEG

DECIDED = 1e-6  # a walk is decided when its margin exceeds this (float64 engine, float32 uniforms)
CAP = 0.01  # no comparison may leave out more than this share of its walks
K_SMALL = 64


def uniforms(seed: int, K: int, T: int) -> np.ndarray:
    """[K, T] float32 in [0, 1): float64 draws cast to float32 (a cast that rounds up to 1 is pulled back)."""
    u = np.random.default_rng(seed).random((K, T)).astype(np.float32)
    return np.minimum(u, np.nextafter(np.float32(1.0), np.float32(0.0)))


def small_uniforms(i: int, T: int, K: int = K_SMALL) -> np.ndarray:
    """The uniforms of lattice i of the six small lattices at truncation T."""
    return uniforms(7 * i + T, K, T)


def beta_rows(l, score, pos, T: int) -> np.ndarray:
    """log beta_t(s) [T + 1, n] in float64, as ``positional_ref.sum_product`` computes them."""
    n, sink = l.n_rows, sink_of(l.n_rows, l.src, l.dst)
    live = np.nonzero(l.src != l.dst)[0]
    s, d, lab = l.src[live].astype(np.int64), l.dst[live].astype(np.int64), l.label[live].astype(np.int64)
    sc = np.asarray(score, np.float64)[live]
    P = None if pos is None else np.asarray(pos, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        beta = np.full((T + 1, n), NEG)
        beta[:, sink] = 0.0
        for t in range(T - 1, -1, -1):
            term = (sc if P is None else sc + P[t, lab]) + beta[t + 1, d]
            row = np.full(n, NEG)
            np.logaddexp.at(row, s, np.where(np.isnan(term), NEG, term))
            row[sink] = 0.0
            beta[t] = row
    return beta


class Sampler:
    """The walks of one lattice under (score [A] float64, pos [T, V] or None, T)."""

    def __init__(self, l, score, pos, T: int):
        self.l, self.T = l, T
        self.score = np.asarray(score, np.float64)
        self.P = None if pos is None else np.asarray(pos, np.float64)
        self.beta = beta_rows(l, score, pos, T)
        self.logz = float(self.beta[0, 0])
        self.sink = sink_of(l.n_rows, l.src, l.dst)
        order = np.nonzero(l.src != l.dst)[0]
        self.out = [order[l.src[order] == s] for s in range(l.n_rows)]  # canonical order within a state

    def arc_logw(self, t: int, arcs) -> np.ndarray:
        x = self.score[arcs]
        return x if self.P is None else x + self.P[t, self.l.label[arcs]]

    def step_probs(self, t: int, s: int):
        """(the out-arcs of s, their probabilities at position t)."""
        arcs = self.out[s]
        with np.errstate(invalid="ignore", over="ignore"):
            x = self.arc_logw(t, arcs) + self.beta[t + 1, self.l.dst[arcs]] - self.beta[t, s]
            p = np.exp(np.where(np.isnan(x), NEG, x))
        return arcs, p

    def path_logprob(self, arcs) -> float:
        """log of the product of the per-step probabilities along a path (-inf if the path is longer than T)."""
        if len(arcs) > self.T:
            return NEG
        s, lp = 0, 0.0
        for t, a in enumerate(arcs):
            out, p = self.step_probs(t, s)
            with np.errstate(divide="ignore"):
                lp += float(np.log(p[int(np.nonzero(out == a)[0][0])]))
            s = int(self.l.dst[a])
        return lp if s == self.sink else NEG

    def path_score(self, arcs) -> float:
        return float(sum(self.arc_logw(t, np.asarray([a]))[0] for t, a in enumerate(arcs)))

    def walk(self, u) -> dict:
        """{"arcs", "labels", "length", "logq", "margin"} of the walk that reads the uniforms u [T]."""
        if not np.isfinite(self.logz):
            return {"arcs": [], "labels": [], "length": 0, "logq": 0.0, "margin": np.inf}
        s, arcs, S, margin = 0, [], 0.0, np.inf
        for t in range(self.T):
            if s == self.sink:
                break
            out, p = self.step_probs(t, s)
            cdf = np.cumsum(p)
            ok = np.nonzero(p > 0.0)[0]
            hit = ok[cdf[ok] > float(u[t])]
            j = int(hit[0]) if len(hit) else int(ok[-1])
            if len(ok) > 1:
                lo = cdf[j] - p[j]
                margin = min(margin, abs(float(u[t]) - lo), abs(cdf[j] - float(u[t])))
            a = int(out[j])
            arcs.append(a)
            S += float(self.arc_logw(t, np.asarray([a]))[0])
            s = int(self.l.dst[a])
        assert s == self.sink
        return {"arcs": arcs, "labels": [int(self.l.label[a]) for a in arcs], "length": len(arcs), "logq": S - self.logz,
                "margin": margin}

    def walks(self, U) -> list:
        return [self.walk(u) for u in U]


def undecided(walks, threshold: float = DECIDED) -> int:
    return sum(w["margin"] <= threshold for w in walks)


def forced_score(l, score, pos, marks) -> tuple:
    """(path score float64, end state, length) of the forced walk of ``marks`` from state 0: the arc of the current state
    with the mark's label scores score[a] + pos[t, label]; the sink's pad loop scores nothing and ends the count; a mark
    without an arc gives (-inf, 0, the marks consumed so far)."""
    P = None if pos is None else np.asarray(pos, np.float64)
    s, tot, n, counting = 0, 0.0, 0, True
    for t, mk in enumerate(marks):
        a = np.nonzero((l.src == s) & (l.label == mk))[0]
        if len(a) == 0:
            return NEG, 0, n
        a = int(a[0])
        d = int(l.dst[a])
        if d != s:
            with np.errstate(invalid="ignore"):
                tot += float(score[a]) + (0.0 if P is None else float(P[t, mk]))
            n += counting
        else:
            counting = False
        s = d
    return tot, s, n

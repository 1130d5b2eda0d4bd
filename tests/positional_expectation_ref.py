"""NumPy restatement of ``nfst_positional_expectation`` on one lattice, in float64 (test helper, not a test module; beside
tests/positional_ref.py, whose ``arc_score64`` and ``enumerate_paths`` it uses).

Paths, positions and truncation are those of ``positional_ref.sum_product``.  The arc at position t carries
    v_t(a) = pos_values[t, label] + label_values[label] + arc_values[a] + coef * (score[a] + pos[t, label])
(every term optional); a term of weight zero (score or pos entry at -inf) has no value: its entries may be anything.

``expectation``  alpha_t / beta_t in the log domain and the conditional expectations
                     R_t(s)       = sum_a exp(w_t(a) + beta_{t+1}(d) - beta_t(s)) (v_t(a) + R_{t+1}(d))
                     R^alpha_{t+1}(d) = sum_a exp(alpha_t(s) + w_t(a) - alpha_{t+1}(d)) (R^alpha_t(s) + v_t(a))
                 then c_{a,t} = P(a at t) (R^alpha_t(s) + v_t(a) + R_{t+1}(d) - E[V])
``brute_force``  the same quantities path by path
"""
from __future__ import annotations

import numpy as np

from tests.expectation_ref import sink_of
from tests.positional_ref import NEG, enumerate_paths

KEYS = ("logz", "ev", "M", "pos_post", "arc_post", "pos_cov", "arc_cov")


def tables(l, score, pos, T: int, pos_values=None, label_values=None, arc_values=None, coef: float = 0.0):
    """(W [T, A] float64 log weight of every arc at every position, -inf where it is zero or the arc is a self loop;
    Vt [T, A] its value, 0 where the weight is zero)."""
    lab = l.label.astype(np.int64)
    sc = np.asarray(score, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        W = np.repeat(sc[None, :], T, axis=0)
        if pos is not None:
            W = W + np.asarray(pos, np.float64)[:, lab]
        W = np.where(np.isnan(W) | (l.src == l.dst)[None, :], NEG, W)
        Vt = np.zeros((T, l.n_arcs))
        if pos_values is not None:
            Vt = Vt + np.asarray(pos_values, np.float64)[:, lab]
        if label_values is not None:
            Vt = Vt + np.asarray(label_values, np.float64)[lab][None, :]
        if arc_values is not None:
            Vt = Vt + np.asarray(arc_values, np.float64)[None, :]
        if coef != 0.0:
            Vt = Vt + float(coef) * W
    return W, np.where(np.isfinite(W), Vt, 0.0)


def _empty(l, T):
    return {"logz": NEG, "ev": 0.0, "M": 0.0, "pos_post": np.zeros((T, l.vocab)), "arc_post": np.zeros(l.n_arcs),
            "pos_cov": np.zeros((T, l.vocab)), "arc_cov": np.zeros(l.n_arcs)}


def expectation(l, score, pos, T: int, pos_values=None, label_values=None, arc_values=None, coef: float = 0.0) -> dict:
    """{"logz", "ev", "M" = sum_{t,a} P(a at t) |v_t(a)|, "pos_post" [T, V], "arc_post" [A], "pos_cov" [T, V], "arc_cov"
    [A]} in float64.  ``score`` [A] float64 (``positional_ref.arc_score64``), ``pos`` / ``pos_values`` [T, V] or None,
    ``label_values`` [V] or None, ``arc_values`` [A] or None."""
    n, sink = l.n_rows, sink_of(l.n_rows, l.src, l.dst)
    s, d, lab = l.src.astype(np.int64), l.dst.astype(np.int64), l.label.astype(np.int64)
    W, Vt = tables(l, score, pos, T, pos_values, label_values, arc_values, coef)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        beta = np.full((T + 1, n), NEG)
        beta[:, sink] = 0.0
        Rb = np.zeros((T + 1, n))
        for t in range(T - 1, -1, -1):
            term = W[t] + beta[t + 1, d]
            row = np.full(n, NEG)
            np.logaddexp.at(row, s, term)
            row[sink] = 0.0
            beta[t] = row
            share = np.where(np.isfinite(term), np.exp(term - row[s]), 0.0)
            np.add.at(Rb[t], s, share * (Vt[t] + Rb[t + 1, d]))
            Rb[t, sink] = 0.0
        logz = float(beta[0, 0])
        if not np.isfinite(logz):
            return _empty(l, T)
        out = _empty(l, T)
        out["logz"], out["ev"] = logz, float(Rb[0, 0])
        alpha = np.full(n, NEG)
        alpha[0] = 0.0
        Ra = np.zeros(n)
        for t in range(T):
            term = alpha[s] + W[t]
            nxt = np.full(n, NEG)
            np.logaddexp.at(nxt, d, term)
            share = np.where(np.isfinite(term), np.exp(term - nxt[d]), 0.0)
            so_far = Ra[s] + Vt[t]
            nRa = np.zeros(n)
            np.add.at(nRa, d, share * so_far)
            lp = term + beta[t + 1, d] - logz
            p = np.where(np.isfinite(lp), np.exp(lp), 0.0)
            c = p * (so_far + Rb[t + 1, d] - out["ev"])
            out["M"] += float((p * np.abs(Vt[t])).sum())
            np.add.at(out["pos_post"][t], lab, p)
            np.add.at(out["pos_cov"][t], lab, c)
            out["arc_post"] += p
            out["arc_cov"] += c
            nxt[sink] = NEG  # nothing leaves the sink
            alpha, Ra = nxt, nRa
    return out


def brute_force(l, score, pos, T: int, pos_values=None, label_values=None, arc_values=None, coef: float = 0.0, paths=None) -> dict:
    """The quantities of ``expectation``, path by path: c_{a,t} = sum_pi p(pi) 1[a at t] (V(pi) - E[V]); also "H" =
    -sum p log p and "S", "V", "p" per path that fits."""
    paths = enumerate_paths(l) if paths is None else paths
    W, Vt = tables(l, score, pos, T, pos_values, label_values, arc_values, coef)
    fit = [p for p in paths if len(p) <= T]
    S = np.array([sum(W[t, a] for t, a in enumerate(p)) for p in fit], np.float64)
    Vp = np.array([sum(Vt[t, a] for t, a in enumerate(p)) for p in fit], np.float64)
    ok = np.isfinite(S)
    out = _empty(l, T)
    out.update(H=0.0, S=S, V=Vp, p=np.zeros(len(fit)))
    if not ok.any():
        return out
    logz = float(np.logaddexp.reduce(S[ok]))
    pp = np.where(ok, np.exp(np.where(ok, S, 0.0) - logz), 0.0)
    ev = float((pp * np.where(ok, Vp, 0.0)).sum())
    out.update(logz=logz, ev=ev, p=pp, H=float(-(pp[ok] * (S[ok] - logz)).sum()))
    for p, w, val in zip(fit, pp, Vp):
        if w == 0.0:
            continue
        for t, a in enumerate(p):
            out["pos_post"][t, l.label[a]] += w
            out["arc_post"][a] += w
            out["pos_cov"][t, l.label[a]] += w * (val - ev)
            out["arc_cov"][a] += w * (val - ev)
            out["M"] += w * abs(Vt[t, a])
    return out

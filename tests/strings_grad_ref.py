"""NumPy float64 restatement of ``nfst_string_logprob_grad`` (test helper, not a test module): the suffix tables G, G0,
G1 and z of ``strings_ref.string_log_prob``, the prefix tables F, F0, F1 and az of include/nfst_hip.h over one lattice
in the engine's numbering, and from them the posterior of every canonical arc among the paths that spell a string and
among all paths, and ``grad_arc``.  Also the same quantities by brute force over every path.
tests/test_strings_grad_cpu.py holds the two to each other and to central differences of ``strings_ref``.
"""
from __future__ import annotations

import numpy as np

from tests import strings_ref as SR
from tests.expectation_ref import levels, sink_of

F64 = np.float64
NEG = -np.inf


def tables(l, score, y, keep=None, marker=None) -> dict:
    """G0, G1, Z (suffixes, as ``strings_ref.string_log_prob`` builds them) and F0, F1, AZ (prefixes) of the states that
    state 0 reaches, each row over the columns 0 .. n; in keep mode G1 and F1 stay -inf."""
    assert (keep is None) != (marker is None)
    src, dst, label = np.asarray(l.src, np.int64), np.asarray(l.dst, np.int64), np.asarray(l.label, np.int64)
    score = np.asarray(score, F64)
    y = np.asarray(y, np.int64).reshape(-1)
    n = len(y)
    sink = sink_of(l.n_rows, src, dst)
    depth = levels(l.n_rows, src, dst)
    out, inn = [[] for _ in range(l.n_rows)], [[] for _ in range(l.n_rows)]
    for a in range(len(src)):  # (canonical order on both sides)
        if src[a] != dst[a] and depth[src[a]] >= 0:
            out[int(src[a])].append(a)
            inn[int(dst[a])].append(a)
    kept = None if keep is None else set(int(x) for x in keep)
    none = np.full(n + 1, NEG)

    def down(row, lab):  # (j < n and y[j] == lab) ? row[j + 1] : -inf
        r = none.copy()
        r[:n] = np.where(y == lab, row[1:], NEG)
        return r

    def up(row, lab):  # (j >= 1 and y[j - 1] == lab) ? row[j - 1] : -inf
        r = none.copy()
        r[1:] = np.where(y == lab, row[:n], NEG)
        return r

    reach = [r for r in range(l.n_rows) if depth[r] >= 0]
    G0, G1, Z, F0, F1, AZ = {}, {}, {}, {}, {}, {}
    for s in sorted(reach, key=lambda r: -depth[r]):
        if s == sink:
            G0[s], G1[s], Z[s] = np.where(np.arange(n + 1) == n, 0.0, NEG), none.copy(), 0.0
            continue
        t0, t1, tz = [none], [none], [np.array(NEG)]
        for a in out[s]:
            d, lab, w = int(dst[a]), int(label[a]), score[a]
            tz.append(np.array(w + Z[d]))
            if kept is not None:
                t0.append(w + (down(G0[d], lab) if lab in kept else G0[d]))
            else:
                t0.append(w + (G1[d] if lab == marker else G0[d]))
                t1.append(w + down(G0[d], lab))
        G0[s], G1[s], Z[s] = SR._lse_rows(t0), SR._lse_rows(t1), float(SR._lse_rows(tz))
    for s in sorted(reach, key=lambda r: depth[r]):
        if s == 0:
            F0[s], F1[s], AZ[s] = np.where(np.arange(n + 1) == 0, 0.0, NEG), none.copy(), 0.0
            continue
        t0, t1, tz = [none], [none], [np.array(NEG)]
        for a in inn[s]:
            u, lab, w = int(src[a]), int(label[a]), score[a]
            tz.append(np.array(w + AZ[u]))
            if kept is not None:
                t0.append(w + (up(F0[u], lab) if lab in kept else F0[u]))
            else:
                (t1 if lab == marker else t0).append(w + F0[u])
                t0.append(w + up(F1[u], lab))
        F0[s], F1[s], AZ[s] = SR._lse_rows(t0), SR._lse_rows(t1), float(SR._lse_rows(tz))
    return dict(G0=G0, G1=G1, Z=Z, F0=F0, F1=F1, AZ=AZ, n=n, y=y, kept=kept, marker=marker, sink=sink)


def _exp_sum(t) -> float:
    t = np.asarray(t, F64)
    return float(np.exp(t[t > NEG]).sum())


def posteriors(l, score, y, keep=None, marker=None) -> tuple:
    """``(post_y [n_arcs], post_z [n_arcs], log_num, logz)``: of every canonical arc its share of the weight of the paths
    that spell y (zeros when none does) and of all paths (zeros when there is none)."""
    t = tables(l, score, y, keep, marker)
    src, dst, label = np.asarray(l.src, np.int64), np.asarray(l.dst, np.int64), np.asarray(l.label, np.int64)
    score = np.asarray(score, F64)
    n, yy = t["n"], t["y"]
    log_num, logz = float(t["G0"][0][0]), float(t["Z"][0])
    py, pz = np.zeros(len(src)), np.zeros(len(src))
    for a in range(len(src)):
        s, d, lab, w = int(src[a]), int(dst[a]), int(label[a]), score[a]
        if s == d or s not in t["F0"] or d not in t["G0"]:
            continue
        if logz > NEG:
            pz[a] = _exp_sum([t["AZ"][s] + w + t["Z"][d] - logz])
        if not log_num > NEG:
            continue
        match = np.concatenate([yy == lab, [False]])  # j < n and y[j] == lab
        nxt = np.concatenate([t["G0"][d][1:], [NEG]])  # G0[d][j + 1]
        if t["kept"] is not None:
            if lab in t["kept"]:
                py[a] = _exp_sum((t["F0"][s] + w + nxt - log_num)[match])
            else:
                py[a] = _exp_sum(t["F0"][s] + w + t["G0"][d] - log_num)
        else:
            py[a] = _exp_sum(t["F0"][s] + w + (t["G1"] if lab == t["marker"] else t["G0"])[d] - log_num) \
                + _exp_sum((t["F1"][s] + w + nxt - log_num)[match])
    return py, pz, log_num, logz


def grad_arc(l, score, cands, g_num, g_z, keep=None, marker=None) -> np.ndarray:
    """grad_arc of one lattice: g_z post_z + the sum over its candidates ``cands`` of g_num[m] post_m, in ascending m; a
    candidate with g_num[m] == 0 is left out."""
    known = {}  # (candidate lists repeat their strings)

    def post(y):
        if tuple(y) not in known:
            known[tuple(y)] = posteriors(l, score, y, keep, marker)
        return known[tuple(y)]

    g = g_z * post(cands[0] if len(cands) else [])[1]
    for m, y in enumerate(cands):
        if g_num[m] != 0:
            g = g + g_num[m] * post(y)[0]
    return g


def of_batch(lats, theta, cands, g_num, g_z, keep=None, marker=None, asc=None) -> np.ndarray:
    """grad_arc [total_arcs] for per-lattice candidate lists ``cands[b]``, g_num [B, M] and g_z [B]; theta [V] or [B, V],
    asc over the batch's arcs (``strings_ref.of_batch``'s arguments)."""
    from tests.edge_cases import score64

    out, a0 = [], 0
    for b, l in enumerate(lats):
        th = theta[b] if np.ndim(theta) == 2 else theta
        s64 = score64(l, th, None if asc is None else asc[a0:a0 + l.n_arcs])
        a0 += l.n_arcs
        out.append(grad_arc(l, s64, cands[b], np.asarray(g_num, F64)[b], float(np.asarray(g_z, F64)[b]), keep, marker) if l.n_arcs
                   else np.zeros(0))
    return np.concatenate(out) if out else np.zeros(0)


def brute_posteriors(l, score, keep=None, marker=None) -> tuple:
    """``({string: post_y [n_arcs]}, post_z [n_arcs], dangling [n_arcs], D)`` by enumeration of every path: the share of
    a string's path weight that passes through each arc, the same over all paths, and in marker mode the gradient of
    the share D of the paths that end on an active marker (zeros and 0.0 in keep mode)."""
    by, logz, paths = SR.brute_force(l, score, keep, marker)
    A = len(np.asarray(l.src))
    lab = np.asarray(l.label)
    num = {y: np.zeros(A) for y in by}
    pz, dang, D = np.zeros(A), np.zeros(A), 0.0
    for sc, p in paths:
        p = np.asarray(p, np.int64)
        pz[p] += np.exp(sc - logz)
        if marker is not None and SR.dangling(lab[p], marker):
            dang[p] += np.exp(sc - logz)
            D += float(np.exp(sc - logz))
            continue
        y = SR.project(lab[p], keep, marker)
        num[y][p] += np.exp(sc - by[y])
    return num, pz, dang - D * pz, D

"""NumPy restatements of ``nfst_merge_paths`` and ``nfst_string_logprob`` (test helper, not a test module): the projection
of a label sequence onto the output tape, the merge of a path set by projected string with the weights' arithmetic
operation for operation (so that the float64 bits are the kernel's), the recurrence of include/nfst_hip.h over one
lattice in float64 log weights with the arcs in canonical order, and a brute force over every path.
tests/test_strings_cpu.py holds them to each other and to ``intersect_wide_ref.live_sets`` on the matching automata.
"""
from __future__ import annotations

import numpy as np

from tests import kbest_ref
from tests.expectation_ref import levels, sink_of

F64 = np.float64
NEG = -np.inf


# ----------------------------------------------------------------------------- the tape
def project(labels, keep=None, marker=None) -> tuple:
    """The string of a label sequence: with ``keep`` its labels that belong to the set; with ``marker`` the labels that
    directly follow an active marker (a label that follows one is a symbol even if it is the marker, and it is then not
    active itself; a marker with nothing behind it yields nothing); with neither the sequence itself."""
    labels = [int(x) for x in labels]
    if keep is not None:
        assert marker is None
        keep = set(int(x) for x in keep)
        return tuple(x for x in labels if x in keep)
    if marker is None:
        return tuple(labels)
    out, armed = [], False
    for x in labels:
        if armed:
            out.append(x)
            armed = False
        else:
            armed = x == marker
    return tuple(out)


def dangling(labels, marker) -> bool:
    """The sequence ends on an active marker: it spells no string."""
    armed = False
    for x in labels:
        armed = (not armed) and int(x) == marker
    return armed


# ----------------------------------------------------------------------------- the merged weight's arithmetic
_EXP_C = [1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0,
          1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0]
_LOG_C = [1.0 / 23.0, 1.0 / 21.0, 1.0 / 19.0, 1.0 / 17.0, 1.0 / 15.0, 1.0 / 13.0, 1.0 / 11.0, 1.0 / 9.0, 1.0 / 7.0, 1.0 / 5.0,
          1.0 / 3.0, 1.0]


def sm_exp(x: float) -> float:
    """exp(x), x <= 0, in IEEE products and sums one by one (Python floats are float64 and never fused)."""
    x = float(x)
    if not x > -700.0:
        return 0.0
    k = float(np.rint(x * 1.4426950408889634))
    t = (x - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10
    p = _EXP_C[0]
    for c in _EXP_C[1:]:
        p = p * t + c
    return float(np.ldexp(p, int(k)))


def sm_log(s: float) -> float:
    """log(s), s >= 1: 2 atanh((m - 1) / (m + 1)) of the mantissa plus e ln 2."""
    m, e = np.frexp(float(s))
    m, e = float(m), int(e)
    if m < 0.70710678118654752:
        m = m * 2.0
        e -= 1
    f = m - 1.0
    z = f / (2.0 + f)
    z2 = z * z
    p = _LOG_C[0]
    for c in _LOG_C[1:]:
        p = p * z2 + c
    return float(e) * 0.6931471805599453 + (2.0 * z) * p


def merged_weight(ws) -> float:
    """max + log(sum exp(w - max)) over ``ws`` in the order given"""
    mx = max(ws)
    s = 0.0
    for w in ws:
        s += sm_exp(float(w) - mx)
    return mx + sm_log(s)


# ----------------------------------------------------------------------------- the merge
def merge(paths, lengths, log_weights, n_paths=None, keep=None, marker=None, pad=0) -> dict:
    """Every output of ``nfst_merge_paths``: strings, lengths, log_weights (float64), n_strings, group, first.  A length
    outside [0, L] makes the row invalid (the kernel also sets its status word)."""
    paths, lengths = np.asarray(paths, np.int64), np.asarray(lengths, np.int64)
    w = np.asarray(log_weights, F64)
    B, K, L = paths.shape
    out = {"strings": np.full((B, K, L), pad, np.int32), "lengths": np.zeros((B, K), np.int32), "log_weights": np.full((B, K), NEG),
           "n_strings": np.zeros(B, np.int32), "group": np.full((B, K), -1, np.int32), "first": np.full((B, K), -1, np.int32)}
    for b in range(B):
        n_in = K if n_paths is None else int(n_paths[b])
        members = {}  # string -> rows, ascending (dicts keep the order of insertion: by lowest member)
        for k in range(K):
            if k < n_in and w[b, k] > NEG and 0 <= lengths[b, k] <= L:
                members.setdefault(project(paths[b, k, :lengths[b, k]], keep, marker), []).append(k)
        entries = []
        for y, rows in members.items():
            ws = [float(w[b, k]) for k in rows]
            entries.append((merged_weight(ws), rows[0], rows[int(np.argmax(ws))], y, rows))  # (argmax: the first maximum)
        entries.sort(key=lambda e: (-e[0], e[1]))
        out["n_strings"][b] = len(entries)
        for r, (mw, _, first, y, rows) in enumerate(entries):
            out["strings"][b, r, :len(y)] = y
            out["lengths"][b, r] = len(y)
            out["log_weights"][b, r] = mw
            out["first"][b, r] = first
            out["group"][b, rows] = r
    return out


# ----------------------------------------------------------------------------- the recurrence
def _lse_rows(terms) -> np.ndarray:
    """log of the sum of exp over axis 0, -inf where every term is -inf"""
    t = np.asarray(terms, F64)
    mx = t.max(axis=0)
    safe = np.where(mx > NEG, mx, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(mx > NEG, safe + np.log(np.exp(t - safe).sum(axis=0)), NEG)


def string_log_prob(l, score, y, keep=None, marker=None) -> tuple:
    """``(log_num, logz)`` of the string ``y`` on one lattice in the engine's numbering; ``score``: float64 per arc
    (``edge_cases.score64``).  G[s][j] as include/nfst_hip.h states it, one row per state (two in marker mode)."""
    assert (keep is None) != (marker is None)
    src, dst, label = np.asarray(l.src, np.int64), np.asarray(l.dst, np.int64), np.asarray(l.label, np.int64)
    score = np.asarray(score, F64)
    y = np.asarray(y, np.int64).reshape(-1)
    n = len(y)
    sink = sink_of(l.n_rows, src, dst)
    depth = levels(l.n_rows, src, dst)
    out = [[] for _ in range(l.n_rows)]
    for a in range(len(src)):
        if src[a] != dst[a]:
            out[int(src[a])].append(a)
    kept = None if keep is None else set(int(x) for x in keep)
    none = np.full(n + 1, NEG)
    G0, G1, Z = {}, {}, {}

    def shifted(row, lab):  # (j < n and y[j] == lab) ? row[j + 1] : -inf
        r = none.copy()
        r[:n] = np.where(y == lab, row[1:], NEG)
        return r

    for s in sorted((r for r in range(l.n_rows) if depth[r] >= 0), key=lambda r: -depth[r]):
        if s == sink:
            G0[s] = np.where(np.arange(n + 1) == n, 0.0, NEG)
            G1[s] = none.copy()
            Z[s] = 0.0
            continue
        t0, t1, tz = [none], [none], [np.array(NEG)]
        for a in out[s]:
            d, lab, w = int(dst[a]), int(label[a]), score[a]
            tz.append(np.array(w + Z[d]))
            if kept is not None:
                t0.append(w + (shifted(G0[d], lab) if lab in kept else G0[d]))
            else:
                t0.append(w + (G1[d] if lab == marker else G0[d]))
                t1.append(w + shifted(G0[d], lab))
        G0[s], G1[s], Z[s] = _lse_rows(t0), _lse_rows(t1), float(_lse_rows(tz))
    return float(G0[0][0]), float(Z[0])


def of_batch(lats, theta, cands, keep=None, marker=None, asc=None) -> tuple:
    """``(log_num [B, M], logz [B])`` for per-lattice candidate lists ``cands[b]`` (M strings each); theta [V] or [B, V],
    asc over the batch's arcs."""
    from tests.edge_cases import score64

    B, M = len(lats), len(cands[0])
    num, z = np.full((B, M), NEG), np.zeros(B)
    a0 = 0
    for b, l in enumerate(lats):
        th = theta[b] if np.ndim(theta) == 2 else theta
        s64 = score64(l, th, None if asc is None else asc[a0:a0 + l.n_arcs])
        a0 += l.n_arcs
        for m, y in enumerate(cands[b]):
            num[b, m], z[b] = string_log_prob(l, s64, y, keep, marker)
        if not M:
            z[b] = string_log_prob(l, s64, [], keep, marker)[1]
    return num, z


# ----------------------------------------------------------------------------- shared cases
MARK = 4  # synth.edit_lattice's output mark
SEED1 = dict(x=[6, 7, 6], symbols=[8, 9, 10], max_out=3, vocab=12)  # 78 rows, 1948 paths, 40 strings
SMALL = dict(x=[6, 7], symbols=[8, 9], max_out=2, vocab=12)


def denominator(shape=SEED1):
    from tests import intersect_wide_ref

    return intersect_wide_ref.edit_denominator(shape["x"], shape["symbols"], shape["max_out"], vocab=shape["vocab"])


def tape_lattice():
    """Seven states over 12 labels for the corners of the marker tape: a symbol that is the marker itself (state 2 and
    state 4 are entered by an active marker and leave by label 4), and a last arc labelled with the marker, which ends
    the path on a marker with nothing behind it."""
    from nfst_amd import synth

    arcs = [(0, synth.BOS, 1), (1, MARK, 2), (1, 7, 3), (2, MARK, 3), (2, 8, 3), (3, MARK, 4), (3, 9, 5), (4, 8, 5), (4, MARK, 5),
            (5, MARK, 6), (5, synth.EOS, 6)]
    return synth._finish(7, 12, [a[0] for a in arcs], [a[1] for a in arcs], [a[2] for a in arcs])


def layered_case():
    """(lattice, keep, y): the 1200-state lattice whose product with ``projected_sequence(keep, y)`` has more live pairs
    than NFST_MAX_ROWS; y = the kept labels of the path that ``default_rng(0)`` walks, uniform over each state's out-arcs
    that are not self loops."""
    from nfst_amd import synth

    l = synth.layered_lattice(11, n_states=1200, avg_degree=5.0, vocab=12, width=8, span=6)
    keep = {3, 5, 7, 9, 11}
    rng = np.random.default_rng(0)
    first = np.searchsorted(l.src, np.arange(l.n_rows + 1))
    s, sink, y = 0, sink_of(l.n_rows, l.src, l.dst), []
    while s != sink:
        arcs = [a for a in range(int(first[s]), int(first[s + 1])) if l.dst[a] != s]
        a = arcs[int(rng.integers(len(arcs)))]
        if int(l.label[a]) in keep:
            y.append(int(l.label[a]))
        s = int(l.dst[a])
    return l, keep, y


# ----------------------------------------------------------------------------- brute force
def brute_force(l, score, keep=None, marker=None) -> tuple:
    """``({string: log of the summed weight of its paths}, log Z over all paths, the paths best first)`` by enumeration;
    a path that ends on an active marker is in log Z and under no string."""
    src, dst = np.asarray(l.src), np.asarray(l.dst)
    paths = kbest_ref.enumerate_paths(l.n_rows, src, dst, score, sink_of(l.n_rows, src, dst))
    by = {}
    for sc, p in paths:
        labs = np.asarray(l.label)[p]
        if marker is not None and dangling(labs, marker):
            continue
        by.setdefault(project(labs, keep, marker), []).append(sc)
    lse = lambda xs: float(_lse_rows(np.asarray(xs, F64)[:, None])[0]) if len(xs) else NEG
    return {y: lse(v) for y, v in by.items()}, lse([sc for sc, _ in paths]), paths

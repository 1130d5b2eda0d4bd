"""NumPy restatement of ``nfst_lattice_edit`` on one lattice (test helper, not a test module): the recurrence over cells
E[s][j] = (dist, score) and the walk of DESIGN.md section 2, with float32 adds in the engine's order, and a brute force
over every path (``kbest_ref.enumerate_paths``, the tables of ``edit_ref``, float64 scores).

A candidate is ordered by one unsigned key, smaller = better: dist above the complement of the score's order-preserving
bits (least distance, then greatest score; scores are ordered by their bits, +0.0 above -0.0).  A score of -inf or NaN is
no candidate.
"""
from __future__ import annotations

import numpy as np

from tests import edge_cases, edit_ref, kbest_ref
from tests.expectation_ref import levels, sink_of

F32 = np.float32
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def _ord(x) -> np.ndarray:
    """Order-preserving uint32 of float32 values ("greater" as unsigned integers)."""
    u = np.asarray(x, F32).view(np.uint32)
    return u ^ np.where(u >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def _unord(o) -> np.ndarray:
    """The float32 values of order-preserving bits: the inverse of ``_ord``."""
    o = np.asarray(o, np.uint32)
    return (o ^ np.where(o >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(F32)


def _keys(dist, c) -> np.ndarray:
    """uint64 keys of candidates (dist int64 array, < 0 = none; c float32 array)."""
    c = np.asarray(c, F32)
    ok = (dist >= 0) & (c > -np.inf)
    k = (np.where(ok, dist, 0).astype(np.uint64) << np.uint64(32)) | (~_ord(c)).astype(np.uint64)
    return np.where(ok, k, NONE)


def _out_arcs(n_rows, src, dst):
    out = [[] for _ in range(n_rows)]
    for a in range(len(src)):
        if src[a] != dst[a]:
            out[int(src[a])].append(a)
    return out


def lattice_edit(n_rows: int, src, dst, label, th, e, ref, sink: int) -> dict:
    """{"distance", "score" (float32), "arcs" (relative to the lattice), "align", "counts" (sub, ins, del)} of the
    oracle path against ``ref``; th / e: float32 per-arc terms (``kbest_ref.arc_terms``), or None for "no scores" (every
    term 0.0).  Without a candidate path: distance -1, score -inf, no arcs."""
    src, dst, label = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(label, np.int64)
    ref = np.asarray(ref, np.int64).reshape(-1)
    n = len(ref)
    scored = th is not None
    if scored:
        th, e = np.asarray(th, F32), np.asarray(e, F32)
    depth = levels(n_rows, src, dst)
    out = _out_arcs(n_rows, src, dst)
    dist, score = {}, {}  # per state: int64 [n + 1] (-1 = none), float32 [n + 1]

    def extend(a, v):  # c = e_a + (theta[label_a] + v), float32
        return (e[a] + (th[a] + v)).astype(F32) if scored else np.zeros(len(v), F32)

    def candidates(s, a):
        """keys and scores [n + 1] of the insertion and the match/substitution through arc a"""
        d = int(dst[a])
        ci = extend(a, score[d])
        ki = _keys(np.where(dist[d] >= 0, dist[d] + 1, -1), ci)
        cs = np.zeros(n + 1, F32)
        ks = np.full(n + 1, NONE)
        if n:
            cs[:n] = extend(a, score[d][1:])
            ks[:n] = _keys(np.where(dist[d][1:] >= 0, dist[d][1:] + (label[a] != ref), -1), cs[:n])
        return ki, ci, ks, cs

    with np.errstate(invalid="ignore", over="ignore"):
        for s in sorted((r for r in range(n_rows) if depth[r] >= 0), key=lambda r: -depth[r]):
            if s == sink:
                dist[s], score[s] = (n - np.arange(n + 1)).astype(np.int64), np.zeros(n + 1, F32)
                continue
            key, sc = np.full(n + 1, NONE), np.zeros(n + 1, F32)
            for a in out[s]:
                for k, c in zip(*[iter(candidates(s, a))] * 2):
                    better = k < key
                    key, sc = np.where(better, k, key), np.where(better, c, sc).astype(F32)
            # the deletion chain E[j] = best(C[j], (E[j + 1].dist + 1, E[j + 1].score)), j = n - 1 .. 0: the candidate
            # C[k] reaches column j <= k at k - j more edits with its score unchanged, so E[j] is the least key of
            # C[k] + k over k >= j, less j (the score travels in the key's low word)
            col = np.arange(n + 1, dtype=np.uint64) << np.uint64(32)
            shifted = np.where(key != NONE, key + col, NONE)
            best = np.minimum.accumulate(shifted[::-1])[::-1]
            key = np.where(best != NONE, best - col, NONE)
            dd = np.where(key != NONE, (key >> np.uint64(32)).astype(np.int64), -1)
            sc = np.where(key != NONE, _unord(~key.astype(np.uint32)), F32(0)).astype(F32)
            dist[s], score[s] = dd, sc
        if dist[0][0] < 0:
            return {"distance": -1, "score": F32(-np.inf), "arcs": [], "align": [], "counts": (0, 0, 0)}
        s, j = 0, 0
        arcs, align, n_sub, n_ins, n_del = [], [], 0, 0, 0
        while s != sink:
            cell = (int(dist[s][j]), score[s][j:j + 1].view(np.uint32)[0])
            for a in out[s]:
                ki, ci, ks, cs = candidates(s, a)
                hit = None
                if j < n and ks[j] != NONE and (int(ks[j] >> np.uint64(32)), cs[j:j + 1].view(np.uint32)[0]) == cell:
                    hit = True
                elif ki[j] != NONE and (int(ki[j] >> np.uint64(32)), ci[j:j + 1].view(np.uint32)[0]) == cell:
                    hit = False
                if hit is not None:
                    arcs.append(a)
                    align.append(j if hit else -1)
                    if hit:
                        n_sub += int(label[a] != ref[j])
                        j += 1
                    else:
                        n_ins += 1
                    s = int(dst[a])
                    break
            else:
                assert j < n and dist[s][j + 1] + 1 == cell[0]
                j += 1
                n_del += 1
        n_del += n - j
    return {"distance": int(dist[0][0]), "score": score[0][0], "arcs": arcs, "align": align, "counts": (n_sub, n_ins, n_del)}


def of_lattice(l, ref, theta_b=None, arc_scores=None) -> dict:
    """``lattice_edit`` of a synth lattice: theta_b [V] (None: no scores), arc_scores over the lattice's arcs."""
    th = e = None
    if theta_b is not None:
        th, e = kbest_ref.arc_terms(l, theta_b, arc_scores)
    return lattice_edit(l.n_rows, l.src, l.dst, l.label, th, e, ref, sink_of(l.n_rows, l.src, l.dst))


def of_batch(lats, refs, theta=None, asc=None) -> list:
    """One result per lattice; refs: a list of token sequences; theta [V] or [B, V]; asc over the batch's arcs."""
    out, a0 = [], 0
    for b, l in enumerate(lats):
        th = None if theta is None else (theta[b] if np.ndim(theta) == 2 else theta)
        out.append(of_lattice(l, refs[b], th, None if asc is None else asc[a0:a0 + l.n_arcs]))
        a0 += l.n_arcs
    return out


def brute_force(l, ref, score64=None) -> dict:
    """{"distance": the least Levenshtein distance over every path of finite score (-1 without one), "best": the greatest
    float64 score among the paths at that distance, "best_arcs": that path, "ties": the distinct float64 scores at that
    distance, "n": paths}."""
    s64 = np.zeros(l.n_arcs) if score64 is None else np.asarray(score64, np.float64)
    paths = kbest_ref.enumerate_paths(l.n_rows, l.src, l.dst, s64, sink_of(l.n_rows, l.src, l.dst))
    if not paths:
        return {"distance": -1, "best": -np.inf, "best_arcs": [], "ties": [], "n": 0}
    # every path against ref in one table (edit_ref.distance_table, held to edit_ref.levenshtein in test_edit_cpu.py)
    lens = np.array([[len(p) for _, p in paths]])
    rows = np.zeros((1, len(paths), max(1, int(lens.max()))), np.int64)
    for i, (_, p) in enumerate(paths):
        rows[0, i, :len(p)] = l.label[p]
    r = np.asarray(ref, np.int64).reshape(1, 1, -1)
    ds = edit_ref.distance_table(rows, lens, r if r.shape[2] else np.zeros((1, 1, 1), np.int64), [[r.shape[2]]])[0, :, 0].tolist()
    d = min(ds)
    at = [(sc, p) for (sc, p), x in zip(paths, ds) if x == d]  # (best first, as enumerate_paths lists them)
    return {"distance": d, "best": at[0][0], "best_arcs": at[0][1], "ties": sorted({sc for sc, _ in at}), "n": len(paths)}


DEAD_SEED = 10  # the seed of dead_label_theta in the dead-label tests, chosen on this restatement (test_lattice_edit_cpu.py asserts it)


def dead_label_case():
    """(lats, theta, refs): the weighted batch's lattices, six labels at -inf, and per lattice the labels of its best
    path under the same scores without dead labels, every third token replaced."""
    lats = edge_cases.weighted_lats(False)
    theta = edge_cases.dead_label_theta(seed=DEAD_SEED)
    alive = np.where(np.isfinite(theta), theta, np.float32(-2.0))
    refs = []
    for l in lats:
        th, e = kbest_ref.arc_terms(l, alive)
        y = l.label[kbest_ref.k_best(l.n_rows, l.src, l.dst, th, e, 1, sink_of(l.n_rows, l.src, l.dst))["arcs"][0]].astype(np.int64)
        y[1::3] = edge_cases.DEAD[np.arange(len(y[1::3])) % len(edge_cases.DEAD)]
        refs.append(y)
    return lats, theta, refs

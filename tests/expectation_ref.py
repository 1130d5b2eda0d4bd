"""Float64 reference of the expectation semiring on one lattice (test helper, not a test module).

Arcs are the canonical arcs of a lattice (``src``, ``dst`` relative to it), ``score`` their float64 log weights and
``value`` the additive per-arc values v_a.  The alpha / beta masses come from the oracle's float64
``forward_backward``; the conditional expectations
    R_alpha(d) = sum_{a: s -> d} alpha(s) w_a (R_alpha(s) + v_a) / alpha(d)
    R_beta(s)  = sum_{a: s -> d} w_a beta(d) (v_a + R_beta(d)) / beta(s)
are swept level by level (levels: longest distance from state 0, by Kahn's algorithm), vectorised over the arcs of a
level.  Self loops (the sink's pad loop) lie on no path and are left out, as the engine does.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O


def levels(n_rows: int, src, dst) -> np.ndarray:
    """Longest distance from state 0 of every row (Kahn's algorithm over the arcs without self loops); -1 for rows
    that state 0 does not reach."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    keep = src != dst
    s, d = src[keep], dst[keep]
    indeg = np.bincount(d, minlength=n_rows)
    order = np.argsort(s, kind="stable")
    s, d = s[order], d[order]
    start = np.searchsorted(s, np.arange(n_rows + 1))
    depth = np.full(n_rows, -1, np.int64)
    reach = np.zeros(n_rows, bool)
    reach[0] = True
    depth[0] = 0
    frontier = [r for r in range(n_rows) if indeg[r] == 0]
    while frontier:
        nxt = []
        for r in frontier:
            for k in range(start[r], start[r + 1]):
                t = d[k]
                if reach[r]:
                    reach[t] = True
                    depth[t] = max(depth[t], depth[r] + 1)
                indeg[t] -= 1
                if indeg[t] == 0:
                    nxt.append(t)
        frontier = nxt
    if indeg.any():
        raise ValueError("the lattice has a cycle")
    depth[~reach] = -1
    return depth


def sink_of(n_rows: int, src, dst) -> int:
    """The sink as the packers take it from the arcs: the one state that state 0 reaches and that has no out-arc other
    than self loops (asserted: exactly one).  Arcs of states that state 0 does not reach are ignored, cycles among them
    included; on every ``nfst_amd.synth`` lattice this is ``n_rows - 1``."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    keep = src != dst
    s, d = src[keep], dst[keep]
    order = np.argsort(s, kind="stable")
    s, d = s[order], d[order]
    start = np.searchsorted(s, np.arange(n_rows + 1))
    reach = np.zeros(n_rows, bool)
    reach[0] = True
    frontier = np.zeros(1, np.int64)
    while frontier.size:  # breadth first from state 0, a level per trip
        nxt = np.unique(np.concatenate([d[start[r]:start[r + 1]] for r in frontier]))
        frontier = nxt[~reach[nxt]]
        reach[frontier] = True
    sinks = np.nonzero(reach & (np.diff(start) == 0))[0]
    assert len(sinks) == 1, f"{len(sinks)} reachable states without an out-arc: {sinks.tolist()[:8]}"
    return int(sinks[0])


def expectation(n_rows: int, src, dst, score, value) -> dict:
    """{"logZ", "ev" (E[V]), "posterior" p_a, "cov" c_a = p_a (E[V | a] - E[V]), "r_alpha", "r_beta"}."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    score, value = np.asarray(score, np.float64), np.asarray(value, np.float64)
    o = O.forward_backward(n_rows, src.astype(np.int32), dst.astype(np.int32), score)
    la, lb, lz = np.asarray(o["logalpha"], np.float64), np.asarray(o["logbeta"], np.float64), float(o["logZ"])
    depth = levels(n_rows, src, dst)
    live = (src != dst) & np.isfinite(score) & (depth[src] >= 0)
    ra = np.zeros(n_rows)
    rb = np.zeros(n_rows)
    with np.errstate(invalid="ignore", over="ignore"):
        fa = np.where(live & np.isfinite(la[dst]), np.exp(la[src] + score - la[dst]), 0.0)  # share of the in-mass of dst
        fb = np.where(live & np.isfinite(lb[src]), np.exp(score + lb[dst] - lb[src]), 0.0)  # share of the out-mass of src
    fa = np.nan_to_num(fa)
    fb = np.nan_to_num(fb)
    v = np.where(live, value, 0.0)
    by_dst = [np.nonzero(live & (depth[dst] == k))[0] for k in range(int(depth.max()) + 1)]
    for idx in by_dst:  # alpha: every source of a level's in-arcs lies on an earlier level
        if len(idx):
            np.add.at(ra, dst[idx], fa[idx] * (ra[src[idx]] + v[idx]))
    for k in range(int(depth.max()), -1, -1):  # beta: every destination of a level's out-arcs lies on a later level
        idx = np.nonzero(live & (depth[src] == k))[0]
        if len(idx):
            np.add.at(rb, src[idx], fb[idx] * (v[idx] + rb[dst[idx]]))
    with np.errstate(invalid="ignore", over="ignore"):
        post = np.where(live, np.exp(la[src] + score + lb[dst] - lz), 0.0)
    post = np.nan_to_num(post)
    ev = rb[0]
    cov = np.where(post > 0, post * (ra[src] + v + rb[dst] - ev), 0.0)
    return {"logZ": lz, "ev": ev, "posterior": post, "cov": cov, "r_alpha": ra, "r_beta": rb}


def entropy(n_rows: int, src, dst, score) -> dict:
    """H = log Z - E[S]; dH/ds_a = -c_a(v = s)."""
    e = expectation(n_rows, src, dst, score, score)
    return {"H": e["logZ"] - e["ev"], "grad": -e["cov"], "logZ": e["logZ"], "posterior": e["posterior"]}


def label_sums(label, x, vocab: int) -> np.ndarray:
    return np.bincount(np.asarray(label, np.int64), weights=np.asarray(x, np.float64), minlength=vocab)


def brute_force(n_rows: int, src, dst, score, value, sink: int) -> dict:
    """The same quantities by enumerating every path from state 0 to ``sink`` (small lattices only)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    out = {r: [] for r in range(n_rows)}
    for a in range(len(src)):
        if src[a] != dst[a]:
            out[int(src[a])].append(a)
    paths = []

    def walk(r, arcs):
        if r == sink:
            paths.append(list(arcs))
            return
        for a in out[r]:
            walk(int(dst[a]), arcs + [a])

    walk(0, [])
    S = np.array([score[p].sum() for p in paths])
    Vp = np.array([value[p].sum() for p in paths])
    lz = np.logaddexp.reduce(S)
    pp = np.exp(S - lz)
    ev = float((pp * Vp).sum())
    post = np.zeros(len(src))
    cov = np.zeros(len(src))
    for p, w, val in zip(paths, pp, Vp):
        for a in p:
            post[a] += w
            cov[a] += w * (val - ev)
    return {"logZ": float(lz), "ev": ev, "posterior": post, "cov": cov, "H": float(-(pp * np.log(pp)).sum()),
            "n_paths": len(paths)}


def all_paths_equal(n: int):
    """A lattice with n parallel two-arc paths 0 -> i -> sink (n + 2 states): n equally weighted paths."""
    sink = n + 1
    src = [0] * n + list(range(1, n + 1))  # (sorted by source, as the oracle wants them)
    dst = list(range(1, n + 1)) + [sink] * n
    return n + 2, np.array(src), np.array(dst), sink

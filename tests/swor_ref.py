"""NumPy float64 restatement of ``nfst_swor`` (include/nfst_hip.h) on one lattice, path enumeration, the exact inclusion
probabilities of a k-draw and the shared inputs of tests/test_swor_cpu.py and tests/test_gpu_swor.py (test helper, not a
test module).

``search`` takes logbeta and log Z as inputs: the GPU tests feed it the very tensors the op consumed, the CPU tests a
float64 backward pass rounded to float32.  Per lattice it reports a ``margin``: the smallest, over all steps, of the gap
between the k-th and (k+1)-th perturbed score, the gap between the best and second-best noise of any slot, and the gaps
between consecutive final perturbed scores.  A lattice is *decided* when its margin exceeds ``DECIDED``: only then do the
reference and the kernel, whose transcendentals differ in their last bits, have to agree on which paths were drawn.
"""
from __future__ import annotations

import itertools

import numpy as np

from nfst_amd import synth
from tests import edge_cases as E
from tests.expectation_ref import levels, sink_of

F32 = np.float32
NEG = -np.inf
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
ERR_ARG, ERR_LENGTH = -1, -9
# Margin above which a lattice is compared.  The largest |G_gpu - G_ref| over decided lattices measured on the MI355X is
# in profiles/swor.json ("max_gumbel_error"); this stays at least 100 times that value.
DECIDED = 1e-9
CAP = 0.01  # share of its lattices a comparison may leave out
KS = (1, 2, 7, 20, 64)


# ----------------------------------------------------------------------------- scores and the backward pass
def arc_score32(l, theta_b, asc=None) -> np.ndarray:
    """The arcs' float32 scores in the engine's rounding: (theta[label] + arc_w) + arc_scores, each term if present."""
    s = np.asarray(theta_b, F32)[l.label]
    if l.weight is not None:
        s = (s + np.asarray(l.weight, F32)).astype(F32)
    if asc is not None:
        s = (s + np.asarray(asc, F32)).astype(F32)
    return s.astype(F32)


def out_arcs(l):
    """row_ptr of the canonical arc list (sorted by source)."""
    return np.searchsorted(l.src, np.arange(l.n_rows + 1)).astype(np.int64)


def backward64(l, e) -> tuple:
    """(logbeta float64 [n_rows], log Z) of arc scores ``e`` (self loops are on no path)."""
    e = np.asarray(e, np.float64)
    depth = levels(l.n_rows, l.src, l.dst)
    rp = out_arcs(l)
    sink = sink_of(l.n_rows, l.src, l.dst)
    lb = np.full(l.n_rows, NEG)
    lb[sink] = 0.0
    for s in sorted((r for r in range(l.n_rows) if depth[r] >= 0 and r != sink), key=lambda r: -depth[r]):
        a = np.arange(rp[s], rp[s + 1])
        a = a[l.dst[a] != s]
        with np.errstate(invalid="ignore"):
            c = e[a] + lb[l.dst[a]]
        c = c[c > NEG]
        if len(c):
            mx = c.max()
            lb[s] = mx + np.log(np.exp(c - mx).sum())
    return lb, float(lb[0])


def rounded_beta(l, e) -> tuple:
    """What nfst_backward hands the op, as the CPU tests model it: float64 values, logbeta rounded to float32."""
    lb, z = backward64(l, e)
    return lb.astype(F32), z


# ----------------------------------------------------------------------------- the search
def search(l, e, logbeta, Z, k: int, max_len: int, uniforms) -> dict:
    """``nfst_swor`` on one lattice.  e: float32 arc scores (arc_score32); logbeta [n_rows]; uniforms [max_len, k, D]
    float32.  Returns arcs (list of arc lists, ranked), logp float32 [n] (logp64: before that rounding), gumbel float64 [n], kappa, n_paths, status,
    margin, steps, max_candidates (the most candidates of any step, self loops included as the kernel lists them) and
    dropped (candidates whose phi was not > -inf)."""
    e = np.asarray(e, F32).astype(np.float64)
    logbeta = np.asarray(logbeta, np.float64)
    Z = float(Z)
    empty = dict(arcs=[], logp=np.zeros(0, F32), logp64=np.zeros(0), gumbel=np.zeros(0), kappa=NEG, n_paths=0, status=0, margin=np.inf, steps=0,
                 max_candidates=0, dropped=0)
    if not np.isfinite(Z):
        return empty
    rp = out_arcs(l)
    sink = sink_of(l.n_rows, l.src, l.dst)
    D = uniforms.shape[2]
    st, S, G = np.array([0]), np.array([0.0]), np.array([np.inf])
    hist = [[]]  # arcs of every slot's prefix
    kappa, margin, status, t, most, dropped = NEG, np.inf, 0, 0, 0, 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        while np.any(st != sink):
            if t >= max_len:
                return dict(empty, status=ERR_LENGTH, steps=t, max_candidates=most)
            cj, ca, cS, cG = [], [], [], []
            listed = 0
            for j in range(len(st)):
                s = int(st[j])
                if s == sink:
                    cj.append([j]); ca.append([-1]); cS.append([S[j]]); cG.append([G[j]])
                    listed += 1
                    continue
                a = np.arange(rp[s], rp[s + 1])
                listed += len(a)
                r = a - rp[s]
                live = l.dst[a] != s
                a, r = a[live], r[live]
                Sp = S[j] + e[a]
                phi = Sp + logbeta[l.dst[a]] - Z
                ok = phi > NEG
                dropped += int((~ok).sum())
                if np.any(r[ok] >= D):
                    status = ERR_ARG
                    ok &= r < D
                a, r, Sp, phi = a[ok], r[ok], Sp[ok], phi[ok]
                if not len(a):
                    continue
                x = uniforms[t, j, r].astype(np.float64) + 2.0 ** -25
                g = phi - np.log(-np.log(x))
                if len(g) > 1:
                    top = np.sort(g)[-2:]
                    margin = min(margin, top[1] - top[0])
                if G[j] == np.inf:
                    gt = g
                else:
                    M = g.max()
                    v = G[j] - g + np.log(-np.expm1(g - M))
                    gt = G[j] - np.maximum(v, 0.0) - np.log1p(np.exp(-np.abs(v)))
                    gt[int(np.argmax(g))] = G[j]  # (argmax: the first on an exact tie)
                cj.append(np.full(len(a), j)); ca.append(a); cS.append(Sp); cG.append(gt)
            most = max(most, listed)
            if not cj:
                st = st[:0]
                break
            cj, ca = np.concatenate(cj).astype(np.int64), np.concatenate(ca).astype(np.int64)
            cS, cG = np.concatenate(cS), np.concatenate(cG)
            if len(cG) > k:
                order = np.lexsort((np.arange(len(cG)), -cG))  # G~ descending, ties to the earlier flat index
                margin = min(margin, cG[order[k - 1]] - cG[order[k]])
                kappa = max(kappa, cG[order[k]])
                keep = np.sort(order[:k])  # the new slots in flat order
            else:
                keep = np.arange(len(cG))
            hist = [hist[cj[i]] + ([int(ca[i])] if ca[i] >= 0 else []) for i in keep]
            st = np.array([sink if ca[i] < 0 else int(l.dst[ca[i]]) for i in keep], np.int64)
            S, G = cS[keep], cG[keep]
            t += 1
    n = len(st)
    order = np.lexsort((np.arange(n), -G[:n])) if n else np.zeros(0, np.int64)
    Gs = G[order] if n else np.zeros(0)
    if n > 1:
        margin = min(margin, float(np.min(Gs[:-1] - Gs[1:])))
    return dict(arcs=[hist[i] for i in order], logp=(S[order] - Z).astype(F32) if n else np.zeros(0, F32), logp64=(S[order] - Z) if n else np.zeros(0), gumbel=Gs, kappa=float(kappa),
                n_paths=n, status=status, margin=float(margin), steps=t, max_candidates=most, dropped=dropped)


def decided(ref, threshold=None) -> bool:
    return ref["margin"] > (DECIDED if threshold is None else threshold)


def log_weights(ref) -> np.ndarray:
    """The Horvitz-Thompson log weights of a reference result (float64): swor.log_weights' definition."""
    lp = ref["logp"].astype(np.float64)
    if ref["kappa"] == NEG:
        return lp
    return lp - np.log(-np.expm1(-np.exp(lp - ref["kappa"])))


# ----------------------------------------------------------------------------- enumeration
def enumerate_paths(l, e):
    """[(arcs, score)] of every path of finite score, in the lexicographic order of the arcs."""
    e = np.asarray(e, np.float64)
    rp = out_arcs(l)
    sink = sink_of(l.n_rows, l.src, l.dst)
    out = []

    def walk(s, arcs, tot):
        if s == sink:
            out.append((tuple(arcs), tot))
            return
        for a in range(rp[s], rp[s + 1]):
            if l.dst[a] != s and e[a] > NEG:
                walk(int(l.dst[a]), arcs + [a], tot + e[a])

    walk(0, [], 0.0)
    return out


def path_probs(l, e):
    """({arcs: p}) normalised over the enumeration."""
    paths = enumerate_paths(l, e)
    sc = np.array([s for _, s in paths])
    p = np.exp(sc - sc.max())
    p /= p.sum()
    return {a: float(q) for (a, _), q in zip(paths, p)}


def inclusion_probs(p: np.ndarray, k: int) -> np.ndarray:
    """P(i is among k draws without replacement) by enumerating the ordered k-prefixes: a prefix (i1 .. ik) has
    probability prod_j p_ij / (1 - p_i1 - .. - p_i(j-1))."""
    p = np.asarray(p, np.float64)
    n = len(p)
    k = min(k, n)
    inc = np.zeros(n)
    for tup in itertools.permutations(range(n), k):
        q, rest = 1.0, 1.0
        for i in tup:
            q *= p[i] / rest
            rest -= p[i]
        inc[list(tup)] += q
    return inc


# ----------------------------------------------------------------------------- shared inputs
def over_cap_lattice(vocab=256, hub=64, fan=121):
    """state 0 -bos-> hub; the hub has ``hub`` arcs into states of ``fan`` arcs each, which meet in ``fan`` states that
    end in one.  With 64 slots in the fanned states a step lists 64 * 121 = 7744 candidates: more than the 7680 keys the
    kernel keeps in LDS."""
    mid0, col0 = 2, 2 + hub
    pre, sink = col0 + fan, col0 + fan + 1
    src, lab, dst = [0], [BOS], [1]
    for i in range(hub):
        src.append(1); lab.append(3 + i); dst.append(mid0 + i)
        for r in range(fan):
            src.append(mid0 + i); lab.append(3 + r); dst.append(col0 + r)
    for r in range(fan):
        src.append(col0 + r); lab.append(5); dst.append(pre)
    src.append(pre); lab.append(EOS); dst.append(sink)
    return synth._finish(sink + 1, vocab, src, lab, dst)


def small_lattice():
    """Six paths of lengths 4 to 6 over 9 states: the lattice the frequency tests replicate."""
    #   0 -> 1 -> {2, 3, 4}; 2 -> {5, 7}; 3 -> {5, 6}; 4 -> {6, 7}; 5 -> 6; 6 -> 7; 7 -> sink(8)
    src = [0, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 6, 7]
    lab = [BOS, 3, 4, 5, 6, 7, 6, 8, 9, 7, 10, 11, EOS]
    dst = [1, 2, 3, 4, 5, 7, 5, 6, 6, 7, 6, 7, 8]
    return synth._finish(9, 16, src, lab, dst)


SMALL_THETA_SEED, SMALL_COPIES = 5, 2048


def small_theta():
    return np.random.default_rng(SMALL_THETA_SEED).normal(-1.0, 0.8, size=16).astype(F32)


def degree(lats) -> int:
    return max(int(np.diff(out_arcs(l)).max()) for l in lats)


def max_len_of(lats) -> int:
    return max(int(levels(l.n_rows, l.src, l.dst).max()) for l in lats) + 1


def uniforms_for(lats, k, seed, max_len=None) -> np.ndarray:
    """[B, max_len, k, D] float32 in [0, 1) from a seeded generator; lattice b's block depends on (seed, b) alone."""
    L, D = max_len or max_len_of(lats), degree(lats)
    return np.stack([np.random.default_rng([seed, b]).random((L, k, D), dtype=F32) for b in range(len(lats))])


class Case:
    """One comparison of the GPU tests: lattices, scores, packing options and the ks it runs."""

    def __init__(self, tag, lats, theta, asc=None, ks=KS, opts=None, seed=0, boundary=False, tied=False):
        self.tag, self.lats, self.theta, self.asc, self.ks, self.opts, self.seed = tag, lats, np.asarray(theta, F32), asc, ks, opts or {}, seed
        self.boundary, self.tied = boundary, tied

    def uniforms(self, k, max_len=None):
        """The case's uniforms [B, max_len, k, D]; with ``boundary`` a quarter of them are 0 and another quarter the
        largest float32 below 1; with ``tied`` all of them are 0.5."""
        u = uniforms_for(self.lats, k, self.seed, max_len)
        if self.tied:
            u[:] = 0.5
        if self.boundary:
            pick = np.random.default_rng([self.seed, 99]).random(u.shape)
            u[pick < 0.25] = 0.0
            u[(pick >= 0.25) & (pick < 0.5)] = np.nextafter(F32(1), F32(0))
        return u

    def theta_of(self, b):
        return self.theta[b] if self.theta.ndim == 2 else self.theta

    def scores(self):
        sl = E.arc_slices(self.lats)
        return [arc_score32(l, self.theta_of(b), None if self.asc is None else self.asc[sl[b]]) for b, l in enumerate(self.lats)]

    def references(self, k, betas=None, uniforms=None, max_len=None):
        """search() per lattice; betas: [(logbeta, Z)] per lattice (default: the rounded float64 backward pass)."""
        es = self.scores()
        L = max_len or max_len_of(self.lats)
        u = self.uniforms(k, L) if uniforms is None else uniforms
        out = []
        for b, l in enumerate(self.lats):
            lb, z = rounded_beta(l, es[b]) if betas is None else betas[b]
            out.append(search(l, es[b], lb, z, k, L, u[b]))
        return out


def tie_case():
    """The star beside the over-cap lattice with every label at -0.25 and every uniform at 0.5: the candidates of a step
    tie exactly whenever their log beta does, which the rounded float64 backward pass (``Case.references`` without
    betas) guarantees for states that look alike.  Not among ``cases()``: every lattice is undecided on purpose, and
    what is compared is that ties go to the earlier flat index."""
    return Case("ties", [E.star(), over_cap_lattice()], np.full(256, -0.25, F32), ks=(7, 64), tied=True)


def weighted_asc(lats, seed=0):
    return np.random.default_rng(seed).normal(0.0, 0.3, size=sum(l.n_arcs for l in lats)).astype(F32)


def cases() -> dict:
    """{name: builder of a Case}: every comparison of tests/test_gpu_swor.py against the restatement."""
    def mixed():
        return Case("mixed", E.mixed_batch(), synth.label_scores(8, E.V_MIXED))

    def mixed_per_lattice():
        lats = E.mixed_batch()
        return Case("mixed per lattice", lats, np.stack([synth.label_scores(40 + b, E.V_MIXED) for b in range(len(lats))]), seed=1)

    def weighted():
        lats = E.weighted_batch()
        return Case("weighted", lats, np.random.default_rng(0).normal(-2.0, 0.7, size=E.V_WEIGHTED).astype(F32), weighted_asc(lats), seed=2)

    def star():
        return Case("star", [E.star(), over_cap_lattice()], synth.label_scores(3, 256, mean=-1.0, std=1.0), ks=(7, 64), seed=3)

    def dead_labels():
        return Case("dead labels", E.weighted_batch(), E.dead_label_theta(), ks=(7, 64), seed=4)

    def no_path():
        lats, theta = E.no_path_case(True)
        return Case("no path", lats, theta, ks=(7,), seed=5)

    def few_paths():
        lats, theta, _, _ = E.few_paths_case()
        return Case("few paths", lats, theta, ks=(64,), seed=6)

    def boundary():
        lats = E.weighted_batch()
        return Case("boundary", lats, np.random.default_rng(1).normal(-2.0, 0.7, size=E.V_WEIGHTED).astype(F32), weighted_asc(lats, 3),
                    ks=(7, 64), seed=8, boundary=True)

    def many_small():
        lats, theta, asc = E.many_small()
        return Case("many small", lats, theta, asc, ks=(4,), seed=7)

    return {f.__name__: f for f in (mixed, mixed_per_lattice, weighted, star, dead_labels, no_path, few_paths, boundary, many_small)}

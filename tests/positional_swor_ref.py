"""NumPy float64 restatement of ``nfst_positional_swor`` (include/nfst_hip.h) on one lattice and the shared inputs of
tests/test_positional_swor_cpu.py and tests/test_gpu_positional_swor.py (test helper, not a test module).

``search`` is ``swor_ref.search`` with the two differences of the positional op: the prefix score of arc a at step t is
``Sp = (S[j] + e[a]) + pos[t, label]`` and the continuation is ``logbeta[t + 1, dst]``, a row per position.  It takes the
beta rows and log Z_T as inputs; both test files feed it ``positional_sample_ref.beta_rows``, a float64 backward pass of
its own, NOT the rows the kernel stored: |G_gpu - G_ref| therefore includes the difference between the two backward
passes.  ``margin``, ``steps`` and ``dropped`` are reported as by ``swor_ref.search``; a lattice is *decided* when its
margin exceeds ``DECIDED``.

The cases are ``swor_ref.cases()`` with, per (lattice, T), position scores ~ N(0, 1) float32 of which 5 % are -inf, each
at three budgets T: the longest, a middle and the shortest path length of the batch.
"""
from __future__ import annotations

import numpy as np

from tests import edge_cases as E
from tests import positional_ref as P
from tests import positional_sample_ref as PS
from tests import swor_ref as R
from tests.expectation_ref import sink_of

F32 = np.float32
NEG = -np.inf
ERR_ARG = R.ERR_ARG
# Margin above which a lattice is compared.  The largest |G_gpu - G_ref| over decided lattices measured on the MI355X is in
# profiles/positional_swor.json ("max_gumbel_error"); this stays at least 100 times that value (the rule of swor_ref.py).
DECIDED = R.DECIDED
CAP = R.CAP
POS_DEAD = 0.05  # share of the position scores at -inf
# Seed of a case's position scores where it is not 0 (chosen on the reference: tests/test_positional_swor_cpu.py holds
# every case to the cap on undecided lattices; with seeds 0 and 1 one of the four lattices of "boundary" has a margin
# below 1e-9 at some budget, with seed 2 the smallest margin of the case is 5e-9; with seed 0 the over-cap lattice of
# "star", a chain but for two steps, meets a -inf on its chain and has no path, with seed 1 it keeps all its paths)
POS_SEED = {"boundary": 2, "star": 1}


def search(l, e, pos, logbeta, Z, k: int, T: int, uniforms) -> dict:
    """``nfst_positional_swor`` on one lattice.  e: float32 arc scores (swor_ref.arc_score32); pos [T, V] float32 or None;
    logbeta [T + 1, n_rows] float64; uniforms [T, k, D] float32.  Returns what ``swor_ref.search`` returns; ``steps``
    never exceeds T on consistent inputs (beta_T is -inf off the sink), which the function asserts."""
    e = np.asarray(e, F32).astype(np.float64)
    pos64 = None if pos is None else np.asarray(pos, F32).astype(np.float64)
    logbeta = np.asarray(logbeta, np.float64)
    Z = float(Z)
    empty = dict(arcs=[], logp=np.zeros(0, F32), logp64=np.zeros(0), gumbel=np.zeros(0), kappa=NEG, n_paths=0, status=0, margin=np.inf,
                 steps=0, max_candidates=0, dropped=0)
    if not np.isfinite(Z):
        return empty
    rp = R.out_arcs(l)
    sink = sink_of(l.n_rows, l.src, l.dst)
    D = uniforms.shape[2]
    st, S, G = np.array([0]), np.array([0.0]), np.array([np.inf])
    hist = [[]]  # arcs of every slot's prefix
    kappa, margin, status, t, most, dropped = NEG, np.inf, 0, 0, 0, 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        while np.any(st != sink):
            assert t < T, "a slot off the sink after T steps: the beta rows do not belong to this T"
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
                if pos64 is not None:
                    Sp = Sp + pos64[t, l.label[a]]
                phi = Sp + logbeta[t + 1, l.dst[a]] - Z
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
    return dict(arcs=[hist[i] for i in order], logp=(S[order] - Z).astype(F32) if n else np.zeros(0, F32),
                logp64=(S[order] - Z) if n else np.zeros(0), gumbel=Gs, kappa=float(kappa), n_paths=n, status=status,
                margin=float(margin), steps=t, max_candidates=most, dropped=dropped)


def decided(ref, threshold=None) -> bool:
    return ref["margin"] > (DECIDED if threshold is None else threshold)


# ----------------------------------------------------------------------------- enumeration under a budget
def path_probs(l, e, pos, T: int) -> dict:
    """{arcs: p_T} over the paths of at most T arcs, path by path in float64."""
    e = np.asarray(e, np.float64)
    paths = [a for a, _ in R.enumerate_paths(l, e) if len(a) <= T]
    sc = np.array([sum(e[a] + (0.0 if pos is None else float(pos[t, l.label[a]])) for t, a in enumerate(p)) for p in paths])
    keep = sc > NEG
    paths, sc = [p for p, ok in zip(paths, keep) if ok], sc[keep]
    w = np.exp(sc - sc.max())
    w /= w.sum()
    return {a: float(q) for a, q in zip(paths, w)}


def small_pos(T: int) -> np.ndarray:
    """The [T, V] table of the frequency tests on ``swor_ref.small_lattice()`` (no entry at -inf: the admitted paths are
    the lattice's paths of at most T arcs)."""
    return np.random.default_rng([23, T]).normal(0.0, 1.0, size=(T, 16)).astype(F32)


def small_value(l, arcs) -> float:
    """A value of a path that does not decompose over (position, label): it couples the whole label sequence."""
    lab = l.label[list(arcs)].astype(np.float64)
    return float(np.sin(np.sum(lab * np.arange(1, len(lab) + 1))) + len(set(lab.tolist())) * (lab[1] == 3.0))


# ----------------------------------------------------------------------------- shared inputs
def budgets(lats) -> tuple:
    """(longest, middle, shortest): the longest path length of the batch, the shortest of any of its lattices and the
    value halfway between; duplicates dropped, in descending order."""
    mm = [P.min_max_len(l) for l in lats]
    hi, lo = max(m[1] for m in mm), min(m[0] for m in mm)
    return tuple(sorted({hi, (hi + lo) // 2, lo}, reverse=True))


def pos_for(case, T: int) -> np.ndarray:
    """[B, T, V] float32 ~ N(0, 1) with 5 % of the entries at -inf; lattice b's block depends on (the case's seed, b, T)."""
    V = case.lats[0].vocab
    out = []
    for b in range(len(case.lats)):
        rng = np.random.default_rng([case.seed, b, T, 31, POS_SEED.get(case.tag, 0)])
        p = rng.normal(0.0, 1.0, size=(T, V)).astype(F32)
        p[rng.random((T, V)) < POS_DEAD] = NEG
        out.append(p)
    return np.stack(out)


def beta_rows(case, T: int, pos=None, with_pos=True) -> list:
    """[(log beta rows [T + 1, n], log Z_T)] per lattice from ``positional_sample_ref.beta_rows`` on the float64 arc
    scores of the backward pass (``positional_ref.arc_score64``)."""
    pos = pos_for(case, T) if pos is None and with_pos else pos
    sl = E.arc_slices(case.lats)
    out = []
    for b, l in enumerate(case.lats):
        sc = P.arc_score64(l, case.theta_of(b), None if case.asc is None else case.asc[sl[b]])
        rows = PS.beta_rows(l, sc, None if pos is None else pos[b], T)
        out.append((rows, float(rows[0, 0])))
    return out


_REFS = {}


def references(name: str, T: int, k: int) -> tuple:
    """(case, pos [B, T, V], uniforms [B, T, k, D], [search() per lattice]) of ``swor_ref.cases()[name]`` at budget T,
    computed once per process and shared by the CPU and the GPU tests."""
    key = (name, T, k)
    if key not in _REFS:
        case = R.cases()[name]()
        pos = pos_for(case, T)
        u = case.uniforms(k, T)
        es = case.scores()
        betas = _betas(name, T, case, pos)
        _REFS[key] = (case, pos, u, [search(l, es[b], pos[b], betas[b][0], betas[b][1], k, T, u[b]) for b, l in enumerate(case.lats)])
    return _REFS[key]


_BETAS = {}


def _betas(name, T, case, pos):
    if (name, T) not in _BETAS:
        _BETAS[(name, T)] = beta_rows(case, T, pos)
    return _BETAS[(name, T)]


def case_budgets(name: str) -> tuple:
    return budgets(R.cases()[name]().lats)

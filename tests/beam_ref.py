"""Float32 NumPy reference of ``nfst_beam_step`` and of a whole ``BeamDecoder.decode`` (test helper, not a test module),
written from the rules of include/nfst_hip.h, and the inputs that tests/test_beam_cpu.py and tests/test_gpu_beam.py share.

A candidate is (j, a): a live slot j (beam_score > -inf, state in range) and an arc a out of its state with label l that
is legal: l != bos; l == pad exactly when inp[j] is eos or pad; with has_to_end a slot that has not ended takes eos only.
    c = beam_score[j] + (x + w_a)     x = scores[j, l] (0.0f for pad), w_a = arc_w[a] or 0.0f      (float32, this order)
    r = c + lookahead[dst_a]          (r = c without lookahead)
Dropped unless c > -inf and r > -inf.  Order: (r desc, j asc, l asc), -0.0 == +0.0.  Rank i gets (c, j, l, dst_a); the
ranks beyond the candidates get (-inf, -1, pad, 0).
"""
from __future__ import annotations

import numpy as np

from nfst_amd import synth
from tests.expectation_ref import sink_of

F32 = np.float32
NEG = F32(-np.inf)
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS


def row_ptr(l):
    return np.searchsorted(l.src, np.arange(l.n_rows + 1)).astype(np.int64)


def candidates(l, state, inp, beam_score, scores, lookahead, has_to_end, pad=PAD, bos=BOS, eos=EOS):
    """(c, r, j, label, dst) float32 / int64 arrays of the candidates of one lattice, in no particular order."""
    rp = row_ptr(l)
    cs, rs, js, ls, ds = [], [], [], [], []
    for j in range(len(state)):
        s = int(state[j])
        if not (beam_score[j] > NEG) or not 0 <= s < l.n_rows:
            continue
        ended = int(inp[j]) in (eos, pad)
        for a in range(rp[s], rp[s + 1]):
            lab, d = int(l.label[a]), int(l.dst[a])
            if lab == bos or (lab != pad if ended else lab == pad):
                continue
            if has_to_end and not ended and lab != eos:
                continue
            x = F32(0.0) if lab == pad else F32(scores[j, lab])
            w = F32(l.weight[a]) if l.weight is not None else F32(0.0)
            with np.errstate(invalid="ignore"):  # (+inf + -inf: NaN, dropped)
                c = F32(beam_score[j]) + F32(x + w)
                r = c if lookahead is None else F32(c + F32(lookahead[d]))
            if c > NEG and r > NEG:
                cs.append(c); rs.append(r); js.append(j); ls.append(lab); ds.append(d)
    return (np.array(cs, F32), np.array(rs, F32), np.array(js, np.int64), np.array(ls, np.int64), np.array(ds, np.int64))


def lattice_step(l, state, inp, beam_score, scores, lookahead=None, has_to_end=False, pad=PAD, bos=BOS, eos=EOS):
    """One step of one lattice's beam of K = len(state) slots: dict(score, parent, symbol, next_state, n_candidates, r)."""
    K = len(state)
    c, r, j, lab, d = candidates(l, state, inp, beam_score, scores, lookahead, has_to_end, pad, bos, eos)
    o = np.lexsort((lab, j, -(r + F32(0.0))))[:K]  # (-0.0 + 0.0 = +0.0)
    n = len(o)
    out = dict(score=np.full(K, NEG, F32), parent=np.full(K, -1, np.int32), symbol=np.full(K, pad, np.int64),
               next_state=np.zeros(K, np.int64), n_candidates=len(c), r=np.sort(r)[::-1])
    out["score"][:n], out["parent"][:n], out["symbol"][:n], out["next_state"][:n] = c[o], j[o], lab[o], d[o]
    return out


def batch_step(lats, K, state, inp, beam_score, scores, lookahead=None, has_to_end=False, pad=PAD, bos=BOS, eos=EOS):
    """The step over a batch: arrays over N = B * K slots, lookahead over the batch's rows; n_open as the kernel counts."""
    B = len(lats)
    row_off = np.concatenate([[0], np.cumsum([l.n_rows for l in lats])])
    out = dict(score=np.empty(B * K, F32), parent=np.empty(B * K, np.int32), symbol=np.empty(B * K, np.int64),
               next_state=np.empty(B * K, np.int64), n_candidates=np.empty(B, np.int32))
    for b, l in enumerate(lats):
        sl = slice(b * K, (b + 1) * K)
        la = None if lookahead is None else lookahead[row_off[b]:row_off[b + 1]]
        o = lattice_step(l, state[sl], inp[sl], beam_score[sl], scores[sl], la, has_to_end, pad, bos, eos)
        for name in ("score", "parent", "symbol", "next_state"):
            out[name][sl] = o[name]
        out["n_candidates"][b] = o["n_candidates"]
    out["n_open"] = int(np.sum((out["parent"] >= 0) & (out["symbol"] != pad)))
    return out


def first_state(l, bos=BOS):
    """The state after the implicit bos (0 where state 0 has no bos arc, as nfst_step)."""
    rp = row_ptr(l)
    for a in range(rp[0], rp[1]):
        if l.label[a] == bos:
            return int(l.dst[a])
    return 0


def backtrack(parent, symbol, score, B, K, n_steps, max_len, pad=PAD):
    """(paths [B, K, max_len] int32, lengths [B, K] int32) of parent / symbol [T, B * K]."""
    paths = np.full((B, K, max_len), pad, np.int32)
    lengths = np.zeros((B, K), np.int32)
    for b in range(B):
        for i in range(K):
            if not score[b * K + i] > NEG:
                continue
            cur, marks = i, []
            for t in range(n_steps - 1, -1, -1):
                if not 0 <= cur < K:
                    break
                s = int(symbol[t, b * K + cur])
                if s != pad:
                    marks.append(s)
                cur = int(parent[t, b * K + cur])
            marks.reverse()
            paths[b, i, :len(marks)] = marks
            lengths[b, i] = len(marks)
    return paths, lengths


def decode(lats, K, score_fn, max_length, lookahead=None, hx=None, pad=PAD, bos=BOS, eos=EOS):
    """The whole search, step by step: ``score_fn(hx, inp) -> (hx, scores [N, V])`` on NumPy arrays, ``hx`` an array with
    the slots along axis 0 (or None).  dict(paths, lengths, scores [B, K], n_steps)."""
    B, N = len(lats), len(lats) * K
    T = max_length + 1
    inp = np.full(N, bos, np.int64)
    state = np.repeat([first_state(l, bos) for l in lats], K).astype(np.int64)
    score = np.full(N, NEG, F32)
    score[::K] = 0.0
    own, base = np.arange(N), np.arange(N) - np.arange(N) % K
    parents, symbols, n_steps = np.zeros((T, N), np.int32), np.zeros((T, N), np.int64), 0
    for t in range(T):
        hx, scores = score_fn(hx, inp)
        o = batch_step(lats, K, state, inp, score, np.asarray(scores, F32), lookahead, (t + 1) > max_length, pad, bos, eos)
        parents[t], symbols[t] = o["parent"], o["symbol"]
        if hx is not None:
            hx = hx[np.where(o["parent"] >= 0, base + o["parent"], own)]
        state, inp, score = o["next_state"], o["symbol"], o["score"]
        n_steps = t + 1
        if o["n_open"] == 0:
            break
    paths, lengths = backtrack(parents, symbols, score, B, K, n_steps, T, pad)
    return dict(paths=paths, lengths=lengths, scores=score.reshape(B, K).copy(), n_steps=n_steps)


def stateless(scores_bv, K):
    """score_fn of a scorer that is a per-lattice label score [B, V] (or [V]): the same row for every slot of a lattice."""
    s = np.asarray(scores_bv, F32)

    def fn(hx, inp):
        n = len(inp)
        return hx, (np.repeat(s, K, axis=0) if s.ndim == 2 else np.broadcast_to(s, (n, s.shape[0]))).astype(F32)

    return fn


def vbeta(l, theta_b):
    """Exact max-plus beta* of one lattice, float32 with the adds of nfst_arc_slack: vbeta(sink) = 0, vbeta(s) = max over
    the out-arcs without self loops of e_a + (theta[l_a] + vbeta(dst_a)); -inf for rows on no path of finite score."""
    from tests.expectation_ref import levels

    depth = levels(l.n_rows, l.src, l.dst)
    rp = row_ptr(l)
    v = np.full(l.n_rows, NEG, F32)
    sink = sink_of(l.n_rows, l.src, l.dst)
    v[sink] = 0.0
    th = np.asarray(theta_b, F32)
    for s in sorted((r for r in range(l.n_rows) if depth[r] >= 0 and r != sink), key=lambda r: -depth[r]):
        for a in range(rp[s], rp[s + 1]):
            if l.dst[a] != s:
                e = F32(l.weight[a]) if l.weight is not None else F32(0.0)
                v[s] = max(v[s], F32(e + F32(th[l.label[a]] + v[l.dst[a]])))
    return v


# ----------------------------------------------------------------------------- shared inputs
def step_case(lats, K, seed, lookahead=False, quarter=False):
    """Inputs of one step over a batch: states drawn from every row (the rows of the synthetic lattices are all reachable),
    ``inp`` a mix of ordinary marks, eos and pad (a slot that has ended sits in the sink, where the pad loop is), a quarter
    of the slots dead, scores with -inf entries and one NaN, a look-ahead with -inf rows."""
    rng = np.random.default_rng(seed)
    B, V = len(lats), lats[0].vocab
    N = B * K
    state, inp = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for b, l in enumerate(lats):
        sink = sink_of(l.n_rows, l.src, l.dst)
        for i in range(K):
            n = b * K + i
            u = rng.random()
            if u < 0.2:
                state[n], inp[n] = sink, (EOS if u < 0.1 else PAD)
            else:
                state[n], inp[n] = rng.integers(0, l.n_rows), rng.integers(synth.N_SPECIAL, V)
    beam_score = rng.normal(-5.0, 2.0, size=N).astype(F32)
    beam_score[rng.random(N) < 0.25] = NEG
    beam_score[N // 2] = NEG
    scores = rng.normal(-2.0, 1.0, size=(N, V)).astype(F32)
    scores[rng.random((N, V)) < 0.1] = NEG
    look = None
    if lookahead:
        look = rng.normal(-3.0, 1.0, size=sum(l.n_rows for l in lats)).astype(F32)
        look[rng.random(len(look)) < 0.15] = NEG
    if quarter:
        q = lambda x: (np.round(np.asarray(x, np.float64) * 4) / 4).astype(F32)
        beam_score, scores, look = q(beam_score), q(scores), None if look is None else q(look)
    # one NaN, on a label that a live slot can take
    for n in range(N):
        b = n // K
        l = lats[b]
        rp = row_ptr(l)
        labs = l.label[rp[state[n]]:rp[state[n] + 1]]
        labs = labs[labs >= synth.N_SPECIAL]
        if beam_score[n] > NEG and inp[n] not in (EOS, PAD) and len(labs):
            scores[n, labs[0]] = np.nan
            break
    return dict(state=state, inp=inp, beam_score=beam_score, scores=scores, lookahead=look)


def tie_case(lats, K, seed=5):
    """Ties that the (slot, label) order must decide: the slots of a lattice share one state (the one with the most
    out-arcs) and one score, in groups of three slots with the same row of scores; the scores lie on a grid of 0.5 with
    four values only, so that labels tie inside a slot as well."""
    rng = np.random.default_rng(seed)
    B, V = len(lats), lats[0].vocab
    N = B * K
    state, inp = np.zeros(N, np.int64), np.full(N, synth.N_SPECIAL, np.int64)
    scores = np.zeros((N, V), F32)
    for b, l in enumerate(lats):
        deg = np.diff(row_ptr(l))
        deg[sink_of(l.n_rows, l.src, l.dst)] = 0
        state[b * K:(b + 1) * K] = int(np.argmax(deg))
        for i in range(K):
            if i % 3 == 0:
                row = (-0.5 * rng.integers(1, 5, size=V)).astype(F32)
            scores[b * K + i] = row
    beam_score = np.full(N, -1.25, F32)
    return dict(state=state, inp=inp, beam_score=beam_score, scores=scores, lookahead=None)


def hashed_scorer(V, M=257, seed=11):
    """A path-dependent scorer: hx [N] int64 is a hash of the prefix, the step's scores are table[hx % M].  Returns
    (table [M, V] float32 log-probabilities, update(hx, inp) -> hx) with NumPy / torch-agnostic integer arithmetic."""
    rng = np.random.default_rng(seed)
    t = rng.normal(0.0, 1.5, size=(M, V))
    t = t - np.log(np.exp(t).sum(axis=1, keepdims=True))
    return t.astype(F32), (lambda hx, inp: (hx * 31 + inp + 7) % 1000003)

"""Plain NumPy references of the path-side kernels on one lattice (test helper, not a test module): Viterbi in the
engine's float32 add orders and in float64, a float32 restatement of one proposal step (a yardstick for tolerances
only), and the inputs that tests/test_gpu_paths.py and tests/test_paths_ref_cpu.py share -- the GPU file compares
walks and walkers with the oracle only where the uniform stays clear of every CDF boundary (``margin > 1e-5``), and
the CPU file proves on the oracle alone that every such case keeps more than 90 % of them.

A path runs from state 0 to the sink (``expectation_ref.sink_of``: taken from the arcs); self loops lie on no path.  Arcs are the
canonical arcs of a lattice, sorted by (source, label).
"""
from __future__ import annotations

import numpy as np

from nfst_amd import synth
from oracle import oracle as O
from tests.expectation_ref import levels, sink_of
from tests.kbest_ref import enumerate_paths

F32 = np.float32
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
MARGIN = 1e-5  # walks / walkers whose uniforms stay this clear of every CDF boundary are compared exactly
CAP = 0.9      # ... and they must be more than this share of every case


# ----------------------------------------------------------------------------- Viterbi
def _row_ptr(n_rows, src):
    return np.searchsorted(np.asarray(src, np.int64), np.arange(n_rows + 1))


def viterbi_ref(l, theta, arc_w=None, arc_scores=None, order="general") -> dict:
    """float32 max-plus from the sink back, in the add order each kernel flavour documents (include/nfst_hip.h):
        order="general":     c = e_a + (theta[l] + v(d)),  e_a = 0 (+ w) (+ s)
        order="tile_waves":  c = v(d) + (theta[l] + e_a),  e_a = w + s, w or s   (c = v(d) + theta[l] without extras)
    v(sink) = 0; v(s) = the largest candidate, the smaller canonical arc on exactly tied candidates.  A lattice with
    no path of finite score: best = -inf and an empty path.  {"best": float32, "arcs": int64 [n] relative to the
    lattice, "labels": int32 [n], "length": n, "ties": the states on the path whose largest candidate was tied}."""
    src, dst = np.asarray(l.src, np.int64), np.asarray(l.dst, np.int64)
    th = np.asarray(theta, F32)[l.label].astype(F32)
    w = None if arc_w is None else np.asarray(arc_w, F32)
    s = None if arc_scores is None else np.asarray(arc_scores, F32)
    if order == "general":
        e = np.zeros(l.n_arcs, F32)
        if w is not None:
            e = e + w
        if s is not None:
            e = e + s
    elif order == "tile_waves":
        e = (w + s) if (w is not None and s is not None) else (w if w is not None else s)
    else:
        raise ValueError(order)
    sink = sink_of(l.n_rows, l.src, l.dst)
    depth = levels(l.n_rows, src, dst)
    rp = _row_ptr(l.n_rows, src)
    v = np.full(l.n_rows, -np.inf, F32)
    bp = np.full(l.n_rows, -1, np.int64)
    tied = np.zeros(l.n_rows, bool)
    v[sink] = 0.0
    for r in sorted((r for r in range(l.n_rows) if depth[r] >= 0 and r != sink), key=lambda r: -depth[r]):
        a = np.arange(rp[r], rp[r + 1])
        a = a[dst[a] != r]
        if a.size == 0:
            continue
        if order == "general":
            c = e[a] + (th[a] + v[dst[a]])
        else:
            c = v[dst[a]] + (th[a] if e is None else th[a] + e[a])
        assert c.dtype == F32
        j = int(np.argmax(c))  # the first of the largest: the smaller canonical arc
        if c[j] > -np.inf:
            v[r], bp[r], tied[r] = c[j], a[j], (c == c[j]).sum() > 1
    arcs, ties = [], 0
    at = 0
    while at != sink and bp[at] >= 0:
        arcs.append(int(bp[at]))
        ties += int(tied[at])
        at = int(dst[bp[at]])
    arcs = np.asarray(arcs, np.int64)
    return {"best": F32(v[0]), "arcs": arcs, "labels": np.asarray(l.label)[arcs].astype(np.int32), "length": len(arcs), "ties": ties}


def viterbi_f64(l, score64) -> dict:
    """The optimum in float64: {"best", "arcs"} (ties: the smaller arc; -inf and no arcs without a finite path)."""
    src, dst = np.asarray(l.src, np.int64), np.asarray(l.dst, np.int64)
    sc = np.asarray(score64, np.float64)
    sink = sink_of(l.n_rows, l.src, l.dst)
    depth = levels(l.n_rows, src, dst)
    rp = _row_ptr(l.n_rows, src)
    v = np.full(l.n_rows, -np.inf)
    bp = np.full(l.n_rows, -1, np.int64)
    v[sink] = 0.0
    for r in sorted((r for r in range(l.n_rows) if depth[r] >= 0 and r != sink), key=lambda r: -depth[r]):
        a = np.arange(rp[r], rp[r + 1])
        a = a[dst[a] != r]
        if a.size == 0:
            continue
        c = sc[a] + v[dst[a]]
        j = int(np.argmax(c))
        if c[j] > -np.inf:
            v[r], bp[r] = c[j], a[j]
    arcs, at = [], 0
    while at != sink and bp[at] >= 0:
        arcs.append(int(bp[at]))
        at = int(dst[bp[at]])
    return {"best": float(v[0]), "arcs": np.asarray(arcs, np.int64)}


def brute_force_best(l, score64):
    """(best float64 score, number of paths of finite score) by enumerating every path: lattices of a few hundred
    paths at most."""
    paths = enumerate_paths(l.n_rows, l.src, l.dst, score64, sink_of(l.n_rows, l.src, l.dst))
    return (paths[0][0] if paths else -np.inf), len(paths)


def score64(l, theta, arc_w=None, arc_scores=None) -> np.ndarray:
    sc = np.asarray(theta, F32)[l.label].astype(np.float64)
    if arc_w is not None:
        sc = sc + np.asarray(arc_w, np.float64)
    if arc_scores is not None:
        sc = sc + np.asarray(arc_scores, np.float64)
    return sc


def path_guard(l, sc64, arcs) -> tuple:
    """(gap, bound) of a returned path against the float64 optimum, independent of any add order: gap = optimum -
    float64 score of ``arcs``; bound = depth * 2^-23 * M with depth the arcs of the longer of the two paths and M the
    largest |partial sum| (from the sink backwards, as the sweeps add) along either: one float32 rounding (2^-24
    relative) per add on each of the two paths compared."""
    opt = viterbi_f64(l, sc64)
    arcs = np.asarray(arcs, np.int64)
    big = 0.0
    for p in (arcs, opt["arcs"]):
        if len(p):
            big = max(big, float(np.max(np.abs(np.cumsum(sc64[p][::-1])))))
    depth = max(len(arcs), len(opt["arcs"]))
    return opt["best"] - float(sc64[arcs].sum()), depth * 2.0 ** -23 * big


# ----------------------------------------------------------------------------- one proposal step in float32
def proposal_step_f32(mask, scores, gathered, pad: int, temperature: float, symbol, penalty=None):
    """One proposal step's logits, logsumexp and log q in ``np.float32`` arithmetic with NumPy's pairwise sums: a
    yardstick for what float32 can give (its error against the float64 oracle is E32), never a reference.
    mask [N, V] float32 = mask_out_invalid (emission row + legality); gathered / penalty [N, V] or None: the values
    of the next states and the insertion / length penalties.  Returns (logz [N], logq [N]) float32."""
    x = np.asarray(scores, F32).copy()
    if gathered is not None:
        x = x + np.asarray(gathered, F32)
    if penalty is not None:
        x = x - np.asarray(penalty, F32)
    x[:, pad] = 0.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = ((x + np.asarray(mask, F32)) / F32(temperature)).astype(F32)
        mx = x.max(axis=1, keepdims=True)
        sm = np.exp((x - mx).astype(F32)).astype(F32).sum(axis=1, dtype=F32)
        lz = (mx[:, 0] + np.log(sm).astype(F32)).astype(F32)
        lq = (x[np.arange(x.shape[0]), symbol] - lz).astype(F32)
    return lz, lq


# ----------------------------------------------------------------------------- lattices of the shared cases
def hub_lattice(seed: int, vocab: int, hub_degree: int, weighted: bool = False, tail: int = 5, width: int = 6):
    """0 --bos--> hub; the hub leaves by min(hub_degree, vocab - 3) distinct labels to as many states; those lead
    through ``tail`` layers of ``width`` states (1 .. 3 arcs each, labels drawn from the whole vocabulary) to a last
    state that leaves by eos to the sink.  Any vocab >= 5; a high-degree state whose legal marks are spread over the
    whole label range, so that a 64-wide scan over the marks carries its running sum over many chunks."""
    rng = np.random.default_rng(seed)
    labels = np.arange(synth.N_SPECIAL, vocab)
    D = int(min(hub_degree, labels.size))
    width = min(width, D)
    src, lab, dst = [0], [BOS], [1]
    first = np.arange(2, 2 + D)
    layers = [first] + [np.arange(2 + D + i * width, 2 + D + (i + 1) * width) for i in range(tail)]
    last = 2 + D + tail * width
    src += [1] * D
    lab += sorted(rng.choice(labels, size=D, replace=False).tolist())
    dst += first.tolist()
    for i, cur in enumerate(layers):
        nxt = layers[i + 1] if i + 1 < len(layers) else np.array([last])
        for j, s in enumerate(cur):
            n = int(min(rng.integers(1, 4), labels.size, nxt.size))
            d = rng.choice(nxt, size=n, replace=False).tolist()
            if j < nxt.size and nxt[j] not in d:  # every state of the next layer is reached (no layer is wider than the one before)
                d[0] = int(nxt[j])
            for mark, t in zip(sorted(rng.choice(labels, size=len(d), replace=False).tolist()), d):
                src.append(int(s)); lab.append(int(mark)); dst.append(int(t))
    src.append(last); lab.append(EOS); dst.append(last + 1)
    wt = rng.normal(-0.5, 0.8, size=len(src)).astype(F32) if weighted else None
    return synth._finish(last + 2, vocab, src, lab, dst, wt)


def dense_rows(l, states, weighted: bool):
    """The rows of the dense tables that walkers in ``states`` read (the arc-list form of ``l.dense()`` for
    vocabularies whose tables are too large to build): (emission [N, 1, V], transition [N, 1, V]); a state out of
    range reads an empty row.  Index them with state 0."""
    N = len(states)
    em = np.full((N, 1, l.vocab), -np.inf, F32) if weighted else np.zeros((N, 1, l.vocab), np.bool_)
    tr = np.zeros((N, 1, l.vocab), np.int64)
    rp = _row_ptr(l.n_rows, l.src)
    for n, s in enumerate(states):
        if 0 <= s < l.n_rows:
            a = np.arange(rp[s], rp[s + 1])
            em[n, 0, l.label[a]] = (l.weight[a] if l.weight is not None else 0.0) if weighted else True
            tr[n, 0, l.label[a]] = l.dst[a]
    return em, tr


# ----------------------------------------------------------------------------- the walker cases
WALKER_VOCABS = (5, 63, 64, 65, 96, 700, 3413, 4096)
WALKER_KS = (1, 3)
WALKER_B = 3  # lattices: N = 3 or 9 walkers, never a multiple of the four walkers of a block


def walker_lattices(V: int, weighted: bool):
    hub = 300 if V >= 700 else 60
    return [hub_lattice(9000 + 10 * V + b, V, hub_degree=hub, weighted=weighted) for b in range(WALKER_B)]


def walker_positions(lats, k: int, seed: int):
    """Per walker (value_state, inp, state): an arc of its lattice (the state before the previous symbol, the symbol,
    the state after).  Walker 0 of every lattice sits on the hub after bos, and with k = 3 walker 2 of every lattice
    has ended: in the sink after eos (even lattices) or pad."""
    rng = np.random.default_rng(seed)
    N = len(lats) * k
    vstate, inp, state = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64)
    for n in range(N):
        l, j = lats[n // k], n % k
        if j == 0:
            vstate[n], inp[n], state[n] = 0, BOS, 1
        elif j == 2:
            sink = sink_of(l.n_rows, l.src, l.dst)
            if (n // k) % 2 == 0:
                vstate[n], inp[n], state[n] = sink - 1, EOS, sink
            else:
                vstate[n], inp[n], state[n] = sink, PAD, sink
        else:
            a = int(rng.integers(0, l.n_arcs - 1))  # (the last arc is the sink's pad loop)
            if n // k == 0:  # ... of the first lattice: on the last state, the one with the eos arc
                a = int(np.flatnonzero(l.dst == l.n_rows - 2)[0])
            vstate[n], inp[n], state[n] = l.src[a], l.label[a], l.dst[a]
    return vstate, inp, state


STEP_CONFIGS = (  # (tag, temperature, values, value_state, has_to_end)
    ("plain", 1.0, False, False, False),
    ("values", 0.7, True, False, False),
    ("value_state", 1.3, True, True, False),
    ("has_to_end", 1.0, False, False, True),
)


VALUE_STATE_MAX_VOCAB = 3413  # values + a value state: four walkers x three rows of V words in 160 KiB of LDS


def step_configs(V: int):
    """The configurations a vocabulary of V takes (beyond 3413 a value state is refused: tested on its own)."""
    return tuple(c for c in STEP_CONFIGS if not (c[3] and V > VALUE_STATE_MAX_VOCAB))


def walker_inputs(V: int, k: int, weighted: bool):
    """Everything one proposal step of the walker cases reads, as NumPy arrays (the same for the GPU and the oracle)."""
    lats = walker_lattices(V, weighted)
    vstate, inp, state = walker_positions(lats, k, seed=100 * V + k)
    rng = np.random.default_rng(7 * V + k + (1000 if weighted else 0))
    N = len(lats) * k
    # (peaked scores: std 3 keeps the share of probability near any one CDF boundary small at hundreds of marks)
    scores = rng.normal(0.0, 3.0, size=(N, V)).astype(F32)
    u = rng.random(N).astype(F32)
    values = rng.normal(0.0, 0.5, size=sum(l.n_rows for l in lats)).astype(F32)
    row_off = np.concatenate([[0], np.cumsum([l.n_rows for l in lats])[:-1]]).astype(np.int64)
    return dict(lats=lats, vstate=vstate, inp=inp, state=state, scores=scores, u=u, values=values, row_off=row_off, N=N)


def oracle_step(d: dict, k: int, weighted: bool, cfg, forced=None, penalties=None, length=None, scores=None, inp=None,
                state=None, vstate=None, u=None):
    """``oracle.proposal_step`` lattice by lattice on the dense tables of the walker case ``d``; also the float32
    yardstick's (logz, logq) at the oracle's symbols.  Returns a dict of [N] arrays."""
    _, temperature, use_values, own, has_to_end = cfg
    scores = d["scores"] if scores is None else scores
    inp, state = d["inp"] if inp is None else inp, d["state"] if state is None else state
    vstate, u = d["vstate"] if vstate is None else vstate, d["u"] if u is None else u
    out = {key: [] for key in ("symbol", "logq", "logz", "next_state", "margin", "logz32", "logq32")}
    for b, l in enumerate(d["lats"]):
        sl = slice(b * k, (b + 1) * k)
        em, tr = l.dense(weighted=weighted)
        em_k, tr_k = np.broadcast_to(em[None], (k,) + em.shape), np.broadcast_to(tr[None], (k,) + tr.shape)
        r0 = int(d["row_off"][b])
        beta = np.broadcast_to(d["values"][r0:r0 + l.n_rows][None], (k, l.n_rows)) if use_values else None
        if length is None:
            ln, max_length = (5, 3) if has_to_end else (2, 300)
        else:
            ln, max_length = length, 300
        pen = None
        if penalties is not None:
            pen = dict(penalties, accumulated=penalties["accumulated"][sl], vocab_use=penalties["vocab_use"][sl])
        o = O.proposal_step(em_k, tr_k, scores[sl], inp[sl], state[sl], ln, max_length, PAD, BOS, EOS, temperature=temperature,
                            beta=beta, uniforms=None if forced is not None else u[sl].astype(np.float64),
                            forced=None if forced is None else forced[sl], value_state=vstate[sl] if (use_values and own) else None,
                            penalties=pen)
        # the float32 yardstick on the same inputs (the counters were just updated in place by the oracle)
        mask = O.mask_out_invalid(em_k, inp[sl], state[sl], ln, max_length, PAD, BOS, EOS)
        gathered = O.beta_logits(tr_k, beta, vstate[sl] if own else state[sl]) if use_values else None
        pv = None
        if pen is not None:
            pv = np.zeros((k, l.vocab), np.float64)
            if pen["insert_threshold"] > 0:
                pv[pen["accumulated"] > pen["insert_threshold"], pen["insertion_mark"]] += pen["insert_penalty"] * (ln - pen["insert_threshold"])
            if 0 < pen["length_threshold"] < ln:
                pv = pv + pen["vocab_use"].astype(np.float64) * pen["length_penalty"]
        lz32, lq32 = proposal_step_f32(mask, scores[sl], gathered, PAD, temperature, o["symbol"], pv)
        for key in ("symbol", "logq", "logz", "next_state", "margin"):
            out[key].append(o[key])
        out["logz32"].append(lz32)
        out["logq32"].append(lq32)
    return {key: np.concatenate(v) for key, v in out.items()}


def e32(o: dict) -> float:
    """E32: the largest error of the float32 yardstick against the float64 oracle over the finite entries."""
    err = 0.0
    for a, b in (("logz32", "logz"), ("logq32", "logq")):
        ok = np.isfinite(o[b])
        if ok.any():
            err = max(err, float(np.max(np.abs(o[a][ok].astype(np.float64) - o[b][ok]))))
    return err


def safe_share(o: dict):
    """(mask of the walkers compared exactly, its share among the walkers with a legal mark)."""
    finite = np.isfinite(o["logz"])
    safe = (o["margin"] > MARGIN) & finite
    return safe, (safe.sum() / finite.sum() if finite.any() else 1.0)


# the chained steps with the penalties on
CHAIN_VOCABS = (65, 700)
CHAIN_STEPS = 5
CHAIN_PEN = dict(insert_threshold=1, insert_penalty=0.7, length_threshold=1, length_penalty=0.3)


def chain_inputs(V: int, k: int = 3):
    lats = walker_lattices(V, True)
    rng = np.random.default_rng(31 * V)
    N = len(lats) * k
    scores = rng.normal(0.0, 3.0, size=(CHAIN_STEPS, N, V)).astype(F32)
    u = rng.random((CHAIN_STEPS, N)).astype(F32)
    # the insertion mark: the label most arcs carry, so that its counter passes the threshold on some walkers
    marks = np.concatenate([l.label[l.label >= synth.N_SPECIAL] for l in lats])
    mark = int(np.bincount(marks).argmax())
    row_off = np.concatenate([[0], np.cumsum([l.n_rows for l in lats])[:-1]]).astype(np.int64)
    values = rng.normal(0.0, 0.5, size=sum(l.n_rows for l in lats)).astype(F32)
    # (the counters carry from earlier steps: every third walker starts above the insertion threshold)
    return dict(lats=lats, scores=scores, u=u, mark=mark, N=N, row_off=row_off, values=values, accumulated=np.arange(N, dtype=np.int64) % 3,
                state=np.ones(N, np.int64), inp=np.full(N, BOS, np.int64), vstate=np.zeros(N, np.int64))


# ----------------------------------------------------------------------------- the sampler cases
BIG_V = 30000


def oracle_walks(l, sc64, u):
    """(oracle.sample_paths on float64 scores with the oracle's own beta, log Z, log beta)."""
    o = O.forward_backward(l.n_rows, l.src, l.dst, sc64)
    with np.errstate(invalid="ignore"):
        ref = O.sample_paths(l.n_rows, l.src, l.label, l.dst, sc64, o["logbeta"], u.astype(np.float64), PAD)
    return ref, o["logZ"], o["logbeta"]


def beta_me(logbeta) -> np.ndarray:
    """float64 log beta -> the engine's (mantissa, exponent) pairs [n, 2] int32 words: beta = m * 2^e with the float32
    bits of m in word 0 and the integer e in word 1 (an exact zero: m = 0, e = -2^28).  For vocabularies too large
    for the sweeps' LDS, where the sampler takes its beta from the caller."""
    lb = np.asarray(logbeta, np.float64)
    live = lb > -np.inf
    e = np.where(live, np.floor(np.where(live, lb, 0.0) / np.log(2.0)), -(1 << 28))
    m = np.where(live, np.exp(np.where(live, lb, 0.0) - e * np.log(2.0)), 0.0).astype(F32)
    return np.stack([m.view(np.int32), e.astype(np.int32)], axis=1)


def sampler_case(name: str) -> dict:
    """lats, theta ([V] or [B, V]), arc_scores (over the batch's arcs, or None), K, dead (labels at -inf)."""
    if name == "big_vocab":  # max_rows * 8 + vocab * 4 > 96 KiB: the label scores stay in global memory
        lats = [synth.layered_lattice(600 + i, n_states=40 + 30 * i, avg_degree=4.0, vocab=BIG_V, width=4, span=2) for i in range(4)]
        return dict(lats=lats, theta=synth.label_scores(21, BIG_V, mean=-1.0, std=1.0), asc=None, K=24, dead=None)
    if name == "big_vocab_big_lattice":  # ... and a lattice whose CSR does not fit LDS: arcs read from global memory
        lats = [synth.layered_lattice(41, n_states=3000, avg_degree=10.0, vocab=BIG_V, width=16, span=6)]
        return dict(lats=lats, theta=synth.label_scores(22, BIG_V, mean=-1.0, std=1.0), asc=None, K=24, dead=None)
    V = 64
    lats = [synth.layered_lattice(80 + i, n_states=60 + 70 * i, avg_degree=6.0, vocab=V, width=6, span=3, weighted=True) for i in range(4)]
    n_arcs = sum(l.n_arcs for l in lats)
    if name.startswith("per_lattice_k"):
        K = int(name[len("per_lattice_k"):])
        theta = np.stack([synth.label_scores(50 + b, V, mean=-1.0, std=1.0) for b in range(len(lats))])
        asc = np.random.default_rng(8).normal(0.0, 0.5, size=n_arcs).astype(F32)
        return dict(lats=lats, theta=theta, asc=asc, K=K, dead=None)
    if name == "dead_labels":
        theta = synth.label_scores(60, V, mean=-1.0, std=1.0)
        dead = np.array([5, 9, 17, 23, 31, 40, 41, 55])
        theta[dead] = -np.inf
        return dict(lats=lats, theta=theta, asc=None, K=64, dead=dead)
    raise KeyError(name)


SAMPLER_CASES = ("big_vocab", "big_vocab_big_lattice", "per_lattice_k1", "per_lattice_k5", "per_lattice_k17", "per_lattice_k100",
                 "dead_labels")


def sampler_uniforms(c: dict, name: str) -> np.ndarray:
    T = max(int(levels(l.n_rows, l.src, l.dst).max()) for l in c["lats"]) + 1
    return np.random.default_rng(abs(hash_name(name))).random((len(c["lats"]), c["K"], T)).astype(F32)


def hash_name(name: str) -> int:
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))  # (a seed that does not depend on PYTHONHASHSEED)


def sampler_refs(c: dict, u: np.ndarray):
    """Per lattice: (oracle walks, log Z, float64 arc scores, log beta)."""
    out, a0 = [], 0
    for b, l in enumerate(c["lats"]):
        th = c["theta"][b] if c["theta"].ndim == 2 else c["theta"]
        sc = score64(l, th, l.weight, None if c["asc"] is None else c["asc"][a0:a0 + l.n_arcs])
        ref, logz, logbeta = oracle_walks(l, sc, u[b])
        out.append((ref, logz, sc, logbeta))
        a0 += l.n_arcs
    return out

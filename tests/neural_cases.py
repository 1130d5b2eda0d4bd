"""Inputs of the edge tests of the neuralised beta kernels (test helper, not a test module).

tests/test_gpu_neural_edges.py runs ``nfst_backward_neural`` / ``nfst_backward_neural_grad`` on these inputs against the
float64 oracle; tests/test_neural_cases_cpu.py proves on the host -- with the launchers' predicates restated below and
the host packer's tile programs -- that the inputs reach the branches they are named for.  Both sides build their
inputs here, so they cannot drift apart.
"""
from __future__ import annotations

import functools

import numpy as np

from nfst_amd import _lib, synth
from nfst_amd.lattice import LatticeBatch
from oracle import oracle as O

PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
PARAMS = ("emb", "Wx", "Wh", "W", "bias")

# ----------------------------------------------------------------------------- the launchers, restated
MAX_LDS = 160 * 1024                      # kMaxLds (kernels.hip)
ROWS_LDS = 32                             # kNeuRows (neural_kernels.h): states of a tile whose rows stay in LDS
STAGE_WORDS = 64 + 256 + 256 + 64 + 4     # kNeuStageWords
GRAD_STAGE_WORDS = STAGE_WORDS + 256      # kNeuGradStageWords
MAX_HID = 512                             # kNeuMaxHid


def with_hid(hid):
    """with_hid (kernels.hip): ('small', LPR) up to 32, then ('two_phase', HC)."""
    if hid <= 8:
        return "small", 8
    if hid <= 16:
        return "small", 16
    if hid <= 32:
        return "small", 32
    if hid <= 64:
        return "two_phase", 1
    if hid <= 128:
        return "two_phase", 2
    if hid <= 256:
        return "two_phase", 4
    return "two_phase", 8


CLASSES = [("small", 8), ("small", 16), ("small", 32), ("two_phase", 1), ("two_phase", 2), ("two_phase", 4), ("two_phase", 8)]
CLASS_RANGE = {("small", 8): (1, 8), ("small", 16): (9, 16), ("small", 32): (17, 32), ("two_phase", 1): (33, 64),
               ("two_phase", 2): (65, 128), ("two_phase", 4): (129, 256), ("two_phase", 8): (257, 512)}


def wh_packed(hid):
    """pack_wh's predicate (kernels.hip): phase B on three bfloat16 parts of Wh."""
    return hid % 64 == 0 and hid >= 256


def phase_b_path(hid):
    """The path neu_phase_b takes (two-phase kernels): `whb` set | (hid & 15) == 0, with or without passes of its
    16-wide tail loop `for (; h < hid; h += 16)` | the scalar loop."""
    if wh_packed(hid):
        return "packed"
    if hid % 16 == 0:
        return "f32_tail16" if hid % 64 else "f32"
    return "scalar"


def class_paths(cls):
    """Every phase-B path a two-phase class can take."""
    lo, hi = CLASS_RANGE[cls]
    return {phase_b_path(h) for h in range(lo, hi + 1)}


def rows_al(rows):  # neu_rows_al
    return (rows + 1) & ~1


def row_stride(hid):  # NeuLds::row_stride
    return ((hid + 15) & ~15) + 4


def planes_bytes(hid):  # NeuLds::planes_bytes
    return 3 * 16 * (hid + 8) * 2


def _al16(x):
    return (x + 15) & ~15


def neu_lds_bytes(rows, hid):
    """NeuLds(rows, hid).bytes(): the dynamic LDS of nfst_backward_neural (both of its kernels)."""
    return _al16(rows_al(rows) * 8 + 2 * STAGE_WORDS * 4 + ROWS_LDS * row_stride(hid) * 4) + planes_bytes(hid)


def neu_grad_lds_bytes(rows, hid):
    """NeuGradLds(rows, hid).bytes(): the dynamic LDS of k_backward_neural_grad."""
    b0 = rows_al(rows) * 8 + ((rows + 3) & ~3) * 4 + 2 * GRAD_STAGE_WORDS * 4 + ROWS_LDS * row_stride(hid) * 4 + 16
    return _al16(b0) + planes_bytes(hid)


def lds_small0(rows):
    """lds_small0 of nfst_backward_neural_grad: k_backward_neural_grad_small without its dL/dx table."""
    return rows_al(rows) * 8 + ((rows + 3) & ~3) * 4 + 2 * GRAD_STAGE_WORDS * 4 + 16


def gx_in_lds(rows, hid, vocab):
    """The gx_in_lds predicate of nfst_backward_neural_grad."""
    return hid <= 8 and lds_small0(rows) + vocab * hid * 4 <= MAX_LDS


def largest_rows(fn, hid):
    """The largest max_rows whose `fn(rows, hid)` bytes fit the 160 KiB of a workgroup."""
    lo, hi = 1, 1 << 14
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if fn(mid, hid) <= MAX_LDS else (lo, mid - 1)
    assert fn(lo, hid) <= MAX_LDS < fn(lo + 1, hid)
    return lo


# ----------------------------------------------------------------------------- tile programs on the host
def leaders_per_tile(lat, b, direction):
    """Group leaders (bit 31 of the control word, tile_format.h) of every tile of lattice b's program."""
    m = lat.meta_host[b]
    if direction == "fwd":
        s, off, tiles, u = lat.fwd_stream, int(m[_lib.META_FWD_OFF]), int(m[_lib.META_FWD_TILES]), int(m[_lib.META_FWD_U]) & 0xFF
    else:
        s, off, tiles, u = lat.bwd_stream, int(m[_lib.META_BWD_OFF]), int(m[_lib.META_BWD_TILES]), int(m[_lib.META_BWD_U]) & 0xFF
    s = s.cpu().numpy().view(np.uint32)
    out = []
    for T in range(tiles):
        if u == 8:  # compact: 16 bytes per lane, the control word first
            ctl = s[off + T * 256: off + (T + 1) * 256: 4]
        else:
            st = 64 * (1 + u)
            ctl = s[off + T * st: off + T * st + 64]
        out.append(int(np.count_nonzero(ctl >> 31)))
    return out


def max_leaders(lat, direction):
    return max(max(leaders_per_tile(lat, b, direction), default=0) for b in range(lat.meta_host.shape[0]))


# ----------------------------------------------------------------------------- parameters and references
def neural_params(seed, V, H, scale=2.0, emb_scale=1.0):
    """As _neural_params of tests/test_gpu_parity.py (xavier_uniform like the reference's scorer), Wh times `scale`."""
    g = np.random.default_rng(seed)
    lim = np.sqrt(6.0 / (2 * H))
    return dict(emb=(emb_scale * g.standard_normal((V, H))).astype(np.float32), Wx=g.uniform(-lim, lim, (H, H)).astype(np.float32),
                Wh=(scale * g.uniform(-lim, lim, (H, H))).astype(np.float32),
                W=g.uniform(-np.sqrt(6.0 / (1 + H)), np.sqrt(6.0 / (1 + H)), (1, H)).astype(np.float32),
                bias=(0.3 * g.standard_normal(H)).astype(np.float32))


def coefficients(seed, l, H, zero_rows=None):
    """dL/d log beta [n_rows] and dL/d beta_hat [n_rows, H] of the test's loss."""
    g = np.random.default_rng(seed)
    c, ch = g.normal(size=l.n_rows), 0.3 * g.normal(size=(l.n_rows, H))
    if zero_rows is not None:
        c[zero_rows] = 0.0
        ch[zero_rows] = 0.0
    return c, ch


def oracle_forward(l, p):
    return O.beta_neural(l.n_rows, l.src, l.label, l.dst, p["emb"], p["Wx"], p["Wh"], p["W"], p["bias"], arc_w=l.weight)


def oracle_grad(l, p, coef, coef_hat):
    """(log beta, beta_hat, {name: gradient shaped like the parameter}) in float64."""
    _, logb, bhat, g = O.beta_neural_grad(l.n_rows, l.src, l.label, l.dst, p["emb"], p["Wx"], p["Wh"], p["W"], p["bias"], coef,
                                          arc_w=l.weight, coef_hat=coef_hat)
    return logb, bhat, {k: g[k].reshape(np.shape(p[k])) for k in PARAMS}


# ----------------------------------------------------------------------------- hidden sizes
# the first size above every with_hid boundary, H = 1, the 16-wide tail of phase B's float32 path (48, 80, 144, 208,
# 272), <8> unpacked (257, 272, 300, 500) and packed H = 448
HIDDEN = (1, 9, 17, 33, 48, 65, 80, 129, 144, 208, 257, 272, 300, 448, 500)
HIDDEN_PACKINGS = (dict(), dict(group_mode=1, slots_per_lane=1))
V_BATCH, V_STAR = 64, 256


@functools.lru_cache(maxsize=None)
def grad_batch():  # (the batch of test_beta_neural_grad_against_autograd)
    V = V_BATCH
    return (synth.layered_lattice(71, n_states=120, avg_degree=5.0, vocab=V, width=4, span=3, weighted=True),
            synth.layered_lattice(72, n_states=40, avg_degree=3.0, vocab=V, width=1, span=2, weighted=True),
            synth.layered_lattice(73, n_states=200, avg_degree=10.0, vocab=V, width=20, span=2, max_degree=30, weighted=True))


@functools.lru_cache(maxsize=None)
def star(V=V_STAR):
    """A 200-way fan-out and fan-in; the 200 arcs into the last state but one all carry label 5."""
    src = [0] + [1] * 200 + list(range(2, 202)) + [202]
    lab = [BOS] + list(range(3, 203)) + [5] * 200 + [EOS]
    dst = [1] + list(range(2, 202)) + [202] * 200 + [203]
    return synth._finish(204, V, src, lab, dst)


@functools.lru_cache(maxsize=None)
def double_funnel(V=V_STAR):
    """The star twice in a row: the scratch rows of its partial groups are rewritten at the next level."""
    src = [0] + [1] * 200 + list(range(2, 202)) + [202] * 200 + list(range(203, 403)) + [403]
    lab = [BOS] + list(range(3, 203)) + [5] * 200 + list(range(3, 203)) + [6] * 200 + [EOS]
    dst = [1] + list(range(2, 202)) + [202] * 200 + list(range(203, 403)) + [403] * 200 + [404]
    return synth._finish(405, V, src, lab, dst)


# ----------------------------------------------------------------------------- many groups per tile
GROUPS_HIDDEN = (33, 64, 100, 256, 272)
GROUPS_PACKINGS = (dict(), dict(slots_per_lane=1), dict(group_mode=2))
FETCH_BACK_LEADERS = 46  # round >= 2 of neu_group_of (groups from 31 on) and a fetch-back pass of phase B with a partial last 16


@functools.lru_cache(maxsize=None)
def wide():
    return synth.layered_lattice(5, n_states=400, avg_degree=1.6, vocab=256, width=48, span=1)


def groups_lattices():
    return dict(star=star(), double_funnel=double_funnel(), wide=wide())


# ----------------------------------------------------------------------------- the dL/dx table of the small gradient kernel
GX_HIDDEN = (5, 8)


@functools.lru_cache(maxsize=None)
def gx_base():
    return (synth.layered_lattice(81, n_states=60, avg_degree=4.0, vocab=256, width=4, span=2), star())


def remap_vocab(l, V):
    """The lattice with its ordinary labels spread monotonically over a vocabulary of V (arc order and determinism stay)."""
    k = (V - synth.N_SPECIAL) // (l.vocab - synth.N_SPECIAL)
    assert k >= 1
    lab = np.where(l.label < synth.N_SPECIAL, l.label, synth.N_SPECIAL + (l.label - synth.N_SPECIAL) * k).astype(np.int32)
    assert lab.max() < V
    return synth.SynthLattice(n_rows=l.n_rows, vocab=V, src=l.src, label=lab, dst=l.dst, weight=l.weight)


@functools.lru_cache(maxsize=None)
def gx_pair(H):
    """(V_in, V_out, max_rows): the largest vocabulary whose [V, H] table still fits beside the rows and staged tiles of
    k_backward_neural_grad_small, and the first that does not."""
    probe = LatticeBatch.from_synth([remap_vocab(l, 5000) for l in gx_base()])
    rows = int(probe.max_rows)
    v_in = (MAX_LDS - lds_small0(rows)) // (H * 4)
    return int(v_in), int(v_in) + 1, rows


def gx_lattices(V):
    return [remap_vocab(l, V) for l in gx_base()]


# ----------------------------------------------------------------------------- LDS limits
LIMIT_HIDDEN = (512, 500)
LIMIT_WIDTH = 64


@functools.lru_cache(maxsize=None)
def limit_lattice(max_rows):
    """A layered lattice of `max_rows` rows, 64 states a level: max_rows = n_states + 1 under the default packing."""
    return synth.layered_lattice(91, n_states=max_rows - 1, avg_degree=2.0, vocab=256, width=LIMIT_WIDTH, span=1)


def limit_rows(H):
    """max_rows of the four limit cases of hidden size H: the largest the forward op takes, one state more in the last
    level, the largest its gradient takes, one state more (the forward takes that one, its gradient does not)."""
    f, g = largest_rows(neu_lds_bytes, H), largest_rows(neu_grad_lds_bytes, H)
    return dict(fwd_fits=f, fwd_refused=f + 1, grad_fits=g, grad_refused=g + 1)


@functools.lru_cache(maxsize=None)
def small_lattice():
    return synth.layered_lattice(92, n_states=50, avg_degree=4.0, vocab=256, width=4, span=2)


# ----------------------------------------------------------------------------- dead rows
DEAD_HIDDEN = (8, 64)
V_DEAD = 64


@functools.lru_cache(maxsize=None)
def dead_case():
    """(lattice, live neighbour, dead state, state with one arc at -inf): every out-arc of `dead` has table weight -inf,
    and so has one arc of `partial`, which keeps live ones."""
    l = synth.layered_lattice(95, n_states=48, avg_degree=4.0, vocab=V_DEAD, width=4, span=2, weighted=True)
    sink = l.n_rows - 1
    outdeg = np.bincount(l.src, minlength=l.n_rows)
    real = l.src != l.dst
    # an interior state all of whose predecessors have another way on
    dead = next(int(s) for s in range(2, sink)
                if outdeg[s] >= 2 and np.any(l.dst == s) and np.all(outdeg[l.src[real & (l.dst == s)]] >= 2)
                and not np.any(l.dst[l.src == s] == sink))
    partial = next(int(s) for s in range(2, sink) if s != dead and outdeg[s] >= 3 and not np.any(l.dst[l.src == s] == dead))
    w = l.weight.copy()
    w[l.src == dead] = -np.inf
    w[np.nonzero(l.src == partial)[0][1]] = -np.inf
    lat = synth.SynthLattice(n_rows=l.n_rows, vocab=l.vocab, src=l.src, label=l.label, dst=l.dst, weight=w)
    live = synth.layered_lattice(96, n_states=70, avg_degree=5.0, vocab=V_DEAD, width=5, span=3, weighted=True)
    return lat, live, dead, partial


def dead_params(H):
    return neural_params(60 + H, V_DEAD, H)


def pruned(l, logb):
    """The lattice without its arcs of weight -inf and without every arc that touches a row whose log beta is -inf."""
    gone = np.isneginf(logb)
    keep = ~(np.isneginf(l.weight) | gone[l.src] | gone[l.dst])
    return synth.SynthLattice(n_rows=l.n_rows, vocab=l.vocab, src=l.src[keep], label=l.label[keep], dst=l.dst[keep], weight=l.weight[keep])


# ----------------------------------------------------------------------------- exponent range
RANGE_HIDDEN = (8, 64)
RANGE_WEIGHTS = (0.0, -30.0, -80.0, -100.0)
DROP_NATS = 120 * np.log(2.0)  # neu_scale(d > 120) = 0: a sibling more than 120 binary orders below the largest is dropped
ME_LOG32_EXACT = 1419.0        # |log beta| up to which the product e * ln2_high of me_log32 is exact


@functools.lru_cache(maxsize=None)
def range_lattice():
    """Eleven levels whose table weights are drawn from RANGE_WEIGHTS."""
    l = synth.layered_lattice(97, n_states=56, avg_degree=5.0, vocab=64, width=6, span=2, weighted=True)
    w = np.random.default_rng(98).choice(np.array(RANGE_WEIGHTS, np.float32), size=l.n_arcs).astype(np.float32)
    w[l.src == l.dst] = 0.0
    return synth.SynthLattice(n_rows=l.n_rows, vocab=l.vocab, src=l.src, label=l.label, dst=l.dst, weight=w)


def range_params(H):
    return neural_params(40 + H, 64, H, scale=2.0, emb_scale=8.0)


def arc_logits(l, p, logb, bhat):
    """z_a = W . t_a + arc_w + log beta(dst) of every arc, float64, from the oracle's rows."""
    x = p["emb"].astype(np.float64) @ p["Wx"].T.astype(np.float64) + p["bias"]
    t = np.tanh(x[l.label] + bhat[l.dst] @ p["Wh"].T.astype(np.float64))
    return t @ p["W"].reshape(-1).astype(np.float64) + l.weight + logb[l.dst]


# ----------------------------------------------------------------------------- the recurrence in float32
def beta_neural_f32(l, p):
    """The recurrence of the kernels in NumPy float32, state after state in topological order: beta as a float32 mantissa
    with an integer exponent (as the kernels keep it), tanh, exp and every sum in float32.  What float32 arithmetic alone
    leaves of the float64 oracle on a lattice: (log beta as float64 of the pair, beta_hat float32)."""
    f32 = np.float32
    keep = l.src != l.dst
    src, label, dst = l.src[keep].astype(np.int64), l.label[keep].astype(np.int64), l.dst[keep].astype(np.int64)
    aw = (np.zeros(src.shape[0], f32) if l.weight is None else l.weight[keep].astype(f32))
    emb, Wx, Wh, W, bias = (np.asarray(p[k], f32) for k in PARAMS)
    W = W.reshape(-1)
    x = (emb @ Wx.T + bias).astype(f32)
    n, H = l.n_rows, emb.shape[1]
    order = np.argsort(src, kind="stable")
    first = np.searchsorted(src[order], np.arange(n + 1))
    pending = np.bincount(src, minlength=n)
    into = [[] for _ in range(n)]
    for a in range(src.shape[0]):
        into[dst[a]].append(a)
    sink = n - 1
    mant, expo = np.zeros(n, f32), np.zeros(n, np.int64)
    bhat = np.zeros((n, H), f32)
    mant[sink], expo[sink] = 0.5, 1
    ready = [sink]
    while ready:
        s2 = ready.pop()
        for a in into[s2]:
            s = src[a]
            pending[s] -= 1
            if pending[s]:
                continue
            ready.append(s)
            arcs = order[first[s]:first[s + 1]]
            t = np.tanh((x[label[arcs]] + bhat[dst[arcs]] @ Wh.T).astype(f32)).astype(f32)
            sc = (t @ W + aw[arcs]).astype(f32)
            live = (mant[dst[arcs]] > 0) & np.isfinite(sc)
            if not np.any(live):
                continue
            wm, we = np.frexp(np.exp(sc[live].astype(np.float64)).astype(np.float64))  # exp to float32 accuracy below
            wm = wm.astype(f32)
            m = (wm * mant[dst[arcs]][live]).astype(f32)
            e = we + expo[dst[arcs]][live]
            q = np.ldexp(m, (e - e.max()).astype(np.int64)).astype(f32)
            tot = f32(q.sum(dtype=f32))
            bhat[s] = ((q / tot).astype(f32) @ t[live]).astype(f32)
            mant[s], ex = np.frexp(tot)
            expo[s] = ex + e.max()
    logb = np.where(mant > 0, np.log(np.maximum(mant.astype(np.float64), 1e-300)) + expo * np.log(2.0), -np.inf)
    return logb, bhat


def grad_f32(l, p, coef, coef_hat):
    """The gradients of the test's loss by torch.autograd over the same recurrence in float32.  log beta(s) is carried as
    a float64 constant plus a small float32 remainder (the kernels' mantissa and exponent), so that no rounding at the
    magnitude of log beta enters; tanh, exp, every sum and the whole backward pass are float32."""
    import torch
    f32 = torch.float32
    keep = l.src != l.dst
    src, label, dst = l.src[keep].astype(np.int64), l.label[keep].astype(np.int64), l.dst[keep].astype(np.int64)
    aw = torch.zeros(src.shape[0], dtype=f32) if l.weight is None else torch.tensor(l.weight[keep], dtype=f32)
    P = {k: torch.tensor(np.asarray(p[k], np.float32).reshape(-1) if k == "W" else np.asarray(p[k], np.float32), dtype=f32,
                         requires_grad=True) for k in PARAMS}
    n, H = l.n_rows, P["emb"].shape[1]
    x = P["emb"] @ P["Wx"].T + P["bias"]
    order = np.argsort(src, kind="stable")
    first = np.searchsorted(src[order], np.arange(n + 1))
    pending = np.bincount(src, minlength=n)
    into = [[] for _ in range(n)]
    for a in range(src.shape[0]):
        into[dst[a]].append(a)
    sink = n - 1
    off = np.zeros(n)
    res, bhat = [None] * n, [None] * n
    res[sink], bhat[sink] = torch.zeros((), dtype=f32), torch.zeros(H, dtype=f32)
    ready = [sink]
    while ready:
        s2 = ready.pop()
        for a in into[s2]:
            s = src[a]
            pending[s] -= 1
            if pending[s]:
                continue
            ready.append(s)
            arcs = order[first[s]:first[s + 1]]
            d = dst[arcs]
            t = torch.tanh(x[torch.as_tensor(label[arcs])] + torch.stack([bhat[i] for i in d]) @ P["Wh"].T)
            off[s] = off[d].max()
            lm = t @ P["W"] + aw[torch.as_tensor(arcs)] + torch.stack([res[i] for i in d]) + torch.tensor(off[d] - off[s], dtype=f32)
            res[s] = torch.logsumexp(lm, 0)
            bhat[s] = torch.softmax(lm, 0) @ t
    loss = torch.zeros((), dtype=f32)
    ch = torch.tensor(np.asarray(coef_hat, np.float32))
    for s in range(n):
        if res[s] is not None:
            loss = loss + float(coef[s]) * res[s] + (ch[s] * bhat[s]).sum()
    loss.backward()
    return {k: P[k].grad.numpy().astype(np.float64).reshape(np.shape(p[k])) for k in PARAMS}

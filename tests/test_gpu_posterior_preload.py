"""The label weights of the preloaded arc groups, gathered in front of the barrier ("The epilogue").

A forward-backward launch of the tile-wave flavour without per-arc extras and without label sums runs an instantiation in
which the helper waves that are no tile waves (10 .. 15: the second half of every block of 3072 preloaded arcs) gather ``th[label]``
for their 7 preloaded groups of 4 arcs while the sweeps run and keep the (mantissa, exponent) pairs in registers in place of
the labels; behind the barrier only the ``alpha`` / ``beta`` gathers remain for them.  The
arithmetic is ``arc_posterior`` on the same table entries, so every posterior must have the bits of the pipeline flavour
(``tuning(tw=0)``), which computes the same function and never takes that path, and lie within 2e-6 of the float64 oracle
(the bound of tests/test_gpu_epilogue.py).

Arc counts straddle the thread mapping -- fewer arcs than one aligned group, one group per helper thread (3072), the last
preloaded and the first remainder group (21,504) -- alone and behind a lattice with 4k+1 / 4k+2 / 4k+3 arcs (unaligned
``arc_off``: the aligned interior and with it every boundary moves).  Lattices are explicit arc lists: a layered lattice
padded with parallel arcs to the exact count (a lattice's count includes the sink's pad self loop, so one arc is the
one-row lattice).  Launches with label sums or caller ``arc_scores`` take the instantiations that were there before.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from nfst_amd import ops, synth, _lib
from nfst_amd.lattice import LatticeBatch
from nfst_amd.synth import SynthLattice

pytestmark = pytest.mark.gpu

V = 256
GROUP_ARCS = 768 * 4  # arcs one preloaded group per helper thread covers
PRELOAD_ARCS = 7 * GROUP_ARCS
POST_TOL = 2e-6  # tests/test_gpu_epilogue.py


def padded(l: SynthLattice, n_arcs: int, seed: int) -> SynthLattice:
    """``l`` with parallel arcs added up to exactly ``n_arcs`` arcs: a new arc copies source and destination of an
    existing one (never the sink's self loop) under a label its source does not use yet; levels and depth stay."""
    rng = np.random.default_rng(seed)
    used = np.zeros((l.n_rows, l.vocab), bool)
    used[l.src, l.label] = True
    used[:, :synth.N_SPECIAL] = True
    order = rng.permutation(np.nonzero(l.src != l.dst)[0])
    need = n_arcs - l.n_arcs
    assert need >= 0
    new_s, new_l, new_d = [], [], []
    k = 0
    while need > 0:
        a = int(order[k % order.shape[0]])
        k += 1
        s = int(l.src[a])
        free = np.nonzero(~used[s])[0]
        if free.shape[0] == 0:
            continue
        lab = int(free[rng.integers(0, free.shape[0])])
        used[s, lab] = True
        new_s.append(s); new_l.append(lab); new_d.append(int(l.dst[a]))
        need -= 1
    src = np.concatenate([l.src, np.array(new_s, np.int32)])
    label = np.concatenate([l.label, np.array(new_l, np.int32)])
    dst = np.concatenate([l.dst, np.array(new_d, np.int32)])
    o = np.lexsort((label, src))
    out = SynthLattice(l.n_rows, l.vocab, src[o].astype(np.int32), label[o].astype(np.int32), dst[o].astype(np.int32))
    assert out.n_arcs == n_arcs
    return out


@functools.lru_cache(maxsize=None)
def lattice_of(n_arcs: int, vocab: int = V) -> SynthLattice:
    """A lattice of exactly ``n_arcs`` arcs over ``vocab`` labels."""
    if n_arcs == 1:
        return synth._finish(1, vocab, [], [], [])  # the sink is the start: its pad self loop is the only arc
    if n_arcs == 2:
        return synth._finish(2, vocab, [0], [synth.EOS], [1])
    if n_arcs == 3:
        return synth._finish(3, vocab, [0, 1], [synth.BOS, synth.EOS], [1, 2])
    if n_arcs == 4:
        return synth._finish(3, vocab, [0, 1, 1], [synth.BOS, synth.EOS, 7], [1, 2, 2])
    if n_arcs < 200:
        base = synth.layered_lattice(77, n_states=12, avg_degree=3.0, vocab=vocab, width=3, span=2)
    elif n_arcs < 16000:
        base = synth.layered_lattice(4243, n_states=301, avg_degree=8.0, vocab=vocab, width=32, span=4)
    else:
        base = synth.layered_lattice(4242, n_states=2001, avg_degree=8.0, vocab=vocab, width=128, span=4)
    return padded(base, n_arcs, seed=n_arcs)


@functools.lru_cache(maxsize=None)
def lead_lattice(k: int) -> SynthLattice:
    """A small lattice with 4j + k arcs: the lattice behind it starts at an unaligned ``arc_off``."""
    n = 61
    while n % 4 != k:
        n += 1
    return lattice_of(n)


def theta_plain(vocab: int = V) -> np.ndarray:
    return synth.label_scores(11, vocab)


def theta_extreme(vocab: int = V) -> np.ndarray:
    """Label scores with weight zero (-inf), a weight far below float32's range (-1e4) and one far above 1 (+80); the
    special labels (every path has bos and eos) keep ordinary scores."""
    th = synth.label_scores(12, vocab).copy()
    th[[5, 17, 100, vocab - 1]] = -np.inf
    th[[7, 33]] = -1.0e4
    th[[9, 64]] = 80.0
    return th


_ORACLE = {}


def oracle_posterior(l: SynthLattice, theta: np.ndarray, key, arc_scores=None):
    """float64 arc posteriors of one lattice, computed once per key."""
    if key not in _ORACLE:
        sc = theta[l.label].astype(np.float64)
        if arc_scores is not None:
            sc = sc + arc_scores.astype(np.float64)
        _ORACLE[key] = O.forward_backward(l.n_rows, l.src, l.dst, sc)["posterior"]
    return _ORACLE[key]


def arcs_of(t, lat, b):
    a0, a1 = int(lat.arc_off[b]), int(lat.arc_off[b + 1]) if b + 1 < lat.n_lattices else lat.total_arcs
    return t[a0:a1]


def pack(lattices, dev) -> LatticeBatch:
    lat = LatticeBatch.from_synth(list(lattices), device=dev)
    c = lat.c_struct()
    # all-compact and at most 192 tiles: the float32 tile-wave kernel runs this batch
    assert c.reserved0 & 1 and c.max_tiles <= 192
    assert (c.reserved0 >> 8) == max(l.n_arcs for l in lattices)
    return lat


def check_posteriors(lat, lattices, theta: np.ndarray, keys, per_lattice_theta=None):
    """The posteriors of the default flavour: the bits of the pipeline flavour, and the oracle's values.  ``theta``: [V], or
    [B, V] with ``per_lattice_theta`` (one row per lattice)."""
    th = torch.from_numpy(theta)
    got = ops.forward_backward(lat, th, want_alpha_beta=False)
    with _lib.tuning(tw=0):
        ref = ops.forward_backward(lat, th, want_alpha_beta=False)
    assert torch.equal(got.posterior, ref.posterior), "tile waves against the pipeline"
    assert torch.equal(got.logz64, ref.logz64)
    post = got.posterior.cpu().numpy()
    for b, l in enumerate(lattices):
        row = theta[b] if per_lattice_theta else theta
        o = oracle_posterior(l, row, keys[b])
        p = arcs_of(post, lat, b)
        assert p.shape[0] == l.n_arcs
        err = float(np.max(np.abs(p - o)))
        print(f"lattice {b}: {l.n_arcs} arcs, max |posterior - oracle| = {err:.3g}")
        assert err <= POST_TOL, (b, l.n_arcs, err)
    return got


# fewer arcs than an aligned group; one group per helper thread; the last preloaded and the first remainder group
COUNTS = [1, 2, 3, 4, GROUP_ARCS - 1, GROUP_ARCS, GROUP_ARCS + 1, PRELOAD_ARCS - 1, PRELOAD_ARCS, PRELOAD_ARCS + 1]


@pytest.mark.parametrize("n_arcs", COUNTS)
def test_arc_counts_around_the_thread_mapping(dev, n_arcs):
    """Alone (``arc_off`` 0), and second behind a lattice of 4j + k arcs, k = 1, 2, 3: the same bits as alone."""
    l = lattice_of(n_arcs)
    assert l.n_arcs == n_arcs
    th = theta_plain()
    alone = check_posteriors(pack([l], dev), [l], th, [("plain", n_arcs)])
    for k in (1, 2, 3):
        lead = lead_lattice(k)
        lat = pack([lead, l], dev)
        assert int(lat.arc_off[1]) % 4 == k
        got = check_posteriors(lat, [lead, l], th, [("plain", lead.n_arcs), ("plain", n_arcs)])
        assert torch.equal(arcs_of(got.posterior, lat, 1), alone.posterior), f"behind 4j+{k} arcs against alone"


def test_only_one_lattice_of_the_batch_has_a_remainder(dev):
    """Two lattices in both orders: one within the preload, one with remainder groups, an odd count between them."""
    small, big = lattice_of(PRELOAD_ARCS - 1003), lattice_of(PRELOAD_ARCS + 761)
    th = theta_plain()
    for pair in ((small, big), (big, small)):
        check_posteriors(pack(pair, dev), pair, th, [("plain", l.n_arcs) for l in pair])


@pytest.mark.parametrize("n_arcs", [GROUP_ARCS + 1, PRELOAD_ARCS + 1])
def test_label_weights_zero_tiny_and_huge(dev, n_arcs):
    """Every label of the vocabulary on some arc; scores of -inf (weight zero), -1e4 and +80 (large exponents)."""
    l = lattice_of(n_arcs)
    assert np.unique(l.label).shape[0] == V
    th = theta_extreme()
    got = check_posteriors(pack([l], dev), [l], th, [("extreme", n_arcs)])
    post = got.posterior.cpu().numpy()
    assert np.all(post[np.isneginf(th[l.label])] == 0.0) and np.all(np.isfinite(post)) and post.max() > 0.5


@pytest.mark.parametrize("vocab", [256, 2046])
def test_smallest_vocabulary_and_the_compact_limit(dev, vocab):
    l = lattice_of(GROUP_ARCS + 5, vocab)
    assert l.vocab == vocab and int(l.label.max()) > vocab - 64  # (labels from the whole table)
    check_posteriors(pack([l], dev), [l], theta_extreme(vocab), [("extreme", l.n_arcs, vocab)])


def test_per_lattice_score_rows(dev):
    """``theta`` of shape [B, V] (``theta_stride`` = V): every lattice gathers from its own row."""
    group = [lattice_of(GROUP_ARCS + 1), lead_lattice(3), lattice_of(PRELOAD_ARCS + 1), lattice_of(2)]
    rows = np.stack([theta_plain(), theta_extreme(), theta_extreme(), synth.label_scores(13, V)])
    keys = [("plain", group[0].n_arcs), ("extreme", group[1].n_arcs), ("extreme", group[2].n_arcs), ("row3", 2)]
    check_posteriors(pack(group, dev), group, rows, keys, per_lattice_theta=True)


def test_label_sums_and_arc_scores_take_the_other_instantiations(dev):
    """``want_grad_theta`` and caller ``arc_scores`` run the kernels with labels in registers: posteriors with the pipeline's
    bits.  The label sums are float atomics in LDS whose order is not fixed; on a lattice whose arcs all carry different
    labels every sum has one term, and there they have the pipeline's bits too; on the large lattice they are held to the
    oracle (1e-4, as tests/test_gpu_epilogue.py does)."""
    chain = synth._finish(6, V, [0, 1, 1, 2, 3, 4], [synth.BOS, 10, 11, 12, 13, synth.EOS], [1, 2, 3, 4, 4, 5])
    big = lattice_of(PRELOAD_ARCS + 1)
    th_np = theta_plain()
    th = torch.from_numpy(th_np)
    for l, exact in ((chain, True), (big, False)):
        lat = pack([l], dev)
        xs_np = np.random.default_rng(l.n_arcs).normal(0.0, 0.3, size=l.n_arcs).astype(np.float32)
        xs = torch.from_numpy(xs_np)
        plain = ops.forward_backward(lat, th, want_alpha_beta=False)
        g = ops.forward_backward(lat, th, want_alpha_beta=False, want_grad_theta=True)
        s = ops.forward_backward(lat, th, arc_scores=xs, want_alpha_beta=False)
        with _lib.tuning(tw=0):
            g0 = ops.forward_backward(lat, th, want_alpha_beta=False, want_grad_theta=True)
            s0 = ops.forward_backward(lat, th, arc_scores=xs, want_alpha_beta=False)
        assert torch.equal(g.posterior, g0.posterior) and torch.equal(g.posterior, plain.posterior)
        assert torch.equal(s.posterior, s0.posterior)
        o = oracle_posterior(l, th_np, ("plain", "sel", l.n_arcs))
        assert np.max(np.abs(g.posterior.cpu().numpy() - o)) <= POST_TOL
        assert np.max(np.abs(s.posterior.cpu().numpy() - oracle_posterior(l, th_np, ("scored", l.n_arcs), xs_np))) <= POST_TOL
        if exact:
            assert torch.equal(g.grad_theta, g0.grad_theta)
        assert np.max(np.abs(g.grad_theta[0].cpu().numpy() - np.bincount(l.label, weights=o, minlength=V))) <= 1e-4


def test_scores_overwritten_in_place_between_two_calls(dev):
    """A prepared launch, its score tensor overwritten in place, the launch again: the result of a fresh launch on the new
    scores -- no label weight survives from one call to the next."""
    group = [lead_lattice(1), lattice_of(PRELOAD_ARCS + 1)]
    lat = pack(group, dev)
    old, new = theta_plain(), theta_extreme()
    th = torch.from_numpy(old).to(dev)
    launch = ops.ForwardBackwardLaunch(lat, th, want_alpha_beta=False)
    first = launch().posterior.clone()
    assert torch.equal(first, ops.forward_backward(lat, torch.from_numpy(old), want_alpha_beta=False).posterior)
    th.copy_(torch.from_numpy(new))
    second = launch().posterior.clone()
    fresh = ops.forward_backward(lat, torch.from_numpy(new), want_alpha_beta=False)
    assert torch.equal(second, fresh.posterior) and not torch.equal(second, first)
    for b, l in enumerate(group):
        assert np.max(np.abs(arcs_of(second, lat, b).cpu().numpy() - oracle_posterior(l, new, ("extreme", l.n_arcs)))) <= POST_TOL

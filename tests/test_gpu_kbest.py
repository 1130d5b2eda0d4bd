"""ops.k_best (nfst_kbest: the exact k best paths of every lattice) against the float32 NumPy reference of
tests/kbest_ref.py, bit for bit; entry 0 against ops.viterbi; scores against ops.score_paths; gradients; the
LatticeScorer and JointProb entry points."""
import os

import numpy as np
import pytest
import torch

from nfst_amd import _lib, io, ops, synth
from nfst_amd.joint import JointProb
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from oracle import oracle as O
from tests import kbest_ref as R

pytestmark = pytest.mark.gpu
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
V = 64
KS = (1, 2, 7, 20, 64)


def _mixed_batch():  # (the mixed batch of test_gpu_parity.py)
    return [
        synth.layered_lattice(3, n_states=30, avg_degree=3.0, vocab=V, width=4, span=2),
        synth.layered_lattice(4, n_states=300, avg_degree=8.0, vocab=V, width=9, span=5),
        synth.layered_lattice(5, n_states=90, avg_degree=5.0, vocab=V, width=1, span=6),
        synth.edit_lattice([10, 11, 12, 13, 14], [20, 21, 22, 23], vocab=V, seed=2),
        synth.layered_lattice(6, n_states=700, avg_degree=10.0, vocab=V, width=16, span=8),
        synth._finish(2, V, [0], [synth.EOS], [1]),
    ]


def _weighted_batch(n=4, vocab=48):
    return [synth.layered_lattice(s, n_states=150 + 20 * s, avg_degree=6.0, vocab=vocab, width=7, span=3, weighted=True)
            for s in range(n)]


def _star():  # a state with 200 out-arcs (test_gpu_parity.py): its arcs take four chunks of the sweep
    src = [0] + [1] * 200 + list(range(2, 202)) + [202]
    lab = [BOS] + list(range(3, 203)) + [5] * 200 + [EOS]
    dst = [1] + list(range(2, 202)) + [202] * 200 + [203]
    return synth._finish(204, 256, src, lab, dst)


def _refs(lat, lats, theta, asc=None):
    """The reference at k = 64 per lattice: a list of the top k' is the first k' entries of the top 64."""
    out = []
    for b, l in enumerate(lats):
        a0 = int(lat.arc_off[b])
        th_b = theta[b] if theta.ndim == 2 else theta
        th, e = R.arc_terms(l, th_b, None if asc is None else asc[a0:a0 + l.n_arcs])
        out.append(R.k_best(l.n_rows, l.src, l.dst, th, e, 64, l.n_rows - 1))
    return out


def _check(tag, lat, lats, r, refs, k):
    best, paths, arcs = r.best.cpu().numpy(), r.paths.cpu().numpy(), r.arcs.cpu().numpy()
    lens, npt = r.lengths.cpu().numpy(), r.n_paths.cpu().numpy()
    T = paths.shape[2]
    for b, l in enumerate(lats):
        ref = refs[b]
        a0 = int(lat.arc_off[b])
        n = min(k, ref["n_paths"])
        assert npt[b] == n, (tag, b, k)
        assert np.array_equal(best[b].view(np.int32), ref["best"][:k].view(np.int32)), (tag, b, k)  # bits, -inf incl.
        for j in range(k):
            if j < n:
                p = ref["arcs"][j]
                assert lens[b, j] == len(p), (tag, b, k, j)
                assert np.array_equal(arcs[b, j, :len(p)] - a0, p), (tag, b, k, j)
                assert np.array_equal(paths[b, j, :len(p)], l.label[p]), (tag, b, k, j)
            else:
                assert lens[b, j] == 0
            m = lens[b, j]
            assert np.all(paths[b, j, m:] == PAD) and np.all(arcs[b, j, m:] == -1), (tag, b, k, j)
        # distinct paths, non-increasing scores
        assert len({tuple(arcs[b, j, :lens[b, j]]) for j in range(n)}) == n
        assert np.all(np.diff(best[b, :n]) <= 0)
        assert T >= max(1, int(lens[b].max()))


def _check_viterbi(lat, r, v):
    """Entry 0 is Viterbi's path, bit for bit."""
    assert torch.equal(r.best[:, 0], v.best)
    assert torch.equal(r.lengths[:, 0], v.lengths)
    assert torch.equal(r.paths[:, 0], v.paths)
    assert torch.equal(r.arcs[:, 0], v.arcs)


def _check_scores(lat, theta, r, asc=None):
    """ops.score_paths of the returned marks (a float64 sum, rounded once) within 1e-5 (relative) of best."""
    tot, _ = ops.score_paths(lat, theta, r.paths, arc_scores=asc)
    n = r.n_paths.cpu().numpy()
    tot, best = tot.cpu().numpy().astype(np.float64), r.best.cpu().numpy().astype(np.float64)
    for b in range(lat.n_lattices):
        assert np.all(np.abs(tot[b, :n[b]] - best[b, :n[b]]) <= 1e-5 * np.maximum(1.0, np.abs(best[b, :n[b]]))), b


def _run_all_k(tag, lat, lats, theta_np, dev, asc_np=None, viterbi=True):
    theta = torch.from_numpy(theta_np).to(dev)
    asc = None if asc_np is None else torch.from_numpy(asc_np).to(dev)
    refs = _refs(lat, lats, theta_np, asc_np)
    v = ops.viterbi(lat, theta, arc_scores=asc, pad=PAD)
    for k in KS:
        r = ops.k_best(lat, theta, k, arc_scores=asc, pad=PAD)
        _check(tag, lat, lats, r, refs, k)
        if viterbi:
            _check_viterbi(lat, r, v)
        if k in (7, 64):
            _check_scores(lat, theta, r, asc)
    return refs


# ----------------------------------------------------------------------------- bits against the reference
def test_mixed_batch(dev):
    lats = _mixed_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    refs = _run_all_k("mixed", lat, lats, synth.label_scores(8, V), dev)
    for b, l in enumerate(lats):  # n_paths: min(k, paths)
        n = R.count_finite_paths(l.n_rows, l.src, l.dst, np.zeros(l.n_arcs), l.n_rows - 1)
        assert refs[b]["n_paths"] == min(64, n)
    assert refs[5]["n_paths"] == 1  # (a single-arc lattice: one path)


@pytest.mark.parametrize("with_arc_scores", [False, True])
def test_weighted_batch(dev, with_arc_scores):
    lats = _weighted_batch()
    em, tr = synth.collate_dense([l.dense(weighted=True) for l in lats])
    lat = LatticeBatch.from_dense(em, tr, device=dev)
    assert lat.weighted == 1
    rng = np.random.default_rng(0)
    theta = rng.normal(-2.0, 0.7, size=48).astype(np.float32)
    asc = rng.normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32) if with_arc_scores else None
    _run_all_k("weighted", lat, lats, theta, dev, asc, viterbi=False)
    # entry 0 against Viterbi: bit for bit with its general kernel (the adds of nfst_kbest); its tile-wave flavour
    # adds per-arc extras in another order, so there the scores agree to rounding
    th, a = torch.from_numpy(theta).to(dev), None if asc is None else torch.from_numpy(asc).to(dev)
    r = ops.k_best(lat, th, 3, arc_scores=a, pad=PAD)
    with _lib.tuning(tw=0):
        _check_viterbi(lat, r, ops.viterbi(lat, th, arc_scores=a, pad=PAD))
    v = ops.viterbi(lat, th, arc_scores=a, pad=PAD)
    assert torch.max(torch.abs(v.best - r.best[:, 0])) <= 1e-5 * float(torch.max(torch.abs(v.best)))


def test_per_lattice_theta(dev):
    lats = _mixed_batch()[:5]
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = np.stack([synth.label_scores(20 + b, V) for b in range(len(lats))])
    _run_all_k("per-lattice", lat, lats, theta, dev)


@pytest.mark.parametrize("opts", [dict(group_mode=1), dict(group_mode=2), dict(group_mode=1, slots_per_lane=1),
                                  dict(group_mode=2, slots_per_lane=1), dict(group_mode=1, slots_per_lane=4, no_compact=True)])
def test_star_under_every_packing(dev, opts):
    star = _star()
    theta = synth.label_scores(4, 256)
    lat = LatticeBatch.from_synth([star], device=dev, **opts)
    _run_all_k(f"star {opts}", lat, [star], theta, dev)


def test_snips_shaped_batch_ignores_chunked_programs(dev):
    V2 = 250
    lats = synth.snips_shaped_batch(16, vocab=V2)
    theta_np = synth.label_scores(64, V2, mean=-1.5, std=0.8)
    plain = LatticeBatch.from_synth(lats, device=dev)
    host = LatticeBatch.from_synth(lats)
    assert host.build_chunks(force=True)
    chunked = host.to(dev)
    assert chunked.chunks is not None
    _run_all_k("snips", plain, lats, theta_np, dev)
    theta = torch.from_numpy(theta_np).to(dev)
    for k in (1, 20, 64):
        r1, r2 = ops.k_best(plain, theta, k), ops.k_best(chunked, theta, k)
        for x, y in zip(r1, r2):
            assert torch.equal(x, y)


def test_baseline_batch_subset(dev):
    lats = synth.bench_batch(32)
    lat = LatticeBatch.from_synth(lats, device=dev)
    _run_all_k("baseline", lat, lats, synth.label_scores(1, 256), dev)


# ----------------------------------------------------------------------------- gradients
def test_gradients_count_the_paths_marks_and_arcs(dev):
    lats = _mixed_batch()[:4]
    lat = LatticeBatch.from_synth(lats, device=dev)
    k = 7
    rng = np.random.default_rng(3)
    for per_lattice in (False, True):
        th_np = (np.stack([synth.label_scores(30 + b, V) for b in range(len(lats))]) if per_lattice
                 else synth.label_scores(30, V))
        theta = torch.from_numpy(th_np).to(dev).requires_grad_()
        asc = torch.from_numpy(rng.normal(0, 0.2, size=lat.total_arcs).astype(np.float32)).to(dev).requires_grad_()
        r = ops.k_best(lat, theta, k, arc_scores=asc)
        g = torch.from_numpy(rng.normal(0, 1, size=(len(lats), k)).astype(np.float32)).to(dev)
        (r.best * torch.where(torch.isfinite(r.best), g, torch.zeros_like(g))).sum().backward()
        arcs, lens, n = r.arcs.cpu().numpy(), r.lengths.cpu().numpy(), r.n_paths.cpu().numpy()
        labels = lat.arc_label.cpu().numpy()
        gn = g.cpu().numpy().astype(np.float64)
        ref_arc = np.zeros(lat.total_arcs)
        ref_th = np.zeros((len(lats), V))
        for b in range(len(lats)):
            for j in range(n[b]):
                p = arcs[b, j, :lens[b, j]]
                np.add.at(ref_arc, p, gn[b, j])
                np.add.at(ref_th[b], labels[p], gn[b, j])
        assert np.max(np.abs(asc.grad.cpu().numpy() - ref_arc)) <= 1e-4
        ref_th = ref_th if per_lattice else ref_th.sum(axis=0)
        assert np.max(np.abs(theta.grad.cpu().numpy() - ref_th)) <= 1e-4


def test_gradient_is_the_finite_difference(dev):
    """d best[j] / d arc_scores[a] = [a on path j], checked by central differences on a lattice whose top k + 1 scores
    are separated by more than the step can move them."""
    k, h = 4, 1e-2
    for seed in range(40):
        l = synth.layered_lattice(100 + seed, n_states=14, avg_degree=2.5, vocab=V, width=3, span=2)
        theta_np = synth.label_scores(seed, V, std=1.5)
        th, e = R.arc_terms(l, theta_np)
        ref = R.k_best(l.n_rows, l.src, l.dst, th, e, k + 1, l.n_rows - 1)
        if ref["n_paths"] == k + 1 and np.min(-np.diff(ref["best"].astype(np.float64))) > 40 * h:
            break
    else:
        pytest.fail("no lattice with separated top scores")
    lat = LatticeBatch.from_synth([l], device=dev)
    theta = torch.from_numpy(theta_np).to(dev)
    asc = torch.zeros(lat.total_arcs, device=dev, requires_grad=True)
    r = ops.k_best(lat, theta, k, arc_scores=asc)
    for j in range(k):
        (gr,) = torch.autograd.grad(r.best[0, j], asc, retain_graph=True)
        for a in range(l.n_arcs):
            d = torch.zeros(lat.total_arcs, device=dev)
            d[a] = h
            up = ops.k_best(lat, theta, k, arc_scores=d).best[0, j]
            dn = ops.k_best(lat, theta, k, arc_scores=-d).best[0, j]
            fd = float(up - dn) / (2 * h)
            assert abs(fd - float(gr[a])) <= 1e-2, (j, a, fd, float(gr[a]))


# ----------------------------------------------------------------------------- launches, errors, entry points
def test_repeated_launches_are_bit_identical(dev):
    lats = _mixed_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = torch.from_numpy(synth.label_scores(2, V)).to(dev)
    asc = torch.linspace(-1, 1, lat.total_arcs, device=dev)
    r1, r2 = ops.k_best(lat, theta, 20, arc_scores=asc), ops.k_best(lat, theta, 20, arc_scores=asc)
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)


def test_max_len_too_small_raises_length(dev):
    lat = LatticeBatch.from_synth(_mixed_batch(), device=dev)
    theta = torch.from_numpy(synth.label_scores(2, V)).to(dev)
    with pytest.raises(_lib.NfstError) as e:
        ops.k_best(lat, theta, 5, max_len=3)
    assert e.value.code == _lib.ERR_LENGTH
    with pytest.raises(ValueError):
        ops.k_best(lat, theta, 0)
    with pytest.raises(ValueError):
        ops.k_best(lat, theta, 65)


def test_lattice_scorer_k_best(dev):
    lats = _mixed_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = synth.label_scores(6, V)
    sc = LatticeScorer(V, pad=PAD, bos=BOS, eos=EOS, theta=torch.from_numpy(theta)).to(dev)
    sc.set_lattice(lat)
    r1 = sc.k_best(5)
    r2 = ops.k_best(lat, torch.from_numpy(theta).to(dev), 5)
    for x, y in zip(r1, r2):
        assert torch.equal(x.detach(), y.detach())
    r1.best[torch.isfinite(r1.best)].sum().backward()
    assert sc.theta.grad is not None and float(sc.theta.grad.sum()) > 0


def test_joint_prob_nbest_from_npz(dev, tmp_path):
    V2 = 48
    l = synth.edit_lattice([10, 11, 12, 13], [20, 21, 22], vocab=V2, seed=3)
    theta = synth.label_scores(4, V2)
    em, tr = l.dense()
    path = os.path.join(tmp_path, "x.npz")
    io.save_fsa_npz(path, (em, tr), (em, tr), gs=[1, 2], ps=[3])
    for exact in (True, False):
        jp = JointProb(V2, pad=PAD, bos=BOS, eos=EOS, k=8, theta=torch.from_numpy(theta), exact=exact).to(dev)
        nb = jp.nbest_from_npz(path, 10)
        ref = ops.k_best(jp.tilde_p._lat(), torch.from_numpy(theta).to(dev), 10)
        n = int(ref.n_paths[0])
        assert len(nb) == n == 10
        o = O.forward_backward(l.n_rows, l.src, l.dst, theta[l.label].astype(np.float64))
        for j, (lp, mark) in enumerate(nb):
            m = int(ref.lengths[0, j])
            assert torch.equal(mark.cpu(), ref.paths[0, j, 1:max(m, 2)].cpu().to(torch.int64))
            assert abs(lp - (float(ref.best[0, j]) - o["logZ"])) <= 1e-5
        assert all(nb[j][0] >= nb[j + 1][0] for j in range(n - 1))
    jp = JointProb(V2, pad=PAD, bos=BOS, eos=EOS, k=8, theta=torch.from_numpy(theta)).to(dev)
    _, mark = jp.decode_from_npz(path, V2, PAD)
    assert torch.equal(jp.nbest_from_npz(path, 3)[0][1].cpu(), mark.cpu())

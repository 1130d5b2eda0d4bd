"""ops.k_best (nfst_kbest: the exact k best paths of every lattice) against the float32 NumPy reference of
tests/kbest_ref.py, bit for bit; entry 0 against ops.viterbi; scores against ops.score_paths; gradients; the
LatticeScorer and JointProb entry points.

The edge cases (exact ties across the carry lane, labels at -inf, lattices without a finite path, LDS above 64 KiB, more
lattices than compute units) take their inputs from tests/edge_cases.py; tests/test_kbest_cpu.py proves on the reference
alone that those inputs are what the cases need."""
import os

import numpy as np
import pytest
import torch

from nfst_amd import _lib, io, ops, synth
from nfst_amd.joint import JointProb
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from oracle import oracle as O
from tests import edge_cases as E
from tests import kbest_ref as R

pytestmark = pytest.mark.gpu
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
V = 64
KS = (1, 2, 7, 20, 64)


_mixed_batch, _weighted_batch, _star = E.mixed_batch, E.weighted_batch, E.star  # (one definition: tests/edge_cases.py)


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


# ============================================================================= the edges (inputs: tests/edge_cases.py)
def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _run_all_k_general(tag, lat, lats, theta_np, dev, asc_np=None, ks=KS):
    """Every k of ``ks`` against the reference, bit for bit, with entry 0 held to Viterbi's general kernel (``tw=0``: the
    adds of nfst_kbest) bit for bit and the scores to ops.score_paths at k = 7 and 64.  Returns (references, results
    by k)."""
    with np.errstate(invalid="ignore"):  # (+inf + -inf in the reference: no candidate)
        refs = _refs(lat, lats, theta_np, asc_np)
    theta, asc = _t(theta_np, dev), _t(asc_np, dev)
    with _lib.tuning(tw=0):
        v = ops.viterbi(lat, theta, arc_scores=asc, pad=PAD)
    out = {}
    for k in ks:
        r = ops.k_best(lat, theta, k, arc_scores=asc, pad=PAD)
        _check(tag, lat, lats, r, refs, k)
        _check_viterbi(lat, r, v)
        if k in (7, 64):
            _check_scores(lat, theta, r, asc)
        out[k] = r
    return refs, out


# ----------------------------------------------------------------------------- B1: exact ties
@pytest.mark.parametrize("name", ["star", "star wide", "star one slot", "funnel", "grid", "grid extras"])
def test_exact_ties(dev, name):
    """Scores on a grid of 0.25: whole paths tie, and the order (score desc, arc asc, rank asc) decides every entry --
    within a chunk of 64 lanes, between the carry list in lane 63 and the later chunks of a state with 200 out-arcs, and
    where the list is cut at k.  The packing of the tile programs must not matter: k-best reads the canonical arcs."""
    lats, theta, asc, opts = E.tie_cases()[name]
    lat = LatticeBatch.from_synth(lats, device=dev, **opts)
    refs, _ = _run_all_k_general(f"ties {name}", lat, lats, theta, dev, asc)
    for ref in refs:
        assert E.tied_entries(ref) >= 2
    if name.startswith("star"):  # all 200 paths score -1.0: the top 64 are the star's out-arcs 1 .. 64 in order
        assert np.all(refs[0]["best"] == np.float32(-1.0))
        assert [p[1] for p in refs[0]["arcs"]] == list(range(1, 65))
    if name == "funnel":  # the tied top 64 take arcs from more than one chunk of each of the two heavy states
        for pos in (1, 3):
            assert len({E.sweep_chunk(lats[0], p[pos]) for p in refs[0]["arcs"]}) >= 2


# ----------------------------------------------------------------------------- B2: labels at -inf
@pytest.mark.parametrize("with_arc_scores", [False, True])
def test_labels_at_minus_infinity(dev, with_arc_scores):
    """Six labels at -inf (over 120 dead arcs per lattice): states whose whole list is empty, no dead label on any
    returned path; with arc scores, one of +inf on a dead arc of every lattice: +inf + -inf = NaN is no candidate."""
    lats = E.weighted_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = E.dead_label_theta()
    asc = None
    if with_arc_scores:
        asc = np.random.default_rng(0).normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32)
        for b, l in enumerate(lats):
            asc[int(lat.arc_off[b]) + E.reachable_dead_arc(l)] = np.inf
    refs, out = _run_all_k_general("dead labels", lat, lats, theta, dev, asc)
    paths, lens = out[64].paths.cpu().numpy(), out[64].lengths.cpu().numpy()
    for b, l in enumerate(lats):
        assert np.isin(l.label, E.DEAD).sum() > 120 and refs[b]["n_paths"] == 64
        for j in range(64):
            assert not np.isin(paths[b, j, :lens[b, j]], E.DEAD).any()


def test_fewer_finite_paths_than_k(dev):
    """Dead labels leave one lattice of the mixed batch 14 finite paths: 0 < n_paths < k at k = 20 and 64, and the
    padding convention (best = -inf, length 0, pad, -1) holds on a real lattice."""
    lats, theta, b, n = E.few_paths_case()
    assert 0 < n < 20 and n == 14
    lat = LatticeBatch.from_synth(lats, device=dev)
    refs, out = _run_all_k_general("few paths", lat, lats, theta, dev)
    assert refs[b]["n_paths"] == n
    for k in (20, 64):
        assert int(out[k].n_paths[b]) == n
        assert bool(torch.isneginf(out[k].best[b, n:]).all()) and bool((out[k].lengths[b, n:] == 0).all())


# ----------------------------------------------------------------------------- B3: no finite path
@pytest.mark.parametrize("weighted", [False, True])
def test_lattices_without_a_finite_path(dev, weighted):
    lats, theta = E.no_path_case(weighted)
    lat = LatticeBatch.from_synth(lats, device=dev)
    asc = np.random.default_rng(13).normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32) if weighted else None
    refs, out = _run_all_k_general("no finite path", lat, lats, theta, dev, asc, ks=(1, 7, 64))
    assert [r["n_paths"] == 0 for r in refs] == [False, True, False, True, False]
    for k, r in out.items():
        for b in (1, 3):
            assert int(r.n_paths[b]) == 0 and bool(torch.isneginf(r.best[b]).all()) and bool((r.lengths[b] == 0).all())
            assert bool((r.paths[b] == PAD).all()) and bool((r.arcs[b] == -1).all())


# ----------------------------------------------------------------------------- B4: LDS above 64 KiB
def test_large_lattice_beside_a_small_one(dev):
    """8151 rows: k_kbest_levels takes 12 bytes of dynamic LDS per row and k_kbest_sweep 8 bytes per row + 16 KiB,
    both above the 64 KiB a kernel gets without asking."""
    lats = E.large_pair(8150)
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert int(lat.max_rows) * 12 + 16 > 64 * 1024 and 16 * 1024 + (2 * int(lat.max_rows) + 1) * 4 > 64 * 1024
    theta = synth.label_scores(6, 64)
    asc = np.random.default_rng(5).normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32)
    _run_all_k_general("large", lat, lats, theta, dev, asc, ks=(1, 64))  # (scores against ops.score_paths at k = 64)


# ----------------------------------------------------------------------------- B5: more lattices than compute units
def test_more_lattices_than_compute_units(dev):
    lats, theta, asc = E.many_small()
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert lat.n_lattices == 330
    _run_all_k_general("330 lattices", lat, lats, theta, dev, asc, ks=(1, 20))

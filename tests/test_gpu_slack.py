"""ops.arc_slack (nfst_arc_slack: exact arc slack and beam masks) against the float32 NumPy restatement of
tests/slack_ref.py, bit for bit, under every packing; against ops.k_best and ops.viterbi; ops.prune /
LatticeBatch.restrict against the filtered arc lists, the oracle's log Z and k_best with the dropped arcs at -inf."""
import numpy as np
import pytest
import torch

from nfst_amd import ops, synth
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from oracle import oracle as O
from tests import kbest_ref as K
from tests import slack_ref as R
from tests.edge_cases import STAR_PACKINGS

pytestmark = pytest.mark.gpu
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
V = 64
INF = float("inf")
BEAMS = (0.0, 0.5, 3.0, INF)


def _mixed_batch():  # (the six-lattice mixed batch of test_gpu_kbest.py)
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


def _star():  # state 1 has 200 out-arcs, state 202 has 200 in-arcs: carry pieces and tree-combine rows in both programs
    src = [0] + [1] * 200 + list(range(2, 202)) + [202]
    lab = [BOS] + list(range(3, 203)) + [5] * 200 + [EOS]
    dst = [1] + list(range(2, 202)) + [202] * 200 + [203]
    return synth._finish(204, 256, src, lab, dst)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _beam_tensor(B, dev):
    return torch.tensor([BEAMS[b % len(BEAMS)] for b in range(B)], dtype=torch.float32, device=dev)


def _check(tag, lat, lats, theta_np, dev, asc_np=None):
    """Every output of ops.arc_slack has the reference's bits (per-lattice beams 0, 0.5, 3, inf taking turns)."""
    theta = torch.from_numpy(theta_np).to(dev)
    asc = None if asc_np is None else torch.from_numpy(asc_np).to(dev)
    beam = _beam_tensor(lat.n_lattices, dev)
    r = ops.arc_slack(lat, theta, arc_scores=asc, beam=beam, want_rows=True)
    assert r.keep.dtype == torch.bool and r.n_kept.dtype == torch.int32
    best, slack, keep, n_kept = r.best.cpu().numpy(), r.slack.cpu().numpy(), r.keep.cpu().numpy(), r.n_kept.cpu().numpy()
    vbeta, sslack = r.vbeta.cpu().numpy(), r.state_slack.cpu().numpy()
    refs = []
    for b, l in enumerate(lats):
        a0, r0 = int(lat.arc_off[b]), int(lat.row_off[b])
        assert lat.n_arcs[b] == l.n_arcs and lat.n_rows[b] == l.n_rows
        th_b = theta_np[b] if theta_np.ndim == 2 else theta_np
        ref = R.arc_slack(l, th_b, None if asc_np is None else asc_np[a0:a0 + l.n_arcs], beam=BEAMS[b % len(BEAMS)])
        refs.append(ref)
        assert _bits(best[b:b + 1])[0] == _bits([ref["best"]])[0], (tag, b)
        assert np.array_equal(_bits(slack[a0:a0 + l.n_arcs]), _bits(ref["slack"])), (tag, b)
        assert np.array_equal(_bits(vbeta[r0:r0 + l.n_rows]), _bits(ref["vbeta"])), (tag, b)
        assert np.array_equal(_bits(sslack[r0:r0 + l.n_rows]), _bits(ref["state_slack"])), (tag, b)
        assert np.array_equal(keep[a0:a0 + l.n_arcs], ref["keep"]), (tag, b)
        assert n_kept[b] == ref["n_kept"], (tag, b)
        assert R.is_trim(l, keep[a0:a0 + l.n_arcs]), (tag, b)
    # without a beam: the same slack, no mask
    r2 = ops.arc_slack(lat, theta, arc_scores=asc)
    assert r2.keep is None and r2.n_kept is None and r2.vbeta is None and r2.state_slack is None
    assert torch.equal(r2.slack, r.slack) and torch.equal(r2.best, r.best)
    return r, refs


# ----------------------------------------------------------------------------- bits against the reference
def test_mixed_batch(dev):
    lats = _mixed_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    _check("mixed", lat, lats, synth.label_scores(8, V), dev)


@pytest.mark.parametrize("with_arc_scores", [False, True])
def test_weighted_batch(dev, with_arc_scores):
    lats = _weighted_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert lat.weighted == 1
    rng = np.random.default_rng(0)
    theta = rng.normal(-2.0, 0.7, size=48).astype(np.float32)
    asc = rng.normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32) if with_arc_scores else None
    _check("weighted", lat, lats, theta, dev, asc)


def test_per_lattice_theta(dev):
    lats = _mixed_batch()[:5]
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = np.stack([synth.label_scores(20 + b, V) for b in range(len(lats))])
    _check("per-lattice", lat, lats, theta, dev)


STAR_OPTS = STAR_PACKINGS  # (the ten packings are data: tests/edge_cases.py; other GPU modules import the name from here)


@pytest.mark.parametrize("opts", STAR_OPTS)
def test_star_under_every_packing(dev, opts):
    star = _star()
    theta = synth.label_scores(4, 256)
    lat = LatticeBatch.from_synth([star, star, star, star], device=dev, **opts)  # (one lattice per beam)
    _check(f"star {opts}", lat, [star] * 4, theta, dev)


def test_baseline_batch_subset(dev):  # (funnel states summed as trees)
    lats = synth.bench_batch(8)
    lat = LatticeBatch.from_synth(lats, device=dev)
    _check("baseline", lat, lats, synth.label_scores(1, 256), dev)


def test_snips_shaped_batch_ignores_chunked_programs(dev):
    V2 = 250
    lats = synth.snips_shaped_batch(16, vocab=V2)
    theta_np = synth.label_scores(64, V2, mean=-1.5, std=0.8)
    plain = LatticeBatch.from_synth(lats, device=dev)
    assert plain.max_tiles > 192
    host = LatticeBatch.from_synth(lats)
    assert host.build_chunks(force=True)
    chunked = host.to(dev)
    assert chunked.chunks is not None
    r1, _ = _check("snips", plain, lats, theta_np, dev)
    theta, beam = torch.from_numpy(theta_np).to(dev), _beam_tensor(16, dev)
    r2 = ops.arc_slack(chunked, theta, beam=beam, want_rows=True)
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)


def _neg_inf_case():
    """A lattice and a theta with five labels at -inf whose best path is still finite, by the reference."""
    for seed in range(40):
        l = synth.layered_lattice(700 + seed, n_states=120, avg_degree=5.0, vocab=V, width=6, span=3)
        rng = np.random.default_rng(seed)
        theta = synth.label_scores(seed, V)
        theta[rng.choice(np.arange(3, V), size=5, replace=False)] = -np.inf
        ref = R.arc_slack(l, theta)
        if ref["best"] > -np.inf and np.isinf(ref["slack"]).any():
            return l, theta
    raise AssertionError("no lattice with a finite best path under five -inf labels")


def test_neg_inf_labels(dev):
    l, theta = _neg_inf_case()
    lats = [l] * 4
    lat = LatticeBatch.from_synth(lats, device=dev)
    r, refs = _check("-inf labels", lat, lats, theta, dev)
    assert bool(torch.isinf(r.slack).any()) and bool(torch.isfinite(r.best).all())
    assert not bool(r.keep[torch.isinf(r.slack)].any())  # (also under beam inf)


def test_lattice_without_a_finite_path(dev):
    l = synth._finish(3, V, [0, 1], [BOS, 7], [1, 2])  # one path: bos, 7, (eos is the sink's loop)
    theta = synth.label_scores(3, V)
    theta[7] = -np.inf
    lats = [l] * 4
    lat = LatticeBatch.from_synth(lats, device=dev)
    r, _ = _check("no path", lat, lats, theta, dev)
    assert bool((r.best == -INF).all()) and bool((r.slack == INF).all()) and bool((r.n_kept == 0).all())
    assert bool((r.vbeta == -INF).all()) and bool((r.state_slack == INF).all())
    with pytest.raises(ValueError, match="lattice 0"):
        ops.prune(lat, torch.from_numpy(theta).to(dev), INF)


# ----------------------------------------------------------------------------- against the existing ops
def _on_path_slack(r, arcs):
    a = arcs.reshape(arcs.shape[0], -1).to(torch.int64)
    return r.slack[a[a >= 0]]


@pytest.mark.parametrize("batch", ["mixed", "weighted"])
def test_best_and_zero_slack_agree_with_k_best_and_viterbi(dev, batch):
    lats = _mixed_batch() if batch == "mixed" else _weighted_batch()
    vocab = lats[0].vocab
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = torch.from_numpy(synth.label_scores(2, vocab)).to(dev)
    asc = torch.linspace(-1, 1, lat.total_arcs, device=dev)
    for a in (None, asc):
        r = ops.arc_slack(lat, theta, arc_scores=a, beam=1.0)
        kb = ops.k_best(lat, theta, 1, arc_scores=a)
        assert torch.equal(r.best, kb.best[:, 0])
        on = _on_path_slack(r, kb.arcs)
        assert on.numel() > 0 and bool((on == 0).all())
        assert bool((r.slack >= 0).all())
        again = ops.arc_slack(lat, theta, arc_scores=a, beam=1.0)  # two launches: identical bits
        for x, y in zip(r, again):
            assert (x is None and y is None) or torch.equal(x, y)
    if batch == "mixed":  # without per-arc extras: Viterbi's path and score as well
        r = ops.arc_slack(lat, theta)
        v = ops.viterbi(lat, theta)
        assert torch.equal(r.best, v.best)
        assert bool((_on_path_slack(r, v.arcs) == 0).all())


# ----------------------------------------------------------------------------- prune / restrict
def _same_arrays(x: LatticeBatch, y: LatticeBatch):
    assert x._h == y._h
    for k in LatticeBatch._FIELDS:
        a, b = x._t[k], y._t[k]
        assert (a is None) == (b is None), k
        if a is not None:
            assert a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu()), k


@pytest.mark.parametrize("batch", ["mixed", "weighted"])
@pytest.mark.parametrize("beam", [0.0, 1.0, INF])
def test_prune(dev, batch, beam):
    lats = _mixed_batch() if batch == "mixed" else _weighted_batch()
    vocab = lats[0].vocab
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta_np = synth.label_scores(9, vocab)
    theta = torch.from_numpy(theta_np).to(dev)
    asc_np = np.random.default_rng(1).normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32) if batch == "weighted" else None
    asc = None if asc_np is None else torch.from_numpy(asc_np).to(dev)
    p = ops.prune(lat, theta, beam, arc_scores=asc)
    new, arc_map = p.lat, p.arc_map
    am = arc_map.cpu().numpy()
    assert arc_map.dtype == torch.int64 and np.all(np.diff(am) > 0)
    assert new.total_arcs == len(am) == int(p.n_kept.sum()) and np.array_equal(new.n_arcs, p.n_kept.cpu().numpy())
    assert np.array_equal(new.n_rows, lat.n_rows) and new.vocab == lat.vocab and new.n_lattices == lat.n_lattices
    for k in ("arc_label", "arc_src", "arc_dst") + (("arc_w",) if lat.weighted else ()):
        assert torch.equal(new._t[k], lat._t[k][arc_map]), k
    r = ops.arc_slack(lat, theta, arc_scores=asc, beam=beam)
    assert torch.equal(torch.nonzero(r.keep).reshape(-1), arc_map) and torch.equal(r.best, p.best)
    if beam == INF:  # finite scores: nothing is dropped, and the packer gives the original's arrays bit for bit
        assert len(am) == lat.total_arcs
        _same_arrays(new, lat)
    elif beam == 0.0:
        assert len(am) < lat.total_arcs
    # the device route and the host route give identical arrays
    host, host_map = lat.to("cpu").restrict(r.keep.cpu(), n_kept=p.n_kept)
    assert torch.equal(host_map, arc_map.cpu())
    _same_arrays(new, host)
    # log Z of the pruned batch against the oracle's float64 log Z of the filtered arc list
    new_asc = None if asc is None else asc[arc_map]
    logz = ops.log_z(new, theta, new_asc).cpu().numpy().astype(np.float64)
    keep = r.keep.cpu().numpy()
    for b, l in enumerate(lats):
        a0 = int(lat.arc_off[b])
        kb = keep[a0:a0 + l.n_arcs]
        th, e = K.arc_terms(l, theta_np, None if asc_np is None else asc_np[a0:a0 + l.n_arcs])
        s64 = (th.astype(np.float64) + e.astype(np.float64))[kb]
        o = O.forward_backward(l.n_rows, l.src[kb], l.dst[kb], s64)
        print(f"{batch} beam {beam} lattice {b}: kept {int(kb.sum())} of {l.n_arcs}, |log Z error| {abs(logz[b] - o['logZ']):.3g}")
        assert abs(logz[b] - o["logZ"]) <= 1e-5, (b, logz[b], o["logZ"])
    # k best of the pruned batch = k best of the original with the dropped arcs at -inf
    base = torch.zeros(lat.total_arcs, device=dev) if asc is None else asc
    masked = torch.where(r.keep, base, torch.full_like(base, -INF))
    T = int(lat.depth.max()) + 1
    k0 = ops.k_best(lat, theta, 20, arc_scores=masked, max_len=T)
    k1 = ops.k_best(new, theta, 20, arc_scores=masked[arc_map], max_len=T)
    assert torch.equal(k0.best, k1.best) and torch.equal(k0.paths, k1.paths)
    assert torch.equal(k0.lengths, k1.lengths) and torch.equal(k0.n_paths, k1.n_paths)
    mapped = torch.where(k1.arcs >= 0, arc_map[k1.arcs.clamp(min=0).to(torch.int64)].to(torch.int32), k1.arcs)
    assert torch.equal(mapped, k0.arcs)


def test_prune_passes_pack_options_and_chunks(dev):
    lats = synth.snips_shaped_batch(4, vocab=250)
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = torch.from_numpy(synth.label_scores(64, 250, mean=-1.5, std=0.8)).to(dev)
    p = ops.prune(lat, theta, 2.0, chunks="force", group_mode=1)
    assert p.lat.chunks is not None
    q = ops.prune(lat, theta, 2.0, group_mode=1)
    assert q.lat.chunks is None
    _same_arrays(p.lat, q.lat)
    assert bool(torch.isfinite(ops.log_z(p.lat, theta)).all())
    assert torch.allclose(ops.log_z(p.lat, theta), ops.log_z(q.lat, theta), rtol=0, atol=1e-5)


def test_gradient_flows_through_arc_map(dev):
    lats = _mixed_batch()[:4]
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = torch.from_numpy(synth.label_scores(5, V)).to(dev)
    asc = torch.zeros(lat.total_arcs, device=dev, requires_grad=True)
    p = ops.prune(lat, theta, 1.0, arc_scores=asc)
    ops.log_z(p.lat, theta, asc[p.arc_map]).sum().backward()
    g = asc.grad
    dropped = torch.ones(lat.total_arcs, dtype=torch.bool, device=dev)
    dropped[p.arc_map] = False
    assert bool((g[dropped] == 0).all()) and float(g.sum()) > 0


def test_lattice_scorer_prune(dev):
    lats = _mixed_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = synth.label_scores(6, V)
    sc = LatticeScorer(V, pad=PAD, bos=BOS, eos=EOS, theta=torch.from_numpy(theta)).to(dev)
    sc.set_lattice(lat)
    p1 = sc.prune(1.0)
    p2 = ops.prune(lat, torch.from_numpy(theta).to(dev), 1.0)
    assert torch.equal(p1.arc_map, p2.arc_map) and torch.equal(p1.n_kept, p2.n_kept) and torch.equal(p1.best, p2.best)
    _same_arrays(p1.lat, p2.lat)


# ----------------------------------------------------------------------------- argument checks
def test_bad_beams_raise(dev):
    lat = LatticeBatch.from_synth(_mixed_batch(), device=dev)
    theta = torch.from_numpy(synth.label_scores(2, V)).to(dev)
    for beam in (-0.5, float("nan"), torch.full((6,), -1.0), torch.tensor([0.0, 1.0, float("nan"), 0.0, 0.0, 0.0]),
                 torch.zeros(5), torch.zeros(7, device=dev)):
        with pytest.raises(ValueError):
            ops.arc_slack(lat, theta, beam=beam)
        with pytest.raises(ValueError):
            ops.prune(lat, theta, beam)

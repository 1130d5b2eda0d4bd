"""ops.expectation / ops.entropy / ops.kl_divergence and the double backward of ops.log_z (the first-order expectation
semiring, nfst_expectation) against the float64 reference of tests/expectation_ref.py.

Bounds scale with M_b = sum_a p_a |v_a|, the expected absolute path value of lattice b: |dE[V]| and every |dc_a| within
1e-5 max(1, M_b), per-label sums within 1e-5 max(1, M_b) n_l (n_l: arcs with label l in the lattice)."""
import os

import numpy as np
import pytest
import torch

from nfst_amd import ops, synth
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from tests import expectation_ref as X

pytestmark = pytest.mark.gpu
TOL = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
V = 64


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


def _scores(l, theta_b, asc=None):
    s = theta_b[l.label].astype(np.float64)
    if l.weight is not None:
        s = s + l.weight.astype(np.float64)
    if asc is not None:
        s = s + asc.astype(np.float64)
    return s


def _ref(l, theta_b, asc=None, lv_b=None, av=None, coef=0.0):
    """float64 reference for lattice l with the float32 rounding of v_a the engine applies."""
    s = _scores(l, theta_b, asc)
    v = np.zeros(l.n_arcs)
    if lv_b is not None:
        v = v + lv_b[l.label].astype(np.float64)
    if av is not None:
        v = v + av.astype(np.float64)
    v = (v + coef * s).astype(np.float32).astype(np.float64)
    e = X.expectation(l.n_rows, l.src, l.dst, s, v)
    e["M"] = float(np.sum(e["posterior"] * np.abs(v)))
    e["v"] = v
    return e


def _check(tag, l, b, lat, e, ev=None, cov=None, label_cov=None, label_post=None, post=None):
    a0 = int(lat.arc_off[b])
    sc = max(1.0, e["M"])
    n_l = np.maximum(1, np.bincount(l.label, minlength=lat.vocab))
    if ev is not None:
        assert abs(float(ev[b]) - e["ev"]) <= TOL * sc, (tag, b, float(ev[b]), e["ev"])
    if cov is not None:
        err = np.max(np.abs(cov[a0:a0 + l.n_arcs].astype(np.float64) - e["cov"]))
        assert err <= TOL * sc, (tag, b, err, sc)
    if post is not None:
        assert np.max(np.abs(post[a0:a0 + l.n_arcs] - e["posterior"])) <= 2e-6, (tag, b)
    if label_cov is not None:
        ref = X.label_sums(l.label, e["cov"], lat.vocab)
        assert np.all(np.abs(label_cov[b] - ref) <= TOL * sc * n_l), (tag, b)
    if label_post is not None:
        ref = X.label_sums(l.label, e["posterior"], lat.vocab)
        assert np.all(np.abs(label_post[b] - ref) <= TOL * n_l), (tag, b)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


# ----------------------------------------------------------------------------- the raw launch
@pytest.mark.parametrize("which", ["label", "arc", "coef", "all"])
def test_expectation_terms_mixed_batch(dev, which):
    lats = _mixed_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    rng = np.random.default_rng(1)
    theta = synth.label_scores(7, V)
    lv = rng.normal(0.0, 1.5, size=(len(lats), V)).astype(np.float32) if which in ("label", "all") else None
    av = rng.normal(0.0, 1.0, size=lat.total_arcs).astype(np.float32) if which in ("arc", "all") else None
    coef = 1.0 if which == "coef" else (0.5 if which == "all" else 0.0)
    t = lambda x: None if x is None else torch.from_numpy(x).to(dev)
    r = ops.expectation_terms(lat, t(theta), None, t(lv), t(av), coef, want_posterior=True, want_cov=True,
                              want_label_cov=True, want_label_post=True)
    ev, cov, lc, lp, post = _np(r.ev64), _np(r.cov), _np(r.label_cov), _np(r.label_post), _np(r.posterior)
    for b, l in enumerate(lats):
        a0 = int(lat.arc_off[b])
        e = _ref(l, theta, None, None if lv is None else lv[b], None if av is None else av[a0:a0 + l.n_arcs], coef)
        assert abs(float(r.logz64[b]) - e["logZ"]) <= TOL
        _check(which, l, b, lat, e, ev=ev, cov=cov, label_cov=lc, label_post=lp, post=post)
        assert abs(float(r.ev[b]) - e["ev"]) <= TOL * max(1.0, e["M"])


def test_expectation_weighted_tables_and_arc_scores(dev):
    lats = _weighted_batch()
    em, tr = synth.collate_dense([l.dense(weighted=True) for l in lats])
    lat = LatticeBatch.from_dense(em, tr, device=dev)
    assert lat.weighted == 1
    rng = np.random.default_rng(0)
    theta = rng.normal(-2.0, 0.7, size=(len(lats), 48)).astype(np.float32)
    asc = rng.normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32)
    lv = rng.normal(0.0, 1.0, size=48).astype(np.float32)  # one [V] table for the batch
    av = rng.normal(0.0, 1.0, size=lat.total_arcs).astype(np.float32)
    t = lambda x: torch.from_numpy(x).to(dev)
    r = ops.expectation_terms(lat, t(theta), t(asc), t(lv), t(av), 0.25, want_cov=True, want_label_cov=True,
                              want_label_post=True)
    for b, l in enumerate(lats):
        a0 = int(lat.arc_off[b])
        sl = slice(a0, a0 + l.n_arcs)
        e = _ref(l, theta[b], asc[sl], lv, av[sl], 0.25)
        assert abs(float(r.logz64[b]) - e["logZ"]) <= TOL
        _check("weighted", l, b, lat, e, ev=_np(r.ev64), cov=_np(r.cov), label_cov=_np(r.label_cov),
               label_post=_np(r.label_post))


def test_expectation_gradients(dev):
    """ops.expectation: d/d arc_scores = (c + k p) g, d/d theta its per-label sums, d/d arc_values = p g,
    d/d label_values = per-label sums of p g."""
    lats = _mixed_batch()[:4]
    lat = LatticeBatch.from_synth(lats, device=dev)
    rng = np.random.default_rng(5)
    k = 0.5
    theta = torch.from_numpy(synth.label_scores(3, V)).to(dev).requires_grad_()
    asc = torch.from_numpy(rng.normal(0, 0.3, size=lat.total_arcs).astype(np.float32)).to(dev).requires_grad_()
    lv = torch.from_numpy(rng.normal(0, 1, size=(len(lats), V)).astype(np.float32)).to(dev).requires_grad_()
    av = torch.from_numpy(rng.normal(0, 1, size=lat.total_arcs).astype(np.float32)).to(dev).requires_grad_()
    g = torch.from_numpy(rng.normal(0, 1, size=len(lats)).astype(np.float32)).to(dev)
    ev = ops.expectation(lat, theta, asc, lv, av, score_coef=k)
    d_th, d_as, d_lv, d_av = torch.autograd.grad(ev, (theta, asc, lv, av), g)
    d_th, d_as, d_lv, d_av, gn = _np(d_th), _np(d_as), _np(d_lv), _np(d_av), _np(g)
    ref_th = np.zeros(V)
    for b, l in enumerate(lats):
        a0 = int(lat.arc_off[b])
        sl = slice(a0, a0 + l.n_arcs)
        e = _ref(l, _np(theta), _np(asc)[sl], _np(lv)[b], _np(av)[sl], k)
        sc = max(1.0, e["M"]) * max(1.0, abs(gn[b]))
        assert abs(float(ev[b]) - e["ev"]) <= TOL * max(1.0, e["M"])
        assert np.max(np.abs(d_as[sl] - (e["cov"] + k * e["posterior"]) * gn[b])) <= TOL * sc
        assert np.max(np.abs(d_av[sl] - e["posterior"] * gn[b])) <= 2e-6 * max(1.0, abs(gn[b]))
        n_l = np.maximum(1, np.bincount(l.label, minlength=V))
        assert np.all(np.abs(d_lv[b] - X.label_sums(l.label, e["posterior"], V) * gn[b]) <= TOL * n_l * max(1.0, abs(gn[b])))
        ref_th += X.label_sums(l.label, e["cov"] + k * e["posterior"], V) * gn[b]
    assert np.max(np.abs(d_th - ref_th)) <= TOL * 10 * max(1.0, np.max(np.abs(ref_th)))


# ----------------------------------------------------------------------------- entropy
@pytest.mark.parametrize("per_lattice", [False, True])
def test_entropy_value_and_gradients(dev, per_lattice):
    lats = _weighted_batch()
    em, tr = synth.collate_dense([l.dense(weighted=True) for l in lats])
    lat = LatticeBatch.from_dense(em, tr, device=dev)
    rng = np.random.default_rng(2)
    th = rng.normal(-1.5, 0.7, size=(len(lats), 48) if per_lattice else 48).astype(np.float32)
    asc = rng.normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32)
    theta = torch.from_numpy(th).to(dev).requires_grad_()
    a = torch.from_numpy(asc).to(dev).requires_grad_()
    H = ops.entropy(lat, theta, a)
    d_th, d_as = torch.autograd.grad(H.sum(), (theta, a))
    d_th, d_as = _np(d_th), _np(d_as)
    ref_th = np.zeros_like(th, dtype=np.float64)
    for b, l in enumerate(lats):
        a0 = int(lat.arc_off[b])
        sl = slice(a0, a0 + l.n_arcs)
        tb = th[b] if per_lattice else th
        e = _ref(l, tb, asc[sl], coef=1.0)
        sc = max(1.0, e["M"])
        assert abs(float(H[b]) - (e["logZ"] - e["ev"])) <= TOL * sc
        assert np.max(np.abs(d_as[sl] + e["cov"])) <= TOL * sc
        ls = -X.label_sums(l.label, e["cov"], 48)
        if per_lattice:
            assert np.all(np.abs(d_th[b] - ls) <= TOL * sc * np.maximum(1, np.bincount(l.label, minlength=48)))
        else:
            ref_th += ls
    if not per_lattice:
        assert np.max(np.abs(d_th - ref_th)) <= TOL * 50
    # the scorer method is the same op
    s = LatticeScorer(48, theta=torch.from_numpy(th if not per_lattice else th[0])).to(dev)
    s.set_lattice(lat)
    assert s.entropy().shape == (len(lats),)


def test_entropy_closed_forms(dev):
    """One path: H = 0 with a zero gradient; n equally weighted paths: H = log n."""
    one = synth._finish(4, 16, [0, 1, 2], [3, 4, 5], [1, 2, 3])
    n = 5
    lat_n = synth._finish(n + 2, 16, [0] * n + list(range(1, n + 1)), list(range(3, 3 + n)) + [6] * n,
                          list(range(1, n + 1)) + [n + 1] * n)
    lat = LatticeBatch.from_synth([one, lat_n], device=dev)
    theta = torch.full((16,), -0.4, device=dev, requires_grad=True)
    H = ops.entropy(lat, theta)
    assert abs(float(H[0])) <= 1e-6
    assert abs(float(H[1]) - np.log(n)) <= 1e-6
    (g,) = torch.autograd.grad(H[0], theta)
    assert float(g.abs().max()) <= 1e-6


# ----------------------------------------------------------------------------- KL
def test_kl_of_a_distribution_with_itself_is_zero(dev):
    lats = _mixed_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    th = torch.from_numpy(synth.label_scores(4, V)).to(dev)
    tp, tq = th.clone().requires_grad_(), th.clone().requires_grad_()
    kl = ops.kl_divergence(lat, tp, tq)
    assert float(kl.abs().max()) <= 1e-6
    gp, gq = torch.autograd.grad(kl.sum(), (tp, tq))
    assert float(gp.abs().max()) <= 1e-6 and float(gq.abs().max()) <= 1e-6


def test_kl_value_and_gradients(dev):
    lats = _weighted_batch()
    em, tr = synth.collate_dense([l.dense(weighted=True) for l in lats])
    lat = LatticeBatch.from_dense(em, tr, device=dev)
    rng = np.random.default_rng(9)
    thp = rng.normal(-1.5, 0.6, size=48).astype(np.float32)
    thq = rng.normal(-1.5, 0.6, size=(len(lats), 48)).astype(np.float32)
    asp = rng.normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32)
    asq = rng.normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32)
    ts = [torch.from_numpy(x).to(dev).requires_grad_() for x in (thp, thq, asp, asq)]
    kl = ops.kl_divergence(lat, *ts)
    gp, gq, gap, gaq = [_np(x) for x in torch.autograd.grad(kl.sum(), ts)]
    ref_gp = np.zeros(48)
    for b, l in enumerate(lats):
        a0 = int(lat.arc_off[b])
        sl = slice(a0, a0 + l.n_arcs)
        sp, sq = _scores(l, thp, asp[sl]), _scores(l, thq[b], asq[sl])
        v = (thp[l.label].astype(np.float64) - thq[b][l.label] + asp[sl] - asq[sl])
        ep = X.expectation(l.n_rows, l.src, l.dst, sp, v)
        eq = X.expectation(l.n_rows, l.src, l.dst, sq, np.zeros(l.n_arcs))
        sc = max(1.0, float(np.sum(ep["posterior"] * np.abs(v))))
        assert abs(float(kl[b]) - (eq["logZ"] - ep["logZ"] + ep["ev"])) <= TOL * sc
        assert np.max(np.abs(gap[sl] - ep["cov"])) <= TOL * sc
        assert np.max(np.abs(gaq[sl] - (eq["posterior"] - ep["posterior"]))) <= 4e-6
        n_l = np.maximum(1, np.bincount(l.label, minlength=48))
        assert np.all(np.abs(gq[b] - X.label_sums(l.label, eq["posterior"] - ep["posterior"], 48)) <= TOL * n_l)
        ref_gp += X.label_sums(l.label, ep["cov"], 48)
    assert np.max(np.abs(gp - ref_gp)) <= TOL * 50


# ----------------------------------------------------------------------------- double backward of log_z
def _hvp_case(dev, per_lattice):
    lats = _mixed_batch()[:5]
    lat = LatticeBatch.from_synth(lats, device=dev)
    rng = np.random.default_rng(11)
    th = synth.label_scores(5, V)
    if per_lattice:
        th = np.stack([th + rng.normal(0, 0.2, size=V).astype(np.float32) for _ in lats])
    asc = rng.normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32)
    u_th = rng.normal(0.0, 1.0, size=th.shape).astype(np.float32)
    u_as = rng.normal(0.0, 1.0, size=lat.total_arcs).astype(np.float32)
    return lats, lat, th, asc, u_th, u_as


@pytest.mark.parametrize("per_lattice", [False, True])
def test_log_z_hessian_vector_product(dev, per_lattice):
    lats, lat, th, asc, u_th, u_as = _hvp_case(dev, per_lattice)
    theta = torch.from_numpy(th).to(dev).requires_grad_()
    a = torch.from_numpy(asc).to(dev).requires_grad_()
    z = ops.log_z(lat, theta, a)
    g_th, g_as = torch.autograd.grad(z.sum(), (theta, a), create_graph=True)
    assert g_th.requires_grad and g_as.requires_grad
    dot = (g_th * torch.from_numpy(u_th).to(dev)).sum() + (g_as * torch.from_numpy(u_as).to(dev)).sum()
    h_th, h_as = [_np(x) for x in torch.autograd.grad(dot, (theta, a))]
    ref_th = np.zeros_like(th, dtype=np.float64)
    for b, l in enumerate(lats):
        a0 = int(lat.arc_off[b])
        sl = slice(a0, a0 + l.n_arcs)
        tb = th[b] if per_lattice else th
        e = _ref(l, tb, asc[sl], u_th[b] if per_lattice else u_th, u_as[sl])
        sc = max(1.0, e["M"])
        assert np.max(np.abs(h_as[sl] - e["cov"])) <= TOL * sc, b
        ls = X.label_sums(l.label, e["cov"], V)
        if per_lattice:
            assert np.all(np.abs(h_th[b] - ls) <= TOL * sc * np.maximum(1, np.bincount(l.label, minlength=V)))
        else:
            ref_th += ls
    if not per_lattice:
        assert np.max(np.abs(h_th - ref_th)) <= TOL * 50


def test_log_z_second_derivative_of_a_nonlinear_loss(dev):
    """d/ds [u . d(sum z^2)/ds] = 2 (u . p) p + 2 z c(v = u): the term through the incoming gradient 2 z must be there."""
    lats, lat, th, asc, _, u_as = _hvp_case(dev, False)
    a = torch.from_numpy(asc).to(dev).requires_grad_()
    theta = torch.from_numpy(th).to(dev)
    z = ops.log_z(lat, theta, a)
    (g,) = torch.autograd.grad((z ** 2).sum(), a, create_graph=True)
    (h,) = torch.autograd.grad((g * torch.from_numpy(u_as).to(dev)).sum(), a)
    h = _np(h)
    zz = _np(z).astype(np.float64)
    for b, l in enumerate(lats):
        a0 = int(lat.arc_off[b])
        sl = slice(a0, a0 + l.n_arcs)
        e = _ref(l, th, asc[sl], None, u_as[sl])
        ref = 2.0 * e["ev"] * e["posterior"] + 2.0 * zz[b] * e["cov"]
        sc = max(1.0, e["M"]) * max(1.0, 2 * abs(zz[b]))
        assert np.max(np.abs(h[sl] - ref)) <= TOL * sc, b


def test_log_z_first_order_is_unchanged(dev):
    lats = _mixed_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = torch.from_numpy(synth.label_scores(7, V)).to(dev)
    a = torch.zeros(lat.total_arcs, device=dev, requires_grad=True)
    (g,) = torch.autograd.grad(ops.log_z(lat, theta, a).sum(), a)
    r = ops.forward_backward(lat, theta, arc_scores=a.detach())
    assert torch.equal(g, r.posterior)


# ----------------------------------------------------------------------------- depth, precision, size
def test_deep_chain_and_a_program_beyond_the_precise_threshold(dev):
    d = np.load(os.path.join(GOLDEN, "fuzz_deep_chain.npz"))
    l = synth.SynthLattice(int(d["n_rows"]), int(d["vocab"]), d["src"], d["label"], d["dst"], d["weight"])
    theta, asc = d["theta"], d["arc_scores"]
    lat = LatticeBatch.from_synth([l], device=dev)
    assert int(lat.max_tiles) > 192  # (kPreciseTiles)
    assert int(lat.depth.max()) >= 900
    rng = np.random.default_rng(3)
    lv = rng.normal(0.0, 2.0, size=int(d["vocab"])).astype(np.float32)
    t = lambda x: torch.from_numpy(x).to(dev)
    for coef, lvv in ((1.0, None), (0.0, lv), (0.5, lv)):
        r = ops.expectation_terms(lat, t(theta), t(asc), None if lvv is None else t(lvv), None, coef, want_cov=True,
                                  want_label_cov=True)
        e = _ref(l, theta, asc, lvv, None, coef)
        assert abs(float(r.logz64[0]) - e["logZ"]) <= 1e-8
        _check(f"deep {coef}", l, 0, lat, e, ev=_np(r.ev64), cov=_np(r.cov), label_cov=_np(r.label_cov))


def test_baseline_batch_subset(dev):
    """The BASELINE batch (256 lattices, tree-summed funnel states with carry and combine records); 16 lattices checked."""
    lats = synth.bench_batch(256)
    theta = synth.label_scores(1, 256)
    lat = LatticeBatch.from_synth(lats, device=dev)
    r = ops.expectation_terms(lat, torch.from_numpy(theta).to(dev), score_coef=1.0, want_cov=True, want_label_cov=True)
    ev, cov, lc = _np(r.ev64), _np(r.cov), _np(r.label_cov)
    for b in range(0, 256, 16):
        l = lats[b]
        e = _ref(l, theta, coef=1.0)
        assert abs(float(r.logz64[b]) - e["logZ"]) <= TOL
        _check("baseline", l, b, lat, e, ev=ev, cov=cov, label_cov=lc)


def test_snips_shaped_batch_ignores_chunked_programs(dev):
    V2 = 250
    lats = synth.snips_shaped_batch(16, vocab=V2)
    theta = torch.from_numpy(synth.label_scores(64, V2, mean=-1.5, std=0.8)).to(dev)
    plain = LatticeBatch.from_synth(lats, device=dev)
    host = LatticeBatch.from_synth(lats)
    assert host.build_chunks(force=True)
    chunked = host.to(dev)
    assert chunked.chunks is not None
    r1 = ops.expectation_terms(plain, theta, score_coef=1.0, want_posterior=True, want_cov=True)
    r2 = ops.expectation_terms(chunked, theta, score_coef=1.0, want_posterior=True, want_cov=True)
    for x, y in zip((r1.logz64, r1.ev64, r1.posterior, r1.cov), (r2.logz64, r2.ev64, r2.posterior, r2.cov)):
        assert torch.equal(x, y)
    for b in range(0, 16, 5):
        e = _ref(lats[b], _np(theta), coef=1.0)
        _check("snips", lats[b], b, plain, e, ev=_np(r1.ev64), cov=_np(r1.cov))


def test_repeated_launches_are_bit_identical(dev):
    lats = _mixed_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = torch.from_numpy(synth.label_scores(2, V)).to(dev)
    av = torch.linspace(-1, 1, lat.total_arcs, device=dev)
    kw = dict(arc_values=av, score_coef=1.0, want_posterior=True, want_cov=True, want_label_post=True)
    r1 = ops.expectation_terms(lat, theta, **kw)
    r2 = ops.expectation_terms(lat, theta, **kw)  # (the per-label sums of p too: they are summed exactly)
    for x, y in zip(r1, r2):
        if x is not None:
            assert torch.equal(x, y)


def test_bad_arguments_raise_value_error(dev):
    lats = _mixed_batch()[:2]
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = torch.zeros(V, device=dev)
    with pytest.raises(ValueError):
        ops.expectation(lat, torch.zeros(V + 1, device=dev))
    with pytest.raises(ValueError):
        ops.expectation(lat, theta, label_values=torch.zeros(3, V, device=dev))
    with pytest.raises(ValueError):
        ops.expectation(lat, theta, arc_values=torch.zeros(lat.total_arcs + 1, device=dev))
    with pytest.raises(ValueError):
        ops.expectation(lat, theta, arc_values=torch.zeros(lat.total_arcs))  # on the host
    with pytest.raises(ValueError):
        ops.entropy(lat, torch.zeros(V, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        ops.entropy(lat, theta, arc_scores=torch.zeros(lat.total_arcs, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.kl_divergence(lat, theta, torch.zeros(V))
    with pytest.raises(ValueError):
        ops.expectation(lat, theta, score_coef=float("nan"))

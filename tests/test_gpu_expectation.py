"""ops.expectation / ops.entropy / ops.kl_divergence and the double backward of ops.log_z (the first-order expectation
semiring, nfst_expectation) against the float64 reference of tests/expectation_ref.py.

Bounds scale with M_b = sum_a p_a |v_a|, the expected absolute path value of lattice b: |dE[V]| and every |dc_a| within
1e-5 max(1, M_b), per-label sums within 1e-5 max(1, M_b) n_l (n_l: arcs with label l in the lattice).

The float64 outputs of the raw launch are held as float64 (``_check64``): |logz64 - ref| <= 1e-9 max(1, |ref|) and
|ev64 - ref| <= 1e-9 max(1, M_b).  The kernel's arithmetic is float64 end to end (relative error 2e-16 per exp_split64
and per add, at most about 3e4 arcs per lattice here), so 1e-9 leaves a margin of more than 100 over eps * n_arcs.  The
largest value of every error ratio goes to expectation_errors.json in the directory of run outputs (profiles/README.md).

The edge cases (every packing, 32-bit records, LDS above 64 KiB and the last legal row count, labels at -inf, lattices
without a finite path, large exponents, more lattices than compute units) take their inputs from tests/edge_cases.py;
tests/test_expectation_cpu.py proves on the reference alone that those inputs are what the cases need."""
import functools
import glob
import json
import os

import numpy as np
import pytest
import torch

from nfst_amd import _lib, ops, synth
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from tests import edge_cases as E
from tests import expectation_ref as X
from tests import paths_ref as P
from tests.test_gpu_slack import STAR_OPTS

pytestmark = pytest.mark.gpu
TOL = 1e-5
TOL64 = 1e-9  # the float64 outputs (module docstring)
ERR_LIMIT = -6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
V = 64


_mixed_batch, _weighted_batch = E.mixed_batch, E.weighted_batch  # (one definition: tests/edge_cases.py)


# largest error ratios seen per check (err / scale: the bounds are TOL64, TOL and 2e-6), written at the end of the module
_ERR = {}


def rec(tag, err):
    _ERR[tag] = max(_ERR.get(tag, 0.0), float(err))
    return float(err)


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    # the directory of run outputs at the repository's root, as in test_gpu_paths.py (a run that wants the figures
    # creates it; nothing is written without it)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for out in sorted(glob.glob(os.path.join(root, "*_out"))):
        if _ERR and os.path.isdir(out):
            with open(os.path.join(out, "expectation_errors.json"), "w") as f:
                json.dump(dict(sorted(_ERR.items())), f, indent=1)


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
    with np.errstate(invalid="ignore", over="ignore"):
        v = (v + coef * s).astype(np.float32).astype(np.float64)
    v = np.where(np.isfinite(s), v, 0.0)  # an arc of weight zero has no value (exp_arc_value)
    e = X.expectation(l.n_rows, l.src, l.dst, s, v)
    e["M"] = float(np.sum(e["posterior"] * np.abs(v)))
    e["v"] = v
    return e


def _check(tag, l, b, lat, e, ev=None, cov=None, label_cov=None, label_post=None, post=None):
    a0 = int(lat.arc_off[b])
    sc = max(1.0, e["M"])
    n_l = np.maximum(1, np.bincount(l.label, minlength=lat.vocab))
    name = tag.split(" ")[0]
    if ev is not None:
        rec(f"{name} ev / M", abs(float(ev[b]) - e["ev"]) / sc)
        assert abs(float(ev[b]) - e["ev"]) <= TOL * sc, (tag, b, float(ev[b]), e["ev"])
    if cov is not None:
        err = np.max(np.abs(cov[a0:a0 + l.n_arcs].astype(np.float64) - e["cov"]))
        rec(f"{name} cov / M", err / sc)
        assert err <= TOL * sc, (tag, b, err, sc)
    if post is not None:
        err = np.max(np.abs(post[a0:a0 + l.n_arcs] - e["posterior"]))
        rec(f"{name} posterior", err)
        assert err <= 2e-6, (tag, b, err)
    if label_cov is not None:
        ref = X.label_sums(l.label, e["cov"], lat.vocab)
        rec(f"{name} label_cov / (M n_l)", np.max(np.abs(label_cov[b] - ref) / (sc * n_l)))
        assert np.all(np.abs(label_cov[b] - ref) <= TOL * sc * n_l), (tag, b)
    if label_post is not None:
        ref = X.label_sums(l.label, e["posterior"], lat.vocab)
        rec(f"{name} label_post / n_l", np.max(np.abs(label_post[b] - ref) / n_l))
        assert np.all(np.abs(label_post[b] - ref) <= TOL * n_l), (tag, b)


def _check64(tag, r, b, e):
    """The float64 outputs of the raw launch as float64, and the float32 copy of E[V] at the file's float32 bound."""
    name = tag.split(" ")[0]
    z, ev, ev32 = float(r.logz64[b]), float(r.ev64[b]), float(r.ev[b])
    sc = max(1.0, e["M"])
    if np.isfinite(e["logZ"]):
        err = abs(z - e["logZ"]) / max(1.0, abs(e["logZ"]))
        print(f"{tag} b={b}: |dlogz64| / max(1, |logZ|) = {err:.3e}, |dev64| / max(1, M) = {abs(ev - e['ev']) / sc:.3e}")
        rec(f"{name} logz64 / max(1, |logZ|)", err)
        assert err <= TOL64, (tag, b, z, e["logZ"])
    else:
        assert z == e["logZ"], (tag, b, z, e["logZ"])
    rec(f"{name} ev64 / M", abs(ev - e["ev"]) / sc)
    assert abs(ev - e["ev"]) <= TOL64 * sc, (tag, b, ev, e["ev"], sc)
    assert abs(ev32 - e["ev"]) <= TOL * sc, (tag, b, ev32, e["ev"], sc)


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
        _check64(f"mixed {which}", r, b, e)
        _check("mixed", l, b, lat, e, ev=ev, cov=cov, label_cov=lc, label_post=lp, post=post)


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


# ============================================================================= the edges (inputs: tests/edge_cases.py)
def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _theta_of(theta, b):
    return theta[b] if theta.ndim == 2 else theta


def _run_and_check(tag, dev, lat, lats, theta, asc=None, lv=None, av=None, coef=0.0, every=1, arcs=True):
    """One raw launch with all five optional outputs against the reference, lattice by lattice (every ``every``-th):
    the float64 outputs at TOL64, the float32 ones at the file's bounds.  ``arcs=False``: log Z and E[V] only.
    Returns (the launch's result, the references by lattice index)."""
    r = ops.expectation_terms(lat, _t(theta, dev), _t(asc, dev), _t(lv, dev), _t(av, dev), coef, want_posterior=True,
                              want_cov=True, want_label_cov=True, want_label_post=True)
    out = [_np(x) for x in (r.ev64, r.cov, r.label_cov, r.label_post, r.posterior)]
    for x in [_np(r.logz64), _np(r.ev)] + out:
        assert not np.isnan(x).any(), tag
    refs = {}
    for b in range(0, len(lats), every):
        l = lats[b]
        a0 = int(lat.arc_off[b])
        sl = slice(a0, a0 + l.n_arcs)
        e = _ref(l, _theta_of(theta, b), None if asc is None else asc[sl], None if lv is None else _theta_of(lv, b),
                 None if av is None else av[sl], coef)
        _check64(tag, r, b, e)
        if arcs:
            _check(tag, l, b, lat, e, ev=out[0], cov=out[1], label_cov=out[2], label_post=out[3], post=out[4])
        refs[b] = e
    return r, refs


def _fmt(lat):
    """(format codes, wide bits) of the batch's programs, both directions."""
    w = lat.meta_host[:, [_lib.META_FWD_U, _lib.META_BWD_U]].astype(np.int64)
    return w & 0xff, (w >> 8) & 1


# ----------------------------------------------------------------------------- A1: every packing
@functools.lru_cache(maxsize=None)
def _packings():
    """What the ten packings give on the host (the same packer as on the device path of from_synth): per option the
    (format codes, wide bits, scratch rows)."""
    out = []
    for opts in STAR_OPTS:
        lat = LatticeBatch.from_synth(E.packing_lattices(), **opts)
        codes, wide = _fmt(lat)
        out.append((set(codes.ravel().tolist()), set(wide.ravel().tolist()), int(lat.max_rows) > int(max(lat.n_rows))))
    return out


@pytest.mark.parametrize("i", range(len(STAR_OPTS)), ids=[str(i) for i in range(len(STAR_OPTS))])
def test_every_packing(dev, i):
    """The star, the double funnel and a lattice with states of 40 out-arcs under the ten packings: compact tiles and
    32-bit records with one, two and four slots per lane (the ``j >= U`` select), narrow and wide groups (all six
    stages of the group reduction), tree-summed states with carry and combine records."""
    opts = STAR_OPTS[i]
    lats = E.packing_lattices()
    lat = LatticeBatch.from_synth(lats, device=dev, **opts)
    codes, wide = _fmt(lat)
    # this packing is what its options say ...
    want = opts.get("slots_per_lane", 0)
    want = 8 if want in (0, 4) and not opts.get("no_compact") else want
    assert np.all(codes == want), (opts, codes)
    if opts.get("group_mode") == 2:
        assert np.all(wide == 1)
    if opts.get("group_mode") == 1:
        assert np.all(wide == 0)
    # ... and the ten of them reach every branch of the sweep
    seen = _packings()
    assert seen[i] == (set(codes.ravel().tolist()), set(wide.ravel().tolist()), int(lat.max_rows) > int(max(lat.n_rows)))
    assert set().union(*[s[0] for s in seen]) == {1, 2, 4, 8}
    assert set().union(*[s[1] for s in seen]) == {0, 1}
    assert any(s[2] for s in seen)  # scratch rows: tree-summed states
    rng = np.random.default_rng(40)
    theta = synth.label_scores(4, 256)
    lv = rng.normal(0.0, 1.5, size=(len(lats), 256)).astype(np.float32)
    av = rng.normal(0.0, 1.0, size=lat.total_arcs).astype(np.float32)
    _run_and_check(f"packing {opts}", dev, lat, lats, theta, None, lv, av, 0.5)


# ----------------------------------------------------------------------------- A2: 32-bit records
def test_big_vocabulary_takes_32_bit_records(dev):
    V2 = P.BIG_V
    lats = [synth.layered_lattice(50, n_states=150, avg_degree=4.0, vocab=V2, width=4, span=2),
            synth.layered_lattice(51, n_states=400, avg_degree=6.0, vocab=V2, width=8, span=3)]
    lat = LatticeBatch.from_synth(lats, device=dev)
    codes, _ = _fmt(lat)
    assert np.all(codes != 8), codes  # labels beyond the 11 bits of a compact record
    lv = np.random.default_rng(41).normal(0.0, 1.5, size=V2).astype(np.float32)
    _run_and_check("bigvocab", dev, lat, lats, synth.label_scores(21, V2, mean=-1.0, std=1.0), None, lv, None, 0.0)


# ----------------------------------------------------------------------------- A3: LDS above 64 KiB, the last legal row count
@pytest.mark.parametrize("n_states", [7800, 8150, 8190])
def test_large_lattice_beside_a_small_one(dev, n_states):
    """156 .. 160 KiB of dynamic LDS (20 bytes per row + 16); 8191 rows is the last count that fits 160 KiB.  The small
    neighbour's outputs are the bits of a launch of the neighbour alone (but for label_cov: float64 atomics, whose
    order is free)."""
    lats = E.large_pair(n_states)
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert int(lat.max_rows) == n_states + 1 == int(max(lat.n_rows))  # (no scratch rows)
    assert (20 * int(lat.max_rows) + 16 <= 160 * 1024) and 20 * int(lat.max_rows) + 16 > 64 * 1024
    if n_states == 8190:
        assert int(lat.max_rows) == 8191 and 20 * 8191 + 16 == 160 * 1024 - 4
    rng = np.random.default_rng(42)
    theta = synth.label_scores(6, 64)
    asc = rng.normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32)
    lv = rng.normal(0.0, 1.5, size=64).astype(np.float32)
    r, _ = _run_and_check(f"large {n_states}", dev, lat, lats, theta, asc, lv, None, 0.5)
    a0 = int(lat.arc_off[1])
    alone = LatticeBatch.from_synth(lats[1:], device=dev)
    q = ops.expectation_terms(alone, _t(theta, dev), _t(asc[a0:], dev), _t(lv, dev), None, 0.5, want_posterior=True,
                              want_cov=True, want_label_post=True)
    for x, y in ((r.logz64[1:], q.logz64), (r.ev64[1:], q.ev64), (r.ev[1:], q.ev), (r.posterior[a0:], q.posterior),
                 (r.cov[a0:], q.cov), (r.label_post[1:], q.label_post)):
        assert torch.equal(x, y)


def test_one_row_beyond_lds_is_refused(dev):
    """8192 rows: legal for the packer and for forward_backward (its fused flavour, which keeps 16 bytes per row: more
    lattices than compute units, no per-arc extras), 20 bytes more than 160 KiB of LDS here.  The launcher refuses
    (NFST_ERR_LIMIT, no launch) from every op that rests on it, and the next launch is undisturbed."""
    lats = E.large_pair(8191)
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert int(lat.max_rows) == 8192 and 20 * 8192 + 16 > 160 * 1024
    theta = synth.label_scores(6, 64)
    th = _t(theta, dev)
    with pytest.raises(_lib.NfstError) as err:  # two lattices with table weights: the ring pipeline, no room for four slots
        ops.forward_backward(lat, th)
    assert err.value.code == ERR_LIMIT
    with pytest.raises(_lib.NfstError) as err:
        ops.expectation_terms(lat, th, score_coef=1.0)
    assert err.value.code == ERR_LIMIT
    with pytest.raises(_lib.NfstError) as err:
        ops.entropy(lat, th)
    assert err.value.code == ERR_LIMIT
    # log_z runs on a batch of 8192 rows; its double backward is an expectation launch
    many = E.beyond_lds_batch()
    lat_many = LatticeBatch.from_synth(many, device=dev)
    assert int(lat_many.max_rows) == 8192 and lat_many.n_lattices == 301
    tg = _t(theta, dev).requires_grad_()
    z = ops.log_z(lat_many, tg)
    e = _ref(many[0], theta)
    assert abs(float(z[0]) - e["logZ"]) <= 2e-5 * max(1.0, abs(e["logZ"]))  # (float32: the project's bound on log Z)
    (g,) = torch.autograd.grad(z.sum(), tg, create_graph=True)
    with pytest.raises(_lib.NfstError) as err:
        torch.autograd.grad((g * g).sum(), tg)
    assert err.value.code == ERR_LIMIT
    small = LatticeBatch.from_synth(lats[1:], device=dev)
    _run_and_check("after-refusal", dev, small, lats[1:], theta, None, None, None, 1.0)


# ----------------------------------------------------------------------------- A4: labels at -inf
def _dead_values(lats, lat, with_av):
    """label_values with +inf on a dead label and (with_av) arc_values with NaN on dead arcs only."""
    rng = np.random.default_rng(43)
    lv = rng.normal(0.0, 1.5, size=E.V_WEIGHTED).astype(np.float32)
    lv[E.DEAD[0]] = np.inf
    av = None
    if with_av:
        av = rng.normal(0.0, 1.0, size=lat.total_arcs).astype(np.float32)
        for b, l in enumerate(lats):
            dead = np.nonzero(np.isin(l.label, E.DEAD))[0]
            av[int(lat.arc_off[b]) + dead[::3]] = np.nan
    return lv, av


@pytest.mark.parametrize("with_av", [False, True])
@pytest.mark.parametrize("coef", [1.0, 0.5])
def test_labels_at_minus_infinity(dev, coef, with_av):
    """Six labels at -inf: over 120 arcs of weight zero per lattice.  A dead arc has no value (exp_arc_value): coef * s
    = -inf there, and a label value of +inf or an arc value of NaN on it must not reach any output."""
    lats = E.weighted_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = E.dead_label_theta(shape=(len(lats), E.V_WEIGHTED))
    asc = np.random.default_rng(44).normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32)
    lv, av = _dead_values(lats, lat, with_av)
    r, _ = _run_and_check(f"dead coef={coef} av={with_av}", dev, lat, lats, theta, asc, lv, av, coef)
    post, cov, lc, lp = _np(r.posterior), _np(r.cov), _np(r.label_cov), _np(r.label_post)
    for x in (_np(r.logz64), _np(r.ev64), _np(r.ev), post, cov, lc, lp):
        assert np.isfinite(x).all()
    for b, l in enumerate(lats):
        dead = int(lat.arc_off[b]) + np.nonzero(np.isin(l.label, E.DEAD))[0]
        assert len(dead) > 120
        assert np.all(post[dead] == 0.0) and np.all(cov[dead] == 0.0)
        assert np.all(lc[b, E.DEAD] == 0.0) and np.all(lp[b, E.DEAD] == 0.0)


def test_entropy_with_labels_at_minus_infinity(dev):
    lats = E.weighted_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    th = E.dead_label_theta(shape=(len(lats), E.V_WEIGHTED))
    asc = np.random.default_rng(44).normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32)
    theta, a = _t(th, dev).requires_grad_(), _t(asc, dev).requires_grad_()
    H = ops.entropy(lat, theta, a)
    d_th, d_as = [_np(x) for x in torch.autograd.grad(H.sum(), (theta, a))]
    assert np.isfinite(_np(H)).all() and np.isfinite(d_th).all() and np.isfinite(d_as).all()
    assert np.all(d_th[:, E.DEAD] == 0.0)
    for b, l in enumerate(lats):
        a0 = int(lat.arc_off[b])
        sl = slice(a0, a0 + l.n_arcs)
        e = _ref(l, th[b], asc[sl], coef=1.0)
        sc = max(1.0, e["M"])
        assert rec("dead entropy / M", abs(float(H[b]) - (e["logZ"] - e["ev"])) / sc) <= TOL
        assert rec("dead d_arc / M", np.max(np.abs(d_as[sl] + e["cov"])) / sc) <= TOL
        assert np.all(d_as[sl][np.isin(l.label, E.DEAD)] == 0.0)
        n_l = np.maximum(1, np.bincount(l.label, minlength=E.V_WEIGHTED))
        assert np.all(np.abs(d_th[b] + X.label_sums(l.label, e["cov"], E.V_WEIGHTED)) <= TOL * sc * n_l)


# ----------------------------------------------------------------------------- A5: no finite path
def test_lattices_without_a_finite_path(dev):
    """The convention of include/nfst_hip.h (nfst_expectation): a lattice all of whose paths have weight zero gets
    log Z = -inf, E[V] = 0 and zeros in every per-arc and per-label output; never a NaN; its neighbours in the batch
    are not disturbed.  Its entropy is -inf, with a zero gradient."""
    lats, th = E.no_path_case(True)
    lat = LatticeBatch.from_synth(lats, device=dev)
    rng = np.random.default_rng(45)
    asc = rng.normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32)
    lv = rng.normal(0.0, 1.5, size=th.shape).astype(np.float32)
    av = rng.normal(0.0, 1.0, size=lat.total_arcs).astype(np.float32)
    r, refs = _run_and_check("nopath", dev, lat, lats, th, asc, lv, av, 0.5)  # (all five lattices, NaN checks included)
    assert [bool(np.isneginf(refs[b]["logZ"])) for b in range(5)] == [False, True, False, True, False]
    for b in (1, 3):
        a0 = int(lat.arc_off[b])
        sl = slice(a0, a0 + lats[b].n_arcs)
        assert float(r.logz64[b]) == -np.inf and float(r.ev64[b]) == 0.0 and float(r.ev[b]) == 0.0
        for x in (r.posterior[sl], r.cov[sl], r.label_cov[b], r.label_post[b]):
            assert bool((x == 0.0).all())
    theta, a = _t(th, dev).requires_grad_(), _t(asc, dev).requires_grad_()
    H = ops.entropy(lat, theta, a)
    Hn = _np(H)
    assert np.all(np.isneginf(Hn[[1, 3]])) and np.isfinite(Hn[[0, 2, 4]]).all()
    g = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0], device=dev)
    d_th, d_as = [_np(x) for x in torch.autograd.grad(H, (theta, a), g)]
    assert not np.isnan(d_th).any() and not np.isnan(d_as).any()
    assert np.all(d_th[[1, 3]] == 0.0)
    for b in (0, 2, 4):
        e = _ref(lats[b], th[b], asc[int(lat.arc_off[b]):int(lat.arc_off[b]) + lats[b].n_arcs], coef=1.0)
        assert abs(Hn[b] - (e["logZ"] - e["ev"])) <= TOL * max(1.0, e["M"])


# ----------------------------------------------------------------------------- A6: exponent range and cancellation
@pytest.mark.parametrize("name", E.RANGE_CASES)
def test_exponent_range_and_cancelling_values(dev, name):
    """Path weights around e^+-1e3 (label scores * 30, per-arc scores +-40), e^+-5e4 (* 3000) and e^-4e5 (every label
    shifted by -2e4), with values of +-1e3 whose expectation cancels.  The posteriors have not collapsed to one path:
    asserted on the reference here, proved for these seeds in tests/test_expectation_cpu.py."""
    lats, theta, asc, av = E.range_case(name)
    lat = LatticeBatch.from_synth(lats, device=dev)
    spread = name in E.RANGE_SPREAD
    _, refs = _run_and_check(f"range-{name}", dev, lat, lats, theta, asc, None, av, 0.0, arcs=spread)
    for b, e in refs.items():
        if spread:
            assert int(np.sum((e["posterior"] > 0.01) & (e["posterior"] < 0.99))) >= E.SPREAD_MIN, (name, b)
        assert abs(e["ev"]) <= 0.5 * e["M"], (name, b)  # (the values cancel)
    assert max(abs(e["logZ"]) for e in refs.values()) > E.RANGE_LOGZ[name]


# ----------------------------------------------------------------------------- A7: more lattices than compute units
def test_more_lattices_than_compute_units(dev):
    lats, theta, asc = E.many_small()
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert lat.n_lattices == 330
    lv = np.random.default_rng(46).normal(0.0, 1.5, size=theta.shape).astype(np.float32)
    r, _ = _run_and_check("many", dev, lat, lats, theta, asc, lv, None, 0.0, every=7)
    z = ops.log_z(lat, _t(theta, dev), _t(asc, dev)).double()  # (float32: the project's bound on log Z, 2e-5)
    assert float(torch.max(torch.abs(r.logz64 - z) / torch.clamp(z.abs(), min=1.0))) <= 2e-5

"""nfst_amd.swor (nfst_swor: k distinct paths per lattice drawn without replacement by stochastic beam search) against
the float64 NumPy restatement of tests/swor_ref.py, which is fed the very logbeta / log Z tensors the op consumed.

Lattices whose reference margin exceeds swor_ref.DECIDED are compared as a map from path to (length, marks, arcs, logp,
gumbel), with kappa, n_paths and the output order; tests/test_swor_cpu.py proves on the reference alone that no case
leaves out more than 1 % of its lattices and that the cases are what they claim to be."""
import numpy as np
import pytest
import torch

from nfst_amd import _lib, ops, swor, synth
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from tests import edge_cases as E
from tests import swor_ref as R

pytestmark = pytest.mark.gpu
PAD = synth.PAD
NEG = -np.inf
G_TOL = R.DECIDED / 10
ERRORS = {"gumbel": 0.0}  # the largest |G_gpu - G_ref| over decided lattices seen by this module


def _betas(lat, beta):
    lb, z = beta.logbeta.cpu().numpy(), beta.logz64.cpu().numpy()
    return [(lb[int(lat.row_off[b]):int(lat.row_off[b]) + int(lat.n_rows[b])], float(z[b])) for b in range(lat.n_lattices)]


def _run(case, dev, k, lat=None, u=None, max_len=None, **kw):
    """(lat, result, references): the op on the case's uniforms and the restatement on the op's own beta."""
    lat = lat or LatticeBatch.from_synth(case.lats, device=dev, **case.opts)
    theta = torch.from_numpy(case.theta).to(dev)
    asc = None if case.asc is None else torch.from_numpy(case.asc).to(dev)
    L = max_len or int(lat.depth.max()) + 1
    u = case.uniforms(k, L) if u is None else u
    beta = ops.backward(lat, theta, asc)
    r = swor.sample(lat, theta, k, arc_scores=asc, max_len=L, uniforms=torch.from_numpy(u), pad=PAD, beta=beta, **kw)
    return lat, r, case.references(k, betas=_betas(lat, beta), uniforms=u, max_len=L)


def _np(r):
    return {f: (None if v is None else v.cpu().numpy()) for f, v in r._asdict().items()}


def _check(tag, lat, lats, r, refs, k):
    o = _np(r)
    left_out = 0
    for b, (l, ref) in enumerate(zip(lats, refs)):
        n = int(o["n_paths"][b])
        # the layout holds for every lattice, decided or not
        assert np.all(o["lengths"][b, n:] == 0) and np.all(o["logp"][b, n:] == NEG) and np.all(o["gumbel"][b, n:] == NEG), (tag, b, k)
        for i in range(k):
            m = int(o["lengths"][b, i])
            assert np.all(o["paths"][b, i, m:] == PAD) and np.all(o["arcs"][b, i, m:] == -1), (tag, b, k, i)
        assert np.all(np.diff(o["gumbel"][b, :n]) <= 0), (tag, b, k)
        assert n == 0 or o["gumbel"][b, n - 1] >= o["kappa"][b]
        a0 = int(lat.arc_off[b])
        got = {tuple(o["arcs"][b, i, :o["lengths"][b, i]] - a0): i for i in range(n)}
        assert len(got) == n, (tag, b, k)  # distinct paths
        if not R.decided(ref):
            left_out += 1
            continue
        assert n == ref["n_paths"], (tag, b, k)
        for j, p in enumerate(ref["arcs"]):
            assert tuple(p) in got, (tag, b, k, j)
            i = got[tuple(p)]
            assert i == j, (tag, b, k, j)  # ranked by gumbel as the reference ranks them
            assert np.array_equal(o["paths"][b, i, :len(p)], l.label[p]), (tag, b, k, j)
            assert abs(float(o["logp"][b, i]) - float(ref["logp"][j])) <= 1e-6, (tag, b, k, j)
            err = abs(float(o["gumbel"][b, i]) - float(ref["gumbel"][j]))
            ERRORS["gumbel"] = max(ERRORS["gumbel"], err)
            assert err <= G_TOL, (tag, b, k, j, err)
        if ref["kappa"] == NEG:
            assert o["kappa"][b] == NEG, (tag, b, k)
        else:
            err = abs(float(o["kappa"][b]) - ref["kappa"])
            ERRORS["gumbel"] = max(ERRORS["gumbel"], err)
            assert err <= G_TOL, (tag, b, k, err)
    assert left_out <= R.CAP * len(lats), (tag, k, left_out)
    print(f"{tag} k={k}: largest |G_gpu - G_ref| so far {ERRORS['gumbel']:.3e}")


# ----------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("name", list(R.cases()))
def test_against_the_reference(dev, name):
    """The mixed batch (shared theta, per-lattice theta), the weighted batch (table weights and arc_scores), the star
    beside the lattice whose candidates exceed the LDS cap, labels at -inf, lattices without a finite path, fewer paths
    than k, uniforms on the boundaries, more lattices than compute units."""
    case = R.cases()[name]()
    lat = LatticeBatch.from_synth(case.lats, device=dev, **case.opts)
    for k in case.ks:
        _, r, refs = _run(case, dev, k, lat=lat)
        _check(case.tag, lat, case.lats, r, refs, k)


def test_finished_slots_wait_at_the_sink(dev):
    """The edit lattice's paths differ in length: a slot that reached the sink is carried through the later steps."""
    case = R.cases()["mixed"]()
    lat, r, refs = _run(case, dev, 20)
    lens = r.lengths.cpu().numpy()[3]
    assert len(set(lens[:int(r.n_paths[3])].tolist())) > 1
    assert R.decided(refs[3]) and refs[3]["steps"] == lens.max()


def test_rows_without_a_path(dev):
    case = R.cases()["no_path"]()
    lat, r, refs = _run(case, dev, 7)
    o = _np(r)
    for b in (1, 3):
        assert refs[b]["n_paths"] == 0 and o["n_paths"][b] == 0 and o["kappa"][b] == NEG
        assert np.all(o["lengths"][b] == 0) and np.all(o["paths"][b] == PAD) and np.all(o["arcs"][b] == -1)
        assert np.all(o["logp"][b] == NEG) and np.all(o["gumbel"][b] == NEG)
    lw = swor.log_weights(r).cpu().numpy()
    assert np.all(lw[[1, 3]] == NEG) and np.all(np.isfinite(lw[[0, 2, 4]]))


def test_fewer_paths_than_k(dev):
    case = R.cases()["few_paths"]()
    _, _, b, n = E.few_paths_case()
    lat, r, refs = _run(case, dev, 64)
    assert int(r.n_paths[b]) == n and float(r.kappa[b]) == NEG
    w = torch.exp(swor.log_weights(r))[b].cpu().numpy()
    assert np.array_equal(w[:n], np.exp(r.logp[b, :n].double().cpu().numpy())) and np.all(w[n:] == 0)
    assert abs(w.sum() - 1.0) <= 1e-5
    # everything was drawn: the estimate of any expectation is the exact one
    lens = r.lengths.double()
    exact = float((torch.exp(r.logp[b, :n].double()) * lens[b, :n]).sum())
    assert abs(float(swor.expectation(r, lens)[b]) - exact) <= 1e-12
    assert abs(float(swor.expectation(r, lens, normalize=True)[b]) - exact) <= 1e-4


def test_length_budget(dev):
    """A max_len one below the longest drawn path raises the length error; the default does not."""
    case = R.cases()["mixed"]()
    lat, r, _ = _run(case, dev, 7)
    L = r.paths.shape[2]
    longest = int(r.lengths.max())
    assert longest < L
    u = case.uniforms(7, L)
    theta = torch.from_numpy(case.theta).to(dev)
    again = swor.sample(lat, theta, 7, max_len=longest, uniforms=torch.from_numpy(u[:, :longest].copy()), pad=PAD)
    assert torch.equal(again.paths, r.paths[:, :, :longest]) and torch.equal(again.gumbel, r.gumbel)
    with pytest.raises(_lib.NfstError) as ei:
        swor.sample(lat, theta, 7, max_len=longest - 1, uniforms=torch.from_numpy(u[:, :longest - 1].copy()), pad=PAD)
    assert ei.value.code == _lib.ERR_LENGTH
    swor.sample(lat, theta, 7, pad=PAD)  # default max_len, Philox noise
    with pytest.raises(_lib.NfstError) as ei:  # uniforms narrower than the largest out-degree
        swor.sample(lat, theta, 7, max_len=L, uniforms=torch.from_numpy(u[:, :, :, :2].copy()), pad=PAD)
    assert ei.value.code == R.ERR_ARG


@pytest.mark.parametrize("value", [0.0, float(np.nextafter(np.float32(1), np.float32(0)))])
def test_uniforms_all_on_a_boundary(dev, value):
    """Every uniform 0, or the largest float32 below 1: the noise stays finite (x = u + 2^-25 lies inside (0, 1))."""
    case = R.cases()["weighted"]()
    lat = LatticeBatch.from_synth(case.lats, device=dev)
    L, k = int(lat.depth.max()) + 1, 20
    u = np.full((len(case.lats), L, k, R.degree(case.lats)), value, np.float32)
    _, r, refs = _run(case, dev, k, lat=lat, u=u)
    o = _np(r)
    assert np.all(o["n_paths"] == k) and np.all(np.isfinite(o["gumbel"])) and np.all(np.isfinite(o["kappa"]))
    if all(R.decided(x) for x in refs):  # (equal uniforms tie candidates of equal phi only)
        _check(f"all {value}", lat, case.lats, r, refs, k)
    for b in range(len(case.lats)):
        assert len({tuple(o["arcs"][b, i, :o["lengths"][b, i]]) for i in range(k)}) == k
        assert np.all(np.diff(o["gumbel"][b]) <= 0) and o["gumbel"][b, -1] >= o["kappa"][b]


def test_exact_ties_go_to_the_earlier_flat_index(dev):
    """Every label at -0.25, every uniform 0.5 and the log beta of the rounded float64 backward pass handed to the op, so
    that states that look alike carry the same bits: whole steps tie, below and above 256 candidates and beyond the LDS
    cap, and the op keeps what the restatement keeps: the first k of the flat index, ranked by slot."""
    case = R.tie_case()
    lat = LatticeBatch.from_synth(case.lats, device=dev)
    theta = torch.from_numpy(case.theta).to(dev)
    betas = [R.rounded_beta(l, e) for l, e in zip(case.lats, case.scores())]
    lb = torch.from_numpy(np.concatenate([b[0] for b in betas])).to(dev)
    assert [int(x) for x in lat.n_rows] == [l.n_rows for l in case.lats] and lb.shape[0] == lat.total_rows
    z = torch.tensor([b[1] for b in betas], dtype=torch.float64, device=dev)
    beta = ops.BackwardResult(lb, z.float(), z, None)
    L = int(lat.depth.max()) + 1
    for k in case.ks:
        u = case.uniforms(k, L)
        r = swor.sample(lat, theta, k, max_len=L, uniforms=torch.from_numpy(u), pad=PAD, beta=beta)
        refs = case.references(k, betas=betas, uniforms=u, max_len=L)
        o = _np(r)
        for b, ref in enumerate(refs):
            assert ref["margin"] == 0.0 and o["n_paths"][b] == ref["n_paths"] == k
            a0 = int(lat.arc_off[b])
            for j, p in enumerate(ref["arcs"]):
                assert o["lengths"][b, j] == len(p) and np.array_equal(o["arcs"][b, j, :len(p)] - a0, p), (k, b, j)
            assert np.max(np.abs(o["gumbel"][b] - ref["gumbel"])) <= G_TOL and abs(o["kappa"][b] - ref["kappa"]) <= G_TOL


# ----------------------------------------------------------------------------- determinism
def _bits(r):
    return [None if v is None else v.cpu().numpy().copy() for v in r[:7]]


def _same(x, y, rows=None, arc_shift=None):
    for i, (a, b) in enumerate(zip(x, y)):
        if rows is not None:
            b = b[rows]
        if i == 1 and arc_shift is not None:  # arc ids are canonical in the batch: they move with the lattice
            a, b = np.where(a >= 0, a - arc_shift[0][:, None, None], -1), np.where(b >= 0, b - arc_shift[1][:, None, None], -1)
        assert np.array_equal(a, b, equal_nan=True), i


def test_two_launches_and_a_permuted_batch(dev):
    case = R.cases()["mixed"]()
    k = 20
    lat, r, _ = _run(case, dev, k)
    _, r2, _ = _run(case, dev, k, lat=lat)
    _same(_bits(r), _bits(r2))
    perm = [4, 0, 5, 2, 1, 3]
    L = r.paths.shape[2]
    u = case.uniforms(k, L)
    lat_p = LatticeBatch.from_synth([case.lats[i] for i in perm], device=dev)
    rp = swor.sample(lat_p, torch.from_numpy(case.theta).to(dev), k, max_len=L, uniforms=torch.from_numpy(u[perm].copy()), pad=PAD)
    off, off_p = np.asarray(lat.arc_off)[perm], np.asarray(lat_p.arc_off)
    _same([x[perm] for x in _bits(r)], _bits(rp), arc_shift=(off, off_p))


def test_packings_give_the_same_bits(dev):
    case = R.cases()["star"]()
    k = 64
    base = None
    for opts in (E.STAR_PACKINGS[0], E.STAR_PACKINGS[2], E.STAR_PACKINGS[8]):
        lat = LatticeBatch.from_synth(case.lats, device=dev, **opts)
        _, r, _ = _run(case, dev, k, lat=lat)
        if base is None:
            base = _bits(r)
        else:
            _same(base, _bits(r))


# ----------------------------------------------------------------------------- Philox
def test_philox(dev):
    case = R.cases()["mixed"]()
    lat = LatticeBatch.from_synth(case.lats, device=dev)
    theta = torch.from_numpy(case.theta).to(dev)
    a, b, c = (swor.sample(lat, theta, 7, seed=s, pad=PAD) for s in (5, 5, 6))
    _same(_bits(a), _bits(b))
    assert not torch.equal(a.paths, c.paths)
    o = _np(a)
    for bb in range(lat.n_lattices):
        n = int(o["n_paths"][bb])
        assert len({tuple(o["arcs"][bb, i, :o["lengths"][bb, i]]) for i in range(n)}) == n
        assert np.all(np.diff(o["gumbel"][bb, :n]) <= 0) and (n == 0 or o["gumbel"][bb, n - 1] >= o["kappa"][bb])


@pytest.mark.parametrize("k", [1, 3])
def test_philox_frequencies(dev, k):
    """The small lattice 2048 times in one batch: the frequency of every path among the drawn sets against its exact
    inclusion probability (0.05 is 4.5 binomial standard deviations), and the Horvitz-Thompson estimate of the
    expected length within 5 of its own standard errors."""
    l = R.small_lattice()
    e = R.arc_score32(l, R.small_theta())
    probs = R.path_probs(l, e)
    keys = list(probs)
    p = np.array([probs[a] for a in keys])
    want = p if k == 1 else R.inclusion_probs(p, k)
    lat = LatticeBatch.from_synth([l] * R.SMALL_COPIES, device=dev)
    r = swor.sample(lat, torch.from_numpy(R.small_theta()).to(dev), k, seed=17, pad=PAD)
    o = _np(r)
    assert np.all(o["n_paths"] == k)
    rel = o["arcs"] - np.asarray(lat.arc_off)[:, None, None]
    count = {a: 0 for a in keys}
    for b in range(R.SMALL_COPIES):
        for i in range(k):
            count[tuple(rel[b, i, :o["lengths"][b, i]])] += 1
    freq = np.array([count[a] for a in keys]) / R.SMALL_COPIES
    assert np.max(np.abs(freq - want)) <= 0.05, (freq, want)
    est = swor.expectation(r, r.lengths.double()).cpu().numpy()
    exact = sum(len(a) * q for a, q in probs.items())
    assert abs(est.mean() - exact) <= 5 * est.std(ddof=1) / np.sqrt(len(est))


# ----------------------------------------------------------------------------- log-probabilities and their gradient
@pytest.mark.parametrize("name", ["mixed_per_lattice", "weighted"])
def test_log_prob_and_its_gradient(dev, name):
    """swor.log_prob repeats r.logp (to float32 rounding of the path score and of log Z, each below 2^-23 of its size)
    and its gradient is the path's label / arc counts minus the posteriors of ops.forward_backward."""
    case = R.cases()[name]()
    k = 7
    lat, r, _ = _run(case, dev, k)
    theta = torch.from_numpy(case.theta).to(dev).requires_grad_(True)
    asc0 = case.asc if case.asc is not None else np.zeros(lat.total_arcs, np.float32)
    asc = torch.from_numpy(asc0).to(dev).requires_grad_(True)
    lp = swor.log_prob(lat, theta, r, arc_scores=asc)
    ok = torch.arange(k, device=dev)[None, :] < r.n_paths[:, None]  # (the single-arc lattice has one path)
    assert bool(torch.all(lp.detach()[~ok] == NEG)) and bool(torch.all(r.logp[~ok] == NEG))
    score = ops.score_paths(lat, theta.detach(), r.paths, arc_scores=asc.detach())[0]
    size = float(score[ok].abs().max()) + float(r.logz.abs().max())
    assert float((lp.detach() - r.logp)[ok].abs().max()) <= 4 * size * 2.0 ** -23
    g = torch.from_numpy(np.random.default_rng(3).normal(size=(lat.n_lattices, k)).astype(np.float32)).to(dev) * ok
    (torch.where(ok, lp, torch.zeros_like(lp)) * g).sum().backward()
    fb = ops.forward_backward(lat, theta.detach(), asc.detach(), want_alpha_beta=False, want_posterior=True, want_grad_theta=True)
    arcs, gn = r.arcs.cpu().numpy(), g.cpu().numpy().astype(np.float64)
    want_arc = -fb.posterior.double().cpu().numpy() * gn.sum(axis=1)[lat.arc_lattice().cpu().numpy()]
    want_theta = -fb.grad_theta.double().cpu().numpy() * gn.sum(axis=1)[:, None]
    label = lat.arc_label.cpu().numpy()
    for b in range(lat.n_lattices):
        for i in range(k):
            for a in arcs[b, i][arcs[b, i] >= 0]:
                want_arc[a] += gn[b, i]
                want_theta[b, label[a]] += gn[b, i]
    if case.theta.ndim == 1:
        want_theta = want_theta.sum(axis=0)
    assert np.max(np.abs(asc.grad.double().cpu().numpy() - want_arc)) <= 1e-5
    assert np.max(np.abs(theta.grad.double().cpu().numpy() - want_theta)) <= 1e-5


def test_scorer_entry_point(dev):
    case = R.cases()["mixed"]()
    lat = LatticeBatch.from_synth(case.lats, device=dev)
    scorer = LatticeScorer(E.V_MIXED, theta=torch.from_numpy(case.theta)).to(dev).set_lattice(lat)
    a = scorer.sample_without_replacement(7, seed=9)
    b = swor.sample(lat, torch.from_numpy(case.theta).to(dev), 7, seed=9, pad=PAD)
    _same(_bits(a), _bits(b))
    assert torch.equal(a.logz, b.logz)

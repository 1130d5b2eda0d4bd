"""ops.positional_* (nfst_positional, nfst_positional_viterbi: time-synchronous sweeps under position-dependent scores)
against the NumPy restatement of tests/positional_ref.py, which tests/test_positional_cpu.py proves against path
enumeration.

Bounds.  The sum-product kernel computes in (float64 mantissa, int32 exponent) end to end, so its float64 outputs
(logz64, every finite len_logz entry) are held to 1e-9 * max(1, |ref|), as tests/test_gpu_expectation.py holds
nfst_expectation's; the float32 log Z to the project's 1e-5 * max(1, |ref|); posteriors to 2e-6 absolute; the max-plus
outputs (best, labels, arcs, lengths) to the float32 restatement bit for bit.  The largest error of every kind goes to
positional_errors.json in the directory of run outputs (profiles/README.md)."""
import dataclasses
import glob
import json
import os

import numpy as np
import pytest
import torch

from nfst_amd import ops, synth
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from tests import positional_ref as R
from tests.test_positional_cpu import small_lattices, truncations

pytestmark = pytest.mark.gpu
PAD, BOS = synth.PAD, synth.BOS
NEG = -np.inf
TOL64, TOL32, TOLP = 1e-9, 1e-5, 2e-6

_ERR = {}


def rec(tag, err):
    _ERR[tag] = max(_ERR.get(tag, 0.0), float(err))
    return float(err)


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for out in sorted(glob.glob(os.path.join(root, "*_out"))):
        if _ERR and os.path.isdir(out):
            with open(os.path.join(out, "positional_errors.json"), "w") as f:
                json.dump(dict(sorted(_ERR.items())), f, indent=1)


def _same_vocab(lats):
    V = max(l.vocab for l in lats)
    return [dataclasses.replace(l, vocab=V) for l in lats]


_SMALL = []


def small6():
    if not _SMALL:
        _SMALL.extend(_same_vocab(small_lattices()))
    return list(_SMALL)


def _inputs(lats, seed, T, shared_pos=False, shared_theta=True):
    rng = np.random.default_rng(seed)
    B, V = len(lats), lats[0].vocab
    theta = rng.normal(-1.0, 0.8, size=(V,) if shared_theta else (B, V)).astype(np.float32)
    pos = rng.normal(0.0, 1.0, size=(T, V) if shared_pos else (B, T, V)).astype(np.float32)
    pos[..., PAD] = np.nan  # the pad column enters no output
    return theta, pos


def _per(x, b, shared_ndim):
    return None if x is None else (x if x.ndim == shared_ndim else x[b])


def reference(lat, lats, theta, pos, T, asc=None):
    out = []
    for b, l in enumerate(lats):
        a0 = int(lat.arc_off[b])
        asc_b = None if asc is None else asc[a0:a0 + l.n_arcs]
        th_b, pos_b = _per(theta, b, 1), _per(pos, b, 2)
        ref = R.sum_product(l, R.arc_score64(l, th_b, asc_b), pos_b, T)
        ref["mp"] = R.max_plus(l, th_b, pos_b, T, asc_b)
        out.append(ref)
    return out


def run(lat, theta, pos, T, dev, asc=None):
    t = lambda x: None if x is None else torch.from_numpy(x).to(dev)
    r = ops.positional_forward_backward(lat, t(theta), t(pos), T=T, arc_scores=t(asc), want_pos_posterior=True,
                                        want_arc_posterior=True, want_len=True)
    v = ops.positional_viterbi(lat, t(theta), t(pos), T=T, arc_scores=t(asc), pad=PAD)
    return r, v


def check(tag, lat, lats, r, v, refs, T):
    z64, z32 = r.logz64.cpu().numpy(), r.logz.cpu().numpy()
    ll, pp, ap = r.len_logz.cpu().numpy(), r.pos_posterior.cpu().numpy(), r.arc_posterior.cpu().numpy()
    best, paths, arcs, lens = (x.cpu().numpy() for x in v)
    assert pp.shape == (len(lats), T, lat.vocab) and ll.shape == (len(lats), T + 1) and paths.shape == (len(lats), T)
    assert not np.isnan(z64).any() and not np.isnan(ll).any() and not np.isnan(pp).any() and not np.isnan(ap).any()
    for b, (l, ref) in enumerate(zip(lats, refs)):
        a0 = int(lat.arc_off[b])
        if np.isfinite(ref["logz"]):
            scale = max(1.0, abs(ref["logz"]))
            assert rec(tag + ".logz64", abs(z64[b] - ref["logz"]) / scale) <= TOL64, (tag, b, z64[b], ref["logz"])
            assert rec(tag + ".logz32", abs(float(z32[b]) - ref["logz"]) / scale) <= TOL32, (tag, b)
        else:
            assert z64[b] == NEG and z32[b] == NEG, (tag, b)
        fin = np.isfinite(ref["len_logz"])
        assert np.all(ll[b][~fin] == NEG), (tag, b)
        if fin.any():
            e = np.abs(ll[b][fin] - ref["len_logz"][fin]) / np.maximum(1.0, np.abs(ref["len_logz"][fin]))
            assert rec(tag + ".len_logz", e.max()) <= TOL64, (tag, b)
        assert rec(tag + ".pos_post", np.abs(pp[b] - ref["pos_post"]).max()) <= TOLP, (tag, b)
        assert rec(tag + ".arc_post", np.abs(ap[a0:a0 + l.n_arcs] - ref["arc_post"]).max()) <= TOLP, (tag, b)
        mp = ref["mp"]
        assert best[b:b + 1].view(np.int32)[0] == mp["best"].view(np.int32), (tag, b, best[b], mp["best"])
        n = len(mp["arcs"])
        assert lens[b] == n, (tag, b)
        assert np.array_equal(arcs[b, :n] - a0, mp["arcs"]) and np.array_equal(paths[b, :n], mp["labels"]), (tag, b)
        assert np.all(paths[b, n:] == PAD) and np.all(arcs[b, n:] == -1), (tag, b)


def _all_T(lats):
    return sorted({T for l in lats for _, T in truncations(l)})


# ----------------------------------------------------------------------------- (a) six small lattices, every truncation
@pytest.mark.parametrize("shared_pos", [False, True])
def test_small_batch_at_every_truncation(dev, shared_pos):
    lats = small6()
    lat = LatticeBatch.from_synth(lats, device=dev)
    cases = set()
    for T in _all_T(lats):
        theta, pos = _inputs(lats, 1000 + T, T, shared_pos=shared_pos)
        refs = reference(lat, lats, theta, pos, T)
        r, v = run(lat, theta, pos, T, dev)
        check(f"a{int(shared_pos)}", lat, lats, r, v, refs, T)
        dead = [not np.isfinite(x["logz"]) for x in refs]
        cases.add((any(dead), not all(dead)))
        for b, l in enumerate(lats):
            cases.update((b, name) for name, Tb in truncations(l) if Tb == T)
    assert (True, True) in cases  # some lattices of one launch got -inf while others did not
    assert all((b, name) in cases for b in range(6) for name in ("below", "shortest", "between", "depth", "beyond"))


# ----------------------------------------------------------------------------- (b) more rows than threads
_BIG = {}


def big_pair():
    if not _BIG:
        big = synth.layered_lattice(22, n_states=1100, avg_degree=6.0, vocab=70, width=24, span=4, max_degree=24)
        tiny = synth.layered_lattice(3, n_states=12, avg_degree=2.0, vocab=70, width=3, span=3, max_degree=4)
        assert tiny.n_rows == 13 and big.n_rows > 1024 and big.vocab % 64
        _BIG["lats"] = [big, tiny]
        _BIG["T"] = R.min_max_len(big)[1]
    return _BIG["lats"], _BIG["T"]


@pytest.mark.parametrize("shared_pos", [False, True])
def test_more_rows_than_threads(dev, shared_pos):
    lats, T = big_pair()
    assert T == 48
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert int(lat.depth[0]) == T
    theta, pos = _inputs(lats, 22, T, shared_pos=shared_pos)
    refs = reference(lat, lats, theta, pos, T)
    assert np.isfinite(refs[0]["len_logz"]).sum() == 34  # distinct path lengths
    r, v = run(lat, theta, pos, T, dev)
    check(f"b{int(shared_pos)}", lat, lats, r, v, refs, T)


# ----------------------------------------------------------------------------- (c) a state's arcs span waves
@pytest.mark.parametrize("shared_pos", [False, True])
def test_high_degree(dev, shared_pos):
    l = synth.layered_lattice(24, n_states=200, avg_degree=90.0, vocab=140, width=8, span=3, max_degree=130)
    deg = np.bincount(l.src[l.src != l.dst])
    assert deg.max() == 119 and l.n_arcs > 17000
    T = 27
    assert R.min_max_len(l)[1] <= T
    lat = LatticeBatch.from_synth([l], device=dev)
    theta, pos = _inputs([l], 24, T, shared_pos=shared_pos)
    r, v = run(lat, theta, pos, T, dev)
    check(f"c{int(shared_pos)}", lat, [l], r, v, reference(lat, [l], theta, pos, T), T)


# ----------------------------------------------------------------------------- (d) 601 positions, few labels
@pytest.mark.parametrize("shared_pos", [False, True])
def test_deep(dev, shared_pos):
    l = synth.layered_lattice(25, n_states=1200, avg_degree=2.5, vocab=27, width=2, span=2, max_degree=6, weighted=True)
    T = 601
    assert R.min_max_len(l) == (379, 601)
    lat = LatticeBatch.from_synth([l], device=dev)
    rng = np.random.default_rng(25)
    theta = synth.label_scores(25, 27)[None, :].copy()
    asc = rng.normal(0.0, 0.3, size=l.n_arcs).astype(np.float32)
    pos = rng.normal(0.0, 1.0, size=(T, 27) if shared_pos else (1, T, 27)).astype(np.float32)
    refs = reference(lat, [l], theta, pos, T, asc)
    assert abs(refs[0]["logz"]) > 100.0
    r, v = run(lat, theta, pos, T, dev, asc)
    check(f"d{int(shared_pos)}", lat, [l], r, v, refs, T)


# ----------------------------------------------------------------------------- (e) beyond the compact record format
@pytest.mark.parametrize("shared_pos", [False, True])
def test_wide_vocab(dev, shared_pos):
    l = synth.layered_lattice(26, n_states=12, avg_degree=2.0, vocab=2100, width=3, span=3, max_degree=4)
    T = 8
    assert R.min_max_len(l)[1] <= T
    lat = LatticeBatch.from_synth([l], device=dev)
    theta, pos = _inputs([l], 26, T, shared_pos=shared_pos)
    r, v = run(lat, theta, pos, T, dev)
    check(f"e{int(shared_pos)}", lat, [l], r, v, reference(lat, [l], theta, pos, T), T)


# ----------------------------------------------------------------------------- (f) more workgroups than CUs
def _bits(r, v):
    return [x.cpu().numpy() for x in (r.logz64, r.logz, r.len_logz, r.pos_posterior, r.arc_posterior, v.best, v.paths, v.lengths)]


@pytest.mark.parametrize("shared_pos", [False, True])
def test_three_hundred_lattices_equal_three(dev, shared_pos):
    base = small6()[:3]
    T = 6
    theta, pos = _inputs(base, 31, T, shared_pos=shared_pos)
    lat3 = LatticeBatch.from_synth(base, device=dev)
    r3, v3 = run(lat3, theta, pos, T, dev)
    check(f"f{int(shared_pos)}", lat3, base, r3, v3, reference(lat3, base, theta, pos, T), T)
    lat = LatticeBatch.from_synth(base * 100, device=dev)
    r, v = run(lat, theta, pos if shared_pos else np.tile(pos, (100, 1, 1)), T, dev)
    small, many = _bits(r3, v3), _bits(r, v)
    arcs3, arcs = v3.path_arcs.cpu().numpy(), v.path_arcs.cpu().numpy()
    for k in range(100):
        for x3, x in zip(small, many):
            if x3.shape[0] == 3:
                assert np.array_equal(x[3 * k:3 * k + 3].view(np.uint8), x3.view(np.uint8)), k
        n = lat3.total_arcs
        assert np.array_equal(many[4][n * k:n * (k + 1)].view(np.int32), small[4].view(np.int32)), k
        assert np.array_equal(np.where(arcs[3 * k:3 * k + 3] >= 0, arcs[3 * k:3 * k + 3] - n * k, -1), arcs3), k


# ----------------------------------------------------------------------------- (g) -inf entries
def test_minus_infinity_entries(dev):
    lats = small6()[:3]
    T = 6
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta, pos = _inputs(lats, 41, T)
    # lattice 0: exactly one path left alive; lattice 1: a position at which every label is -inf; lattice 2: untouched
    keep = R.enumerate_paths(lats[0])[5]
    one = np.full((T, lat.vocab), NEG, np.float32)
    for t, a in enumerate(keep):
        one[t, lats[0].label[a]] = pos[0, t, lats[0].label[a]]
    pos[0] = one
    pos[1, 1, :] = NEG
    refs = reference(lat, lats, theta, pos, T)
    r, v = run(lat, theta, pos, T, dev)
    check("g", lat, lats, r, v, refs, T)
    pp = r.pos_posterior.cpu().numpy()
    assert set(np.unique(pp[0])) <= {0.0, 1.0} and pp[0].sum() == len(keep)
    assert np.array_equal(v.path_arcs.cpu().numpy()[0, :len(keep)], keep)
    assert float(r.logz64[1]) == NEG and not pp[1].any() and int(v.lengths[1]) == 0 and float(v.best[1]) == NEG
    assert np.isfinite(float(r.logz64[2])) and np.isfinite(refs[2]["logz"])
    # theta with a -inf label: one arc out of state 1 (after bos) is gone
    theta2 = theta.copy()
    l = lats[2]
    theta2[l.label[np.nonzero(l.src == l.dst[0])[0][0]]] = NEG
    _, pos2 = _inputs(lats, 42, T)
    r, v = run(lat, theta2, pos2, T, dev)
    check("g.theta", lat, lats, r, v, reference(lat, lats, theta2, pos2, T), T)


# ----------------------------------------------------------------------------- identities with the other ops
@pytest.mark.parametrize("which", ["a", "b"])
def test_without_positions_it_is_forward_backward_and_k_best(dev, which):
    lats = small6() if which == "a" else big_pair()[0]
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = torch.from_numpy(synth.label_scores(5, lat.vocab)).to(dev)
    for extra in (0, 3):
        T = int(lat.depth.max()) + extra
        r = ops.positional_forward_backward(lat, theta, None, T=None if extra == 0 else T, want_arc_posterior=True, want_len=True)
        assert r.pos_posterior.shape[1] == T
        fb = ops.forward_backward(lat, theta)
        z, zf = r.logz64.cpu().numpy(), fb.logz64.cpu().numpy()
        assert rec("id.logz", (np.abs(z - zf) / np.maximum(1.0, np.abs(zf))).max()) <= TOL32
        assert rec("id.arc_post", (r.arc_posterior - fb.posterior).abs().max().item()) <= TOLP
        v = ops.positional_viterbi(lat, theta, None, T=T, pad=PAD)
        kb = ops.k_best(lat, theta, 1, max_len=T, pad=PAD)
        assert torch.equal(v.best.view(torch.int32), kb.best[:, 0].view(torch.int32))
        assert torch.equal(v.paths, kb.paths[:, 0]) and torch.equal(v.path_arcs, kb.arcs[:, 0]) and torch.equal(v.lengths, kb.lengths[:, 0])
        # the identities of the semantics on the GPU outputs
        pp = r.pos_posterior.double().cpu().numpy()
        ll = r.len_logz.cpu().numpy()
        for b, l in enumerate(lats):
            p_len = np.exp(ll[b] - z[b])
            assert abs(p_len.sum() - 1.0) <= 1e-9
            assert np.abs(pp[b].sum(axis=1) - (1.0 - np.cumsum(p_len)[:T])).max() <= TOLP * lat.vocab
            assert abs(pp[b, 0, BOS] - 1.0) <= TOLP


# ----------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("shared", [False, True])
def test_autograd(dev, which, shared):
    lats, T = (small6(), 13) if which == "a" else big_pair()
    lat = LatticeBatch.from_synth(lats, device=dev)
    B = len(lats)
    theta_np, pos_np = _inputs(lats, 51, T, shared_pos=shared, shared_theta=shared)
    pos_np[..., PAD] = 0.0  # (a NaN input would give a NaN * 0 gradient in torch's own arithmetic)
    asc_np = np.random.default_rng(52).normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32)
    g_np = np.linspace(0.5, 2.0, B).astype(np.float32)
    theta, pos, asc = (torch.from_numpy(x).to(dev).requires_grad_(True) for x in (theta_np, pos_np, asc_np))
    z = ops.positional_log_z(lat, theta, pos, asc)
    z.backward(torch.from_numpy(g_np).to(dev))
    refs = reference(lat, lats, theta_np, pos_np, T, asc_np)
    d_pos = np.stack([x["pos_post"] * g for x, g in zip(refs, g_np)])
    d_theta = d_pos.sum(axis=1)
    d_arc = np.concatenate([x["arc_post"] * g for x, g in zip(refs, g_np)])
    if shared:
        d_pos, d_theta = d_pos.sum(axis=0), d_theta.sum(axis=0)
    tol = TOLP * max(1.0, float(np.abs(g_np).max()))
    assert pos.grad.shape == pos.shape and theta.grad.shape == theta.shape and asc.grad.shape == asc.shape
    assert rec("grad.pos", np.abs(pos.grad.cpu().numpy() - d_pos).max()) <= tol
    assert rec("grad.theta", np.abs(theta.grad.cpu().numpy() - d_theta).max()) <= tol
    assert rec("grad.arc", np.abs(asc.grad.cpu().numpy() - d_arc).max()) <= tol
    for b, x in enumerate(refs):
        if np.isfinite(x["logz"]):
            assert abs(float(z.detach()[b]) - x["logz"]) <= TOL32 * max(1.0, abs(x["logz"]))


def test_second_backward_raises(dev):
    lats = small6()[:3]
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta_np, pos_np = _inputs(lats, 61, 6)
    pos_np[..., PAD] = 0.0
    theta = torch.from_numpy(theta_np).to(dev).requires_grad_(True)
    pos = torch.from_numpy(pos_np).to(dev).requires_grad_(True)
    z = ops.positional_log_z(lat, theta, pos)
    (g,) = torch.autograd.grad(z.sum(), pos, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


# ----------------------------------------------------------------------------- repeatability
def test_two_launches_and_another_batch_order_give_the_same_bits(dev):
    lats = small6() + big_pair()[0]
    lats = _same_vocab(lats)
    T = 30
    theta, pos = _inputs(lats, 71, T)
    lat = LatticeBatch.from_synth(lats, device=dev)
    r1, v1 = run(lat, theta, pos, T, dev)
    r2, v2 = run(lat, theta, pos, T, dev)
    for x, y in zip(_bits(r1, v1) + [v1.path_arcs.cpu().numpy()], _bits(r2, v2) + [v2.path_arcs.cpu().numpy()]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    order = [7, 2, 5, 0, 6, 3, 1, 4]
    lat_p = LatticeBatch.from_synth([lats[i] for i in order], device=dev)
    rp, vp = run(lat_p, theta, pos[order], T, dev)
    a, p = _bits(r1, v1), _bits(rp, vp)
    arcs, arcs_p = v1.path_arcs.cpu().numpy(), vp.path_arcs.cpu().numpy()
    for j, i in enumerate(order):
        for x, y in zip(a, p):
            if x.shape[0] == len(lats):
                assert np.array_equal(x[i:i + 1].view(np.uint8), y[j:j + 1].view(np.uint8)), (i, j)
        a0, p0, n = int(lat.arc_off[i]), int(lat_p.arc_off[j]), lats[i].n_arcs
        assert np.array_equal(a[4][a0:a0 + n].view(np.int32), p[4][p0:p0 + n].view(np.int32)), (i, j)
        assert np.array_equal(np.where(arcs[i] >= 0, arcs[i] - a0, -1), np.where(arcs_p[j] >= 0, arcs_p[j] - p0, -1))


# ----------------------------------------------------------------------------- wrappers
def test_wrapper_errors_raise_before_any_launch(dev):
    lats = small6()[:3]
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = torch.zeros(lat.vocab, device=dev)
    good = torch.zeros(3, 6, lat.vocab, device=dev)
    for bad in (torch.zeros(3, 6, lat.vocab + 1, device=dev), torch.zeros(2, 6, lat.vocab, device=dev), torch.zeros(lat.vocab, device=dev)):
        for fn in (ops.positional_forward_backward, ops.positional_viterbi, ops.positional_log_z):
            with pytest.raises(ValueError):
                fn(lat, theta, bad)
    for fn in (ops.positional_forward_backward, ops.positional_viterbi):
        with pytest.raises(ValueError):
            fn(lat, theta, None, T=0)
        with pytest.raises(ValueError):
            fn(lat, theta, good, T=5)
    with pytest.raises(ValueError):
        ops.length_distribution(lat, theta, T=0)
    for fn in (ops.positional_forward_backward, ops.positional_viterbi, ops.positional_log_z):
        with pytest.raises(ValueError):
            fn(lat, theta, good.cpu())  # a CPU tensor with a GPU batch
        with pytest.raises(ValueError):
            fn(lat, theta.cpu(), good)


def test_length_distribution_and_scorer_methods(dev):
    lats = small6()
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta_np = synth.label_scores(9, lat.vocab)
    theta = torch.from_numpy(theta_np).to(dev)
    for T in (None, 10):
        logp, z = ops.length_distribution(lat, theta, T=T)
        Tn = int(lat.depth.max()) if T is None else T
        assert logp.shape == (6, Tn + 1) and logp.dtype == torch.float64
        refs = reference(lat, lats, theta_np, None, Tn)
        for b, ref in enumerate(refs):
            got = logp[b].cpu().numpy()
            if not np.isfinite(ref["logz"]):
                assert np.all(got == NEG) and float(z[b]) == NEG
                continue
            assert abs(np.exp(got).sum() - 1.0) <= 1e-6
            want = ref["len_logz"] - ref["logz"]
            fin = np.isfinite(want)
            assert np.all(got[~fin] == NEG)
            assert rec("length_distribution", np.abs(got[fin] - want[fin]).max()) <= TOL64 * max(1.0, abs(ref["logz"]))
    sc = LatticeScorer(lat.vocab, theta=theta_np).to(dev).set_lattice(lat)
    _, pos_np = _inputs(lats, 81, 24)
    pos_np[..., PAD] = 0.0
    pos = torch.from_numpy(pos_np).to(dev).requires_grad_(True)
    z = sc.positional_log_z(pos)
    z.sum().backward()
    assert sc.theta.grad is not None and pos.grad.shape == pos.shape
    r = ops.positional_forward_backward(lat, theta, pos.detach())
    assert torch.equal(z.detach(), r.logz) and torch.equal(pos.grad, r.pos_posterior)
    v = sc.positional_viterbi(pos.detach())
    assert torch.equal(v.best, ops.positional_viterbi(lat, theta, pos.detach(), pad=PAD).best)
    logp, _ = sc.length_distribution()
    assert torch.equal(logp, ops.length_distribution(lat, theta)[0])

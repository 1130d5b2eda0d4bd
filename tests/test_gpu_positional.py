"""ops.positional_* (nfst_positional, nfst_positional_viterbi: time-synchronous sweeps under position-dependent scores)
against the NumPy restatement of tests/positional_ref.py, which tests/test_positional_cpu.py proves against path
enumeration.

Bounds.  The sum-product kernel computes in (float64 mantissa, int32 exponent) end to end, so its float64 outputs
(logz64, every finite len_logz entry) are held to 1e-9 * max(1, |ref|), as tests/test_gpu_expectation.py holds
nfst_expectation's; the float32 log Z to the project's 1e-5 * max(1, |ref|); posteriors to 2e-6 absolute; the max-plus
outputs (best, labels, arcs, lengths) to the float32 restatement bit for bit.  The largest error of every kind goes to
positional_errors.json in the directory of run outputs (profiles/README.md)."""
import ctypes as C
import dataclasses
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


def check_sum(tag, lat, lats, r, refs, T):
    z64, z32 = r.logz64.cpu().numpy(), r.logz.cpu().numpy()
    ll, pp, ap = r.len_logz.cpu().numpy(), r.pos_posterior.cpu().numpy(), r.arc_posterior.cpu().numpy()
    assert pp.shape == (len(lats), T, lat.vocab) and ll.shape == (len(lats), T + 1)
    assert not np.isnan(z64).any() and not np.isnan(ll).any() and not np.isnan(pp).any() and not np.isnan(ap).any()
    assert not np.isnan(z32).any()
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


def check_vit(tag, lat, lats, v, refs, T):
    best, paths, arcs, lens = (x.cpu().numpy() for x in v)
    assert paths.shape == (len(lats), T) and arcs.shape == (len(lats), T)
    for b, (l, ref) in enumerate(zip(lats, refs)):
        a0 = int(lat.arc_off[b])
        mp = ref["mp"]
        assert best[b:b + 1].view(np.int32)[0] == mp["best"].view(np.int32), (tag, b, best[b], mp["best"])
        n = len(mp["arcs"])
        assert lens[b] == n, (tag, b)
        assert np.array_equal(arcs[b, :n] - a0, mp["arcs"]) and np.array_equal(paths[b, :n], mp["labels"]), (tag, b)
        assert np.all(paths[b, n:] == PAD) and np.all(arcs[b, n:] == -1), (tag, b)


def check(tag, lat, lats, r, v, refs, T):
    check_sum(tag, lat, lats, r, refs, T)
    check_vit(tag, lat, lats, v, refs, T)


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


# =============================================================================================================
# Every launch branch (inputs: the positional section of tests/edge_cases.py; tests/test_positional_cpu.py proves on the
# reference and the plan query alone that they are what the cases need).  ops.positional_plan is the rule the launchers
# themselves call, so "staged" below is what the launch took.
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def large(which, weighted=False):
    """`big` or `mid` of tests/edge_cases.py and its longest path, built once per module (nothing here changes a lattice)."""
    def make():
        l = E.pos_large(which, weighted)
        return l, R.min_max_len(l)[1]
    return cached(("large", which, weighted), make)


def staged(lat):
    """(nfst_positional stages its arcs, nfst_positional_viterbi does)."""
    return ops.positional_plan(lat, False)[1], ops.positional_plan(lat, True)[1]


def out_bits(lat, lats, r, v):
    """Per lattice, every output as raw bytes (path_arcs relative to the lattice)."""
    z64, z32, ll, pp, ap = (None if x is None else x.cpu().numpy() for x in (r.logz64, r.logz, r.len_logz, r.pos_posterior, r.arc_posterior))
    best, paths, arcs, lens = (x.cpu().numpy() for x in v)
    out = []
    for b, l in enumerate(lats):
        a0 = int(lat.arc_off[b])
        rel = np.where(arcs[b] >= 0, arcs[b] - a0, -1).astype(np.int32)
        per = dict(logz64=z64[b:b + 1], logz=z32[b:b + 1], best=best[b:b + 1], paths=paths[b], lengths=lens[b:b + 1], path_arcs=rel)
        if ll is not None:
            per["len_logz"] = ll[b]
        if pp is not None:
            per["pos_posterior"] = pp[b]
        if ap is not None:
            per["arc_posterior"] = ap[a0:a0 + l.n_arcs]
        out.append({k: np.ascontiguousarray(x).view(np.uint8).copy() for k, x in per.items()})
    return out


def same_bits(x, y, where):
    assert x.keys() == y.keys(), where
    for k in x:
        assert np.array_equal(x[k], y[k]), (where, k)


ALL_OUTPUTS = {"logz64", "logz", "len_logz", "pos_posterior", "arc_posterior", "best", "paths", "lengths", "path_arcs"}


# ----------------------------------------------------------------------------- (a) the STAGED = false flavours
def _large_case(which, variant):
    """(lats, theta, pos, asc, T): `big` beside a 13-row neighbour, or `mid` alone, at its longest path.  Every variant
    has inputs of its own (no table, a shared one, one per lattice, extras), so each has a reference of its own."""
    weighted = variant == "extras"
    l, T = large(which, weighted)
    lats = [l] + ([cached(("neighbour", weighted), lambda: E.pos_neighbour(weighted=weighted))] if which == "big" else [])
    theta, pos = _inputs(lats, 270 + len(variant), T, shared_pos=variant == "shared", shared_theta=variant != "per lattice")
    if variant == "no pos":
        pos = None
    asc = np.random.default_rng(271).normal(0.0, 0.3, size=sum(l.n_arcs for l in lats)).astype(np.float32) if weighted else None
    return lats, theta, pos, asc, T


@pytest.mark.parametrize("variant", ["no pos", "shared", "per lattice", "extras"])
@pytest.mark.parametrize("which", ["big", "mid"])
def test_unstaged_flavours(dev, which, variant):
    """k_positional<EXTRA, false> and k_positional_viterbi<false> (PosArcsGlobal, the forward pass over in_ptr / in_rec of
    the workspace) against the reference; on `mid` the sum-product reads the canonical arrays while max-plus stages."""
    lats, theta, pos, asc, T = _large_case(which, variant)
    assert T == (62 if which == "big" else 57)
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert staged(lat) == ((False, False) if which == "big" else (False, True))
    assert (lat.weighted != 0) == (variant == "extras")
    refs = reference(lat, lats, theta, pos, T, asc)
    assert all(np.isfinite(x["logz"]) for x in refs)
    if which == "big":
        assert np.isfinite(refs[0]["len_logz"]).sum() == 41
    r, v = run(lat, theta, pos, T, dev, asc)
    check(f"unstaged.{which}.{variant}", lat, lats, r, v, refs, T)


# ----------------------------------------------------------------------------- (b) staged and unstaged: the same bits
def degree_classes():
    return list(cached("degree classes", E.pos_degree_classes))


def shared_lattices():  # the six small lattices and the degree classes at one vocabulary
    return list(cached("shared", lambda: [dataclasses.replace(l, vocab=E.POS_V) for l in small_lattices()] + degree_classes()))


@pytest.mark.parametrize("extras", [False, True])
def test_staged_and_unstaged_give_the_same_bits(dev, extras):
    """"the same bits".  The same lattices and inputs in a batch whose arcs are staged in LDS and, beside
    `big`, in one that reads the canonical arrays."""
    lats = shared_lattices()
    assert all(l.vocab == E.POS_V for l in lats)
    big = large("big")[0]
    T = cached("shared T", lambda: max(R.min_max_len(l)[1] for l in lats))
    theta, pos = _inputs(lats + [big], 280, T)
    n = sum(l.n_arcs for l in lats)
    asc = np.random.default_rng(281).normal(0.0, 0.3, size=n + big.n_arcs).astype(np.float32) if extras else None
    lat_s = LatticeBatch.from_synth(lats, device=dev)
    lat_u = LatticeBatch.from_synth(lats + [big], device=dev)
    assert staged(lat_s) == (True, True) and staged(lat_u) == (False, False)
    rs, vs = run(lat_s, theta, pos[:-1], T, dev, None if asc is None else asc[:n])
    ru, vu = run(lat_u, theta, pos, T, dev, asc)
    bs, bu = out_bits(lat_s, lats, rs, vs), out_bits(lat_u, lats, ru, vu)
    for b in range(len(lats)):
        assert set(bs[b]) == ALL_OUTPUTS
        same_bits(bs[b], bu[b], b)
    refs = reference(lat_s, lats, theta, pos[:-1], T, None if asc is None else asc[:n])
    check(f"bits.{int(extras)}", lat_s, lats, rs, vs, refs, T)
    assert sum(np.isfinite(x["logz"]) for x in refs) == len(lats)


# ----------------------------------------------------------------------------- (c) every group size
def test_every_group_size(dev):
    """G = 8, 16 and 32 (by the mean degree alone and through the widening loop) against the reference, at the longest
    path and at a truncation; with the other batches of this file every G the kernel can choose."""
    lats = degree_classes()
    lat = LatticeBatch.from_synth(lats, device=dev)
    groups = R.batch_groups(lat)
    assert groups == [g for _, g in E.POS_DEGREE_CLASSES.values()] and {8, 16, 32} == set(groups)
    everything = set(groups)
    for other in (small6(), E.mixed_batch(), [large("big")[0]], E.packing_lattices()):
        everything |= set(R.batch_groups(LatticeBatch.from_synth(other)))
    assert everything == {1, 2, 4, 8, 16, 32, 64}
    hi = max(R.min_max_len(l)[1] for l in lats)
    assert hi == 17
    for T in (hi, 6):
        theta, pos = _inputs(lats, 290 + T, T)
        refs = reference(lat, lats, theta, pos, T)
        live = [np.isfinite(x["logz"]) for x in refs]
        assert all(live) if T == hi else (any(live) and not all(live))
        r, v = run(lat, theta, pos, T, dev)
        check(f"groups.{T}", lat, lats, r, v, refs, T)


# ----------------------------------------------------------------------------- (d) output subsets, need_alpha == 0
def test_output_subsets(dev, monkeypatch):
    lats = E.mixed_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    T = 46
    theta_np, pos_np = _inputs(lats, 300, T)  # (NaN in the pad column: no subset of the outputs may read it)
    theta, pos = torch.from_numpy(theta_np).to(dev), torch.from_numpy(pos_np).to(dev)
    seen = []
    real = ops._positional_ws

    def spy(lat, T, flags):
        ws, n = real(lat, T, flags)
        seen.append((flags, n))
        return ws, n

    monkeypatch.setattr(ops, "_positional_ws", spy)
    full = ops.positional_forward_backward(lat, theta, pos, want_pos_posterior=True, want_arc_posterior=True, want_len=True)
    refs = reference(lat, lats, theta_np, pos_np, T)
    check_sum("subsets", lat, lats, full, refs, T)
    eq = lambda x, y: torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    for want in range(8):
        wp, wa, wl = bool(want & 1), bool(want & 2), bool(want & 4)
        r = ops.positional_forward_backward(lat, theta, pos, want_pos_posterior=wp, want_arc_posterior=wa, want_len=wl)
        assert eq(r.logz64, full.logz64) and eq(r.logz, full.logz), want
        for got, ref, on in ((r.pos_posterior, full.pos_posterior, wp), (r.arc_posterior, full.arc_posterior, wa), (r.len_logz, full.len_logz, wl)):
            assert (got is not None) == on, want
            if on:
                assert eq(got, ref), want
        if want == 0:  # log Z only: the flags-0 workspace of 12 bytes per arc, no stored rows
            flags, n = seen[-1]
            small = _lib.lib.nfst_positional_ws_bytes(C.byref(lat.c_struct()), T, 0)
            assert flags == 0 and n == small and 12 * lat.total_arcs <= small < 12 * lat.total_arcs + 2 * 256 + 1
            assert small < 12 * (T + 1) * lat.total_rows <= _lib.lib.nfst_positional_ws_bytes(C.byref(lat.c_struct()), T, 1)
        else:
            assert seen[-1][0] == 1
    z = ops.positional_log_z(lat, theta, pos)  # nothing requires a gradient: log Z only
    assert seen[-1][0] == 0 and not z.requires_grad
    assert eq(z, full.logz)


# ----------------------------------------------------------------------------- (e) every packing, chunked programs
PACKING_A, PACKING_B = 0, 3  # the default packing and (group_mode=1, slots_per_lane=1): 412 and 430 rows


def _packing_case():
    lats = E.packing_lattices()
    T = max(R.min_max_len(l)[1] for l in lats)
    theta, pos = _inputs(lats, 310, T)
    lat = LatticeBatch.from_synth(lats)
    return lats, theta, pos, T, reference(lat, lats, theta, pos, T)


@pytest.mark.parametrize("i", range(len(E.STAR_PACKINGS)), ids=[str(i) for i in range(len(E.STAR_PACKINGS))])
def test_every_packing(dev, i):
    """The kernels read the canonical arrays only, but max_rows -- the stride of the two LDS rows and of every LDS carve-up
    -- is the packing's (scratch rows).  Fan-out 200 and fan-in 200 at G = 1."""
    lats, theta, pos, T, refs = cached("packing", _packing_case)
    assert T == 15
    rows = cached("packing rows", lambda: [int(LatticeBatch.from_synth(lats, **o).max_rows) for o in E.STAR_PACKINGS])
    assert len(set(rows)) >= 2
    lat = LatticeBatch.from_synth(lats, device=dev, **E.STAR_PACKINGS[i])
    assert int(lat.max_rows) == rows[i] and R.batch_groups(lat)[:2] == [1, 1]
    r, v = run(lat, theta, pos, T, dev)
    check(f"packing.{i}", lat, lats, r, v, refs, T)
    mine = out_bits(lat, lats, r, v)

    def bits_of(j):  # (run on demand, once per module: the comparison holds whichever cases are selected, in any order)
        lat_j = LatticeBatch.from_synth(lats, device=dev, **E.STAR_PACKINGS[j])
        return out_bits(lat_j, lats, *run(lat_j, theta, pos, T, dev))

    # against two fixed packings with different scratch rows: never against this run alone
    assert rows[PACKING_A] != rows[PACKING_B]
    for j in (PACKING_A, PACKING_B):
        other = cached(("packing bits", j), lambda: bits_of(j))
        for b in range(len(lats)):
            same_bits(other[b], mine[b], (j, i, b))


def test_snips_shaped_batch_with_and_without_chunked_programs(dev):
    lats = synth.snips_shaped_batch(4, vocab=250)
    T = max(R.min_max_len(l)[1] for l in lats)
    theta, pos = _inputs(lats, 320, T)
    plain = LatticeBatch.from_synth(lats).to(dev, auto_chunks=False)
    host = LatticeBatch.from_synth(lats)
    assert host.build_chunks(force=True)
    chunked = host.to(dev)
    assert chunked.chunks is not None and plain.chunks is None and plain.device.type == "cuda"
    refs = reference(plain, lats, theta, pos, T)
    r1, v1 = run(plain, theta, pos, T, dev)
    check("snips", plain, lats, r1, v1, refs, T)
    r2, v2 = run(chunked, theta, pos, T, dev)
    for b, (x, y) in enumerate(zip(out_bits(plain, lats, r1, v1), out_bits(chunked, lats, r2, v2))):
        same_bits(x, y, b)


# ----------------------------------------------------------------------------- (f) exponent range
@pytest.mark.parametrize("name", E.RANGE_CASES)
def test_exponent_range(dev, name):
    """|log Z| up to 2.6e5: what the (mantissa, exponent) pairs are for."""
    lats, theta, asc, pos, T = E.pos_range_inputs(name)
    lat = LatticeBatch.from_synth(lats, device=dev)
    refs = reference(lat, lats, theta, pos, T, asc)
    assert max(abs(x["logz"]) for x in refs) > E.RANGE_LOGZ[name]
    for x in refs:
        for p in (x["arc_post"], x["pos_post"]):
            assert np.sum((p > 0.01) & (p < 0.99)) >= E.SPREAD_MIN
    r, v = run(lat, theta, pos, T, dev, asc)
    assert all(torch.isfinite(x).all() for x in (r.logz64, r.logz, r.pos_posterior, r.arc_posterior, v.best))
    check(f"range.{name}", lat, lats, r, v, refs, T)


# ----------------------------------------------------------------------------- (g) limits
def _refused(fn):
    with pytest.raises(_lib.NfstError) as e:
        fn()
    assert e.value.code == -6
    torch.cuda.synchronize()


@pytest.mark.parametrize("over", [0, 1])
def test_row_limit(dev, over):
    """The most rows nfst_positional takes at vocabulary 256 (160 KiB of LDS to the byte), and one row more: refused
    on the host, while nfst_positional_viterbi still runs."""
    lats = E.pos_rowmax_batch(over)
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert E.pos_sum_lds(lat.max_rows, lat.vocab) == E.POS_LDS_LIMIT + 24 * over
    T = 53
    assert max(R.min_max_len(l)[1] for l in lats) == T
    theta, pos = _inputs(lats, 330 + over, T)
    refs = reference(lat, lats, theta, pos, T)
    t = lambda x: torch.from_numpy(x).to(dev)
    assert ops.positional_plan(lat, True)[1] is False
    v = ops.positional_viterbi(lat, t(theta), t(pos), T=T, pad=PAD)
    check_vit(f"rows+{over}", lat, lats, v, refs, T)
    fb = lambda: ops.positional_forward_backward(lat, t(theta), t(pos), T=T, want_pos_posterior=True, want_arc_posterior=True, want_len=True)
    if over:
        _refused(lambda: ops.positional_plan(lat, False))
        _refused(fb)
        _refused(lambda: ops.positional_forward_backward(lat, t(theta), t(pos), T=T, want_pos_posterior=False))
    else:
        assert ops.positional_plan(lat, False) == (E.POS_LDS_LIMIT, False)
        check_sum("rows+0", lat, lats, fb(), refs, T)


@pytest.mark.parametrize("over", [0, 1, "max"])
def test_vocabulary_limit(dev, over):
    """13 rows: vocabulary 7 970 is the last nfst_positional takes; nfst_positional_viterbi runs up to NFST_MAX_VOCAB,
    where a staged record carries a label in bits 16 .. 30."""
    V = E.POS_WIDE_VOCAB if over == "max" else E.pos_vocab_limit(13) + over
    lats = [E.pos_wide(V)]
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert lat.max_rows == 13 and V == {0: 7970, 1: 7971, "max": 32767}[over]
    T = 6
    theta, pos = _inputs(lats, 340, T)
    refs = reference(lat, lats, theta, pos, T)
    t = lambda x: torch.from_numpy(x).to(dev)
    assert ops.positional_plan(lat, True)[1] is True
    v = ops.positional_viterbi(lat, t(theta), t(pos), T=T, pad=PAD)
    check_vit(f"vocab.{over}", lat, lats, v, refs, T)
    if over == "max":
        assert lats[0].label.max() >= 1 << 14
    fb = lambda: ops.positional_forward_backward(lat, t(theta), t(pos), T=T, want_pos_posterior=True, want_arc_posterior=True, want_len=True)
    if over:
        _refused(fb)
    else:
        assert ops.positional_plan(lat, False)[1] is False
        check_sum("vocab.0", lat, lats, fb(), refs, T)


# ----------------------------------------------------------------------------- (h) truncation extremes
@pytest.mark.parametrize("T", [1, 9, 90])
def test_truncation_extremes(dev, T):
    """A single-arc lattice beside paths of up to 90 arcs: one position, a truncation that cuts most lattices, all of it."""
    lats = E.mixed_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta, pos = _inputs(lats, 350 + T, T)
    refs = reference(lat, lats, theta, pos, T)
    live = [bool(np.isfinite(x["logz"])) for x in refs]
    assert live == {1: [False] * 5 + [True], 9: [True, True, False, False, True, True], 90: [True] * 6}[T]
    r, v = run(lat, theta, pos, T, dev)
    check(f"trunc.{T}", lat, lats, r, v, refs, T)


# ----------------------------------------------------------------------------- (i) exact ties on the walk
@pytest.mark.parametrize("name", sorted(E.POS_TIE_SEED))
def test_exact_ties(dev, name):
    """Scores on the 0.25 grid: float32 sums are exact and candidates tie bit for bit, so "the smallest canonical arc"
    decides the path (tests/test_positional_cpu.py: it does, on the walked path of these inputs)."""
    lats, theta, asc, pos, T = E.pos_tie_inputs(name)
    opts = E.tie_cases()[name][3]
    lat = LatticeBatch.from_synth(lats, device=dev, **opts)
    refs = reference(lat, lats, theta, pos, T, asc)
    assert sum(max(x["mp"]["ties"]) >= 2 for x in refs) >= E.POS_TIE_LATTICES[name]
    r, v = run(lat, theta, pos, T, dev, asc)
    check(f"ties.{name}", lat, lats, r, v, refs, T)

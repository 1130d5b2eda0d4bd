"""The gradient of ops.string_log_prob (nfst_string_logprob_grad) against the NumPy restatement of
tests/strings_grad_ref.py, which tests/test_strings_grad_cpu.py holds to brute force over every path and to central
differences: grad_arc within BOUND, exact zeros where the entry point promises them, the same bits at every launch, under
every packing and slicing; the theta gradient, the product route and the log Z term by the tolerances of the ops they are
compared with.  The largest error of every kind goes to strings_grad_errors.json in the directory of run outputs
(profiles/README.md)."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from nfst_amd import _lib, ops, strings, synth
from nfst_amd.constraints import WideDFA
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from tests import edge_cases as E
from tests import pack_cases as PC
from tests import strings_grad_ref as GR
from tests import strings_ref as SR
from tests import structure_cases as S
from tests.test_lattice_edit_cpu import small_lattices

pytestmark = pytest.mark.gpu
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
NEG = -np.inf
MARK = SR.MARK
# The largest absolute error of grad_arc against strings_grad_ref over this module's cases, measured on the MI355X, is
# 2.3e-15 (profiles/strings_grad_errors.json, "structure grad_arc"); x 16 for the exp / log of two libraries differing by
# a few ulp per cell over the depth of two sweeps, rounded up to a power of ten.  Measured against the restatement, never
# against a second GPU run.
BOUND = 1e-13
BRUTE = 1e-12     # the restatement against brute force (tests/test_strings_grad_cpu.py)
POSTERIOR = 2e-6  # ops.forward_backward's float32 arc posteriors (tests/test_gpu_structure.py "fb posterior", tests/test_gpu_epilogue.py)
PRODUCT = 1e-5    # per product arc that an entry's gradient sums (tests/test_gpu_intersect_wide.py: "each held to 1e-5")

_ERR = {}


def rec(tag, err):
    _ERR[tag] = max(_ERR.get(tag, 0.0), float(err))
    print(f"{tag}: {float(err):.3g}")
    return float(err)


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for out in sorted(glob.glob(os.path.join(root, "*_out"))):
        if _ERR and os.path.isdir(out):
            with open(os.path.join(out, "strings_grad_errors.json"), "w") as f:
                json.dump(dict(sorted(_ERR.items())), f, indent=1)


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _cand_rows(cands, N=None, tail=8):
    """(strings [B, M, N] int32 with every row's tail filled with ``tail``, lengths [B, M])"""
    n = np.array([[len(y) for y in row] for row in cands], np.int32).reshape(len(cands), -1)
    out = np.full((len(cands), n.shape[1], max(1, int(n.max(initial=0)) if N is None else N)), tail, np.int32)
    for b, row in enumerate(cands):
        for m, y in enumerate(row):
            out[b, m, :len(y)] = y
    return out, n


def _launch(lat, theta, rows, n, tape, dev, g_num, g_z, asc=None, max_workspace_bytes=1 << 30):
    """The entry point through the wrapper's slicing, without its read-back of the status: (grad_arc, status)"""
    c = strings._candidates(lat, _t(rows, dev), _t(n, dev), tape.get("keep"), tape.get("marker"), max_workspace_bytes)
    sc, alive = ops._scores(lat, _t(np.asarray(theta, np.float32), dev), _t(asc, dev))
    grad, status = strings._grad_launches(c, sc, _t(np.asarray(g_num, np.float64).reshape(rows.shape[:2]), dev), _t(np.asarray(g_z, np.float64), dev))
    del alive
    return grad.cpu().numpy(), int(status.item())


def _grad(lat, theta, cands, tape, dev, g_num, g_z, asc=None, N=None, **kw):
    rows, n = _cand_rows(cands, N)
    got, status = _launch(lat, theta, rows, n, tape, dev, g_num, g_z, asc, **kw)
    assert status == 0 and got.dtype == np.float64 and got.shape == (lat.total_arcs,) and not np.isnan(got).any()
    return got


def _hold(tag, got, want, bound=None):
    """grad_arc against the restatement: zeros exactly where it has them, everything else within BOUND"""
    assert got.shape == want.shape, tag
    if got.size:
        assert not got[want == 0.0].any(), tag
        assert rec(f"{tag.split(':')[0]} grad_arc", np.abs(got - want).max()) <= (BOUND if bound is None else bound), tag


def _weights(shape, seed):
    """Upstream gradients in [-1, 1] with zeros and negative entries, whose magnitudes add up to at most 1 per lattice
    (so that an error of the posteriors is not scaled up)."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(-1.0, 1.0, size=shape)
    g[rng.random(shape) < 0.25] = 0.0
    if g.shape[-1] > 1:
        g[..., 1] = 0.0
    return g / np.maximum(np.abs(g).sum(axis=-1, keepdims=True), 1.0)


# ============================================================================= the graph
@pytest.fixture(scope="module")
def grids():
    """The denominator batch of tests/test_gpu_strings.py: three edit grids over 12 labels."""
    from tests import intersect_wide_ref as IW

    lats = [SR.denominator(SR.SEED1), SR.denominator(SR.SMALL), IW.edit_denominator([7, 6, 6, 8], [8, 9, 10], 2, vocab=12)]
    return lats, synth.label_scores(1, 12, mean=-1.0, std=0.5)


def test_results_carry_a_gradient(dev, grids):
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    rows, n = _cand_rows([[[8], [8, 9], []]] * 3)
    plain = ops.string_log_prob(lat, _t(theta, dev), _t(rows, dev), _t(n, dev), marker=MARK)
    assert not plain.log_prob.requires_grad and not plain.logz.requires_grad
    th = _t(theta, dev).requires_grad_()
    r = ops.string_log_prob(lat, th, _t(rows, dev), _t(n, dev), marker=MARK)
    assert r.log_prob.requires_grad and r.log_num.requires_grad and r.logz.requires_grad
    assert all(torch.equal(a, b.detach()) for a, b in zip(plain, r))  # the forward's bits
    asc = torch.zeros(lat.total_arcs, device=dev, requires_grad=True)
    r = ops.string_log_prob(lat, _t(theta, dev), _t(rows, dev), _t(n, dev), marker=MARK, arc_scores=asc)
    assert r.log_prob.requires_grad
    with torch.no_grad():
        assert not ops.string_log_prob(lat, th, _t(rows, dev), _t(n, dev), marker=MARK).log_prob.requires_grad


# ============================================================================= grad_arc against the restatement
@pytest.fixture(scope="module")
def long_grid():
    """The long grid of tests/test_gpu_strings.py: it spells every string over {8, 9} of up to 129 symbols, in both tape
    modes; 65 candidates (16 distinct ones), the lengths around the strips of 64 columns first."""
    from tests import intersect_wide_ref as IW

    l = IW.edit_denominator([6], [8, 9], 129, vocab=12)
    theta = synth.label_scores(4, 12, mean=-1.0, std=0.5)
    rng = np.random.default_rng(2)
    lens = [0, 1, 63, 64, 65, 128, 129] + [int(x) for x in rng.integers(0, 130, size=9)]
    pool = [[int(t) for t in rng.integers(8, 10, size=n)] for n in lens]
    return l, theta, [pool[i % 16] for i in range(65)], E.score64(l, theta)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128])
def test_strips(dev, long_grid, n):
    """N + 1 in {1, 2, 64, 65, 66, 129}: a strip, the strip boundary, three strips; the row stride is the length itself.
    Both tape modes (the kept labels are the symbols), and two launches give the same bits."""
    l, theta, cands, s64 = long_grid
    lat = LatticeBatch.from_synth([l], device=dev)
    y = cands[[0, 1, 63, 64, 65, 128].index(n)]
    assert len(y) == n
    for tape in (dict(marker=MARK), dict(keep={8, 9})):
        want = GR.grad_arc(l, s64, [y], [1.0], -0.5, **tape)
        got = _grad(lat, theta, [[y]], tape, dev, [[1.0]], [-0.5], N=max(n, 1))
        _hold(f"strips: n={n} {tape}", got, want)
        again = _grad(lat, theta, [[y]], tape, dev, [[1.0]], [-0.5], N=max(n, 1))
        assert np.array_equal(_bits(got), _bits(again))
        assert np.abs(want).max() > 0.1


@pytest.mark.parametrize("M", [1, 3, 65])
def test_candidates_of_different_lengths_in_one_launch(dev, long_grid, M):
    """Candidates of every length under one row stride, weighed by upstream gradients with zeros and negative entries;
    slices of one or two candidates (5 MiB of forward workspace) give the bits of the one launch."""
    l, theta, cands, s64 = long_grid
    lat = LatticeBatch.from_synth([l], device=dev)
    pick = list(range(65)) if M == 65 else [5, 0, 3][:M]
    ys = [cands[i] for i in pick]
    g_num, g_z = _weights((1, M), M), [0.25]
    assert M == 1 or ((g_num == 0).any() and (g_num < 0).any() and (g_num > 0).any())
    want = GR.grad_arc(l, s64, ys, g_num[0], g_z[0], marker=MARK)
    got = _grad(lat, theta, [ys], dict(marker=MARK), dev, g_num, g_z, N=130)
    _hold(f"mixed lengths: M={M}", got, want)
    sliced = _grad(lat, theta, [ys], dict(marker=MARK), dev, g_num, g_z, N=130, max_workspace_bytes=5 << 20)
    assert np.array_equal(_bits(got), _bits(sliced))
    if M == 3:
        with pytest.raises(ValueError, match="max_workspace_bytes"):
            _grad(lat, theta, [ys], dict(marker=MARK), dev, g_num, g_z, N=130, max_workspace_bytes=1 << 20)


def test_marker_corners(dev):
    """The seven-state lattice of the marker tape's corners: every string it spells and strings it does not, in one
    launch and one by one; a candidate that no path spells gives exact zeros."""
    l = SR.tape_lattice()
    theta = synth.label_scores(3, l.vocab, mean=-1.0, std=0.5)
    s64 = E.score64(l, theta)
    lat = LatticeBatch.from_synth([l], device=dev)
    num, pz, _, D = GR.brute_posteriors(l, s64, marker=MARK)
    assert D > 0 and any(MARK in y for y in num)  # (paths that end on a marker; a symbol that is the marker itself)
    spelled = sorted(num)
    others = [y for y in ([8, 8, 8], [MARK, MARK, MARK], [7], [9], [8, 9], list(spelled[-1]) + [9]) if tuple(y) not in num]
    assert len(others) >= 4
    ys = [list(y) for y in spelled] + others
    g_num = np.ones((1, len(ys)))
    got = _grad(lat, theta, [ys], dict(marker=MARK), dev, g_num, [0.0])
    _hold("marker corners: all", got, GR.grad_arc(l, s64, ys, g_num[0], 0.0, marker=MARK))
    assert rec("marker corners brute", np.abs(got - sum(num[y] for y in spelled)).max()) <= BOUND * len(ys) + BRUTE * len(ys)
    for y in spelled:
        one = _grad(lat, theta, [[list(y)]], dict(marker=MARK), dev, [[1.0]], [0.0])
        _hold("marker corners: one", one, GR.posteriors(l, s64, list(y), marker=MARK)[0])
    for y in others:
        assert not _grad(lat, theta, [[y]], dict(marker=MARK), dev, [[1.0]], [0.0]).any()
    # the -inf candidate passes zeros back through log_prob as well, and no NaN
    rows, n = _cand_rows([[others[0], list(spelled[0])]])
    th = _t(theta, dev).requires_grad_()
    r = ops.string_log_prob(lat, th, _t(rows, dev), _t(n, dev), marker=MARK)
    assert r.log_prob[0].isneginf().tolist() == [True, False]
    r.log_prob[0, 0].backward()
    assert not th.grad.any() and not th.grad.isnan().any()


def _enumerable():
    out = [(f"small{i}", l, 50 + i) for i, l in enumerate(small_lattices())]
    return out + [("seed1", SR.denominator(SR.SEED1), 1), ("grid2", SR.denominator(SR.SMALL), 2), ("tape", SR.tape_lattice(), 3)]


@pytest.mark.parametrize("case", range(7))
def test_every_string_of_an_enumerable_lattice(dev, case):
    """All distinct strings of a lattice and some that no path spells in one launch, weighed, against brute force over
    its paths: the share of every string's path weight through every arc."""
    name, l, seed = _enumerable()[case]
    theta = synth.label_scores(seed, l.vocab, mean=-1.0, std=0.5)
    s64 = E.score64(l, theta)
    lat = LatticeBatch.from_synth([l], device=dev)
    labels = sorted(set(int(x) for x in l.label))
    for tape in (dict(keep=set(labels[1::2]) | {EOS}), dict(marker=MARK if MARK in labels else labels[len(labels) // 2])):
        by, logz, _ = SR.brute_force(l, s64, **tape)
        num, pz, _, _ = GR.brute_posteriors(l, s64, **tape)
        ys = sorted(by, key=lambda y: -by[y])
        extra = [ys[0] + ys[0][-1:], ys[0][:-1], (), tuple(ys[-1]) + (labels[-1],) * 3]
        cands = [list(y) for y in ys + extra]
        g_num, g_z = _weights((1, len(cands)), seed), [0.5]
        want = g_z[0] * pz + sum(g * num[tuple(y)] for g, y in zip(g_num[0], cands) if tuple(y) in num)
        got = _grad(lat, theta, [cands], tape, dev, g_num, g_z)
        assert rec("enumerable brute", np.abs(got - want).max()) <= BOUND + 2 * BRUTE, (name, tape)  # (the weights' magnitudes add up to at most 1.5)
        _hold(f"enumerable: {name} {sorted(tape)}", got, GR.grad_arc(l, s64, cands, g_num[0], g_z[0], **tape))


NAMES = tuple(S.batches())


@pytest.mark.parametrize("name", NAMES)
def test_structure_corpus(dev, name):
    """The corpus of tests/structure_cases.py through both tape modes, with per-arc scores (and the tables' weights in the
    weighted batch): three weighed candidates per lattice -- the string of a path, the empty string, a string that no
    path spells -- against the restatement, and the same bits from both packers and under the three group modes."""
    lats = [S.canonical(l) for l in S.batches()[name]]
    Vb = lats[0].vocab
    theta = S.theta(Vb)
    A = sum(l.n_arcs for l in lats)
    asc = np.random.default_rng(3).normal(0.0, 0.4, size=A).astype(np.float32) if A else None
    n_rows, arc_off, src, label, dst, w = PC.batch_arcs(S.batches()[name])
    mark = 5
    for tape in (dict(keep=set(range(3, Vb, 2)) | {EOS}), dict(marker=mark)):
        cands = []
        for l in lats:
            first = np.searchsorted(l.src, np.arange(l.n_rows + 1))
            s, sink, labs = 0, S.sink(l), []
            while s != sink:  # the first arc out of every state that is no self loop
                a = next(a for a in range(int(first[s]), int(first[s + 1])) if l.dst[a] != s)
                labs.append(int(l.label[a]))
                s = int(l.dst[a])
            y = list(SR.project(labs, **tape))
            cands.append([y, [], y + [Vb - 1]])
        g_num = _weights((len(lats), 3), 7)
        g_num[:, 1] = 0.125  # (the empty string counts: the middle column of _weights is zero)
        g_num[::3, 0] = 0.0
        g_z = np.random.default_rng(8).uniform(-0.5, 0.5, size=len(lats))
        want = GR.of_batch(lats, theta, cands, g_num, g_z, asc=asc, **tape)
        first_bits = None
        for route, gm in (("host", 0), ("device", 0), ("host", 1), ("host", 2), ("device", 2)):
            if route == "host":
                lat = LatticeBatch.from_arcs(n_rows, arc_off, src, label, dst, Vb, arc_w=w, group_mode=gm).to(dev, auto_chunks=False)
            else:
                lat = LatticeBatch.from_arcs_device(n_rows, arc_off, src, label, dst, Vb, arc_w=w, device=dev, group_mode=gm)
            got = _grad(lat, theta, cands, tape, dev, g_num, g_z, asc=asc)
            if first_bits is None:
                _hold(f"structure: {name} {sorted(tape)}", got, want)
                first_bits = got
            assert np.array_equal(_bits(got), _bits(first_bits)), (name, route, gm)
        a0 = 0
        for l in lats:  # a self loop lies on no path
            assert not first_bits[a0:a0 + l.n_arcs][np.asarray(l.src) == np.asarray(l.dst)].any()
            a0 += l.n_arcs
        assert A == 0 or np.abs(want).max() > 0.01
    assert name != "zero_arcs" or any(l.n_arcs == 0 for l in lats)  # (lattices without an arc are part of the corpus)


# ============================================================================= theta, log Z and the product route
def _autograd(lat, theta_t, rows, n, tape, dev, g_num, g_z, asc_t=None):
    """(d theta, d arc_scores) of sum g_num log_num + sum g_z logz through ops.string_log_prob"""
    r = ops.string_log_prob(lat, theta_t, _t(rows, dev), _t(n, dev), arc_scores=asc_t, **tape)
    inputs = [theta_t] + ([] if asc_t is None else [asc_t])
    return torch.autograd.grad([r.log_num, r.logz], inputs, [_t(np.asarray(g_num, np.float64), dev), _t(np.asarray(g_z, np.float64), dev)])


@pytest.mark.parametrize("per_lattice", [False, True])
def test_theta_gradient_is_grad_arc_summed_per_label(dev, grids, per_lattice):
    """theta [V] shared and [B, V] per lattice, float64 (the kernels read it as float32; its gradient comes back in its
    dtype): grad_arc summed per label.  index_add_ adds in any order: at most 2^-53 x the terms of an entry (below 2000)
    x the sum of their magnitudes (the upstream weights, at most 1.5 per lattice, x the length of a path, below 20) <
    1e-11; the float32 theta gets the same sums rounded once more."""
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    B, V = 3, 12
    if per_lattice:
        theta = np.stack([synth.label_scores(1 + b, V, mean=-1.0, std=0.5) for b in range(B)])
    cands = [[[8], [8, 9], [], [9, 8]]] * B
    rows, n = _cand_rows(cands)
    g_num, g_z = _weights((B, 4), 11), np.array([0.5, -0.25, 0.125])
    asc = torch.zeros(lat.total_arcs, dtype=torch.float64, device=dev, requires_grad=True)
    th = _t(theta.astype(np.float64), dev).requires_grad_()
    d_theta, d_arc = _autograd(lat, th, rows, n, dict(marker=MARK), dev, g_num, g_z, asc)
    raw = _grad(lat, theta, cands, dict(marker=MARK), dev, g_num, g_z)
    assert d_arc.dtype == torch.float64 and np.array_equal(_bits(d_arc.cpu().numpy()), _bits(raw))  # grad_arc itself
    want, a0 = np.zeros((B, V)), 0
    for b, l in enumerate(lats):
        want[b] = np.bincount(l.label, weights=raw[a0:a0 + l.n_arcs], minlength=V)
        a0 += l.n_arcs
    want = want if per_lattice else want.sum(axis=0)
    assert d_theta.dtype == torch.float64 and tuple(d_theta.shape) == want.shape
    assert rec("theta per label", np.abs(d_theta.cpu().numpy() - want).max()) <= 1e-11 and np.abs(want).max() > 0.01
    th32 = _t(theta.astype(np.float32), dev).requires_grad_()
    (d32,) = _autograd(lat, th32, rows, n, dict(marker=MARK), dev, g_num, g_z)
    assert d32.dtype == torch.float32 and tuple(d32.shape) == want.shape
    assert np.all(np.abs(d32.cpu().numpy() - want) <= 1e-11 + 2.0 ** -24 * np.abs(want))


def test_the_log_z_term_is_the_arc_posterior(dev, grids):
    """Without candidates (M = 0) and with zero upstream gradients on them, grad_arc under g_z = 1 is the arc posterior
    of ops.forward_backward, held to that op's float32 bound of 2e-6 (tests/test_gpu_structure.py, "fb posterior")."""
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    post = ops.forward_backward(lat, _t(theta, dev)).posterior.double().cpu().numpy()
    none = _grad(lat, theta, [[]] * 3, dict(marker=MARK), dev, np.zeros((3, 0)), np.ones(3), N=1)
    zero = _grad(lat, theta, [[[8], [8, 9]]] * 3, dict(marker=MARK), dev, np.zeros((3, 2)), np.ones(3))
    assert np.array_equal(_bits(none), _bits(zero))
    on = np.concatenate([np.asarray(l.src) != np.asarray(l.dst) for l in lats])  # (a self loop: 0 here, the engine's convention there)
    assert rec("log Z term posterior", np.abs(none - post)[on].max()) <= POSTERIOR and not none[~on].any()
    _hold("log Z term: restatement", none, GR.of_batch(lats, theta, [[]] * 3, np.zeros((3, 0)), np.ones(3), marker=MARK))


def test_agreement_with_the_product_route(dev, grids):
    """Where the product fits, the gradients of log_prob in theta and arc_scores are those of
    ``ops.constraint_log_prob`` on ``WideDFA.marked_sequence``: an entry of that gradient sums the posteriors of n arcs
    of the product and of the lattice, each held to 1e-5 (tests/test_gpu_intersect_wide.py)."""
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    ys = [[8], [8, 9], [], [9, 8]]
    rows, n = _cand_rows([ys] * 3)
    lat_label = lat.arc_label.cpu().numpy()
    for m, y in enumerate(ys):
        th, asc = _t(theta, dev).requires_grad_(), torch.zeros(lat.total_arcs, device=dev, requires_grad=True)
        ops.string_log_prob(lat, th, _t(rows[:, m:m + 1], dev), _t(n[:, m:m + 1], dev), marker=MARK, arc_scores=asc).log_prob.sum().backward()
        th2, asc2 = _t(theta, dev).requires_grad_(), torch.zeros(lat.total_arcs, device=dev, requires_grad=True)
        dfa = WideDFA.marked_sequence(12, MARK, y)
        ops.constraint_log_prob(lat, th2, dfa, arc_scores=asc2).sum().backward()
        res = ops.intersect(lat, dfa)
        n_arc = 1 + np.bincount(res.arc_map.cpu().numpy(), minlength=lat.total_arcs)  # the arc itself and its copies in the product
        n_lab = np.bincount(lat_label, minlength=12) + np.bincount(res.lattice.arc_label.cpu().numpy(), minlength=12)
        on = np.concatenate([np.asarray(l.src) != np.asarray(l.dst) for l in lats])  # (a self loop lies on no path; its gradient
        lab_on = np.bincount(lat_label[~on], minlength=12) == 0                         # there is the engine's convention, as its label's)
        d_arc = np.abs(asc.grad.cpu().numpy() - asc2.grad.cpu().numpy())
        d_th = np.abs(th.grad.cpu().numpy() - th2.grad.cpu().numpy())
        rec("product route arc_scores", (d_arc / n_arc)[on].max())
        rec("product route theta", (d_th / np.maximum(n_lab, 1))[lab_on].max())
        assert np.all(d_arc[on] <= PRODUCT * n_arc[on]) and np.all((d_th <= PRODUCT * np.maximum(n_lab, 1))[lab_on]), y
        assert lab_on.sum() >= 8
        assert float(asc.grad.abs().max()) > 0.1


def test_beyond_the_row_limit(dev):
    """The 1200-state lattice whose product with the string's automaton does not fit: ``intersect`` refuses it, the
    gradient from the lattice alone is the restatement's, and the posteriors of the out-arcs of state 0 add up to 1."""
    l, keep, y = SR.layered_case()
    theta = synth.label_scores(2, 12)
    lat = LatticeBatch.from_synth([l], device=dev)
    with pytest.raises(_lib.NfstError) as e:
        ops.intersect(lat, WideDFA.projected_sequence(12, keep, y))
    assert e.value.code == -6  # NFST_ERR_LIMIT
    s64 = E.score64(l, theta)
    got = _grad(lat, theta, [[y, y[:-1], y + [3]]], dict(keep=keep), dev, [[1.0, 0.0, 0.5]], [-1.0])
    _hold("row limit: layered", got, GR.grad_arc(l, s64, [y, y[:-1], y + [3]], [1.0, 0.0, 0.5], -1.0, keep=keep))
    rows, n = _cand_rows([[y]])
    post = ops.string_arc_posteriors(lat, _t(theta, dev), _t(rows, dev), _t(n, dev), keep=keep)
    assert post.dtype == torch.float64 and tuple(post.shape) == (lat.total_arcs,)
    out0 = np.asarray(l.src) == 0
    assert rec("row limit: out-arcs of state 0", abs(float(post.cpu().numpy()[out0].sum()) - 1.0)) <= BOUND * int(out0.sum())
    _hold("row limit: posteriors", post.cpu().numpy(), GR.posteriors(l, s64, y, keep=keep)[0])


def test_a_bad_length_leaves_the_other_candidates(dev, grids):
    """A length outside [0, N] sets the status word and takes its candidate out: the bits are those of the same launch
    with a good length and a zero upstream gradient there.  The wrappers raise."""
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    rows, n = _cand_rows([[[8], [8, 9], []]] * 3, N=4)
    g_num, g_z = np.array([[0.5, -0.25, 0.125]] * 3), np.array([0.5, 0.25, -0.5])
    bad_n, g_off = n.copy(), g_num.copy()
    bad_n[1, 0], bad_n[2, 2] = 5, -1
    g_off[1, 0] = g_off[2, 2] = 0.0
    good, status = _launch(lat, theta, rows, n, dict(marker=MARK), dev, g_off, g_z)
    assert status == 0
    bad, status = _launch(lat, theta, rows, bad_n, dict(marker=MARK), dev, g_num, g_z)
    assert status == _lib.ERR_LENGTH and np.array_equal(_bits(bad), _bits(good)) and not np.isnan(bad).any()
    for call in (lambda: ops.string_arc_posteriors(lat, _t(theta, dev), _t(rows[:, :1], dev), _t(bad_n[:, :1], dev), marker=MARK),
                 lambda: ops.string_log_prob(lat, _t(theta, dev).requires_grad_(), _t(rows, dev), _t(bad_n, dev), marker=MARK)):
        with pytest.raises(_lib.NfstError) as e:
            call()
        assert e.value.code == _lib.ERR_LENGTH


def test_want_arc_grad(dev, grids):
    """``want_arc_grad=True`` changes no value and leaves the float64 gradient of the arcs' scores on ``arc_offsets``,
    with and without ``arc_scores``, whose own gradient is the same numbers in its dtype."""
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    rows, n = _cand_rows([[[8], [8, 9]]] * 3)
    g_num, g_z = _weights((3, 2), 5) + 0.25, np.array([0.5, -0.25, 0.125])
    asc_np = np.random.default_rng(4).normal(0.0, 0.4, size=lat.total_arcs).astype(np.float32)
    for asc in (None, asc_np):
        plain = ops.string_log_prob(lat, _t(theta, dev), _t(rows, dev), _t(n, dev), marker=MARK, arc_scores=_t(asc, dev))
        assert not hasattr(plain, "arc_offsets")
        a = None if asc is None else _t(asc, dev).requires_grad_()
        r = ops.string_log_prob(lat, _t(theta, dev), _t(rows, dev), _t(n, dev), marker=MARK, arc_scores=a, want_arc_grad=True)
        assert isinstance(r, ops.StringScores) and all(torch.equal(x, y.detach()) for x, y in zip(plain, r))
        torch.autograd.backward([r.log_num, r.logz], [_t(g_num, dev), _t(g_z, dev)])
        raw = _grad(lat, theta, [[[8], [8, 9]]] * 3, dict(marker=MARK), dev, g_num, g_z, asc=asc)
        got = r.arc_offsets.grad
        assert got.dtype == torch.float64 and np.array_equal(_bits(got.cpu().numpy()), _bits(raw))
        assert a is None or (a.grad.dtype == torch.float32 and torch.equal(a.grad, got.float()))


def test_scorer_entries(dev, grids):
    lats, theta = grids
    em, tr = synth.collate_dense([l.dense() for l in lats])
    sc = LatticeScorer(12, pad=PAD, bos=BOS, eos=EOS, theta=torch.from_numpy(theta)).to(dev)
    sc.set_masks(torch.as_tensor(em).to(dev), torch.as_tensor(tr).to(dev))
    lat = sc._lat()
    rows, n = _cand_rows([[[8]], [[8, 9]], [[]]])
    nll = sc.string_nll(_t(rows, dev), _t(n, dev), marker=MARK)
    assert nll.dtype == torch.float64 and nll.requires_grad and float(nll.detach()) > 0
    nll.backward()
    lp = sc.string_log_prob(_t(rows, dev), _t(n, dev), marker=MARK)
    assert lp.requires_grad and float((nll.detach() + lp.detach().mean()).abs()) == 0.0
    # d nll / d theta = (posterior label counts among all paths - among the string's paths) / B
    post = ops.string_arc_posteriors(lat, sc.theta.detach(), _t(rows, dev), _t(n, dev), marker=MARK)
    allp = _t(_grad(lat, theta, [[]] * 3, dict(marker=MARK), dev, np.zeros((3, 0)), np.ones(3), N=1), dev)
    want = torch.zeros(12, dtype=torch.float64, device=dev).index_add_(0, lat.arc_label.to(torch.int64), allp - post) / 3
    assert sc.theta.grad is not None and sc.theta.grad.dtype == torch.float32
    assert rec("scorer nll theta", float((sc.theta.grad.double() - want).abs().max())) <= 1e-11 + 2.0 ** -24 * float(want.abs().max())
    assert float(sc.theta.grad.abs().max()) > 0.01
    with pytest.raises(ValueError, match="probability 0"):
        sc.string_nll(_t(np.full((3, 1, 3), 8, np.int32), dev), _t(np.full((3, 1), 3, np.int32), dev), marker=MARK)
    # string_arc_posteriors is autograd with a one-hot upstream gradient: the same bits
    asc = torch.zeros(lat.total_arcs, dtype=torch.float64, device=dev, requires_grad=True)
    r = ops.string_log_prob(lat, sc.theta.detach(), _t(rows, dev), _t(n, dev), marker=MARK, arc_scores=asc)
    (g,) = torch.autograd.grad(r.log_num.sum(), asc)
    assert torch.equal(g, post) and abs(float(post.sum())) > 1

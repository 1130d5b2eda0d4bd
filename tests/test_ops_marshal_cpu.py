"""The marshalling and gradient-assembly helpers of nfst_amd/ops.py on the host: the backward
passes of the ops are these pure functions, so plain loops over a host-packed batch check what otherwise only runs behind
a GPU forward; and the public surface of ``ops`` is pinned to the list taken from the commit before the helpers."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from nfst_amd import _lib, ops, synth
from nfst_amd.lattice import LatticeBatch
from tests import edge_cases as E

V = 12
BOS, EOS = synth.BOS, synth.EOS
K = 3


# ----------------------------------------------------------------------------- _path_score_grads
def _kbest_backward_before(lat, arcs, g, theta_like, asc_like):
    """``_KBest.backward`` as it stood before ``_path_score_grads`` (both gradients wanted), statement by statement."""
    B, K, T = arcs.shape
    a = arcs.reshape(B, K * T).to(torch.int64)
    on = a >= 0
    gg = torch.where(torch.isfinite(g), g, torch.zeros_like(g)).to(torch.float32)
    w = gg[:, :, None].expand(B, K, T).reshape(B, K * T)[on]
    idx = a[on]
    f32 = dict(dtype=torch.float32, device=arcs.device)
    d_arc = torch.zeros(lat.total_arcs, **f32).index_add_(0, idx, w)
    d_arc = d_arc.to(dtype=asc_like.dtype, device=asc_like.device)
    lab = lat.arc_label.to(torch.int64)[idx]
    V = lat.vocab
    if theta_like.dim() == 1:
        d_theta = torch.zeros(V, **f32).index_add_(0, lab, w)
    else:
        row = torch.arange(B, device=arcs.device)[:, None].expand(B, K * T)[on]
        d_theta = torch.zeros(B * V, **f32).index_add_(0, row * V + lab, w).view(B, V)
    d_theta = d_theta.to(dtype=theta_like.dtype, device=theta_like.device)
    return d_theta, d_arc


@pytest.fixture(scope="module")
def paths():
    """(lat, arcs [2, 3, T] int32, g [2, 3], labels of the canonical arcs): the three best paths of a lattice of 8 states
    and the only path of a chain of two arcs (its other two rows are all -1), T = the longest path + 1."""
    lats = [synth.layered_lattice(21, n_states=7, avg_degree=2.5, vocab=V, width=2, span=2),
            synth._finish(3, V, [0, 1], [BOS, EOS], [1, 2])]
    assert max(l.n_rows for l in lats) <= 8
    lat = LatticeBatch.from_synth(lats)
    label = np.concatenate([l.label for l in lats])
    assert np.array_equal(lat.arc_label.numpy(), label)  # (the canonical order is the lattices' own, one after the other)
    theta = E.quarter(np.random.default_rng(5).normal(-1.0, 0.8, size=V))
    refs = E.kbest_refs(lats, theta, k=K)
    assert refs[0]["n_paths"] == K and refs[1]["n_paths"] == 1
    T = max(len(p) for r in refs for p in r["arcs"]) + 1
    arcs = np.full((2, K, T), -1, np.int32)
    for b, (r, sl) in enumerate(zip(refs, E.arc_slices(lats))):
        for j, p in enumerate(r["arcs"]):
            arcs[b, j, :len(p)] = np.asarray(p) + sl.start
    assert (arcs[:, :, -1] == -1).all() and (arcs[1, 1:] == -1).all() and (arcs[1, 0, 2:] == -1).all() and T > 3  # padded tails
    g = np.array([[2.0, -3.0, 5.0], [4.0, -np.inf, np.nan]], np.float32)  # (integers: every sum is exact)
    return lat, torch.from_numpy(arcs), torch.from_numpy(g), label


def _loops(arcs, g, label, A):
    B, K, T = arcs.shape
    d_arc, d_th, d_thb = np.zeros(A, np.float32), np.zeros(V, np.float32), np.zeros((B, V), np.float32)
    d_pos, d_posb = np.zeros((T, V), np.float32), np.zeros((B, T, V), np.float32)
    for b in range(B):
        for j in range(K):
            for t in range(T):
                a = int(arcs[b, j, t])
                if a < 0:
                    continue
                w = np.float32(g[b, j])
                d_arc[a] += w
                d_th[label[a]] += w
                d_thb[b, label[a]] += w
                d_pos[t, label[a]] += w
                d_posb[b, t, label[a]] += w
    return d_arc, d_th, d_thb, d_pos, d_posb


def test_path_score_grads_equal_a_plain_loop(paths):
    lat, arcs, g, label = paths
    B, _, T = arcs.shape
    A = lat.total_arcs
    d_arc, d_th, d_thb, d_pos, d_posb = _loops(arcs.numpy(), g.numpy(), label, A)
    assert np.isfinite(d_arc).all() and d_arc.any() and d_posb.any()
    for th_like, want_th in ((torch.zeros(V), d_th), (torch.zeros(B, V), d_thb)):
        for pos_like, want_pos in ((torch.zeros(T, V), d_pos), (torch.zeros(B, T, V), d_posb)):
            got_th, got_arc, got_pos = ops._path_score_grads(lat, arcs, g, th_like, torch.zeros(A), pos_like)
            assert np.array_equal(got_arc.numpy(), d_arc)
            assert np.array_equal(got_th.numpy(), want_th)
            assert np.array_equal(got_pos.numpy(), want_pos)
            assert got_th.dtype == got_arc.dtype == got_pos.dtype == torch.float32


def test_path_score_grads_take_the_dtype_of_the_inputs_and_skip_what_is_not_asked(paths):
    lat, arcs, g, label = paths
    B, _, T = arcs.shape
    f64 = dict(dtype=torch.float64)
    got = ops._path_score_grads(lat, arcs, g, torch.zeros(B, V, **f64), torch.zeros(lat.total_arcs, **f64), torch.zeros(T, V, **f64))
    want = _loops(arcs.numpy(), g.numpy(), label, lat.total_arcs)
    for x, w in zip(got, (want[2], want[0], want[3])):
        assert x.dtype == torch.float64 and np.array_equal(x.numpy(), w.astype(np.float64))
    assert ops._path_score_grads(lat, arcs, g) == (None, None, None)
    only_pos = ops._path_score_grads(lat, arcs, g, pos_like=torch.zeros(T, V))
    assert only_pos[0] is None and only_pos[1] is None and np.array_equal(only_pos[2].numpy(), want[3])


def test_path_score_grads_without_positions_are_the_k_best_backward_of_before(paths):
    lat, arcs, g, _ = paths
    B = arcs.shape[0]
    for th_like in (torch.zeros(V), torch.zeros(B, V), torch.zeros(B, V, dtype=torch.float64)):
        asc_like = torch.zeros(lat.total_arcs, dtype=th_like.dtype)
        want_th, want_arc = _kbest_backward_before(lat, arcs, g, th_like, asc_like)
        got_th, got_arc, got_pos = ops._path_score_grads(lat, arcs, g, th_like, asc_like)
        assert got_pos is None
        for got, want in ((got_th, want_th), (got_arc, want_arc)):
            assert got.dtype == want.dtype and got.shape == want.shape and got.device == want.device and torch.equal(got, want)


# ----------------------------------------------------------------------------- _per_label, _per_position, _per_arc
@pytest.fixture(scope="module")
def three():
    lats = [synth.layered_lattice(30 + s, n_states=6 + s, avg_degree=2.0, vocab=V, width=2, span=2) for s in range(3)]
    return lats, LatticeBatch.from_synth(lats)


def _ints(rng, *shape):
    return rng.integers(-4, 5, size=shape).astype(np.float32)  # (integers: the sum over the batch is exact)


def test_per_label_and_per_position_equal_loops():
    rng = np.random.default_rng(2)
    B, T = 3, 4
    g, x, y = _ints(rng, B), _ints(rng, B, V), _ints(rng, B, T, V)
    want_l, want_p = np.zeros((B, V), np.float32), np.zeros((B, T, V), np.float32)
    for b in range(B):
        for v in range(V):
            want_l[b, v] = x[b, v] * g[b]
            for t in range(T):
                want_p[b, t, v] = y[b, t, v] * g[b]
    gt, xt, yt = torch.from_numpy(g), torch.from_numpy(x), torch.from_numpy(y)
    assert np.array_equal(ops._per_label(xt, gt, False).numpy(), want_l)
    assert np.array_equal(ops._per_label(xt, gt, True).numpy(), want_l[0] + want_l[1] + want_l[2])  # a shared table: the batch's sum
    per = ops._per_position(yt, gt, torch.zeros(B, T, V))
    shared = ops._per_position(yt, gt, torch.zeros(T, V, dtype=torch.float64))
    assert per.dtype == torch.float32 and np.array_equal(per.numpy(), want_p)
    assert shared.dtype == torch.float64 and np.array_equal(shared.numpy(), (want_p[0] + want_p[1] + want_p[2]).astype(np.float64))


def test_per_arc_equals_a_loop(three):
    lats, lat = three
    rng = np.random.default_rng(3)
    g, x = _ints(rng, 3), _ints(rng, lat.total_arcs)
    want = np.zeros(lat.total_arcs, np.float32)
    for b, sl in enumerate(E.arc_slices(lats)):
        for a in range(sl.start, sl.stop):
            want[a] = x[a] * g[b]
    assert np.array_equal(ops._per_arc(lat, torch.from_numpy(x), torch.from_numpy(g)).numpy(), want)
    assert np.array_equal(ops._arc_grad(lat, torch.from_numpy(g)).numpy(), np.concatenate([np.full(l.n_arcs, g[b]) for b, l in enumerate(lats)]))


# ----------------------------------------------------------------------------- argument helpers
def test_check_k():
    assert ops.MAX_K == 64
    ops._check_k(1)
    ops._check_k(ops.MAX_K)
    ops._check_k(1000, bounded=False)
    for bad, shown in ((0, "0"), (65, "65"), (True, "True"), (1.0, "1.0"), ("3", "'3'")):
        with pytest.raises(ValueError) as e:
            ops._check_k(bad)
        assert str(e.value) == f"k must be an int in [1, 64], not {shown}"
    for bad, shown in ((0, "0"), (-2, "-2"), (True, "True"), (1.0, "1.0"), ("3", "'3'")):
        with pytest.raises(ValueError) as e:
            ops._check_k(bad, bounded=False)
        assert str(e.value) == f"k must be an int >= 1, not {shown}"


def test_workspace_on_a_host_batch(three):
    _, lat = three
    with pytest.raises(_lib.NfstError, match="nfst_kbest_ws_bytes"):
        ops._workspace(lat, "nfst_kbest_ws_bytes", 65)
    ws, n = ops._workspace(lat, "nfst_kbest_ws_bytes", 3)
    assert n == _lib.lib.nfst_kbest_ws_bytes(C.byref(lat.c_struct()), 3) and n > 0
    assert ws.dtype == torch.uint8 and ws.device == lat.device and ws.numel() == max(n, 16) >= 16


def test_path_outputs_and_default_length(three):
    _, lat = three
    B, L = lat.n_lattices, int(lat.depth.max()) + 1
    assert ops._max_len(lat, None) == L and ops._max_len(lat, 5) == 5
    best, paths_, arcs, lens, n_paths, logq = ops._path_outputs(lat, (B,), L, best=True)
    assert (best.shape, paths_.shape, arcs.shape, lens.shape, n_paths, logq) == ((B,), (B, L), (B, L), (B,), None, None)
    assert (best.dtype, paths_.dtype, arcs.dtype, lens.dtype) == (torch.float32, torch.int32, torch.int32, torch.int32)
    best, paths_, arcs, lens, n_paths, logq = ops._path_outputs(lat, (B, 4), 7, arcs=False, n_paths=True, logq=True)
    assert best is None and arcs is None and paths_.shape == (B, 4, 7) and lens.shape == (B, 4) and n_paths.shape == (B,)
    assert (lens.dtype, n_paths.dtype, logq.dtype, logq.shape) == (torch.int32, torch.int32, torch.float32, (B, 4))


def test_score_args_checks_in_order_and_detaches(three):
    _, lat = three
    B, A = lat.n_lattices, lat.total_arcs
    theta = torch.zeros(B, V, dtype=torch.float64, requires_grad=True)
    asc, pos = torch.zeros(A, requires_grad=True), torch.zeros(B, 4, V)
    sc, keep, p, stride, T = ops._score_args(lat, theta, asc, pos, None)
    assert (sc.theta, sc.theta_stride, sc.arc_scores) == (keep[0].data_ptr(), V, keep[1].data_ptr())
    assert keep[0].dtype == torch.float32 and not keep[0].requires_grad and not keep[1].requires_grad
    assert (stride, T) == (4 * V, 4) and p.data_ptr() == pos.data_ptr()
    assert ops._score_args(lat, torch.zeros(V), None)[2:] == (None, 0, int(lat.depth.max()))
    with pytest.raises(ValueError, match="^theta must be"):
        ops._score_args(lat, torch.zeros(V + 1), torch.zeros(A + 1), torch.zeros(4, V + 1), 0)
    with pytest.raises(ValueError, match="^arc_scores must be"):
        ops._score_args(lat, torch.zeros(V), torch.zeros(A + 1), torch.zeros(4, V + 1), 0)
    with pytest.raises(ValueError, match="^T must be"):
        ops._score_args(lat, torch.zeros(V), torch.zeros(A), torch.zeros(4, V + 1), 0)
    with pytest.raises(ValueError, match="^pos_scores must be"):
        ops._score_args(lat, torch.zeros(V), torch.zeros(A), torch.zeros(4, V + 1), None)


def test_call_marshals_tensors_nulls_and_the_stream(three, monkeypatch):
    _, lat = three
    seen = []

    class Lib:
        def nfst_fake(self, *args):
            seen.append(args)
            return 0

        def nfst_fails(self, *args):
            return -1

        nfst_strerror = staticmethod(_lib.lib.nfst_strerror)

    monkeypatch.setattr(ops, "lib", Lib())
    monkeypatch.setattr(ops, "_stream", lambda: 1234)
    x, sc = torch.zeros(3), _lib.Scores()
    ops._call("nfst_fake", lat, sc, x, None, 7, 0.5)
    ops._call("nfst_fake", None, x, torch.nn.Parameter(x))
    (batch, *rest), no_batch = seen
    assert C.cast(batch, C.POINTER(_lib.Batch)).contents.n_lattices == lat.n_lattices
    assert rest == [sc, x.data_ptr(), None, 7, 0.5, 1234] and no_batch == (x.data_ptr(), x.data_ptr(), 1234)
    with pytest.raises(_lib.NfstError, match="^nfst_fails: "):
        ops._call("nfst_fails", lat, x)


# ----------------------------------------------------------------------------- the public surface
# Taken from the commit before the helpers (inspect.signature / _fields of every public name defined in ops), as data.
PUBLIC = {
    "BackwardResult": ('logbeta', 'logz', 'logz64', 'beta_me'),
    "backward": "(lat: 'LatticeBatch', theta, arc_scores=None, want_logbeta=True, want_me=False) -> 'BackwardResult'",
    "ForwardBackwardResult": ('logz', 'logz64', 'logalpha', 'logbeta', 'posterior', 'grad_theta', 'beta_me'),
    "forward_backward": "(lat: 'LatticeBatch', theta, arc_scores=None, want_alpha_beta=True, want_posterior=True, want_grad_theta=False, want_me=False, out: 'Optional[ForwardBackwardResult]' = None, total=None, total_slot: 'int' = 0) -> 'ForwardBackwardResult'",
    "ForwardBackwardLaunch": "(lat: 'LatticeBatch', theta, arc_scores=None, want_alpha_beta=True, want_posterior=True, want_grad_theta=False, want_me=False, out: 'Optional[ForwardBackwardResult]' = None, total=None)",
    "log_z": "(lat: 'LatticeBatch', theta: 'torch.Tensor', arc_scores: 'Optional[torch.Tensor]' = None) -> 'torch.Tensor'",
    "ExpectationResult": ('logz64', 'ev64', 'ev', 'posterior', 'cov', 'label_cov', 'label_post'),
    "expectation_terms": "(lat: 'LatticeBatch', theta, arc_scores=None, label_values=None, arc_values=None, score_coef: 'float' = 0.0, want_posterior=False, want_cov=False, want_label_cov=False, want_label_post=False) -> 'ExpectationResult'",
    "expectation": "(lat: 'LatticeBatch', theta: 'torch.Tensor', arc_scores: 'Optional[torch.Tensor]' = None, label_values: 'Optional[torch.Tensor]' = None, arc_values: 'Optional[torch.Tensor]' = None, score_coef: 'float' = 0.0) -> 'torch.Tensor'",
    "entropy": "(lat: 'LatticeBatch', theta: 'torch.Tensor', arc_scores: 'Optional[torch.Tensor]' = None) -> 'torch.Tensor'",
    "kl_divergence": "(lat: 'LatticeBatch', theta_p: 'torch.Tensor', theta_q: 'torch.Tensor', arc_scores_p: 'Optional[torch.Tensor]' = None, arc_scores_q: 'Optional[torch.Tensor]' = None) -> 'torch.Tensor'",
    "ViterbiResult": ('best', 'paths', 'arcs', 'lengths'),
    "viterbi": "(lat: 'LatticeBatch', theta, arc_scores=None, max_len: 'Optional[int]' = None, pad: 'int' = 0) -> 'ViterbiResult'",
    "KBestResult": ('best', 'paths', 'arcs', 'lengths', 'n_paths'),
    "k_best_terms": "(lat: 'LatticeBatch', theta, k: 'int', arc_scores=None, max_len: 'Optional[int]' = None, pad: 'int' = 0) -> 'KBestResult'",
    "k_best": "(lat: 'LatticeBatch', theta, k: 'int', arc_scores=None, max_len: 'Optional[int]' = None, pad: 'int' = 0) -> 'KBestResult'",
    "ArcSlackResult": ('best', 'slack', 'keep', 'n_kept', 'vbeta', 'state_slack'),
    "arc_slack": "(lat: 'LatticeBatch', theta, arc_scores=None, beam=None, want_rows: 'bool' = False) -> 'ArcSlackResult'",
    "PruneResult": ('lat', 'arc_map', 'n_kept', 'best'),
    "prune": "(lat: 'LatticeBatch', theta, beam, arc_scores=None, **pack_opts) -> 'PruneResult'",
    "intersect": "(lat: 'LatticeBatch', dfa, **pack_opts) -> 'IntersectResult'",
    "PositionalResult": ('logz', 'logz64', 'pos_posterior', 'arc_posterior', 'len_logz'),
    "PositionalViterbiResult": ('best', 'paths', 'path_arcs', 'lengths'),
    "positional_plan": "(lat: 'LatticeBatch', viterbi: 'bool' = False) -> 'tuple'",
    "positional_forward_backward": "(lat: 'LatticeBatch', theta, pos_scores=None, T: 'Optional[int]' = None, arc_scores=None, want_pos_posterior: 'bool' = True, want_arc_posterior: 'bool' = False, want_len: 'bool' = False) -> 'PositionalResult'",
    "positional_log_z": "(lat: 'LatticeBatch', theta: 'torch.Tensor', pos_scores: 'torch.Tensor', arc_scores: 'Optional[torch.Tensor]' = None) -> 'torch.Tensor'",
    "length_distribution": "(lat: 'LatticeBatch', theta, T: 'Optional[int]' = None, arc_scores=None)",
    "PositionalExpectationResult": ('logz64', 'logz', 'ev64', 'ev', 'pos_posterior', 'arc_posterior', 'pos_cov', 'arc_cov'),
    "positional_expectation_plan": "(lat: 'LatticeBatch') -> 'tuple'",
    "positional_expectation_terms": "(lat: 'LatticeBatch', theta, pos_scores=None, T: 'Optional[int]' = None, arc_scores=None, pos_values=None, label_values=None, arc_values=None, score_coef: 'float' = 0.0, want_pos_posterior: 'bool' = False, want_arc_posterior: 'bool' = False, want_pos_cov: 'bool' = False, want_arc_cov: 'bool' = False) -> 'PositionalExpectationResult'",
    "positional_expectation": "(lat: 'LatticeBatch', theta: 'torch.Tensor', pos_scores: 'Optional[torch.Tensor]' = None, T: 'Optional[int]' = None, arc_scores: 'Optional[torch.Tensor]' = None, pos_values: 'Optional[torch.Tensor]' = None, label_values: 'Optional[torch.Tensor]' = None, arc_values: 'Optional[torch.Tensor]' = None, score_coef: 'float' = 0.0) -> 'torch.Tensor'",
    "positional_entropy": "(lat: 'LatticeBatch', theta: 'torch.Tensor', pos_scores: 'Optional[torch.Tensor]' = None, T: 'Optional[int]' = None, arc_scores: 'Optional[torch.Tensor]' = None) -> 'torch.Tensor'",
    "positional_kl_divergence": "(lat: 'LatticeBatch', theta_p: 'torch.Tensor', pos_p: 'Optional[torch.Tensor]', theta_q: 'torch.Tensor', pos_q: 'Optional[torch.Tensor]', T: 'Optional[int]' = None, arc_scores_p: 'Optional[torch.Tensor]' = None, arc_scores_q: 'Optional[torch.Tensor]' = None) -> 'torch.Tensor'",
    "positional_viterbi": "(lat: 'LatticeBatch', theta, pos_scores=None, T: 'Optional[int]' = None, arc_scores=None, pad: 'int' = 0) -> 'PositionalViterbiResult'",
    "PositionalKBestResult": ('best', 'paths', 'arcs', 'lengths', 'n_paths'),
    "positional_k_best_terms": "(lat: 'LatticeBatch', theta, k: 'int', pos_scores=None, T: 'Optional[int]' = None, arc_scores=None, pad: 'int' = 0) -> 'PositionalKBestResult'",
    "positional_k_best": "(lat: 'LatticeBatch', theta, k: 'int', pos_scores=None, T: 'Optional[int]' = None, arc_scores=None, pad: 'int' = 0) -> 'PositionalKBestResult'",
    "PositionalSampleResult": ('paths', 'arcs', 'lengths', 'logq', 'logz', 'logz64'),
    "positional_sample_paths": "(lat: 'LatticeBatch', theta, k: 'int', pos_scores=None, T: 'Optional[int]' = None, arc_scores=None, uniforms: 'Optional[torch.Tensor]' = None, seed: 'int' = 0, pad: 'int' = 0, want_arcs: 'bool' = True) -> 'PositionalSampleResult'",
    "positional_score_paths": "(lat: 'LatticeBatch', theta, marks: 'torch.Tensor', pos_scores=None, T: 'Optional[int]' = None, arc_scores=None)",
    "SampleResult": ('paths', 'arcs', 'lengths', 'logq', 'logz'),
    "sample_paths": "(lat: 'LatticeBatch', theta, k: 'int', arc_scores=None, max_len: 'Optional[int]' = None, uniforms: 'Optional[torch.Tensor]' = None, seed: 'int' = 0, pad: 'int' = 0, beta: 'Optional[BackwardResult]' = None, want_arcs: 'bool' = True) -> 'SampleResult'",
    "score_paths": "(lat: 'LatticeBatch', theta, marks: 'torch.Tensor', arc_scores=None)",
    "step": "(lat: 'LatticeBatch', state: 'torch.Tensor', label: 'torch.Tensor', k: 'int' = 1) -> 'torch.Tensor'",
    "emission_mask": "(lat: 'LatticeBatch', state: 'torch.Tensor', k: 'int' = 1, inp: 'Optional[torch.Tensor]' = None, pad: 'int' = 0, bos: 'int' = 1, eos: 'int' = 2, has_to_end: 'bool' = False) -> 'torch.Tensor'",
    "beta_logits": "(lat: 'LatticeBatch', values: 'torch.Tensor', state: 'torch.Tensor', k: 'int' = 1) -> 'torch.Tensor'",
    "ProposalStep": ('symbol', 'logq', 'logz', 'next_state'),
    "StepPenalties": "(n_walkers: 'int', vocab: 'int', device, insertion_mark: 'int', insert_threshold: 'int' = 2, insert_penalty: 'float' = 1000.0, length_threshold: 'int' = 0, length_penalty: 'float' = 1000.0)",
    "proposal_step": "(lat: 'LatticeBatch', state: 'torch.Tensor', scores: 'torch.Tensor', k: 'int' = 1, inp: 'Optional[torch.Tensor]' = None, values: 'Optional[torch.Tensor]' = None, pad: 'int' = 0, bos: 'int' = 1, eos: 'int' = 2, has_to_end: 'bool' = False, temperature: 'float' = 1.0, uniforms: 'Optional[torch.Tensor]' = None, forced: 'Optional[torch.Tensor]' = None, value_state: 'Optional[torch.Tensor]' = None, penalties: 'Optional[StepPenalties]' = None, length: 'int' = 1, out=None, not_pad: 'Optional[torch.Tensor]' = None) -> 'ProposalStep'",
    "BeamStep": ('score', 'parent', 'symbol', 'next_state', 'n_candidates'),
    "beam_lds_candidates": "() -> 'int'",
    "beam_step": "(lat: 'LatticeBatch', state: 'torch.Tensor', inp: 'torch.Tensor', beam_score: 'torch.Tensor', scores: 'torch.Tensor', k: 'int', lookahead: 'Optional[torch.Tensor]' = None, pad: 'int' = 0, bos: 'int' = 1, eos: 'int' = 2, has_to_end: 'bool' = False, out=None, n_open: 'Optional[torch.Tensor]' = None) -> 'BeamStep'",
    "beam_backtrack": "(parent: 'torch.Tensor', symbol: 'torch.Tensor', score: 'torch.Tensor', n_lattices: 'int', k: 'int', n_steps: 'Optional[int]' = None, max_len: 'Optional[int]' = None, pad: 'int' = 0)",
    "NeuralBeta": ('log_beta', 'beta_hat'),
    "backward_neural": "(lat: 'LatticeBatch', emb: 'torch.Tensor', Wx: 'torch.Tensor', Wh: 'torch.Tensor', W: 'torch.Tensor', bias: 'torch.Tensor') -> 'NeuralBeta'",
    "gather_label_scores": "(lat: 'LatticeBatch', theta, arc_scores=None) -> 'torch.Tensor'",
    "path_logprob": "(scores: 'torch.Tensor', marks: 'torch.Tensor', pad: 'int' = 0, bos: 'int' = 1, eos: 'int' = 2, max_length: 'Optional[int]' = None, temp: 'float' = 1.0, normalize: 'bool' = True, smoothing: 'float' = 0.0, mask_mode: 'int' = 0) -> 'torch.Tensor'",
    "gpt2_logprob": "(logits: 'torch.Tensor', x: 'torch.Tensor', pad: 'int' = 0) -> 'torch.Tensor'",
    "iwae": "(log_p: 'torch.Tensor', log_q: 'torch.Tensor')",
}
CONSTANTS = {"MAX_K": 64, "MASK_STATICRNN": 0, "MASK_GPT2": 1}


def test_public_surface_is_the_one_before_the_helpers():
    found = {}
    for name, obj in vars(ops).items():
        if name.startswith("_") or getattr(obj, "__module__", None) != ops.__name__:
            continue
        if isinstance(obj, type) and issubclass(obj, tuple) and hasattr(obj, "_fields"):
            found[name] = obj._fields
        elif callable(obj):
            found[name] = str(inspect.signature(obj))
    assert sorted(found) == sorted(PUBLIC)
    for name, want in PUBLIC.items():
        assert found[name] == want, name
    assert {k: getattr(ops, k) for k in CONSTANTS} == CONSTANTS

"""ops.beam_step (nfst_beam_step: one step of lattice-constrained beam search), ops.beam_backtrack and
decoders.BeamDecoder against the float32 NumPy reference of tests/beam_ref.py, bit for bit.

The inputs are built in tests/beam_ref.py and tests/edge_cases.py; tests/test_beam_cpu.py proves on the reference alone
that they are what the cases need (ties across slots and labels at the cut, a beam that dies, a look-ahead that matters)."""
import functools

import numpy as np
import pytest
import torch

from nfst_amd import _lib, ops, synth
from nfst_amd.decoders import BeamDecoder
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from tests import beam_ref as R
from tests import edge_cases as E
from tests.test_beam_cpu import decoded, few_paths, lookahead_case

pytestmark = pytest.mark.gpu
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
NEG = -np.inf
KS = (1, 2, 7, 20, 64)
NFST_BATCH_ALL_COMPACT = 1  # (include/nfst_hip.h)


@functools.lru_cache(maxsize=None)
def _lats(name):
    return {"mixed": E.mixed_batch, "weighted": E.weighted_batch, "star": lambda: [E.star()],
            "many": lambda: E.many_small()[0], "wide": _wide_vocab}[name]()


@functools.lru_cache(maxsize=None)
def _batch(name):
    return LatticeBatch.from_synth(_lats(name), device=torch.device("cuda:0"))


def _wide_vocab():
    return [synth.layered_lattice(50 + s, n_states=40 + 7 * s, avg_degree=5.0, vocab=3000, width=5, span=2, weighted=True)
            for s in range(3)]


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _run(lat, c, K, dev, has_to_end=False, **kw):
    n_open = torch.zeros(1, dtype=torch.int32, device=dev)
    r = ops.beam_step(lat, _t(c["state"], dev), _t(c["inp"], dev), _t(c["beam_score"], dev), _t(c["scores"], dev), K,
                      lookahead=_t(c["lookahead"], dev), pad=PAD, bos=BOS, eos=EOS, has_to_end=has_to_end, n_open=n_open, **kw)
    return r, int(n_open.item())


def _same(tag, r, n_open, ref):
    assert np.array_equal(r.score.cpu().numpy().view(np.int32), ref["score"].view(np.int32)), tag  # bits, -inf included
    assert np.array_equal(r.parent.cpu().numpy(), ref["parent"]), tag
    assert np.array_equal(r.symbol.cpu().numpy(), ref["symbol"]), tag
    assert np.array_equal(r.next_state.cpu().numpy(), ref["next_state"]), tag
    assert np.array_equal(r.n_candidates.cpu().numpy(), ref["n_candidates"]), tag
    assert n_open == ref["n_open"], tag
    assert r.parent.dtype == torch.int32 and r.symbol.dtype == torch.int64 and r.next_state.dtype == torch.int64


def _check(name, K, dev, c, has_to_end=False):
    lats, lat = _lats(name), _batch(name)
    r, n_open = _run(lat, c, K, dev, has_to_end)
    ref = R.batch_step(lats, K, has_to_end=has_to_end, **c)
    _same((name, K, has_to_end), r, n_open, ref)
    return r, ref


# ----------------------------------------------------------------------------- one step
@pytest.mark.parametrize("lookahead", [False, True])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", ["mixed", "weighted"])
def test_step_equals_the_reference(dev, name, K, lookahead):
    lats = _lats(name)
    assert K * lats[0].vocab <= ops.beam_lds_candidates()  # every lattice's candidates stay in LDS
    c = R.step_case(lats, K, seed=100 + K, lookahead=lookahead)
    r, ref = _check(name, K, dev, c)
    assert np.any(ref["parent"] >= 0) and (K == 64 or np.any(ref["n_candidates"] > K))


@pytest.mark.parametrize("K", (7, 20, 64))
def test_exact_ties_go_by_slot_then_label(dev, K):
    c = R.tie_case(_lats("mixed"), K)
    r, ref = _check("mixed", K, dev, c)
    par, sym, sc = ref["parent"].reshape(-1, K), ref["symbol"].reshape(-1, K), ref["score"].reshape(-1, K)
    for b in range(par.shape[0] - 1):  # inside a run of equal scores: (slot, label) ascending
        for i in range(K - 1):
            if sc[b, i] == sc[b, i + 1] and par[b, i + 1] >= 0:
                assert (par[b, i], sym[b, i]) < (par[b, i + 1], sym[b, i + 1])
    q = R.step_case(_lats("weighted"), K, seed=7, lookahead=True, quarter=True)
    _check("weighted", K, dev, q)


def test_wide_fan_out_recomputes_the_candidates(dev):
    """64 slots in the star's state of 200 out-arcs: 12 800 candidates, more than the kernel keeps in LDS, so every pass
    of the selection computes them again; the mixed batch's K * vocab = 4096 stay in LDS."""
    K, l = 64, _lats("star")[0]
    assert 64 * 64 <= ops.beam_lds_candidates() < K * 200
    rng = np.random.default_rng(3)
    c = dict(state=np.ones(K, np.int64), inp=np.full(K, 5, np.int64), beam_score=rng.normal(-4.0, 1.0, size=K).astype(np.float32),
             scores=rng.normal(-2.0, 1.0, size=(K, l.vocab)).astype(np.float32), lookahead=None)
    r, ref = _check("star", K, dev, c)
    assert ref["n_candidates"][0] == 12800
    c["scores"] = E.quarter(c["scores"])  # and with ties
    c["beam_score"] = E.quarter(c["beam_score"])
    c["lookahead"] = E.quarter(rng.normal(-1.0, 1.0, size=l.n_rows))
    _check("star", K, dev, c)


def test_more_lattices_than_compute_units(dev):
    lats = _lats("many")
    assert len(lats) == 330
    _check("many", 4, dev, R.step_case(lats, 4, seed=9, lookahead=True))


def test_wide_vocabulary(dev):
    lats, lat = _lats("wide"), _batch("wide")
    assert lat.vocab == 3000 and not (lat.reserved0 & NFST_BATCH_ALL_COMPACT)
    for K in (3, 64):  # (64 * 3000 labels: the LDS budget, not K * vocab, bounds the kept candidates)
        _check("wide", K, dev, R.step_case(lats, K, seed=K, lookahead=True))


@pytest.mark.parametrize("name", ["mixed", "weighted"])
def test_has_to_end(dev, name):
    """On the last allowed step only eos survives (pad for a hypothesis that has ended); a slot without an eos arc dies."""
    lats, K = _lats(name), 7
    c = R.step_case(lats, K, seed=21)
    for b, l in enumerate(lats):  # some slots in states with an eos arc
        src = l.src[l.label == EOS]
        c["state"][b * K + 1], c["inp"][b * K + 1], c["beam_score"][b * K + 1] = src[0], 5, -1.0
        c["scores"][b * K + 1, EOS] = -0.5
    r, ref = _check(name, K, dev, c, has_to_end=True)
    live = ref["parent"] >= 0
    assert np.any(ref["symbol"][live] == EOS) and np.all(np.isin(ref["symbol"][live], (EOS, PAD)))
    free = R.batch_step(lats, K, has_to_end=False, **c)
    assert np.sum(free["parent"] >= 0) > np.sum(live)  # hypotheses died


def test_cross_check_against_the_composed_ops(dev):
    """On untied inputs the K best scores are torch.topk over beam_score + (scores with the pad column at zero +
    ops.emission_mask): the same float32 adds, so the same bits."""
    for name, K in (("mixed", 20), ("weighted", 7)):
        lats, lat = _lats(name), _batch(name)
        c = R.step_case(lats, K, seed=33)
        c["scores"][np.isnan(c["scores"])] = -1.0
        r, _ = _run(lat, c, K, dev)
        st, inp, bs, sc = (_t(c[n], dev) for n in ("state", "inp", "beam_score", "scores"))
        mask = ops.emission_mask(lat, st, k=K, inp=inp, pad=PAD, bos=BOS, eos=EOS)
        sc = sc.clone()
        sc[:, PAD] = 0.0
        cand = bs[:, None] + (sc + mask)
        top = torch.topk(cand.reshape(len(lats), K * lat.vocab), K, dim=1).values
        got = r.score.reshape(len(lats), K)
        assert torch.equal(top.view(torch.int32), got.view(torch.int32))


def test_errors_and_repeat_launches(dev):
    lats, lat = _lats("mixed"), _batch("mixed")
    B, V = len(lats), lat.vocab

    def args(K):
        N = B * K
        return (torch.zeros(N, dtype=torch.int64, device=dev), torch.zeros(N, dtype=torch.int64, device=dev),
                torch.zeros(N, dtype=torch.float32, device=dev), torch.zeros((N, V), dtype=torch.float32, device=dev))

    with pytest.raises(_lib.NfstError) as e:
        ops.beam_step(lat, *args(65), 65)
    assert e.value.code == -6  # NFST_ERR_LIMIT
    with pytest.raises(_lib.NfstError) as e:
        ops.beam_step(lat, *args(0), 0)
    assert e.value.code == -1  # NFST_ERR_ARG
    st, inp, bs, sc = args(3)
    for bad in ((st[:-1], inp, bs, sc), (st, inp.to(torch.int32), bs, sc), (st, inp, bs.double(), sc), (st, inp, bs, sc[:, :-1]),
                (st, inp, bs, sc.half())):
        with pytest.raises(ValueError):
            ops.beam_step(lat, *bad, 3)
    with pytest.raises(ValueError):
        ops.beam_step(lat, st, inp, bs, sc, 3, lookahead=torch.zeros(lat.total_rows + 1, device=dev))
    with pytest.raises(ValueError):
        ops.beam_step(lat, st, inp, bs, sc, 3, n_open=torch.zeros(2, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.beam_step(lat, st, inp, bs, sc, 3, out=(bs, bs, st, st, bs))
    torch.cuda.synchronize()
    K = 20
    c = R.step_case(lats, K, seed=4, lookahead=True)
    a, na = _run(lat, c, K, dev)
    out = tuple(torch.empty_like(x) for x in a)
    b, nb = _run(lat, c, K, dev, out=out)
    assert na == nb and all(x.data_ptr() == y.data_ptr() for x, y in zip(b, out))
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


# ----------------------------------------------------------------------------- backtrack
def test_backtrack_alone(dev):
    rng = np.random.default_rng(17)
    for B, K, T, n_steps in ((3, 7, 9, 9), (2, 64, 12, 8), (5, 1, 4, 0)):
        N = B * K
        parent = rng.integers(0, K, size=(T, N)).astype(np.int32)
        parent[rng.random((T, N)) < 0.05] = -1  # chains that stop early
        symbol = rng.integers(0, 12, size=(T, N)).astype(np.int64)  # pad (0) anywhere: stripped
        score = rng.normal(size=N).astype(np.float32)
        score[rng.random(N) < 0.3] = NEG
        want_p, want_l = R.backtrack(parent, symbol, score, B, K, n_steps, T + 2)
        p, ln = ops.beam_backtrack(_t(parent, dev), _t(symbol, dev), _t(score, dev), B, K, n_steps=n_steps, max_len=T + 2, pad=PAD)
        assert np.array_equal(p.cpu().numpy(), want_p) and np.array_equal(ln.cpu().numpy(), want_l)
        assert np.all(want_l[score.reshape(B, K) == NEG] == 0)


# ----------------------------------------------------------------------------- whole decodes
def _scorer(lat, V, theta=None, max_length=400):
    m = LatticeScorer(V, pad=PAD, bos=BOS, eos=EOS, max_length=max_length, theta=theta)
    m.to(lat.device)
    return m.set_lattice(lat)


def _stateless(table_nv):
    return lambda hx, inp: (hx, table_nv)


def _same_decode(tag, r, ref):
    assert r.n_steps == ref["n_steps"], tag
    assert np.array_equal(r.scores.cpu().numpy().view(np.int32), ref["scores"].view(np.int32)), tag
    assert np.array_equal(r.lengths.cpu().numpy(), ref["lengths"]), tag
    assert np.array_equal(r.paths.cpu().numpy(), ref["paths"]), tag


def _as_dict(r):
    return dict(paths=r.paths.cpu().numpy(), lengths=r.lengths.cpu().numpy(), scores=r.scores.cpu().numpy())


def test_decode_wide_beam_finds_every_path_and_a_narrow_one_dies(dev):
    l, th, ref = few_paths()
    lat = LatticeBatch.from_synth([l], device=dev)
    for K in (64, 1):
        table = _t(np.broadcast_to(th, (K, len(th))), dev)
        r = BeamDecoder(_scorer(lat, len(th), max_length=l.n_rows), _stateless(table)).decode(K)
        _same_decode(K, r, R.decode([l], K, R.stateless(th, K), max_length=l.n_rows))
        assert decoded(_as_dict(r), 0, K) == (ref if K == 64 else {})
    assert bool(torch.all(r.scores == NEG)) and bool(torch.all(r.lengths == 0))  # K = 1 died


def test_decode_with_exact_lookahead(dev):
    lats, theta, vb, best = lookahead_case()
    lat = LatticeBatch.from_synth(lats, device=dev)
    L = max(l.n_rows for l in lats)
    look = np.concatenate(vb)
    # beta* of nfst_arc_slack (it keeps -inf on rows that no prefix of finite score reaches; no hypothesis gets there)
    vbeta = ops.arc_slack(lat, _t(theta, dev), want_rows=True).vbeta
    on_path = np.isfinite(vbeta.cpu().numpy())
    assert np.array_equal(vbeta.cpu().numpy()[on_path], look[on_path])  # (quartered scores: beta* is exact)
    for K, la in ((1, vbeta), (1, _t(look, dev)), (8, None)):
        table = _t(np.repeat(theta, K, axis=0), dev)
        r = BeamDecoder(_scorer(lat, theta.shape[1], max_length=L), _stateless(table)).decode(K, lookahead=la)
        _same_decode(K, r, R.decode(lats, K, R.stateless(theta, K), max_length=L, lookahead=None if la is None else look))
        d = _as_dict(r)
        if K == 1:
            for b in range(len(lats)):
                assert decoded(d, b, 1) == {best[b][0]: best[b][1]}
        else:
            top = [max(decoded(d, b, K).values(), default=NEG) for b in range(len(lats))]
            assert any(t < best[b][1] for b, t in enumerate(top))


def test_decode_with_viterbi_lookahead_is_viterbi(dev):
    lats, lat = _lats("mixed"), _batch("mixed")
    V = lat.vocab
    theta = synth.label_scores(3, V)
    m = _scorer(lat, V, theta=torch.from_numpy(theta), max_length=int(lat.depth.max()) + 1)
    table1 = _t(np.broadcast_to(theta, (len(lats), V)), dev)
    r = m.beam_decoder(_stateless(table1)).decode(1, lookahead="viterbi")
    v = ops.viterbi(lat, m.theta.detach())
    vp, vl = v.paths.cpu().numpy(), v.lengths.cpu().numpy()
    for b in range(len(lats)):
        want = vp[b, :vl[b]]
        want = want[1:] if want[0] == BOS else want  # (the single-arc lattice has no bos arc)
        got = r.paths[b, 0, :int(r.lengths[b, 0])].cpu().numpy()
        assert np.array_equal(got, want), b
    # a beam of 20: distinct paths, non-increasing scores, and the scores are the paths' scores
    K = 20
    tableK = _t(np.broadcast_to(theta, (len(lats) * K, V)), dev)
    for la in (None, "viterbi", "log_beta") if lat.uniform_rows else (None, "viterbi"):
        r = m.beam_decoder(_stateless(tableK), sync_every=5).decode(K, lookahead=la)
        sc, ln, pa = r.scores.cpu().numpy(), r.lengths.cpu().numpy(), r.paths.cpu().numpy()
        bos_col = torch.full((len(lats), K, 1), BOS, dtype=torch.int32, device=dev)
        tot, end = ops.score_paths(lat, m.theta.detach(), torch.cat([bos_col, r.paths], dim=2))
        tot = tot.cpu().numpy().astype(np.float64)
        for b, l in enumerate(lats[:-1]):
            live = sc[b] > NEG
            n = int(live.sum())
            assert n > 0 and np.all(live[:n]) and np.all(np.diff(sc[b, :n]) <= 0)
            assert len({tuple(pa[b, i, :ln[b, i]]) for i in range(n)}) == n
            assert np.all(pa[b, np.arange(n), ln[b, :n] - 1] == EOS)
            want = tot[b, :n] - float(theta[BOS])
            assert np.all(np.abs(sc[b, :n] - want) <= 1e-5 * np.maximum(1.0, np.abs(want)))
            assert np.all(end[b, :n].cpu().numpy() == l.n_rows - 1)


def test_decode_with_log_beta_lookahead(dev):
    """lookahead="log_beta" is the scorer's compute_log_beta() as a row-indexed tensor (lattices of one row count)."""
    lats = [synth.layered_lattice(70 + s, n_states=40, avg_degree=3.0, vocab=32, width=4, span=2) for s in range(3)]
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = synth.label_scores(5, 32)
    K = 4
    m = _scorer(lat, 32, theta=torch.from_numpy(theta), max_length=45)
    m.set_k(3)  # (the scorer's own k does not matter to the decoder)
    table = _t(np.broadcast_to(theta, (len(lats) * K, 32)), dev)
    look = ops.backward(lat, m.theta.detach()).logbeta
    r = m.beam_decoder(_stateless(table)).decode(K, lookahead="log_beta")
    r2 = m.beam_decoder(_stateless(table)).decode(K, lookahead=look)
    assert torch.equal(r.paths, r2.paths) and torch.equal(r.scores, r2.scores) and r.n_steps == r2.n_steps
    _same_decode("log_beta", r, R.decode(lats, K, R.stateless(theta, K), max_length=45, lookahead=look.cpu().numpy()))
    assert bool(torch.all(r.scores[:, 0] > NEG))


@pytest.mark.parametrize("K", (2, 7))
def test_decode_with_a_path_dependent_scorer(dev, K):
    """score_fn keeps a hash of the prefix in hx and scores by table[hx % M]: parent reordering, backtracking and the
    early stop (sync_every = 1 against 8) against the reference decode with the same function."""
    mixed = _lats("mixed")
    lats = [mixed[0], mixed[1], mixed[3], mixed[5]]
    lat = LatticeBatch.from_synth(lats, device=dev)
    V, N = lat.vocab, len(lats) * K
    table, update = R.hashed_scorer(V)
    M = table.shape[0]
    ref = R.decode(lats, K, lambda hx, inp: (update(hx, inp), table[update(hx, inp) % M]), max_length=60, hx=np.zeros(N, np.int64))
    assert 8 < ref["n_steps"] < 61 and ref["n_steps"] % 8 != 0  # an early stop between two looks at the counters
    assert np.any(ref["scores"] > NEG)
    tt = _t(table, dev)

    def score_fn(hx, inp):
        hx = update(hx, inp)
        return hx, tt[hx % M]

    for every in (1, 8):
        m = _scorer(lat, V, max_length=60)
        r = BeamDecoder(m, score_fn, sync_every=every).decode(K, hx=torch.zeros(N, dtype=torch.int64, device=dev))
        _same_decode((K, every), r, ref)
    # the hard cut: with too few steps only hypotheses that can take eos on the last one survive
    short = R.decode(lats, K, lambda hx, inp: (update(hx, inp), table[update(hx, inp) % M]), max_length=5, hx=np.zeros(N, np.int64))
    r = BeamDecoder(_scorer(lat, V, max_length=400), score_fn).decode(K, max_len=5, hx=torch.zeros(N, dtype=torch.int64, device=dev))
    _same_decode((K, "short"), r, short)
    assert short["n_steps"] == 6 and np.any(short["scores"] == NEG)

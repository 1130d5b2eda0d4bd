"""The float32 NumPy reference of the beam step and decode (tests/beam_ref.py) on the inputs the GPU tests of
ops.beam_step and BeamDecoder use: it finds every path when the beam is wide enough, a narrow beam can die, an exact
look-ahead makes k = 1 exact, the tie inputs really tie; the C entry points exist and check their arguments on the host."""
import ctypes as C

import numpy as np

from nfst_amd import synth
from tests import beam_ref as R
from tests import edge_cases as E
from tests import kbest_ref as KR

NEG = -np.inf
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
ERR_ARG, ERR_LIMIT = -1, -6  # (include/nfst_hip.h)


def few_paths():
    """(lattice, quartered theta of it, its finite paths as {labels after bos: score without the bos arc})."""
    lats, theta, b, n = E.few_paths_case()
    l, th = lats[b], E.quarter(theta[b])
    ref = KR.enumerate_paths(l.n_rows, l.src, l.dst, E.score64(l, th), l.n_rows - 1)
    assert len(ref) == n
    return l, th, {tuple(int(x) for x in l.label[p][1:]): s - float(th[BOS]) for s, p in ref}


def lookahead_case():
    """(lattices, quartered theta [B, V], beta* per lattice, k_best's first entry per lattice as (labels after bos, score
    without the bos arc)): the mixed batch without its single-arc lattice, which has no bos arc."""
    lats, theta, _, _ = E.few_paths_case()
    lats, theta = lats[:-1], E.quarter(theta[:-1])
    best = []
    for l, r in zip(lats, E.kbest_refs(lats, theta, k=1)):
        assert r["n_paths"] == 1
        best.append((tuple(int(x) for x in l.label[r["arcs"][0]][1:]), float(r["best"][0]) - float(theta[len(best), BOS])))
    return lats, theta, [R.vbeta(l, theta[b]) for b, l in enumerate(lats)], best


def decoded(d, b, K):
    """{path: score} of the live final slots of lattice b."""
    return {tuple(int(x) for x in d["paths"][b, i, :d["lengths"][b, i]]): float(d["scores"][b, i])
            for i in range(K) if d["scores"][b, i] > NEG}


def test_wide_beam_finds_every_path():
    l, th, ref = few_paths()
    assert 0 < len(ref) < 64
    d = R.decode([l], 64, R.stateless(th, 64), max_length=l.n_rows)
    got = decoded(d, 0, 64)
    assert got == ref  # (quartered scores: the float32 sums are exact)
    assert int(np.sum(d["scores"] > NEG)) == len(ref)  # pairwise distinct
    live = d["scores"][0][d["scores"][0] > NEG]
    assert np.all(np.diff(live) <= 0)


def test_a_narrow_beam_can_die():
    l, th, ref = few_paths()
    d = R.decode([l], 1, R.stateless(th, 1), max_length=l.n_rows)
    assert np.all(d["scores"] == NEG) and np.all(d["lengths"] == 0)  # the greedy hypothesis runs into a dead label


def test_exact_lookahead_makes_one_hypothesis_exact():
    lats, theta, vb, best = lookahead_case()
    look = np.concatenate(vb)
    L = max(l.n_rows for l in lats)
    d = R.decode(lats, 1, R.stateless(theta, 1), max_length=L, lookahead=look)
    for b in range(len(lats)):
        assert decoded(d, b, 1) == {best[b][0]: best[b][1]}, b
    d8 = R.decode(lats, 8, R.stateless(theta, 8), max_length=L)
    top = [max(decoded(d8, b, 8).values(), default=NEG) for b in range(len(lats))]
    assert all(t <= best[b][1] for b, t in enumerate(top))
    assert any(t < best[b][1] for b, t in enumerate(top)), top  # eight hypotheses without look-ahead miss the best path


def test_tie_inputs_tie_across_slots_and_inside_a_slot():
    lats = E.mixed_batch()
    for K in (7, 20):
        c = R.tie_case(lats, K)
        cut = 0
        for b, l in enumerate(lats[:-1]):
            sl = slice(b * K, (b + 1) * K)
            cc, r, j, lab, _ = R.candidates(l, c["state"][sl], c["inp"][sl], c["beam_score"][sl], c["scores"][sl], None, False)
            assert len(r) > K
            same = r[:, None] == r[None, :]
            assert np.any(same & (j[:, None] != j[None, :]))  # equal ranks across slots
            assert np.any(same & (j[:, None] == j[None, :]) & (lab[:, None] != lab[None, :]))  # and across labels of one slot
            rs = np.sort(r)[::-1]
            cut += int(rs[K - 1] == rs[K])
        assert cut > 0  # the cut at K falls inside a tie: only the (slot, label) order decides who survives


def test_step_inputs_have_what_the_step_test_needs():
    for lats in (E.mixed_batch(), E.weighted_batch()):
        for K in (2, 20):
            c = R.step_case(lats, K, seed=K, lookahead=True)
            assert np.any(c["beam_score"] == NEG) and np.any(c["scores"] == NEG) and np.isnan(c["scores"]).sum() == 1
            assert np.any(c["lookahead"] == NEG)
            assert np.any(c["inp"] == EOS) or np.any(c["inp"] == PAD)
            o = R.batch_step(lats, K, **c)
            assert np.any(o["parent"] >= 0) and np.any(o["n_candidates"] > K)
            assert not np.any(np.isnan(o["score"]))


def test_lib_declares_and_exports_the_new_symbols():
    from nfst_amd import _lib

    for name in ("nfst_beam_step", "nfst_beam_backtrack", "nfst_beam_lds_candidates"):
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib, name)
        assert getattr(_lib.lib, name).argtypes is not None


def test_argument_checks_return_before_any_launch():
    from nfst_amd import _lib
    from nfst_amd.lattice import LatticeBatch

    lats = E.mixed_batch()[:2]
    lat = LatticeBatch.from_synth(lats)  # host-packed: the checks run before anything touches a device
    assert lat.device.type == "cpu"
    lib, bs = _lib.lib, C.byref(lat.c_struct())
    K, B, V = 3, 2, lat.vocab
    N = B * 65
    a = dict(state=np.zeros(N, np.int64), inp=np.zeros(N, np.int64), beam=np.zeros(N, np.float32), scores=np.zeros((N, V), np.float32),
             score=np.zeros(N, np.float32), parent=np.zeros(N, np.int32), symbol=np.zeros(N, np.int64), nxt=np.zeros(N, np.int64))
    p = lambda x: None if x is None else x.ctypes.data

    def call(k, pad=PAD, **kw):
        v = {**a, **kw}
        return lib.nfst_beam_step(bs, p(v["state"]), p(v["inp"]), p(v["beam"]), p(v["scores"]), None, pad, BOS, EOS, 0, k,
                                  p(v["score"]), p(v["parent"]), p(v["symbol"]), p(v["nxt"]), None, None, None)

    assert call(0) == ERR_ARG
    assert call(-1) == ERR_ARG
    assert call(65) == ERR_LIMIT
    for name in a:
        assert call(K, **{name: None}) == ERR_ARG, name
    assert call(K, pad=V) == ERR_ARG
    assert lib.nfst_beam_step(None, p(a["state"]), p(a["inp"]), p(a["beam"]), p(a["scores"]), None, PAD, BOS, EOS, 0, K, p(a["score"]),
                              p(a["parent"]), p(a["symbol"]), p(a["nxt"]), None, None, None) == ERR_ARG
    assert 0 < lib.nfst_beam_lds_candidates() < 64 * 200  # (the star's 12 800 candidates lie beyond it)

    T = 4
    par, sym = np.zeros((T, B * K), np.int32), np.zeros((T, B * K), np.int64)
    paths, lens = np.zeros((B, K, T), np.int32), np.zeros((B, K), np.int32)

    def back(k=K, n_steps=T, max_len=T, par=par, sym=sym, score=a["score"], paths=paths, lens=lens):
        return lib.nfst_beam_backtrack(p(par), p(sym), p(score), n_steps, B, k, max_len, PAD, p(paths), p(lens), None)

    assert back(k=0) == ERR_ARG
    assert back(k=65) == ERR_LIMIT
    assert back(n_steps=T + 1) == ERR_ARG
    assert back(max_len=0) == ERR_ARG
    for kw in (dict(par=None), dict(sym=None), dict(score=None), dict(paths=None), dict(lens=None)):
        assert back(**kw) == ERR_ARG, kw


def test_build_guard_covers_the_beam_step():
    from nfst_amd.build import check_resources

    assert check_resources({"k_beam_step": {"vgpr_spill": 4, "agprs": 0}})

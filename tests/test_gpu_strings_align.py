"""ops.string_viterbi (nfst_string_viterbi), ops.string_sample_paths (nfst_string_sample) and ops.string_alignment_log_prob
against the NumPy restatement of tests/strings_align_ref.py: the best alignment bit for bit on every output, its float64
score included; the draws with given uniforms exactly on every decided walk (at most CAP of a case's walks are left out),
their score and logq within BOUND, log_num and logz with the bits of ops.string_log_prob; the same bits at every launch,
under every packing and slicing.  tests/test_strings_align_cpu.py holds the restatement to brute force over every path
and the cases of this file to the cap on the undecided walks.  The largest error of every kind goes to
strings_align_errors.json in the directory of run outputs (profiles/README.md).

Shapes: N + 1 in {1, 2, 64, 65, 66, 129} (the strip cases), M in {1, 3, 65}, K in {1, 64, 65} (and 2, 3, 4 where the
lattices are large); candidates of different lengths under three different tails behind their ends.
"""
import ctypes as C
import functools
import glob
import json
import os

import numpy as np
import pytest
import torch

from nfst_amd import _lib, ops, synth
from nfst_amd.constraints import WideDFA
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from tests import edge_cases as E
from tests import pack_cases as PC
from tests import strings_align_ref as AR
from tests import strings_grad_ref as GR
from tests import strings_ref as SR
from tests import structure_cases as S

pytestmark = pytest.mark.gpu
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
NEG = -np.inf
MARK = SR.MARK
# The largest absolute error of a draw's score and logq against the restatement over this module's cases, measured on the
# MI355X (profiles/strings_align_errors.json): score 0 (the same adds in the same order), logq 3.6e-15 (it carries the
# error of log_num, a log-sum of exp from two libraries, section 4.21); x 16, rounded up to a power of ten.
BOUND = 1e-13
GRAD_BOUND = 1e-13  # tests/test_gpu_strings_grad.py's, for the gradient of string_alignment_log_prob

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
            with open(os.path.join(out, "strings_align_errors.json"), "w") as f:
                json.dump(dict(sorted(_ERR.items())), f, indent=1)


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, np.float64).view(np.int64)


def _same(a, b):
    """two results of the same op, bit for bit"""
    return all(np.array_equal(_bits(x), _bits(y)) if x.dtype == torch.float64 else torch.equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(aligners [b][m], best alignments [b][m], walks [b][m][k]) of a shared case, computed once"""
    return _ref_of(AR.sample_cases()[name])


def _ref_of(case):
    al = AR.aligners(case)
    U = case["uniforms"]
    best = [[a.viterbi() for a in row] for row in al]
    walks = [[[a.walk(U[b, m, k]) for k in range(U.shape[2])] for m, a in enumerate(row)] for b, row in enumerate(al)]
    return al, best, walks


def _offsets(lats):
    return np.concatenate([[0], np.cumsum([l.n_arcs for l in lats])])


def _expect(r, off, L, pad=PAD):
    """(paths, arcs, align) rows of a restated walk in the engine's layout: canonical arc ids of the batch"""
    n = r["length"]
    paths, arcs, align = np.full(L, pad, np.int32), np.full(L, -1, np.int32), np.full(L, -1, np.int32)
    paths[:n], arcs[:n], align[:n] = r["labels"], np.asarray(r["arcs"], np.int64) + off, r["align"]
    return paths, arcs, align


def _args(case, dev):
    rows, n = AR.rows(case["cands"], case["N"], case["tail"])
    return (_t(case["theta"], dev), _t(rows, dev), _t(n, dev)), dict(arc_scores=_t(case["asc"], dev), max_len=case["L"], pad=PAD, **case["tape"])


def _hold_best(tag, got, case, best):
    """string_viterbi against the restatement: every output exactly, the float64 score bit for bit"""
    off, L = _offsets(case["lats"]), case["L"]
    score, paths, arcs, align, lens = (x.cpu().numpy() for x in got)
    assert paths.dtype == arcs.dtype == align.dtype == lens.dtype == np.int32 and score.dtype == np.float64
    for b, row in enumerate(best):
        for m, r in enumerate(row):
            want = _expect(r, off[b], L)
            assert lens[b, m] == r["length"] and np.array_equal(_bits(score[b, m]), _bits(r["score"])), (tag, b, m, score[b, m], r["score"])
            assert np.array_equal(paths[b, m], want[0]) and np.array_equal(arcs[b, m], want[1]) and np.array_equal(align[b, m], want[2]), (tag, b, m)


def _hold_draws(tag, got, case, al, walks, slp):
    """string_sample_paths against the restatement: every decided walk exactly, score and logq within BOUND, log_num and
    logz with the bits of string_log_prob"""
    off, L = _offsets(case["lats"]), case["L"]
    paths, arcs, align, lens, score, logq, log_num, logz = (x.cpu().numpy() for x in got)
    assert np.array_equal(_bits(log_num), _bits(slp.log_num)) and np.array_equal(_bits(logz), _bits(slp.logz)), tag
    left_out = total = 0
    for b, row in enumerate(walks):
        for m, ws in enumerate(row):
            for k, r in enumerate(ws):
                total += 1
                if not r["margin"] > AR.DECIDED:
                    left_out += 1
                    continue
                want = _expect(r, off[b], L)
                at = (tag, b, m, k)
                assert lens[b, m, k] == r["length"], at
                assert np.array_equal(paths[b, m, k], want[0]) and np.array_equal(arcs[b, m, k], want[1]) and np.array_equal(align[b, m, k], want[2]), at
                if np.isneginf(al[b][m].log_num):
                    assert np.isneginf(score[b, m, k]) and logq[b, m, k] == 0.0 and np.isneginf(log_num[b, m]), at
                    continue
                assert rec(f"{tag.split(':')[0]} score", abs(score[b, m, k] - r["score"])) <= BOUND, at
                assert rec(f"{tag.split(':')[0]} logq", abs(logq[b, m, k] - r["logq"])) <= BOUND, at
                assert rec(f"{tag.split(':')[0]} score - logq - log_num", abs((score[b, m, k] - logq[b, m, k]) - log_num[b, m])) <= BOUND, at
                assert logq[b, m, k] <= BOUND, at
    assert left_out <= AR.CAP * total, (tag, left_out, total)


def _three_slices(lat, case):
    """max_workspace_bytes under which the candidates of a case go in three slices or more"""
    rows, _ = AR.rows(case["cands"], case["N"], case["tail"])
    M, N = rows.shape[1], rows.shape[2]
    q = lambda m: int(_lib.lib.nfst_string_sample_ws_bytes(C.byref(lat.c_struct()), m, N, int("marker" in case["tape"])))
    return q(0) + (q(1) - q(0)) * max(1, M // 3)


CASES = tuple(AR.sample_cases())


@pytest.mark.parametrize("name", CASES)
def test_shared_cases(dev, name):
    """Every case of strings_align_ref.sample_cases: the best alignments and the draws against the restatement, the same
    bits at a second launch and, with three candidates or more, in three slices or more (the Philox draws included)."""
    case = AR.sample_cases()[name]
    al, best, walks = _ref(name)
    lat = LatticeBatch.from_synth(case["lats"], device=dev)
    a, kw = _args(case, dev)
    K, M = case["K"], len(case["cands"][0])
    v = ops.string_viterbi(lat, *a, **kw)
    _hold_best(name, v, case, best)
    slp = ops.string_log_prob(lat, *a, arc_scores=kw["arc_scores"], **case["tape"])
    d = ops.string_sample_paths(lat, *a, K, uniforms=_t(case["uniforms"], dev), **kw)
    _hold_draws(name, d, case, al, walks, slp)
    live = torch.isfinite(slp.log_num)
    assert bool((v.score[live] <= slp.log_num[live]).all()) and bool(v.score[~live].isneginf().all())  # max <= sum
    assert _same(v, ops.string_viterbi(lat, *a, **kw)) and _same(d, ops.string_sample_paths(lat, *a, K, uniforms=_t(case["uniforms"], dev), **kw))
    p = ops.string_sample_paths(lat, *a, K, seed=9, **kw)
    assert _same(p, ops.string_sample_paths(lat, *a, K, seed=9, **kw))
    assert np.array_equal(_bits(p.log_num), _bits(slp.log_num))
    on = torch.isfinite(p.score)
    if bool(on.any()):
        assert float(((p.score - p.logq)[on] - p.log_num[:, :, None].expand_as(p.score)[on]).abs().max()) <= BOUND
    if M >= 3:
        mwb = _three_slices(lat, case)
        assert _same(v, ops.string_viterbi(lat, *a, max_workspace_bytes=mwb, **kw))
        assert _same(d, ops.string_sample_paths(lat, *a, K, uniforms=_t(case["uniforms"], dev), max_workspace_bytes=mwb, **kw))
        assert _same(p, ops.string_sample_paths(lat, *a, K, seed=9, max_workspace_bytes=mwb, **kw))


@pytest.mark.parametrize("M", [3, 65])
def test_two_tails_behind_the_candidates_are_not_read(dev, M):
    """Candidates of different lengths in rows of 130 tokens, filled behind each candidate's end once with a symbol of the
    tape (8), once with another (9) and once with the marker: a token read behind n would change the answer.  The best
    alignments, the draws with given uniforms and the Philox draws have the same bits under the three fills, in one
    launch and in slices, and agree with the restatement, which never sees a tail."""
    name = f"mixed lengths {M}"
    case = AR.sample_cases()[name]
    al, best, walks = _ref(name)
    lat = LatticeBatch.from_synth(case["lats"], device=dev)
    K, U = case["K"], _t(case["uniforms"], dev)
    mwb = _three_slices(lat, case)
    first = None
    for tail in (8, 9, MARK):
        a, kw = _args({**case, "tail": tail}, dev)
        n = a[2].cpu().numpy()
        assert bool((a[1].cpu().numpy()[np.arange(130)[None, None, :] >= n[:, :, None]] == tail).all()) and int(n.max()) < 130
        got = (ops.string_viterbi(lat, *a, **kw), ops.string_sample_paths(lat, *a, K, uniforms=U, **kw),
               ops.string_sample_paths(lat, *a, K, seed=9, **kw), ops.string_viterbi(lat, *a, max_workspace_bytes=mwb, **kw),
               ops.string_sample_paths(lat, *a, K, seed=9, max_workspace_bytes=mwb, **kw))
        _hold_best(f"{name} tail={tail}", got[0], case, best)
        _hold_draws(f"{name} tail={tail}", got[1], case, al, walks, ops.string_log_prob(lat, *a, arc_scores=kw["arc_scores"], **case["tape"]))
        if first is None:
            first = got
        assert all(_same(x, y) for x, y in zip(got, first)), tail
    assert _same(first[0], first[3]) and _same(first[2], first[4])


def test_one_path_per_string_is_the_whole_mass(dev):
    """keep = every label: the string is the path, so the best score is log_num (up to the order of the adds) and every
    draw is that path with logq 0"""
    case = AR.sample_cases()["star keep all"]
    lat = LatticeBatch.from_synth(case["lats"], device=dev)
    a, kw = _args(case, dev)
    v = ops.string_viterbi(lat, *a, **kw)
    d = ops.string_sample_paths(lat, *a, 65, seed=1, **kw)
    assert rec("one path: score - log_num", float((v.score - d.log_num).abs().max())) <= BOUND
    assert bool((d.arcs == v.arcs[:, :, None]).all()) and rec("one path: logq", float(d.logq.abs().max())) <= BOUND


NAMES = tuple(S.batches())


@pytest.mark.parametrize("name", NAMES)
def test_structure_corpus(dev, name):
    """The corpus of tests/structure_cases.py through both tape modes, with per-arc scores (and the tables' weights in the
    weighted batch): the string of a path, the empty string and a string that no path spells per lattice, against the
    restatement, and the same bits from both packers and under the three group modes.  A member whose state 0 is the sink
    has the empty path for the empty string and nothing for any other."""
    lats = [S.canonical(l) for l in S.batches()[name]]
    Vb = lats[0].vocab
    A = sum(l.n_arcs for l in lats)
    asc = np.random.default_rng(3).normal(0.0, 0.4, size=A).astype(np.float32) if A else None
    n_rows, arc_off, src, label, dst, w = PC.batch_arcs(S.batches()[name])
    for tape in (dict(keep=set(range(3, Vb, 2)) | {EOS}), dict(marker=5)):
        cands = []
        for l in lats:
            y = list(SR.project(AR.first_path_labels(l), **tape))
            cands.append([y, [], y + [Vb - 1]])
        case = dict(lats=lats, theta=S.theta(Vb), asc=asc, tape=tape, cands=cands, K=3, N=None, tail=8, L=AR.longest(lats),
                    uniforms=AR.uniforms(17, (len(lats), 3, 3, AR.longest(lats))))
        al, best, walks = _ref_of(case)
        first = None
        for route, gm in (("host", 0), ("device", 0), ("host", 1), ("host", 2), ("device", 2)):
            if route == "host":
                lat = LatticeBatch.from_arcs(n_rows, arc_off, src, label, dst, Vb, arc_w=w, group_mode=gm).to(dev, auto_chunks=False)
            else:
                lat = LatticeBatch.from_arcs_device(n_rows, arc_off, src, label, dst, Vb, arc_w=w, device=dev, group_mode=gm)
            a, kw = _args(case, dev)
            got = (ops.string_viterbi(lat, *a, **kw), ops.string_sample_paths(lat, *a, 3, uniforms=_t(case["uniforms"], dev), **kw),
                   ops.string_sample_paths(lat, *a, 3, seed=4, **kw))
            if first is None:
                _hold_best(f"structure: {name} {sorted(tape)}", got[0], case, best)
                _hold_draws(f"structure: {name} {sorted(tape)}", got[1], case, al, walks, ops.string_log_prob(lat, *a, arc_scores=kw["arc_scores"], **tape))
                first = got
            assert all(_same(x, y) for x, y in zip(got, first)), (name, route, gm)
        for b, l in enumerate(lats):
            if l.n_arcs == 0:  # state 0 is the sink
                assert first[0].score[b].tolist() == [0.0, 0.0, NEG] and first[0].lengths[b].tolist() == [0, 0, 0]
                assert first[1].score[b, :, 0].tolist() == [0.0, 0.0, NEG] and first[1].logq[b].abs().max() == 0 and int(first[1].lengths[b].max()) == 0


def test_the_viterbi_path_is_the_best_alignment_of_its_string(dev):
    """With continuous random scores: string_viterbi on the projection of ops.viterbi's path returns that path (the marks
    exactly, the score within ops.viterbi's float32 bound), in both tape modes."""
    lats = E.mixed_batch()
    Vb = lats[0].vocab
    rng = np.random.default_rng(5)
    theta = rng.normal(-1.0, 0.7, size=(len(lats), Vb)).astype(np.float32)
    asc = rng.normal(0.0, 0.5, size=sum(l.n_arcs for l in lats)).astype(np.float32)
    lat = LatticeBatch.from_synth(lats, device=dev)
    v = ops.viterbi(lat, _t(theta, dev), _t(asc, dev), pad=PAD)
    marks, lens = v.paths.cpu().numpy(), v.lengths.cpu().numpy()
    for tape in (dict(keep=set(range(3, Vb, 2))), dict(marker=10)):
        cands = [[list(SR.project(marks[b, :lens[b]], **tape))] for b in range(len(lats))]
        rows, n = AR.rows(cands)
        got = ops.string_viterbi(lat, _t(theta, dev), _t(rows, dev), _t(n, dev), arc_scores=_t(asc, dev), pad=PAD, **tape)
        assert torch.equal(got.paths[:, 0], v.paths) and torch.equal(got.arcs[:, 0], v.arcs) and torch.equal(got.lengths[:, 0], v.lengths)
        depth = float(lens.max())
        bound = depth * 2.0 ** -23 * float(got.score.abs().max())  # one float32 rounding per add of ops.viterbi's sum
        assert rec("viterbi identity score", float((got.score[:, 0] - v.best.double()).abs().max())) <= bound


def test_agreement_with_the_product_route(dev):
    """Where the product fits, intersect + viterbi gives the same marks."""
    from tests import intersect_wide_ref as IW

    lats = [SR.denominator(SR.SEED1), SR.denominator(SR.SMALL), IW.edit_denominator([7, 6, 6, 8], [8, 9, 10], 2, vocab=12)]
    theta = np.random.default_rng(8).normal(-1.0, 0.6, size=12).astype(np.float32)
    lat = LatticeBatch.from_synth(lats, device=dev)
    # (per-arc scores: under label scores alone two paths with the same labels in another order tie)
    asc = _t(np.random.default_rng(9).normal(0.0, 0.5, size=lat.total_arcs).astype(np.float32), dev)
    ys = [[8], [8, 9], [], [9, 8]]
    rows, n = AR.rows([ys] * 3)
    for tape, dfa in ((dict(marker=MARK), lambda y: WideDFA.marked_sequence(12, MARK, y)),
                      (dict(keep={8, 9, 10}), lambda y: WideDFA.projected_sequence(12, {8, 9, 10}, y))):
        got = ops.string_viterbi(lat, _t(theta, dev), _t(rows, dev), _t(n, dev), arc_scores=asc, pad=PAD, **tape)
        for m, y in enumerate(ys):
            if "keep" in tape and not y:
                continue
            res = ops.intersect(lat, dfa(y))
            v = ops.viterbi(res.lattice, _t(theta, dev), asc[res.arc_map], max_len=got.paths.shape[2], pad=PAD)
            assert torch.equal(v.paths, got.paths[:, m]) and torch.equal(v.lengths, got.lengths[:, m]), (tape, y)
            assert rec("product route score", float((v.best.double() - got.score[:, m]).abs().max())) <= 2e-5


def test_beyond_the_row_limit(dev):
    """The 1200-state lattice whose product with the string's automaton does not fit: intersect refuses it, the sweep
    over the lattice itself aligns (test_shared_cases holds the answer to the restatement)."""
    case = AR.sample_cases()["layered"]
    lat = LatticeBatch.from_synth(case["lats"], device=dev)
    with pytest.raises(_lib.NfstError) as e:
        ops.intersect(lat, WideDFA.projected_sequence(12, case["tape"]["keep"], case["cands"][0][0]))
    assert e.value.code == -6  # NFST_ERR_LIMIT
    a, kw = _args(case, dev)
    v = ops.string_viterbi(lat, *a, **kw)
    y = case["cands"][0][0]
    assert len(y) > 10 and int(v.lengths[0, 0]) > len(y) and int((v.align[0, 0] >= 0).sum()) == len(y) and bool(torch.isfinite(v.score[0, 0]))


def test_errors_leave_the_other_candidates(dev):
    """A bad length and a short max_len: NFST_ERR_LENGTH after the launch, the other candidates' answers intact; the
    shape of the uniforms is checked on the host."""
    case = AR.sample_cases()["tape"]
    lat = LatticeBatch.from_synth(case["lats"], device=dev)
    (theta, rows, n), kw = _args(case, dev)
    M, L, K = rows.shape[1], case["L"], 2
    good_v = ops.string_viterbi(lat, theta, rows, n, **kw)
    good_d = ops.string_sample_paths(lat, theta, rows, n, K, seed=3, **kw)
    bad = n.clone()
    bad[0, 1], bad[0, 3] = rows.shape[2] + 1, -1
    for f in (lambda **k: ops.string_viterbi(lat, theta, rows, bad, **k), lambda **k: ops.string_sample_paths(lat, theta, rows, bad, K, seed=3, **k)):
        with pytest.raises(_lib.NfstError) as e:
            f(**kw)
        assert e.value.code == _lib.ERR_LENGTH
    with pytest.raises(ValueError, match="uniforms"):
        ops.string_sample_paths(lat, theta, rows, n, K, uniforms=torch.zeros((1, M, K, L + 1), device=dev), **kw)
    # the raw entry points: the status word, and what the launch left
    sc, alive = ops._scores(lat, theta, None)
    ws, ws_bytes = ops._workspace(lat, "nfst_string_sample_ws_bytes", M, rows.shape[2], 1)
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    keepers = torch.ones(M, dtype=torch.bool, device=dev)
    keepers[1] = keepers[3] = False

    def raw(lengths, max_len, sample):
        lead = (1, M, K) if sample else (1, M)
        o = dict(score=torch.empty(lead, **f64), logq=torch.empty(lead, **f64), paths=torch.empty(lead + (max_len,), **i32),
                 arcs=torch.empty(lead + (max_len,), **i32), align=torch.empty(lead + (max_len,), **i32), lens=torch.empty(lead, **i32),
                 num=torch.empty((1, M), **f64), z=torch.empty(1, **f64), status=torch.zeros(1, **i32))
        if sample:
            ops._call("nfst_string_sample", lat, sc, rows, lengths, M, rows.shape[2], None, MARK, K, 0, None, C.c_uint64(3), max_len, PAD, ws,
                      ws_bytes, o["num"], o["z"], o["score"], o["logq"], o["paths"], o["arcs"], o["align"], o["lens"], o["status"])
        else:
            ops._call("nfst_string_viterbi", lat, sc, rows, lengths, M, rows.shape[2], None, MARK, max_len, PAD, ws, ws_bytes, o["score"],
                      o["paths"], o["arcs"], o["align"], o["lens"], o["status"])
        return o

    for sample, good in ((False, good_v), (True, good_d)):
        o = raw(bad, L, sample)
        assert int(o["status"].item()) == _lib.ERR_LENGTH
        for k in ("score", "paths", "arcs", "align"):
            g = getattr(good, k)
            assert torch.equal(o[k][0, keepers].view(torch.int64 if g.dtype == torch.float64 else g.dtype),
                               g[0, keepers].view(torch.int64 if g.dtype == torch.float64 else g.dtype)), (sample, k)
        assert torch.equal(o["lens"][0, keepers], good.lengths[0, keepers])
        assert bool(o["score"][0, ~keepers].isneginf().all()) and int(o["lens"][0, ~keepers].max()) == 0
        assert bool((o["paths"][0, ~keepers] == PAD).all()) and bool((o["align"][0, ~keepers] == -1).all()) and bool((o["arcs"][0, ~keepers] == -1).all())
        if sample:
            assert float(o["logq"][0, ~keepers].abs().max()) == 0.0 and torch.equal(o["logq"][0, keepers], good.logq[0, keepers])
        # max_len one short of the longest answer: that answer is cut at max_len, the shorter ones are whole
        longest = int(good.lengths.max())
        o = raw(n, longest - 1, sample)
        assert int(o["status"].item()) == _lib.ERR_LENGTH
        short = good.lengths[0] < longest
        assert bool(short.any()) and torch.equal(o["lens"][0][short], good.lengths[0][short])
        assert torch.equal(o["paths"][0][short], good.paths[0][short][..., :longest - 1]) and int(o["lens"].max()) == longest - 1
    with pytest.raises(_lib.NfstError) as e:
        ops.string_viterbi(lat, theta, rows, n, **{**kw, "max_len": int(good_v.lengths.max()) - 1})
    assert e.value.code == _lib.ERR_LENGTH
    del alive


def test_gradients(dev):
    """d string_viterbi.score / d arc_scores marks the path's arcs and d / d theta counts its labels; candidates of score
    -inf pass nothing back.  string_alignment_log_prob equals the draws' logq, and its gradient is the path's indicator
    less the arc posteriors given the string: the closed form of the gradient, from the float64 restatement
    (strings_grad_ref.posteriors), within that module's bound."""
    case = AR.sample_cases()["mixed"]
    lats = case["lats"]
    lat = LatticeBatch.from_synth(lats, device=dev)
    (theta, rows, n), kw = _args(case, dev)
    off = _offsets(lats)
    B, M, A, Vb = len(lats), rows.shape[1], int(off[-1]), lats[0].vocab
    th = theta.clone().requires_grad_()
    asc = kw["arc_scores"].clone().requires_grad_()
    v = ops.string_viterbi(lat, th, rows, n, **{**kw, "arc_scores": asc})
    coef = torch.from_numpy(np.random.default_rng(0).normal(size=(B, M))).to(dev)
    assert bool(v.score[:, 2].isneginf().all())
    (v.score * coef)[torch.isfinite(v.score)].sum().backward()
    want_arc, want_th = np.zeros(A), np.zeros((B, Vb))
    arcs, lens = v.arcs.cpu().numpy(), v.lengths.cpu().numpy()
    label = np.concatenate([l.label for l in lats])
    for b in range(B):
        for m in range(M):
            for a in arcs[b, m, :lens[b, m]]:
                want_arc[a] += float(coef[b, m])
                want_th[b, label[a]] += float(coef[b, m])
    assert lens[:, :2].min() > 0
    assert rec("viterbi grad arc", np.abs(asc.grad.cpu().numpy() - want_arc).max()) <= 1e-6  # (float32 sums of a few coefficients)
    assert rec("viterbi grad theta", np.abs(th.grad.cpu().numpy() - want_th).max()) <= 1e-5
    # string_alignment_log_prob on drawn alignments
    K = 4
    d = ops.string_sample_paths(lat, theta, rows, n, K, seed=2, **kw)
    th2 = theta.clone().requires_grad_()
    asc2 = kw["arc_scores"].to(torch.float64).clone().requires_grad_()
    lp = ops.string_alignment_log_prob(lat, th2, rows, n, d.arcs, d.lengths, arc_scores=asc2, **case["tape"])
    live = torch.isfinite(d.score)
    assert lp.shape == d.logq.shape and lp.dtype == torch.float64 and bool(live[:, :2].all()) and not bool(live[:, 2].any())
    assert rec("alignment_log_prob - logq", float((lp.detach() - d.logq)[live].abs().max())) <= BOUND and float(lp.detach()[~live].abs().max()) == 0.0
    c2 = torch.from_numpy(np.random.default_rng(1).normal(size=tuple(lp.shape))).to(dev)
    (lp * c2)[live].sum().backward()
    want = np.zeros(A)
    darcs, dlens, c2h = d.arcs.cpu().numpy(), d.lengths.cpu().numpy(), c2.cpu().numpy()
    a0 = 0
    for b, l in enumerate(lats):
        s64 = E.score64(l, case["theta"][b], case["asc"][off[b]:off[b + 1]])
        for m in range(2):
            post = GR.posteriors(l, s64, case["cands"][b][m], **case["tape"])[0]
            for k in range(K):
                want[off[b]:off[b + 1]] -= c2h[b, m, k] * post
                np.add.at(want, darcs[b, m, k, :dlens[b, m, k]], c2h[b, m, k])
    got = asc2.grad.cpu().numpy()
    assert rec("alignment_log_prob grad arc", np.abs(got - want).max()) <= GRAD_BOUND
    want_th = np.zeros((B, Vb))
    for b in range(B):
        np.add.at(want_th[b], label[off[b]:off[b + 1]], want[off[b]:off[b + 1]])
    assert rec("alignment_log_prob grad theta", np.abs(th2.grad.cpu().numpy() - want_th).max()) <= 1e-5  # (theta is float32)


def test_lattice_scorer_entries(dev):
    from tests import intersect_wide_ref as IW

    lats = [SR.denominator(SR.SEED1), SR.denominator(SR.SMALL), IW.edit_denominator([7, 6, 6, 8], [8, 9, 10], 2, vocab=12)]
    theta = synth.label_scores(1, 12, mean=-1.0, std=0.5)
    em, tr = synth.collate_dense([l.dense() for l in lats])
    sc = LatticeScorer(12, pad=PAD, bos=BOS, eos=EOS, theta=torch.from_numpy(theta)).to(dev)
    sc.set_masks(torch.as_tensor(em).to(dev), torch.as_tensor(tr).to(dev))
    rows, n = AR.rows([[[8], [8, 9], [], [11, 11, 11, 11]]] * 3)
    want = ops.string_viterbi(sc._lat(), _t(theta, dev), _t(rows, dev), _t(n, dev), marker=MARK, pad=PAD)
    got = sc.align(_t(rows, dev), _t(n, dev))
    assert len(got) == 3 and len(got[0]) == 4 and got[0][3] == (NEG, [], [])
    for b in range(3):
        for m in range(4):
            k = int(want.lengths[b, m])
            assert got[b][m] == (float(want.score[b, m]), want.paths[b, m, :k].tolist(), want.align[b, m, :k].tolist())
            assert SR.project(got[b][m][1], marker=MARK) == tuple(rows[b, m, :n[b, m]].tolist()) or m == 3
    d = sc.sample_alignments(_t(rows, dev), _t(n, dev), 5, seed=3)
    w = ops.string_sample_paths(sc._lat(), _t(theta, dev), _t(rows, dev), _t(n, dev), 5, marker=MARK, seed=3, pad=PAD)
    assert isinstance(d, ops.StringSampleResult) and _same(d, w) and d.paths.shape[:3] == (3, 4, 5)

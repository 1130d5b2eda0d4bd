"""ops.merge_paths (nfst_merge_paths), ops.string_log_prob (nfst_string_logprob) and the string decoders against the NumPy
restatements of tests/strings_ref.py: the merge exactly on every output, the weights' float64 bits included; the string
weights within BOUND, with -inf exactly where no path spells the string and the same bits at every launch, under every
packing and slicing.  tests/test_strings_cpu.py holds the restatements to brute force over every path.  The largest error
of every kind goes to strings_errors.json in the directory of run outputs (profiles/README.md)."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from nfst_amd import _lib, decoders, ops, strings, swor, synth
from nfst_amd.constraints import WideDFA
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from tests import edge_cases as E
from tests import pack_cases as PC
from tests import strings_ref as SR
from tests import structure_cases as S
from tests.test_lattice_edit_cpu import small_lattices

pytestmark = pytest.mark.gpu
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
NEG = -np.inf
MARK = SR.MARK
# The largest absolute error of log_num, logz and log_prob against strings_ref over this module's cases, measured on the
# MI355X, is 3.6e-15 (profiles/strings_errors.json); x 16 for the exp / log of two libraries differing by a few ulp per cell
# over the depth of a sweep, rounded up to a power of ten.
BOUND = 1e-13

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
            with open(os.path.join(out, "strings_errors.json"), "w") as f:
                json.dump(dict(sorted(_ERR.items())), f, indent=1)


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


# ============================================================================= merge_paths
KEEP = {3, 5, 7}
TAPES = {"keep": dict(keep=KEEP), "marker": dict(marker=MARK), "identity": {}}
V = 12


def _raw_merge(paths, lens, w, n_paths, tape, hash_bits=64, pad=PAD):
    """nfst_merge_paths without the wrapper's read-back of the status: (StringSet, status)"""
    mask, mk, vocab = strings._tape(tape.get("keep"), tape.get("marker"), V if tape else None, paths.device, need_one=False)
    out, status = strings._merge_launch(paths, lens, w, n_paths, mask, mk, vocab, pad, hash_bits)
    return out, int(status.item())


def _same(tag, got, want):
    for name in ops.StringSet._fields:
        g = getattr(got, name).cpu().numpy()
        if name == "log_weights":
            assert np.array_equal(_bits(g), _bits(want[name])), (tag, name, g, want[name])
        else:
            assert g.dtype == np.int32 and np.array_equal(g, want[name]), (tag, name)


def _merge_check(tag, dev, paths, lens, w, n_paths=None, tape=None, want_status=0):
    """The wrapper, and the raw entry point with 64 and with 1 bit of the hash, against the restatement."""
    tape = tape or {}
    want = SR.merge(paths, lens, w, n_paths, pad=PAD, **tape)
    tp, tl, tw, tn = _t(paths.astype(np.int32), dev), _t(lens.astype(np.int32), dev), _t(w.astype(np.float64), dev), _t(None if n_paths is None else np.asarray(n_paths, np.int32), dev)
    for bits in (64, 1):
        got, status = _raw_merge(tp, tl, tw, tn, tape, bits)
        assert status == want_status, (tag, bits, status)
        _same(f"{tag} hash_bits={bits}", got, want)
    if not want_status:
        _same(f"{tag} wrapper", ops.merge_paths(tp, tl, tw, tn, vocab=V if tape else None, pad=PAD, **tape), want)
    return want


def _random_set(seed, B, K, L, tail):
    """Rows drawn from a few base rows over the labels 3 .. 8 (so that strings repeat), a third of them one non-kept label
    longer (equal projection from rows of different raw length), behind every row's end ``tail``; weights in steps of
    0.5 (ties), some -inf and NaN."""
    rng = np.random.default_rng(seed)
    n_base = max(1, K // 3)
    base_len = rng.integers(0, L + 1, size=(B, n_base))
    base_len[:, 0] = L
    if n_base > 1:
        base_len[:, 1] = 0
    base = rng.integers(3, 9, size=(B, n_base, L))
    pick = rng.integers(0, n_base, size=(B, K))
    paths = np.take_along_axis(base, pick[:, :, None], axis=1)
    lens = np.take_along_axis(base_len, pick, axis=1)
    longer = (rng.random((B, K)) < 0.33) & (lens < L)
    for b, k in zip(*np.nonzero(longer)):
        paths[b, k, lens[b, k]] = 6
    lens = lens + longer
    paths = np.where(np.arange(L)[None, None, :] < lens[:, :, None], paths, tail)
    w = np.round(rng.normal(-3.0, 1.5, size=(B, K)) * 2) / 2
    w[rng.random((B, K)) < 0.05] = NEG
    w[rng.random((B, K)) < 0.03] = np.nan
    return paths, lens, w


@pytest.mark.parametrize("K,L", [(1, 65), (2, 1), (63, 63), (64, 64), (65, 129), (256, 65), (1024, 63), (65, 1), (1024, 129)])
@pytest.mark.parametrize("mode", list(TAPES))
def test_merge_sizes(dev, K, L, mode):
    """Every K and raw L around the waves' 64 lanes; the tail behind every row's end would change the strings if read, and
    the answer is the same under two tails."""
    wants = []
    for tail in (MARK, 7):
        paths, lens, w = _random_set(K * 1000 + L, 2, K, L, tail)
        wants.append(_merge_check(f"{mode} K={K} L={L} tail={tail}", dev, paths, lens, w, tape=TAPES[mode]))
    for name in wants[0]:
        assert np.array_equal(wants[0][name], wants[1][name], equal_nan=True)
    n = wants[0]["n_strings"]
    assert K < 3 or ((n >= 1) & (n < K)).all()  # (strings repeat)


def _rows(L, rows, tail=MARK):
    """paths [1, K, L] and lengths from lists of tokens"""
    paths = np.full((1, len(rows), L), tail, np.int64)
    for k, r in enumerate(rows):
        paths[0, k, :len(r)] = r
    return paths, np.array([[len(r) for r in rows]])


def test_merge_kept_positions_and_projected_lengths(dev):
    """Kept tokens at positions 63, 64 and the last one, directly behind a marker at position 63, a run of markers across
    the chunk boundary, a marker at the very end; projected lengths 0, 1, 64 and 65."""
    L, f = 129, 6  # (6 is on neither tape)
    at = lambda pos, tok, n=L: [tok if i in pos else f for i in range(n)]
    keep_rows = [at({63}, 5), at({64}, 5), at({128}, 5), at({63}, 5, 64), at({64}, 5, 65), at(set(), 5), [], [5], [5] * 64 + [f] * 65,
                 [f] * 64 + [5] * 65, [5] * 65, [3, 5] * 32, [5] * 64, at({63, 64}, 5), at({0, 128}, 7), at({0, 128}, 7, 128) + [3]]
    paths, lens = _rows(L, keep_rows, tail=5)
    w = np.linspace(-4.0, -1.0, len(keep_rows))[None, :]
    want = _merge_check("keep positions", dev, paths, lens, w, tape=TAPES["keep"])
    assert {0, 1, 64, 65} <= set(want["lengths"][0, :want["n_strings"][0]].tolist())
    _merge_check("identity positions", dev, paths, lens, w)
    m = MARK
    mk = lambda pairs, n=L: [dict(pairs).get(i, f) for i in range(n)]
    marker_rows = [mk([(63, m), (64, 8)]), mk([(63, m), (64, 8)], 65), mk([(63, m)], 64), mk([(127, m), (128, 8)]), mk([(128, m)]),
                   mk([(i, m) for i in range(60, 67)]), mk([(i, m) for i in range(59, 67)]), [m] * 129, [m] * 128, [m, 8] * 64,
                   [m, m] * 64 + [m], [f] + [m, 8] * 64, [m, 8], [f, m, 8, f], [m], [], mk([(62, m), (63, m), (64, m), (65, 9)]),
                   mk([(62, m), (63, 9)]), mk([(62, m), (63, 10)])]
    paths, lens = _rows(L, marker_rows, tail=m)
    w = np.linspace(-2.0, -5.0, len(marker_rows))[None, :]
    want = _merge_check("marker positions", dev, paths, lens, w, tape=TAPES["marker"])
    got_lens = set(want["lengths"][0, :want["n_strings"][0]].tolist())
    assert {0, 1, 64} <= got_lens and want["group"][0, 0] == want["group"][0, 1] != want["group"][0, 2]
    assert want["group"][0, 17] != want["group"][0, 18]  # equal length, different last token
    # 65 symbols behind markers need 130 tokens
    paths, lens = _rows(130, [[m, 8] * 65, [m, 8] * 64 + [f, f], [m, m] * 65])
    want = _merge_check("marker 65", dev, paths, lens, np.array([[-1.0, -2.0, -3.0]]), tape=TAPES["marker"])
    assert want["lengths"][0].tolist() == [65, 64, 65]


def test_merge_group_structures(dev):
    rng = np.random.default_rng(1)
    K, L = 64, 70
    same = np.tile(rng.integers(3, 9, size=(1, 1, L)), (1, K, 1))
    lens = np.full((1, K), L)
    w = rng.normal(-3, 1, size=(1, K))
    want = _merge_check("all identical", dev, same, lens, w)
    assert want["n_strings"][0] == 1 and want["first"][0, 0] == int(np.argmax(w[0]))
    distinct = same.copy()
    distinct[0, :, L - 1] = 100 + np.arange(K)  # equal length and hash prefix, different last token
    want = _merge_check("all distinct", dev, distinct, lens, w)
    assert want["n_strings"][0] == K and np.array_equal(want["first"][0], np.argsort(-w[0], kind="stable"))
    ties = np.full((1, K), -2.0)  # every merged weight the same: the order is that of the lowest member
    want = _merge_check("ties", dev, distinct, lens, ties)
    assert np.array_equal(want["first"][0], np.arange(K))
    want = _merge_check("pair ties", dev, np.concatenate([distinct[:, :32], distinct[:, :32]], axis=1), lens, ties)
    assert want["n_strings"][0] == 32 and np.array_equal(want["group"][0], np.tile(np.arange(32), 2))


def test_merge_invalid_rows(dev):
    paths, lens, w = _random_set(5, 3, 65, 40, 7)
    n_paths = np.array([65, 20, 0])
    w[0, :] = np.where(np.arange(65) % 2 == 0, NEG, np.nan)  # an all-invalid set by its weights, and one by n_paths
    want = _merge_check("invalid rows", dev, paths, lens, w, n_paths, tape=TAPES["marker"])
    assert want["n_strings"].tolist()[0] == 0 == want["n_strings"].tolist()[2] < want["n_strings"].tolist()[1]
    assert (want["group"][1, 20:] == -1).all() and (want["group"][[0, 2]] == -1).all()


def test_merge_length_outside_its_row(dev):
    paths, lens, w = _random_set(6, 2, 9, 33, 7)
    w = np.nan_to_num(w, nan=-1.0, neginf=-2.0)
    lens[1, 4] = 34
    _merge_check("bad length", dev, paths, lens, w, tape=TAPES["keep"], want_status=_lib.ERR_LENGTH)
    with pytest.raises(_lib.NfstError) as e:
        ops.merge_paths(_t(paths, dev), _t(lens, dev), _t(w, dev), keep=KEEP, vocab=V)
    assert e.value.code == _lib.ERR_LENGTH


def test_merge_input_forms(dev):
    """int64 paths and lengths, float32 weights, views that are not contiguous"""
    paths, lens, w = _random_set(7, 2, 20, 31, 7)
    w = np.nan_to_num(w, nan=NEG, neginf=NEG).astype(np.float32)
    want = SR.merge(paths, lens, w.astype(np.float64), marker=MARK, pad=PAD)
    wide = torch.full((2, 20, 62), 9, dtype=torch.int64, device=dev)
    wide[:, :, ::2] = _t(paths, dev)
    wt = _t(np.ascontiguousarray(w.T), dev).t()
    assert not wide[:, :, ::2].is_contiguous() and not wt.is_contiguous()
    _same("views", ops.merge_paths(wide[:, :, ::2], _t(lens, dev), wt, marker=MARK, vocab=V, pad=PAD), want)
    empty = ops.merge_paths(torch.zeros((2, 0, 5), dtype=torch.int32, device=dev), torch.zeros((2, 0), dtype=torch.int32, device=dev),
                            torch.zeros((2, 0), device=dev), marker=MARK)
    assert empty.n_strings.tolist() == [0, 0] and empty.strings.shape == (2, 0, 5)


def test_merge_gradient(dev):
    paths, lens, w = _random_set(8, 2, 30, 12, 7)
    w = np.nan_to_num(w, nan=NEG) + np.random.default_rng(0).normal(0, 0.1, size=w.shape)
    want = SR.merge(paths, lens, w, keep=KEEP, pad=PAD)
    coef = np.random.default_rng(1).normal(size=w.shape)
    x = _t(w, dev).requires_grad_()
    out = ops.merge_paths(_t(paths, dev), _t(lens, dev), x, keep=KEEP, vocab=V, pad=PAD)
    live = torch.isfinite(out.log_weights.detach())
    (out.log_weights[live] * _t(coef, dev)[live]).sum().backward()
    x64 = torch.from_numpy(w).requires_grad_()
    loss = 0.0
    for b in range(2):
        for g in range(int(want["n_strings"][b])):
            loss = loss + coef[b, g] * torch.logsumexp(x64[b][torch.from_numpy(want["group"][b] == g)], dim=0)
    loss.backward()
    assert float((x.grad.cpu() - x64.grad).abs().max()) <= 1e-12 and float(x.grad.abs().sum()) > 1


@pytest.fixture(scope="module")
def grids():
    """The denominator batch: three edit grids over 12 labels, and label scores under which the best string of the first
    is not its Viterbi path's (test_strings_cpu.py)."""
    from tests import intersect_wide_ref as IW

    lats = [SR.denominator(SR.SEED1), SR.denominator(SR.SMALL), IW.edit_denominator([7, 6, 6, 8], [8, 9, 10], 2, vocab=12)]
    return lats, synth.label_scores(1, 12, mean=-1.0, std=0.5)


def test_merge_real_paths(dev, grids):
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    kb = ops.k_best(lat, _t(theta, dev), 64, pad=PAD)
    sw = swor.sample(lat, _t(theta, dev), 64, seed=3, pad=PAD)
    for tag, r, w in (("k_best", kb, kb.best.double()), ("swor", sw, swor.log_weights(sw))):
        got = ops.merge_paths(r.paths, r.lengths, w, r.n_paths, marker=MARK, vocab=12, pad=PAD)
        want = SR.merge(r.paths.cpu().numpy(), r.lengths.cpu().numpy(), w.cpu().numpy(), r.n_paths.cpu().numpy(), marker=MARK, pad=PAD)
        _same(tag, got, want)
        assert (want["n_strings"] < r.n_paths.cpu().numpy()).all()
    assert int(got.n_strings[0]) > 10


# ============================================================================= string_log_prob
def _cand_rows(cands, N=None, tail=8):
    """(strings [B, M, N] int32 with every row's tail filled with ``tail``, lengths [B, M])"""
    n = np.array([[len(y) for y in row] for row in cands], np.int32)
    out = np.full((len(cands), len(cands[0]), max(1, int(n.max()) if N is None else N)), tail, np.int32)
    for b, row in enumerate(cands):
        for m, y in enumerate(row):
            out[b, m, :len(y)] = y
    return out, n


def _slp(lat, theta, cands, tape, dev, asc=None, N=None, **kw):
    rows, n = _cand_rows(cands, N)
    return ops.string_log_prob(lat, _t(theta, dev), _t(rows, dev), _t(n, dev), arc_scores=_t(asc, dev), **tape, **kw)


def _hold(tag, got, num, z):
    """``got`` against the restatement's (log_num [B, M], logz [B]): -inf exactly, everything else within BOUND"""
    g_num, g_z, g_p = (x.cpu().numpy() for x in got)
    dead = np.isneginf(num)
    assert np.array_equal(np.isneginf(g_num), dead) and np.array_equal(np.isneginf(g_p), dead), tag
    assert not np.isnan(g_num).any() and not np.isnan(g_p).any() and not np.isnan(g_z).any(), tag
    want_p = num - z[:, None]
    live = ~dead
    if live.any():
        assert rec(f"{tag.split(':')[0]} log_num", np.abs(g_num[live] - num[live]).max()) <= BOUND, tag
        assert rec(f"{tag.split(':')[0]} log_prob", np.abs(g_p[live] - want_p[live]).max()) <= BOUND, tag
        assert (g_p[live] <= BOUND).all(), tag
    assert rec(f"{tag.split(':')[0]} logz", np.abs(g_z - z).max()) <= BOUND, tag


@pytest.fixture(scope="module")
def long_grid():
    """One edit grid that spells every string over {8, 9} of up to 129 symbols, in both tape modes (its x is on neither
    tape), with 65 candidates (16 distinct ones): the lengths around the strips of 64 columns first, and their restatement in marker mode."""
    from tests import intersect_wide_ref as IW

    l = IW.edit_denominator([6], [8, 9], 129, vocab=12)
    theta = synth.label_scores(4, 12, mean=-1.0, std=0.5)
    rng = np.random.default_rng(2)
    lens = [0, 1, 63, 64, 65, 128, 129] + [int(x) for x in rng.integers(0, 130, size=9)]
    pool = [[int(t) for t in rng.integers(8, 10, size=n)] for n in lens]
    s64 = E.score64(l, theta)
    pool_ref = [SR.string_log_prob(l, s64, y, marker=MARK) for y in pool]
    cands, ref = [pool[i % 16] for i in range(65)], [pool_ref[i % 16] for i in range(65)]  # (65 candidates, 16 distinct)
    return l, theta, cands, np.array([[r[0] for r in ref]]), np.array([ref[0][1]])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128])
def test_strips(dev, long_grid, n):
    """N + 1 in {1, 2, 64, 65, 66, 129}: a strip, the strip boundary, three strips.  The row stride is the length itself,
    so nothing lies behind the candidate; keep mode gives the marker mode's value (the kept labels are the symbols)."""
    l, theta, cands, num, z = long_grid
    lat = LatticeBatch.from_synth([l], device=dev)
    i = [0, 1, 63, 64, 65, 128].index(n)
    for tape in (dict(marker=MARK), dict(keep={8, 9})):
        got = _slp(lat, theta, [[cands[i]]], tape, dev, N=max(n, 1))
        _hold(f"strips: n={n} {tape}", got, num[:, i:i + 1], z)
        again = _slp(lat, theta, [[cands[i]]], tape, dev, N=max(n, 1))
        assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("M", [1, 3, 65])
def test_candidates_of_different_lengths_in_one_launch(dev, long_grid, M):
    l, theta, cands, num, z = long_grid
    lat = LatticeBatch.from_synth([l], device=dev)
    pick = list(range(65)) if M == 65 else [5, 0, 3][:M]
    got = _slp(lat, theta, [[cands[i] for i in pick]], dict(marker=MARK), dev, N=130)
    _hold(f"mixed lengths: M={M}", got, num[:, pick], z)
    sliced = _slp(lat, theta, [[cands[i] for i in pick]], dict(marker=MARK), dev, N=130, max_workspace_bytes=5 << 20)
    assert all(torch.equal(a, b) for a, b in zip(got, sliced))  # (5 MiB: one or two candidates per slice)
    # a string one symbol longer than any path spells, and the length error
    if M == 3:
        got = _slp(lat, theta, [[cands[6] + [8], cands[6], []]], dict(marker=MARK), dev, N=130)
        assert got.log_num[0].isneginf().tolist() == [True, False, False]
        rows, n = _cand_rows([[cands[1], cands[2], cands[3]]], N=70)
        n[0, 1] = 71
        with pytest.raises(_lib.NfstError) as e:
            ops.string_log_prob(lat, _t(theta, dev), _t(rows, dev), _t(n, dev), marker=MARK)
        assert e.value.code == _lib.ERR_LENGTH
        with pytest.raises(ValueError, match="max_workspace_bytes"):
            _slp(lat, theta, [[cands[5]]], dict(marker=MARK), dev, N=130, max_workspace_bytes=1 << 20)


def test_a_bad_length_leaves_the_other_candidates(dev, grids):
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    cands = [[[8], [8, 9], []]] * 3
    rows, n = _cand_rows(cands, N=4)
    good = ops.string_log_prob(lat, _t(theta, dev), _t(rows, dev), _t(n, dev), marker=MARK)
    n[1, 0], n[2, 2] = 5, -1
    sc, keep_alive = ops._scores(lat, _t(theta, dev), None)
    ws, ws_bytes = ops._workspace(lat, "nfst_string_logprob_ws_bytes", 3, 4, 1)
    num, z = torch.empty((3, 3), dtype=torch.float64, device=dev), torch.empty(3, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ops._call("nfst_string_logprob", lat, sc, _t(rows, dev), _t(n, dev), 3, 4, None, MARK, ws, ws_bytes, num, z, status)
    assert int(status.item()) == _lib.ERR_LENGTH
    bad = torch.zeros((3, 3), dtype=torch.bool, device=dev)
    bad[1, 0] = bad[2, 2] = True
    assert bool(num[bad].isneginf().all()) and torch.equal(num[~bad], good.log_num[~bad]) and torch.equal(z, good.logz)


def _enumerable():
    out = [(f"small{i}", l, 50 + i) for i, l in enumerate(small_lattices())]
    return out + [("seed1", SR.denominator(SR.SEED1), 1), ("grid2", SR.denominator(SR.SMALL), 2), ("tape", SR.tape_lattice(), 3)]


@pytest.mark.parametrize("case", range(7))
def test_every_string_of_an_enumerable_lattice(dev, case):
    """All distinct strings of a lattice in one launch against brute force over its paths (float64 sums of exp): every
    log_prob within BOUND, their exps add up to 1 (less the share of the paths that end on a marker), and strings that no
    path spells -- one symbol more, one symbol less, the empty one where every path spells something -- get -inf."""
    name, l, seed = _enumerable()[case]
    theta = synth.label_scores(seed, l.vocab, mean=-1.0, std=0.5)
    s64 = E.score64(l, theta)
    lat = LatticeBatch.from_synth([l], device=dev)
    labels = sorted(set(int(x) for x in l.label))
    for tape in (dict(keep=set(labels[1::2]) | {EOS}), dict(marker=MARK if MARK in labels else labels[len(labels) // 2])):
        by, logz, paths = SR.brute_force(l, s64, **tape)
        ys = sorted(by, key=lambda y: -by[y])
        extra = [ys[0] + ys[0][-1:], ys[0][:-1], (), tuple(ys[-1]) + (labels[-1],) * 3]
        cands = [[list(y) for y in ys + extra]]
        num = np.array([[by.get(tuple(y), NEG) for y in cands[0]]])
        got = _slp(lat, theta, cands, tape, dev)
        _hold(f"enumerable: {name} {sorted(tape)}", got, num, np.array([logz]))
        lost = sum(np.exp(sc - logz) for sc, p in paths if "marker" in tape and SR.dangling(l.label[p], tape["marker"]))
        total = float(torch.exp(got.log_prob[0, :len(ys)]).sum())
        assert rec("enumerable sum of p", abs(total + lost - 1.0)) <= BOUND, (name, tape)
        assert np.isneginf(num[0, len(ys):]).any()


NAMES = tuple(S.batches())


@pytest.mark.parametrize("name", NAMES)
def test_structure_corpus(dev, name):
    """The corpus of tests/structure_cases.py through both tape modes, with per-arc scores (and the tables' weights in the
    weighted batch): three candidates per lattice -- the string of a path, the empty string, a string that no path
    spells -- against the restatement, and the same bits from both packers and under the three group modes."""
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
        num, z = SR.of_batch(lats, theta, cands, asc=asc, **tape)
        first_bits = None
        for route, gm in (("host", 0), ("device", 0), ("host", 1), ("host", 2), ("device", 2)):
            if route == "host":
                lat = LatticeBatch.from_arcs(n_rows, arc_off, src, label, dst, Vb, arc_w=w, group_mode=gm).to(dev, auto_chunks=False)
            else:
                lat = LatticeBatch.from_arcs_device(n_rows, arc_off, src, label, dst, Vb, arc_w=w, device=dev, group_mode=gm)
            got = _slp(lat, theta, cands, tape, dev, asc=asc)
            if first_bits is None:
                _hold(f"structure: {name} {sorted(tape)}", got, num, z)
                first_bits = got
            assert all(torch.equal(a, b) for a, b in zip(got, first_bits)), (name, route, gm)
        assert np.isfinite(num[:, 0]).all() or name == "many_with_junk" or "marker" in tape
        degenerate = [b for b, l in enumerate(lats) if l.n_arcs == 0]  # state 0 is the sink: the empty path alone
        for b in degenerate:
            assert num[b].tolist() == [0.0, 0.0, NEG] and z[b] == 0.0
            assert first_bits.log_num[b].tolist() == [0.0, 0.0, NEG] and float(first_bits.logz[b]) == 0.0


def test_agreement_with_the_product_route(dev, grids):
    """Where the product fits, log_prob is ``ops.constraint_log_prob`` on the matching automaton, within the float32
    bound of tests/test_gpu_intersect_wide.py (2e-5: two log Z, each held to 1e-5)."""
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    ys = [[8], [8, 9], [], [9, 8]]
    got = _slp(lat, theta, [ys] * 3, dict(marker=MARK), dev)
    kept = _slp(lat, theta, [ys] * 3, dict(keep={8, 9, 10}), dev)
    for m, y in enumerate(ys):
        lp = ops.constraint_log_prob(lat, _t(theta, dev), WideDFA.marked_sequence(12, MARK, y))
        assert rec("product route marker", float((lp.double() - got.log_prob[:, m]).abs().max())) <= 2e-5
        if y:
            lp = ops.constraint_log_prob(lat, _t(theta, dev), WideDFA.projected_sequence(12, {8, 9, 10}, y))
            assert rec("product route keep", float((lp.double() - kept.log_prob[:, m]).abs().max())) <= 2e-5


def test_beyond_the_row_limit(dev):
    """The 1200-state lattice whose product with the string's automaton has 15 934 live pairs: ``intersect`` refuses it,
    the sweep over the lattice itself returns the restatement's value."""
    l, keep, y = SR.layered_case()
    theta = synth.label_scores(2, 12)
    lat = LatticeBatch.from_synth([l], device=dev)
    with pytest.raises(_lib.NfstError) as e:
        ops.intersect(lat, WideDFA.projected_sequence(12, keep, y))
    assert e.value.code == -6  # NFST_ERR_LIMIT
    num, z = SR.string_log_prob(l, E.score64(l, theta), y, keep=keep)
    got = _slp(lat, theta, [[y, y[:-1], y + [3]]], dict(keep=keep), dev)
    _hold("row limit: layered", got._replace(log_num=got.log_num[:, :1], log_prob=got.log_prob[:, :1]), np.array([[num]]), np.array([z]))
    assert NEG < num < z


# ============================================================================= the decoders
def test_decode_strings_on_the_denominator(dev, grids):
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    th = _t(theta, dev)
    r = decoders.decode_strings(lat, th, 64, marker=MARK, rescore=True, pad=PAD)
    v = ops.viterbi(lat, th, pad=PAD)
    assert SR.project(v.paths[0, :int(v.lengths[0])].tolist(), marker=MARK) == ()
    assert r.strings[0, 0, :int(r.lengths[0, 0])].tolist() == [8]  # the best string is not the Viterbi path's
    for b, l in enumerate(lats):
        by, logz, _ = SR.brute_force(l, E.score64(l, theta), marker=MARK)
        n = int(r.n_strings[b])
        for j in range(n):
            y = tuple(r.strings[b, j, :int(r.lengths[b, j])].tolist())
            assert rec("decode log_prob", abs(float(r.log_prob[b, j]) - (by[y] - logz))) <= BOUND
        lp = r.log_prob[b, :n]
        assert bool((lp[:-1] >= lp[1:]).all()) and bool((r.path_mass[b, :n] <= lp + BOUND).all())
        assert bool(r.log_prob[b, n:].isneginf().all()) and bool((r.first_path[b, n:] == -1).all())
    # rescore=False: the merged order, which the restatement reproduces from the same paths
    kb = ops.k_best(lat, th, 64, pad=PAD)
    w64 = decoders.path_scores64(lat, th, kb)  # (the scores of ``best`` summed in float64, as decode_strings weighs the paths)
    assert float((w64 - kb.best.double())[torch.isfinite(kb.best)].abs().max()) <= 1e-5
    want = SR.merge(kb.paths.cpu().numpy(), kb.lengths.cpu().numpy(), w64.cpu().numpy(), kb.n_paths.cpu().numpy(), marker=MARK, pad=PAD)
    m = decoders.decode_strings(lat, th, 64, marker=MARK, rescore=False, pad=PAD)
    assert np.array_equal(m.strings.cpu().numpy(), want["strings"]) and np.array_equal(m.first_path.cpu().numpy(), want["first"])
    assert torch.equal(m.log_prob, m.path_mass) and np.array_equal(m.n_strings.cpu().numpy(), want["n_strings"])
    live = np.arange(64)[None, :] < want["n_strings"][:, None]
    z = ops.string_log_prob(lat, th, r.strings[:, :1], r.lengths[:, :1], marker=MARK).logz.cpu().numpy()
    assert np.array_equal(m.path_mass.cpu().numpy()[live], (want["log_weights"] - z[:, None])[live])
    s = decoders.decode_strings(lat, th, 64, marker=MARK, method="swor", seed=5, pad=PAD)
    assert s.strings[0, 0, :int(s.lengths[0, 0])].tolist() == [8]
    # minimum Bayes risk over the strings is mbr_select fed the restatement's table
    st = ops.merge_paths(kb.paths, kb.lengths, w64, kb.n_paths, marker=MARK, vocab=12, pad=PAD)
    index, risk, D = decoders.mbr_decode_strings(st)
    Dw = ops.pairwise_edit_distance(_t(want["strings"], dev), _t(want["lengths"], dev))
    iw, rw = decoders.mbr_select(Dw, _t(want["log_weights"], dev), _t(want["n_strings"], dev))
    assert torch.equal(index, iw) and torch.equal(risk, rw) and torch.equal(D, Dw) and bool((index >= 0).all())


def test_lattice_scorer_strings(dev, grids):
    lats, theta = grids
    em, tr = synth.collate_dense([l.dense() for l in lats])
    sc = LatticeScorer(12, pad=PAD, bos=BOS, eos=EOS, theta=torch.from_numpy(theta)).to(dev)
    sc.set_masks(torch.as_tensor(em).to(dev), torch.as_tensor(tr).to(dev))
    r = decoders.decode_strings(sc._lat(), _t(theta, dev), 16, marker=MARK, pad=PAD)
    want = [[(float(r.log_prob[b, j]), r.strings[b, j, :int(r.lengths[b, j])].tolist()) for j in range(int(r.n_strings[b]))] for b in range(3)]
    assert sc.decode_strings(16, marker=MARK) == want and want[0][0][1] == [8]
    lp = sc.string_log_prob(r.strings, r.lengths, marker=MARK)
    live = torch.arange(16, device=dev)[None, :] < r.n_strings[:, None]
    assert torch.equal(lp[live], r.log_prob[live])

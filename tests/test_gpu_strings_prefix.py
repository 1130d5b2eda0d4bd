"""ops.string_prefix_log_prob (nfst_string_prefix), ops.string_next_log_probs (nfst_string_next) and
decoders.prefix_search against the NumPy restatement of tests/strings_prefix_ref.py: every output within BOUND, -inf
exactly where the restatement has it, and the same bits at every launch, under every packing and slicing.
tests/test_strings_prefix_cpu.py holds the restatement to brute force over every path.  The largest error of every kind
goes to strings_prefix_errors.json in the directory of run outputs (profiles/README.md)."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from nfst_amd import _lib, decoders, ops, synth
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from tests import edge_cases as E
from tests import pack_cases as PC
from tests import strings_prefix_ref as PR
from tests import strings_ref as SR
from tests import structure_cases as S

pytestmark = pytest.mark.gpu
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
NEG = -np.inf
MARK = SR.MARK
# The largest absolute error over this module's cases, measured on the MI355X (profiles/strings_prefix_errors.json): 1.4e-14
# against strings_prefix_ref (next on the 1200-state lattice, where the weights are near -85 and one ulp is 1.4e-14) and
# 2.8e-14 between two device results there; on the other cases at most 3.6e-15, and 0 on the long edit grid.  The worst x 16
# for the exp / log of two libraries differing by a few ulp per cell over the depth of a sweep is 4.5e-13; rounded up to a
# power of ten:
BOUND = 1e-12

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
            with open(os.path.join(out, "strings_prefix_errors.json"), "w") as f:
                json.dump(dict(sorted(_ERR.items())), f, indent=1)


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _rows(cands, N=None, tail=8):
    """(prefixes [B, M, N] int32 with every row's tail filled with ``tail``, lengths [B, M])"""
    n = np.array([[len(y) for y in row] for row in cands], np.int32)
    out = np.full((len(cands), len(cands[0]), max(1, int(n.max()) if N is None else N)), tail, np.int32)
    for b, row in enumerate(cands):
        for m, y in enumerate(row):
            out[b, m, :len(y)] = y
    return out, n


def _both(lat, theta, cands, tape, dev, asc=None, N=None, **kw):
    """(PrefixScores, NextSymbols) of per-lattice prefix lists"""
    rows, n = _rows(cands, N)
    a = (lat, _t(theta, dev), _t(rows, dev), _t(n, dev))
    return (ops.string_prefix_log_prob(*a, arc_scores=_t(asc, dev), **tape, **kw), ops.string_next_log_probs(*a, arc_scores=_t(asc, dev), **tape, **kw))


def _ref(lats, theta, cands, tape, asc=None):
    """The restatement's (next [B, M, V], eos, log_prefix (F route), log_prefix (H route) [B, M], logz [B])"""
    B, M, V = len(lats), len(cands[0]), lats[0].vocab
    nxt, eos, pf, ph, z = np.full((B, M, V), NEG), np.full((B, M), NEG), np.full((B, M), NEG), np.full((B, M), NEG), np.zeros(B)
    a0 = 0
    for b, l in enumerate(lats):
        s64 = E.score64(l, theta[b] if np.ndim(theta) == 2 else theta, None if asc is None else asc[a0:a0 + l.n_arcs])
        a0 += l.n_arcs
        seen = {}
        for m, y in enumerate(cands[b]):
            if tuple(y) not in seen:
                seen[tuple(y)] = PR.next_log_probs(l, s64, y, **tape) + (PR.prefix_log_prob(l, s64, y, **tape)[0],)
            nxt[b, m], eos[b, m], pf[b, m], z[b], ph[b, m] = seen[tuple(y)]
    return nxt, eos, pf, ph, z


def _near(tag, got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == np.float64 and not np.isnan(got).any(), tag
    dead = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), dead), (tag, got, want)
    if (~dead).any():
        err = rec(tag.split(":")[0], np.abs(got[~dead] - want[~dead]).max())
        print(f"{tag}: {err:.3g}")
        assert err <= BOUND, tag


def _hold(tag, got, ref):
    """(PrefixScores, NextSymbols) against ``_ref``'s tuple; ``tag`` = "kind of case: the case" """
    pre, ns = got
    nxt, eos, pf, ph, z = ref
    kind, case = tag.split(":")
    _near(f"{kind} next:{case}", ns.next, nxt)
    _near(f"{kind} eos:{case}", ns.eos, eos)
    _near(f"{kind} log_prefix F:{case}", ns.log_prefix, pf)
    _near(f"{kind} log_prefix H:{case}", pre.log_prefix, ph)
    _near(f"{kind} logz:{case}", ns.logz, z)
    _near(f"{kind} log_prob:{case}", pre.log_prob, ph - z[:, None])
    assert torch.equal(pre.logz, ns.logz), tag


def _same_bits(a, b):
    return all(torch.equal(x, y) for r, q in zip(a, b) for x, y in zip(r, q))


# ============================================================================= widths and candidate counts
LENS = [0, 1, 63, 64, 65, 128]
MODES = {"marker": dict(marker=MARK), "keep": dict(keep={8, 9})}


@pytest.fixture(scope="module")
def long_grid():
    """One edit grid that spells every string over {8, 9} of up to 129 symbols (its x is on neither tape), and 16 prefixes:
    the lengths around the strips of 64 columns first, one that no path spells (a 10) and random ones, each with its
    restatement in both tape modes."""
    from tests import intersect_wide_ref as IW

    l = IW.edit_denominator([6], [8, 9], 129, vocab=12)
    theta = synth.label_scores(4, 12, mean=-1.0, std=0.5)
    rng = np.random.default_rng(2)
    pool = [[int(t) for t in rng.integers(8, 10, size=n)] for n in LENS + [5] + [int(x) for x in rng.integers(0, 130, size=9)]]
    pool[6][2] = 10  # no path spells it
    refs = {mode: _ref([l], theta, [pool], tape) for mode, tape in MODES.items()}
    return l, theta, pool, refs


def _pick(ref, idx):
    nxt, eos, pf, ph, z = ref
    return nxt[:, idx], eos[:, idx], pf[:, idx], ph[:, idx], z


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", LENS)
def test_strips(dev, long_grid, n, mode):
    """N + 1 in {1, 2, 64, 65, 66, 129}: a strip, the strip boundary, three strips.  The row stride is the length itself,
    so nothing lies behind the prefix; the bits are the same at a second launch."""
    l, theta, pool, refs = long_grid
    lat = LatticeBatch.from_synth([l], device=dev)
    i = LENS.index(n)
    got = _both(lat, theta, [[pool[i]]], MODES[mode], dev, N=max(n, 1))
    _hold(f"strips: n={n} {mode}", got, _pick(refs[mode], [i]))
    assert _same_bits(got, _both(lat, theta, [[pool[i]]], MODES[mode], dev, N=max(n, 1)))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("M", [1, 3, 65])
def test_prefixes_of_different_lengths_in_one_launch(dev, long_grid, M, mode):
    """The empty prefix and the one that no path spells among them; slices of one or two prefixes give the same bits."""
    l, theta, pool, refs = long_grid
    lat = LatticeBatch.from_synth([l], device=dev)
    pick = [i % 16 for i in range(65)] if M == 65 else [5, 0, 6][:M]
    got = _both(lat, theta, [[pool[i] for i in pick]], MODES[mode], dev, N=130)
    _hold(f"mixed lengths: M={M} {mode}", got, _pick(refs[mode], pick))
    if M >= 3:
        bad = pick.index(6)
        assert bool(got[0].log_prefix[0, bad].isneginf()) and bool(got[1].next[0, bad].isneginf().all()) and bool(got[1].eos[0, bad].isneginf())
        per = 8 * 131 * (2 if mode == "marker" else 1) * lat.total_rows  # one prefix's cells
        sliced = _both(lat, theta, [[pool[i] for i in pick]], MODES[mode], dev, N=130, max_workspace_bytes=(2 << 20) + 2 * per)
        assert _same_bits(got, sliced)


def test_a_bad_length_sets_the_status_word(dev, long_grid):
    l, theta, pool, refs = long_grid
    lat = LatticeBatch.from_synth([l], device=dev)
    rows, n = _rows([[pool[1], pool[6], pool[0]]], N=6)
    good = _both(lat, theta, [[pool[1], pool[6], pool[0]]], dict(marker=MARK), dev, N=6)
    n[0, 1] = 7
    for f in (ops.string_prefix_log_prob, ops.string_next_log_probs):
        with pytest.raises(_lib.NfstError) as e:
            f(lat, _t(theta, dev), _t(rows, dev), _t(n, dev), marker=MARK)
        assert e.value.code == _lib.ERR_LENGTH
    sc, keep_alive = ops._scores(lat, _t(theta, dev), None)
    f64 = dict(dtype=torch.float64, device=dev)
    for bad_n in (7, -1):
        n[0, 1] = bad_n
        ws, ws_bytes = ops._workspace(lat, "nfst_string_next_ws_bytes", 3, 6, 1)
        nxt, eos, pre, z = torch.zeros((1, 3, 12), **f64), torch.zeros((1, 3), **f64), torch.zeros((1, 3), **f64), torch.zeros(1, **f64)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ops._call("nfst_string_next", lat, sc, _t(rows, dev), _t(n, dev), 3, 6, None, MARK, ws, ws_bytes, nxt, eos, pre, z, status)
        assert int(status.item()) == _lib.ERR_LENGTH
        assert bool(nxt[0, 1].isneginf().all()) and bool(eos[0, 1].isneginf()) and bool(pre[0, 1].isneginf())
        assert torch.equal(nxt[0, [0, 2]], good[1].next[0, [0, 2]]) and torch.equal(pre[0, [0, 2]], good[1].log_prefix[0, [0, 2]])
        ws, ws_bytes = ops._workspace(lat, "nfst_string_prefix_ws_bytes", 3, 6, 1)
        pre, status = torch.zeros((1, 3), **f64), torch.zeros(1, dtype=torch.int32, device=dev)
        ops._call("nfst_string_prefix", lat, sc, _t(rows, dev), _t(n, dev), 3, 6, None, MARK, ws, ws_bytes, pre, z, status)
        assert int(status.item()) == _lib.ERR_LENGTH and bool(pre[0, 1].isneginf())
        assert torch.equal(pre[0, [0, 2]], good[0].log_prefix[0, [0, 2]]) and torch.equal(z, good[0].logz)


# ============================================================================= the structural corpus
@pytest.mark.parametrize("name", tuple(S.batches()))
def test_structure_corpus(dev, name):
    """The corpus of tests/structure_cases.py (self loops, states that state 0 does not reach, a lattice whose state 0 is
    the sink) through both tape modes, with per-arc scores (and the tables' weights in the weighted batch): three prefixes
    per lattice -- half of a path's string, the empty one, one that no path spells -- against the restatement, eos and
    logz against ops.string_log_prob, and the same bits from both packers and under the three group modes."""
    lats = [S.canonical(l) for l in S.batches()[name]]
    Vb = lats[0].vocab
    theta = S.theta(Vb)
    A = sum(l.n_arcs for l in lats)
    asc = np.random.default_rng(3).normal(0.0, 0.4, size=A).astype(np.float32) if A else None
    n_rows, arc_off, src, label, dst, w = PC.batch_arcs(S.batches()[name])
    for tape in (dict(keep=set(range(3, Vb, 2)) | {EOS}), dict(marker=5)):
        cands = []
        for l in lats:
            first = np.searchsorted(l.src, np.arange(l.n_rows + 1))
            s, sink, labs = 0, S.sink(l), []
            while s != sink:  # the first arc out of every state that is no self loop
                a = next(a for a in range(int(first[s]), int(first[s + 1])) if l.dst[a] != s)
                labs.append(int(l.label[a]))
                s = int(l.dst[a])
            y = list(SR.project(labs, **tape))
            cands.append([y[:(len(y) + 1) // 2], [], y + [Vb - 1]])
        ref = _ref(lats, theta, cands, tape, asc=asc)
        first_bits = None
        for route, gm in (("host", 0), ("device", 0), ("host", 1), ("host", 2), ("device", 2)):
            if route == "host":
                lat = LatticeBatch.from_arcs(n_rows, arc_off, src, label, dst, Vb, arc_w=w, group_mode=gm).to(dev, auto_chunks=False)
            else:
                lat = LatticeBatch.from_arcs_device(n_rows, arc_off, src, label, dst, Vb, arc_w=w, device=dev, group_mode=gm)
            got = _both(lat, theta, cands, tape, dev, asc=asc)
            if first_bits is None:
                _hold(f"structure: {name} {sorted(tape)}", got, ref)
                first_bits = got
                rows, n = _rows(cands)
                slp = ops.string_log_prob(lat, _t(theta, dev), _t(rows, dev), _t(n, dev), arc_scores=_t(asc, dev), **tape)
                assert torch.equal(slp.logz, got[0].logz) and torch.equal(slp.logz, got[1].logz)  # bit for bit
                _near(f"structure eos against log_num: {name}", got[1].eos, slp.log_num.cpu().numpy())
            assert _same_bits(got, first_bits), (name, route, gm)
        for b in (b for b, l in enumerate(lats) if l.n_arcs == 0):  # state 0 is the sink: the empty path alone
            for x in (first_bits[0].log_prefix[b], first_bits[1].log_prefix[b], first_bits[1].eos[b]):
                assert x.tolist() == [0.0, 0.0, NEG]
            assert bool(first_bits[1].next[b].isneginf().all()) and float(first_bits[1].logz[b]) == 0.0


# ============================================================================= identities on the device
@pytest.fixture(scope="module")
def grids():
    from tests import intersect_wide_ref as IW

    lats = [SR.denominator(SR.SEED1), SR.denominator(SR.SMALL), IW.edit_denominator([7, 6, 6, 8], [8, 9, 10], 2, vocab=12)]
    return lats, synth.label_scores(1, 12, mean=-1.0, std=0.5)


def test_the_two_routes_and_the_shorter_prefix_agree(dev, grids):
    """log_prefix by the H sweep, by eos + next over the F sweep, and as next[v] of the prefix one symbol shorter; eos is
    ops.string_log_prob's log_num and logz its logz bit for bit."""
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    ys = [[], [8], [8, 9], [9, 8, 10], [10], [8, 9, 10, 8]]
    for tape in (dict(marker=MARK), dict(keep={8, 9, 10})):
        pre, ns = _both(lat, theta, [ys] * 3, tape, dev)
        rows, n = _rows([ys] * 3)
        slp = ops.string_log_prob(lat, _t(theta, dev), _t(rows, dev), _t(n, dev), **tape)
        assert torch.equal(slp.logz, pre.logz) and torch.equal(slp.logz, ns.logz)
        _near("device eos against log_num: ", ns.eos, slp.log_num.cpu().numpy())
        _near("device H route against F route: ", pre.log_prefix, ns.log_prefix.cpu().numpy())
        for m, y in enumerate(ys):
            if y:
                shorter = ys.index(y[:-1]) if y[:-1] in ys else None
                if shorter is not None:
                    _near("device next of the shorter prefix: ", ns.next[:, shorter, y[-1]], pre.log_prefix[:, m].cpu().numpy())
        total = torch.logsumexp(torch.cat([ns.eos[:, :, None], ns.next], dim=2), dim=2)
        live = ~pre.log_prefix.isneginf()
        assert rec("device identity", float((total - pre.log_prefix)[live].abs().max())) <= BOUND
        assert bool(pre.log_prefix[:, 5].isneginf()[:2].all())  # (four symbols where at most two or three fit)


def test_label_skew(dev):
    """One label (3) owns 100 arcs, more than a strip of 64, label 4 owns none, and the vocabulary (70) is no multiple of
    64: a hub behind BOS whose 66 out-arcs (labels 5 .. 69 and 2) lead to states that all leave by label 3 into 34 states,
    which leave by label 3 again (and half of them by a second label)."""
    n_mid = 66
    hub_labels = list(range(5, 70)) + [EOS]
    arcs = [(0, BOS, 1)] + [(1, hub_labels[i], 2 + i) for i in range(n_mid)]
    arcs += [(2 + i, 3, 2 + n_mid + (i % 34)) for i in range(n_mid)]          # 66 arcs of label 3
    arcs += [(2 + n_mid + j, 3, 2 + n_mid + 34) for j in range(34)]           # 34 more
    arcs += [(2 + n_mid + j, 7 + j, 2 + n_mid + 34) for j in range(0, 34, 2)]  # and a way round label 3
    arcs += [(2 + n_mid + 34, EOS, 2 + n_mid + 35)]
    l = synth._finish(2 + n_mid + 36, 70, [a[0] for a in arcs], [a[1] for a in arcs], [a[2] for a in arcs])
    assert int((l.label == 3).sum()) == 100 and int((l.label == 4).sum()) == 0
    theta = synth.label_scores(9, 70, mean=-1.0, std=0.5)
    lat = LatticeBatch.from_synth([l], device=dev)
    for tape, ys in ((dict(keep={3, 4, 9, 10, 11}), [[], [3], [9, 3], [3, 3], [4], [10, 3, 3]]), (dict(marker=3), [[], [3], [7], [9]])):
        got = _both(lat, theta, [ys], tape, dev)
        ref = _ref([l], theta, [ys], tape)
        _hold(f"label skew: {sorted(tape)}", got, ref)
        assert np.isfinite(ref[0][0, 0, 3]) and np.isneginf(ref[0][0, :, 4]).all()
        assert _same_bits(got, _both(lat, theta, [ys], tape, dev))


def test_beyond_the_product_route(dev):
    """The 1200-state lattice whose product with the string's automaton has 15 934 live pairs: along its 28-symbol string
    eos and next add up to log_prefix at every prefix length, by the H route and against the restatement at three of them."""
    l, keep, y = SR.layered_case()
    theta = synth.label_scores(2, 12)
    lat = LatticeBatch.from_synth([l], device=dev)
    ys = [y[:i] for i in range(len(y) + 1)]
    pre, ns = _both(lat, theta, [ys], dict(keep=keep), dev)
    total = torch.logsumexp(torch.cat([ns.eos[:, :, None], ns.next], dim=2), dim=2)
    assert bool(torch.isfinite(pre.log_prefix).all())
    assert rec("row limit identity", float((total - pre.log_prefix).abs().max())) <= BOUND
    _near("row limit H route against F route: ", pre.log_prefix, ns.log_prefix.cpu().numpy())
    for i in range(len(y)):
        _near("row limit next of the shorter prefix: ", ns.next[:, i, y[i]], pre.log_prefix[:, i + 1].cpu().numpy())
    pick = [0, 14, 28]
    ref = _ref([l], theta, [[ys[i] for i in pick]], dict(keep=keep))
    _hold("row limit: layered", (ops.PrefixScores(*(x[:, pick] if x.dim() == 2 else x for x in pre)),
                        ops.NextSymbols(ns.next[:, pick], ns.eos[:, pick], ns.log_prefix[:, pick], ns.logz)), ref)
    slp = ops.string_log_prob(lat, _t(theta, dev), _t(np.array([[y]], np.int32), dev), _t(np.array([[len(y)]], np.int32), dev), keep=keep)
    _near("row limit eos against log_num: ", ns.eos[:, 28:], slp.log_num.cpu().numpy())


# ============================================================================= the search
def _search_equals(tag, r, b, want):
    n = int(r.n_strings[b])
    got = [tuple(r.strings[b, j, :int(r.lengths[b, j])].tolist()) for j in range(n)]
    assert got == want["strings"] and bool(r.exact[b]) == want["exact"], (tag, got, want)
    _near(f"search log_prob: {tag}", r.log_prob[b, :n], want["log_prob"])
    _near(f"search bound: {tag}", r.bound[b:b + 1], np.array([want["bound"]]))
    assert bool(r.log_prob[b, n:].isneginf().all()) and bool((r.lengths[b, n:] == 0).all()) and bool((r.strings[b, n:] == PAD).all())


@pytest.mark.parametrize("k", [1, 2, 8])
def test_search_on_the_denominator(dev, grids, k):
    """decoders.prefix_search equals the restated search, strings and ``exact`` flags included; the first string of the
    78-row grid is (8,) while its Viterbi path spells the empty string."""
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    r = decoders.prefix_search(lat, _t(theta, dev), k, marker=MARK, pad=PAD)
    for b, l in enumerate(lats):
        _search_equals(f"k={k} b={b}", r, b, PR.prefix_search(l, E.score64(l, theta), k=k, marker=MARK))
    assert r.strings[0, 0, :int(r.lengths[0, 0])].tolist() == [8]
    assert k != 2 or bool(r.exact[0])  # (certified with a beam of two: the pruned prefixes are taken up again)
    again = decoders.prefix_search(lat, _t(theta, dev), k, marker=MARK, pad=PAD)
    assert all(torch.equal(a, b) for a, b in zip(r, again))


def test_search_at_the_edges(dev, grids):
    """``max_len`` cutting the search, k larger than the number of strings (every string, ranked, and certified), the first
    phase alone, a reserve that overflows, a second phase cut short, a reserve smaller than k, keep mode."""
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    for kw in (dict(k=1, max_len=0), dict(k=2, max_len=1), dict(k=64), dict(k=3, max_len=2), dict(k=2, reserve=0, refine_steps=0),
               dict(k=2, reserve=3), dict(k=2, refine_steps=2), dict(k=3, reserve=1), dict(k=2, max_len=2, reserve=5)):
        r = decoders.prefix_search(lat, _t(theta, dev), marker=MARK, pad=PAD, **kw)
        for b, l in enumerate(lats):
            want = PR.prefix_search(l, E.score64(l, theta), marker=MARK, **kw)
            if kw["k"] == 64:  # (permutations of a string tie to round-off: compare the ranked weights and the set)
                n = int(r.n_strings[b])
                got = {tuple(r.strings[b, j, :int(r.lengths[b, j])].tolist()) for j in range(n)}
                assert got == set(want["strings"]) and n == len(want["strings"]) < 64 and bool(r.exact[b]) and want["exact"]
                _near("search log_prob: all strings", r.log_prob[b, :n], want["log_prob"])
                assert bool(r.bound[b].isneginf())
            else:
                _search_equals(f"{kw} b={b}", r, b, want)
    r = decoders.prefix_search(lat, _t(theta, dev), 1, 0, marker=MARK, pad=PAD)
    assert not bool(r.exact.any()) and r.lengths[:, 0].tolist() == [0, 0, 0]
    kept = decoders.prefix_search(lat, _t(theta, dev), 4, keep={8, 9, 10}, pad=PAD)
    for b, l in enumerate(lats):
        _search_equals(f"keep b={b}", kept, b, PR.prefix_search(l, E.score64(l, theta), k=4, keep={8, 9, 10}))


def test_a_certified_string_beats_the_path_list(dev):
    """Wherever ``exact`` is set on a batch of edit grids (``synth.edit_lattice``, whose paths all spell one string, and
    denominator grids, which spell many), the first string's log p is at least that of decode_strings(k=64)'s first
    string."""
    rng = np.random.default_rng(11)
    pairs = [([int(t) for t in rng.integers(6, 8, size=n)], [int(t) for t in rng.integers(8, 11, size=m)]) for n, m in ((2, 3), (3, 1), (1, 0), (4, 4))]
    lats = [synth.edit_lattice(x, y, 12, seed=i) for i, (x, y) in enumerate(pairs)] + _edit_grids()
    theta = synth.label_scores(5, 12, mean=-1.0, std=1.5)
    lat = LatticeBatch.from_synth(lats, device=dev)
    d = decoders.decode_strings(lat, _t(theta, dev), 64, marker=MARK, pad=PAD)
    for k in (2, 64):
        r = decoders.prefix_search(lat, _t(theta, dev), k, marker=MARK, pad=PAD)
        ok = r.exact
        assert bool(ok[:4].all())  # one string: nothing is ever pruned
        assert bool((r.log_prob[ok, 0] >= d.log_prob[ok, 0] - BOUND).all())
        assert bool((r.bound[ok] <= r.log_prob[ok, 0]).all())
    for b, (x, y) in enumerate(pairs):
        assert r.strings[b, 0, :int(r.lengths[b, 0])].tolist() == y and int(r.n_strings[b]) == 1
        assert rec("search one string", abs(float(r.log_prob[b, 0]))) <= BOUND


def _edit_grids():
    from tests import intersect_wide_ref as IW

    rng = np.random.default_rng(7)
    return [IW.edit_denominator([int(t) for t in rng.integers(5, 8, size=n)], [8, 9, 10], 2, vocab=12) for n in (1, 2, 3, 4, 2, 3)]


def test_lattice_scorer_entries(dev, grids):
    lats, theta = grids
    em, tr = synth.collate_dense([l.dense() for l in lats])
    sc = LatticeScorer(12, pad=PAD, bos=BOS, eos=EOS, theta=torch.from_numpy(theta)).to(dev)
    sc.set_masks(torch.as_tensor(em).to(dev), torch.as_tensor(tr).to(dev))
    want = decoders.prefix_search(sc._lat(), _t(theta, dev), 4, marker=MARK, pad=PAD)
    got = sc.prefix_search(4)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and got.strings[0, 0, :1].tolist() == [8]
    rows, n = _rows([[[8], []]] * 3)
    ns = sc.string_next_log_probs(_t(rows, dev), _t(n, dev))
    ref = ops.string_next_log_probs(sc._lat(), _t(theta, dev), _t(rows, dev), _t(n, dev), marker=MARK)
    assert all(torch.equal(a, b) for a, b in zip(ns, ref))
    assert all(torch.equal(a, b) for a, b in zip(sc.string_next_log_probs(_t(rows, dev), _t(n, dev), keep={8, 9, 10}),
                                                  ops.string_next_log_probs(sc._lat(), _t(theta, dev), _t(rows, dev), _t(n, dev), keep={8, 9, 10})))

"""Prefix states (ops.string_prefix_open, PrefixContext.root / extend / next / state_of; nfst_string_prefix_open,
nfst_string_prefix_extend, nfst_string_prefix_state_next) and decoders.prefix_search(incremental=True).  The reference
is ops.string_next_log_probs on the whole prefix, compared as bits (torch.equal): no tolerance is involved.  The NumPy
restatement of tests/strings_extend_ref.py is held at BOUND, the bound that tests/test_gpu_strings_prefix.py derived for
the same quantities.  tests/test_strings_extend_cpu.py holds the restatement to the table references.  The largest error
against the restatement goes to strings_extend_errors.json in the directory of run outputs (profiles/README.md)."""
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
from tests import strings_extend_ref as XR
from tests import strings_ref as SR
from tests import structure_cases as S

pytestmark = pytest.mark.gpu
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
NEG = -np.inf
MARK = SR.MARK
BOUND = 1e-12  # (tests/test_gpu_strings_prefix.py: next, eos and log_prefix against a float64 restatement)
MODES = {"marker": dict(marker=MARK), "keep": dict(keep={8, 9})}

_ERR = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for out in sorted(glob.glob(os.path.join(root, "*_out"))):
        if _ERR and os.path.isdir(out):
            with open(os.path.join(out, "strings_extend_errors.json"), "w") as f:
                json.dump(dict(sorted(_ERR.items())), f, indent=1)


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _rows(cands):
    """(prefixes [B, M, N] int32, lengths [B, M]); a dead slot (None) counts as the empty prefix here"""
    cands = [[[] if y is None else list(y) for y in row] for row in cands]
    n = np.array([[len(y) for y in row] for row in cands], np.int32)
    out = np.full((len(cands), len(cands[0]), max(1, int(n.max()))), 8, np.int32)
    for b, row in enumerate(cands):
        for m, y in enumerate(row):
            out[b, m, :len(y)] = y
    return out, n


def _full(lat, theta, cands, tape, dev, asc=None):
    """ops.string_next_log_probs of per-lattice prefix lists: the reference"""
    rows, n = _rows(cands)
    return ops.string_next_log_probs(lat, _t(theta, dev), _t(rows, dev), _t(n, dev), arc_scores=_t(asc, dev), **tape)


def _same_bits(tag, ns, full, cands):
    """A state's NextSymbols against the reference's: equal bits in every live slot, -inf in every dead one, never NaN"""
    for x in ns:
        assert x.dtype == torch.float64 and not bool(x.isnan().any()), tag
    assert torch.equal(ns.logz, full.logz), tag
    dead = torch.tensor([[y is None for y in row] for row in cands], device=ns.eos.device)
    for got, want in zip(ns[:3], full[:3]):
        d = dead if got.dim() == 2 else dead[:, :, None].expand_as(got)
        assert bool(got[d].isneginf().all()), tag
        assert torch.equal(got[~d], want[~d]), tag


def _near(tag, got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want, np.float64)
    assert got.dtype == np.float64 and not np.isnan(got).any(), tag
    dead = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), dead), (tag, got, want)
    if (~dead).any():
        err = float(np.abs(got[~dead] - want[~dead]).max())
        _ERR[tag.split(":")[0]] = max(_ERR.get(tag.split(":")[0], 0.0), err)
        print(f"{tag}: {err:.3g}")
        assert err <= BOUND, tag


def _restated(lats, theta, cands, tape, asc=None):
    """The restatement's (next [B, M, V], eos, log_prefix [B, M], logz [B]); a dead slot is -inf"""
    B, M, V = len(lats), len(cands[0]), lats[0].vocab
    nxt, eos, pre, z = np.full((B, M, V), NEG), np.full((B, M), NEG), np.full((B, M), NEG), np.zeros(B)
    a0 = 0
    for b, l in enumerate(lats):
        ctx = XR.Context(l, E.score64(l, theta[b] if np.ndim(theta) == 2 else theta, None if asc is None else asc[a0:a0 + l.n_arcs]), **tape)
        a0 += l.n_arcs
        z[b] = ctx.logz
        for m, y in enumerate(cands[b]):
            if y is not None:
                nxt[b, m], eos[b, m], pre[b, m] = ctx.next(ctx.state_of(y))
    return nxt, eos, pre, z


def _hold(tag, ns, ref):
    kind, case = tag.split(":")
    for name, got, want in zip(("next", "eos", "log_prefix", "logz"), ns, ref):
        _near(f"{kind} {name}:{case}", got, want)


def _step(ctx, state, toks, parent, symbol, dev):
    """extend with Python lists [B][M_out], and the children's tokens (None: dead)"""
    new = ctx.extend(state, _t(np.array(parent, np.int32), dev), _t(np.array(symbol, np.int32), dev))
    out = [[None if p == -1 or (p >= 0 and toks[b][p] is None) else ([] if p == -2 else toks[b][p] + [s]) for p, s in zip(pr, sr)]
           for b, (pr, sr) in enumerate(zip(parent, symbol))]
    assert new.lengths.tolist() == [[-1 if y is None else len(y) for y in row] for row in out]
    return new, out


# ============================================================================= the long grid
@pytest.fixture(scope="module")
def long_grid():
    """One edit grid that spells every string over {8, 9} of up to 129 symbols, and one random string of 129"""
    from tests import intersect_wide_ref as IW

    l = IW.edit_denominator([6], [8, 9], 129, vocab=12)
    theta = synth.label_scores(4, 12, mean=-1.0, std=0.5)
    y = [int(t) for t in np.random.default_rng(5).integers(8, 10, size=129)]
    return l, theta, y


@pytest.mark.parametrize("mode", list(MODES))
def test_a_chain_of_129_extends(dev, long_grid, mode):
    """next, eos and log_prefix of the state after n extends equal string_next_log_probs of y[:n] bit for bit at the strip
    boundaries of the table route; logz is string_log_prob's; a second run gives the same bits."""
    l, theta, y = long_grid
    tape = MODES[mode]
    lat = LatticeBatch.from_synth([l], device=dev)
    at = (0, 1, 63, 64, 65, 128, 129)

    def run():
        ctx = ops.string_prefix_open(lat, _t(theta, dev), **tape)
        state, got = ctx.root(), {}
        for n in range(130):
            if n in at:
                got[n] = ctx.next(state)
            if n < 129:
                state = ctx.extend(state, _t(np.array([[0]], np.int32), dev), _t(np.array([[y[n]]], np.int32), dev))
        assert state.lengths.tolist() == [[129]]
        return ctx, got

    ctx, got = run()
    for n in at:
        _same_bits(f"chain n={n} {mode}", got[n], _full(lat, theta, [[y[:n]]], tape, dev), [[y[:n]]])
    slp = ops.string_log_prob(lat, _t(theta, dev), _t(np.array([[y]], np.int32), dev), _t(np.array([[129]], np.int32), dev), **tape)
    assert torch.equal(ctx.logz, slp.logz)
    _, again = run()
    assert all(torch.equal(a, b) for n in at for a, b in zip(got[n], again[n]))
    rs = XR.Context(l, E.score64(l, theta), **tape)
    col = rs.root()
    for n in range(130):
        if n in (0, 1, 64, 129):
            nxt, eos, pre = rs.next(col)
            _hold(f"chain: n={n} {mode}", got[n], (nxt[None, None], [[eos]], [[pre]], [rs.logz]))
        if n < 129:
            col = rs.extend(col, y[n])


@pytest.mark.parametrize("mode", list(MODES))
def test_hypothesis_counts(dev, long_grid, mode):
    """M_out in {1, 3, 64, 65} from M_in in {1, 65}: a permuting parent, two children of one parent with different symbols
    and two with the same, a dead slot and a root slot beside live ones, a symbol that no path spells (-inf, never NaN);
    the 65 children in one call and in slices of 1, 2 and 64 give the same bits, cells included."""
    l, theta, _ = long_grid
    tape = MODES[mode]
    lat = LatticeBatch.from_synth([l], device=dev)
    ctx = ops.string_prefix_open(lat, _t(theta, dev), **tape)
    rng = np.random.default_rng(8)
    sym = lambda n: [int(t) for t in rng.integers(8, 10, size=n)]
    check = lambda tag, st, toks: _same_bits(f"{tag} {mode}", ctx.next(st), _full(lat, theta, toks, tape, dev), toks)
    root, toks0 = ctx.root(1), [[[]]]
    for M in (1, 3, 64):  # 1 -> 1, 3, 64
        st, toks = _step(ctx, root, toks0, [[0] * M], [sym(M)], dev)
        check(f"1 -> {M}", st, toks)
    par, s = [0] * 65, sym(65)
    par[3], par[5], s[7] = -1, -2, 10
    A, tA = _step(ctx, root, toks0, [par], [s], dev)  # 1 -> 65
    check("1 -> 65", A, tA)
    assert tA[0][3] is None and tA[0][5] == [] and tA[0][7] == [10]
    ns = ctx.next(A)
    assert bool(ns.next[0, 7].isneginf().all()) and bool(ns.eos[0, 7].isneginf()) and bool(ns.log_prefix[0, 7].isneginf())
    par, s = [64 - m for m in range(65)], sym(65)  # 65 -> 65, permuting
    par[0], par[1], s[0], s[1] = 10, 10, 8, 9      # one parent, different symbols
    par[2], par[4], s[2], s[4] = 11, 11, 9, 9      # one parent, the same symbol
    par[20], par[21], s[22] = -1, -2, 10
    Bs, tB = _step(ctx, A, tA, [par], [s], dev)
    check("65 -> 65", Bs, tB)
    assert tB[0][0][-1] == 8 and tB[0][1] == tB[0][0][:-1] + [9] and tB[0][2] == tB[0][4] and tB[0][21] == []
    nsB = ctx.next(Bs)
    assert torch.equal(nsB.next[0, 2], nsB.next[0, 4]) and not torch.equal(nsB.next[0, 0], nsB.next[0, 1])
    for M, pick in ((3, [64, 0, 30]), (1, [9]), (64, list(range(1, 65)))):  # 65 -> 3, 1, 64
        st, toks = _step(ctx, Bs, tB, [pick], [sym(M)], dev)
        check(f"65 -> {M}", st, toks)
    # slices of the 65 children
    reach = torch.as_tensor(XR.Context(l, E.score64(l, theta), **tape).by_depth, device=dev)
    cells = lambda st, M: st.cells[:lat.total_rows * ctx.planes * M].view(lat.total_rows, ctx.planes, M)[reach]
    whole = cells(Bs, 65)
    for step in (1, 2, 64):
        for m0 in range(0, 65, step):
            part, _ = _step(ctx, A, tA, [par[m0:m0 + step]], [s[m0:m0 + step]], dev)
            n = min(step, 65 - m0)
            assert torch.equal(cells(part, n), whole[:, :, m0:m0 + n]), (step, m0)
            assert all(torch.equal(a, b[:, m0:m0 + n]) for a, b in zip(ctx.next(part)[:3], nsB[:3])), (step, m0)


# ============================================================================= in-degree
@pytest.mark.parametrize("mode", ["marker", "keep"])
def test_in_degree(dev, mode):
    """70 states funnel into one (its in-arc list is longer than a wave) and the state behind it has one in-arc."""
    n_mid = 70
    arcs = [(0, BOS, 1)] + [(1, 5 + i, 2 + i) for i in range(n_mid)] + [(2 + i, 3, 2 + n_mid) for i in range(n_mid)]
    arcs += [(2 + n_mid, 9, 3 + n_mid), (3 + n_mid, EOS, 4 + n_mid)]
    l = synth._finish(5 + n_mid, 80, [a[0] for a in arcs], [a[1] for a in arcs], [a[2] for a in arcs])
    theta = synth.label_scores(6, 80, mean=-1.0, std=0.5)
    tape, ys = (dict(marker=3), [[], [9], [3], [9, 9]]) if mode == "marker" else (dict(keep={3, 6, 7, 9}), [[], [3], [3, 9], [6], [6, 3], [6, 3, 9], [9], [7, 3, 9, 9]])
    lat = LatticeBatch.from_synth([l], device=dev)
    ctx = ops.string_prefix_open(lat, _t(theta, dev), **tape)
    rows, n = _rows([ys])
    ns = ctx.next(ctx.state_of(_t(rows, dev), _t(n, dev)))
    _same_bits(f"in-degree {mode}", ns, _full(lat, theta, [ys], tape, dev), [ys])
    ref = _restated([l], theta, [ys], tape)
    _hold(f"in-degree: {mode}", ns, ref)
    assert np.isfinite(ref[2][0, 1]) and np.isneginf(ref[2][0, -1])


# ============================================================================= the structural corpus
@pytest.mark.parametrize("name", tuple(S.batches()))
def test_structure_corpus(dev, name):
    """Self loops, states that state 0 does not reach, a lattice whose state 0 is the sink; both tape modes with per-arc
    scores (and the tables' weights in the weighted batch); per lattice half of a path's string, the empty prefix and a
    prefix that no path spells, against the restatement and string_next_log_probs, and the same bits from both packers
    and under the three group modes."""
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
        ref = _restated(lats, theta, cands, tape, asc=asc)
        rows, n = _rows(cands)
        first_bits = None
        for route, gm in (("host", 0), ("device", 0), ("host", 1), ("host", 2), ("device", 2)):
            if route == "host":
                lat = LatticeBatch.from_arcs(n_rows, arc_off, src, label, dst, Vb, arc_w=w, group_mode=gm).to(dev, auto_chunks=False)
            else:
                lat = LatticeBatch.from_arcs_device(n_rows, arc_off, src, label, dst, Vb, arc_w=w, device=dev, group_mode=gm)
            ctx = ops.string_prefix_open(lat, _t(theta, dev), arc_scores=_t(asc, dev), **tape)
            state = ctx.state_of(_t(rows, dev), _t(n, dev))
            assert torch.equal(state.lengths.cpu(), torch.from_numpy(n))
            got = ctx.next(state)
            if first_bits is None:
                _hold(f"structure: {name} {sorted(tape)}", got, ref)
                _same_bits(f"structure {name}", got, _full(lat, theta, cands, tape, dev, asc=asc), cands)
                first_bits = got
            assert all(torch.equal(a, b) for a, b in zip(got, first_bits)), (name, route, gm)


# ============================================================================= scores, labels, size
@pytest.fixture(scope="module")
def grids():
    from tests import intersect_wide_ref as IW

    lats = [SR.denominator(SR.SEED1), SR.denominator(SR.SMALL), IW.edit_denominator([7, 6, 6, 8], [8, 9, 10], 2, vocab=12)]
    return lats, synth.label_scores(1, 12, mean=-1.0, std=0.5)


def test_per_lattice_scores(dev, grids):
    lats, _ = grids
    theta = np.stack([synth.label_scores(20 + b, 12, mean=-1.0, std=0.5) for b in range(3)])
    lat = LatticeBatch.from_synth(lats, device=dev)
    ys = [[], [8], [8, 9], [9, 8, 10], [10], [8, 9, 10, 8]]
    for tape in (dict(marker=MARK), dict(keep={8, 9, 10})):
        ctx = ops.string_prefix_open(lat, _t(theta, dev), **tape)
        rows, n = _rows([ys] * 3)
        ns = ctx.next(ctx.state_of(_t(rows, dev), _t(n, dev)))
        _same_bits("per-lattice theta", ns, _full(lat, theta, [ys] * 3, tape, dev), [ys] * 3)
        _hold(f"per-lattice theta: {sorted(tape)}", ns, _restated(lats, theta, [ys] * 3, tape))
        shared = ops.string_prefix_open(lat, _t(theta[0], dev), **tape)
        assert not torch.equal(shared.next(shared.root()).next[1], ctx.next(ctx.root()).next[1])


def test_label_skew(dev):
    """The label-skew lattice of tests/test_gpu_strings_prefix.py: label 3 owns 100 arcs, label 4 none, 70 labels."""
    n_mid = 66
    hub_labels = list(range(5, 70)) + [EOS]
    arcs = [(0, BOS, 1)] + [(1, hub_labels[i], 2 + i) for i in range(n_mid)]
    arcs += [(2 + i, 3, 2 + n_mid + (i % 34)) for i in range(n_mid)]
    arcs += [(2 + n_mid + j, 3, 2 + n_mid + 34) for j in range(34)]
    arcs += [(2 + n_mid + j, 7 + j, 2 + n_mid + 34) for j in range(0, 34, 2)]
    arcs += [(2 + n_mid + 34, EOS, 2 + n_mid + 35)]
    l = synth._finish(2 + n_mid + 36, 70, [a[0] for a in arcs], [a[1] for a in arcs], [a[2] for a in arcs])
    assert int((l.label == 3).sum()) == 100 and int((l.label == 4).sum()) == 0
    theta = synth.label_scores(9, 70, mean=-1.0, std=0.5)
    lat = LatticeBatch.from_synth([l], device=dev)
    for tape, ys in ((dict(keep={3, 4, 9, 10, 11}), [[], [3], [9, 3], [3, 3], [4], [10, 3, 3]]), (dict(marker=3), [[], [3], [7], [9]])):
        ctx = ops.string_prefix_open(lat, _t(theta, dev), **tape)
        rows, n = _rows([ys])
        ns = ctx.next(ctx.state_of(_t(rows, dev), _t(n, dev)))
        _same_bits(f"label skew {sorted(tape)}", ns, _full(lat, theta, [ys], tape, dev), [ys])
        _hold(f"label skew: {sorted(tape)}", ns, _restated([l], theta, [ys], tape))


def test_beyond_the_product_route(dev):
    """The 1200-state lattice along its 28-symbol string: the bits of string_next_log_probs at every length."""
    l, keep, y = SR.layered_case()
    theta = synth.label_scores(2, 12)
    lat = LatticeBatch.from_synth([l], device=dev)
    ys = [list(y[:i]) for i in range(len(y) + 1)]
    full = _full(lat, theta, [ys], dict(keep=keep), dev)
    ctx = ops.string_prefix_open(lat, _t(theta, dev), keep=keep)
    state = ctx.root()
    for i in range(len(y) + 1):
        ns = ctx.next(state)
        assert torch.equal(ns.next[0, 0], full.next[0, i]) and torch.equal(ns.eos[0, 0], full.eos[0, i]), i
        assert torch.equal(ns.log_prefix[0, 0], full.log_prefix[0, i]) and torch.equal(ns.logz, full.logz), i
        assert bool(torch.isfinite(ns.log_prefix).all())
        if i < len(y):
            state = ctx.extend(state, _t(np.array([[0]], np.int32), dev), _t(np.array([[int(y[i])]], np.int32), dev))


def test_state_of_equals_the_chain(dev, grids):
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    ctx = ops.string_prefix_open(lat, _t(theta, dev), marker=MARK)
    cands = [[[8, 9], [9], None, []], [[9, 9], [], [10, 8], None], [[8, 9, 10], [10, 9], [8], [9, 8, 10]]]
    rows, n = _rows(cands)
    n = np.where(np.array([[y is None for y in row] for row in cands]), -1, n).astype(np.int32)
    st = ctx.state_of(_t(rows, dev), _t(n, dev))
    assert torch.equal(st.lengths.cpu(), torch.from_numpy(n))
    # the chain: every slot from the root by its own symbols, in as many extends as the slot has symbols
    chain, toks = _step(ctx, ctx.root(1), [[[]]] * 3, [[-1 if y is None else -2 for y in row] for row in cands], [[0] * 4] * 3, dev)
    ns = ctx.next(st)
    for t in range(3):
        nxt, toks2 = _step(ctx, chain, toks, [[m if y is not None and len(y) > t else -1 for m, y in enumerate(row)] for row in cands],
                           [[y[t] if y is not None and len(y) > t else 0 for y in row] for row in cands], dev)
        part = ctx.next(nxt)
        for b, row in enumerate(cands):
            for m, y in enumerate(row):
                if y is not None and len(y) == t + 1:
                    assert all(torch.equal(a[b, m], c[b, m]) for a, c in zip(ns[:3], part[:3])), (b, m)
        chain, toks = nxt, toks2
    _same_bits("state_of", ns, _full(lat, theta, cands, dict(marker=MARK), dev), cands)


# ============================================================================= errors
def test_errors(dev, grids):
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    ctx = ops.string_prefix_open(lat, _t(theta, dev), marker=MARK)
    root = ctx.root(2)
    par, sym = np.zeros((3, 4), np.int32), np.full((3, 4), 8, np.int32)
    good = ctx.next(ctx.extend(root, _t(par, dev), _t(sym, dev)))
    for bad_par, bad_sym in ((2, 8), (-3, 8), (0, 12), (0, -1)):
        p, s = par.copy(), sym.copy()
        p[1, 2], s[1, 2] = bad_par, bad_sym
        with pytest.raises(_lib.NfstError) as e:
            ctx.extend(root, _t(p, dev), _t(s, dev))
        assert e.value.code == _lib.ERR_INDEX
        cells, status = ctx._extend(root.cells, 2, _t(p, dev), _t(s, dev))
        assert int(status.item()) == _lib.ERR_INDEX
        ns = ctx.next(ops.PrefixState(cells, torch.ones((3, 4), dtype=torch.int32, device=dev)))
        keep = torch.ones((3, 4), dtype=torch.bool, device=dev)
        keep[1, 2] = False
        assert bool(ns.next[1, 2].isneginf().all()) and bool(ns.eos[1, 2].isneginf()) and bool(ns.log_prefix[1, 2].isneginf())
        assert torch.equal(ns.next[keep], good.next[keep]) and torch.equal(ns.log_prefix[keep], good.log_prefix[keep])
    # a symbol is not read where the parent makes the root or a dead slot
    p, s = par.copy(), sym.copy()
    p[0, 0], p[0, 1], s[0, 0], s[0, 1] = -2, -1, 99, -7
    assert ctx.extend(root, _t(p, dev), _t(s, dev)).lengths[0].tolist() == [0, -1, 1, 1]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.NfstError) as e:  # aliased states
        ops._call("nfst_string_prefix_extend", lat, ctx._sc, None, MARK, ctx.ws, ctx.ws.numel(), root.cells, root.cells.numel() * 8, 2,
                  _t(par[:, :2], dev).contiguous(), _t(sym[:, :2], dev).contiguous(), root.cells, root.cells.numel() * 8, 2, status)
    assert e.value.code == -1 and int(status.item()) == 0
    with pytest.raises(_lib.NfstError) as e:
        ctx.root(ops.STATE_MAX_M + 1)
    assert e.value.code == -6


# ============================================================================= the search
def _equal_results(a, b):
    return all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("k", [1, 2, 8])
def test_incremental_search_equals_the_search(dev, grids, k):
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    want = decoders.prefix_search(lat, _t(theta, dev), k, marker=MARK, pad=PAD)
    got = decoders.prefix_search(lat, _t(theta, dev), k, marker=MARK, pad=PAD, incremental=True)
    assert _equal_results(got, want) and got.strings[0, 0, :int(got.lengths[0, 0])].tolist() == [8]


def test_incremental_search_at_the_edges(dev, grids):
    """``max_len`` cutting the search, the first phase alone, keep mode, k larger than the number of strings"""
    lats, theta = grids
    lat = LatticeBatch.from_synth(lats, device=dev)
    for kw in (dict(k=1, max_len=0, marker=MARK), dict(k=2, max_len=1, marker=MARK), dict(k=3, max_len=2, marker=MARK),
               dict(k=2, reserve=0, refine_steps=0, marker=MARK), dict(k=2, reserve=3, marker=MARK), dict(k=4, keep={8, 9, 10}),
               dict(k=64, marker=MARK)):
        want = decoders.prefix_search(lat, _t(theta, dev), pad=PAD, **kw)
        got = decoders.prefix_search(lat, _t(theta, dev), pad=PAD, incremental=True, **kw)
        assert _equal_results(got, want), kw
    assert int(got.n_strings.max()) < 64 and bool(got.exact.all())


def test_lattice_scorer_entries(dev, grids):
    lats, theta = grids
    em, tr = synth.collate_dense([l.dense() for l in lats])
    sc = LatticeScorer(12, pad=PAD, bos=BOS, eos=EOS, theta=torch.from_numpy(theta)).to(dev)
    sc.set_masks(torch.as_tensor(em).to(dev), torch.as_tensor(tr).to(dev))
    rows, n = _rows([[[8], []]] * 3)
    for kw in (dict(), dict(keep={8, 9, 10})):
        ctx = sc.prefix_context(**kw)
        ns = ctx.next(ctx.state_of(_t(rows, dev), _t(n, dev)))
        assert all(torch.equal(a, b) for a, b in zip(ns, sc.string_next_log_probs(_t(rows, dev), _t(n, dev), **kw)))
    assert _equal_results(sc.prefix_search(4, incremental=True), sc.prefix_search(4))

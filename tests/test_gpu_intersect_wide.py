"""ops.intersect with a constraints.WideDFA (nfst_intersect_wide_count / _write: the product of every lattice with a sparse
automaton of up to 4096 states): every integer output bit for bit against the narrow route where both apply and against
the vectorised restatement of tests/intersect_wide_ref.py elsewhere, the packed product against the host packer on the
reference's arc lists, and the existing ops on the product against the oracle and against path enumeration."""
import functools

import numpy as np
import pytest
import torch

from nfst_amd import _lib, ops, synth
from nfst_amd.constraints import ConstraintDFA, WideDFA
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from oracle import oracle as O
from tests import intersect_ref as R
from tests import intersect_wide_ref as RW
from tests import kbest_ref as K
from tests import test_gpu_intersect as GI
from tests.test_gpu_slack import STAR_OPTS, _same_arrays, _star

pytestmark = pytest.mark.gpu
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
V = GI.V
MAX_ROWS, ERR_LIMIT = GI.MAX_ROWS, GI.ERR_LIMIT


# ----------------------------------------------------------------------------- automata and references, built once
@functools.lru_cache(maxsize=None)
def _chain(vocab, Q, labels, limit=None):
    """count_at_most as a chain of Q states: the count of the arcs with a label of ``labels``, held at Q - 1 once it gets
    there, and no transition beyond ``limit`` of them (if given).  Count c is state -c mod Q: 0, Q-1, Q-2, ..., so the
    first counts live in the LAST bits of the last word of a state set."""
    st = lambda c: (-c) % Q
    dflt = np.arange(Q)
    lab = np.array(sorted(labels), np.int64)
    exc_dst = np.empty((Q, lab.size), np.int64)
    for c in range(Q):
        up = min(c + 1, Q - 1)
        exc_dst[st(c)] = -1 if (limit is not None and c + 1 > limit) else st(up)
    return WideDFA(dflt, np.arange(Q + 1) * lab.size, np.tile(lab, Q), exc_dst.reshape(-1), np.ones(Q), vocab=vocab)


HALF = tuple(range(3, 24))


def _refs(lats, dfa):
    """The restatement's product of every lattice; a wrong shape (empty, or over the row limit) is an error, not a skip."""
    dense = dfa.to_dense()
    refs = [RW.intersect(l, *(dense[b] if dfa.per_lattice else dense)) for b, l in enumerate(lats)]
    assert all(0 < r["n_rows"] <= MAX_ROWS for r in refs), [r["n_rows"] for r in refs]
    return refs


def _run(tag, lats, dfa, dev, **opts):
    lat = LatticeBatch.from_synth(list(lats), device=dev)
    res = ops.intersect(lat, dfa, **opts)
    refs = _refs(lats, dfa)
    GI._check(tag, res, lat, lats, refs)
    return lat, res, refs


def _outputs(res):
    return [res.lattice._t[k] for k in ("arc_src", "arc_label", "arc_dst")] + list(res)[1:]


def _same_product(a, b):
    _same_arrays(a.lattice, b.lattice)
    for x, y in zip(_outputs(a), _outputs(b)):
        assert x.dtype == y.dtype and torch.equal(x, y)


# ----------------------------------------------------------------------------- 1: the narrow corpus through both routes
@pytest.mark.parametrize("lats,dfa", [("mixed", "accept_all"), ("mixed", "count51"), ("mixed", "bigram79"), ("mixed", "parity"),
                                      ("mixed5", "count63"), ("mixed5", "count33")])
def test_both_routes_give_the_same_seven_outputs(dev, lats, dfa):
    narrow = GI._dfa(dfa)
    lat = LatticeBatch.from_synth(GI._lattices(lats), device=dev)
    a, b = ops.intersect(lat, narrow), ops.intersect(lat, WideDFA.from_constraint(narrow))
    assert len(_outputs(a)) == 7
    _same_product(a, b)


def test_both_routes_with_per_lattice_automata(dev):
    lats = [synth.edit_lattice(x, y, vocab=V, seed=7 + i) for i, (x, y) in enumerate(GI._EDIT_XY)]
    narrow = ConstraintDFA.stack([ConstraintDFA.marked_sequence(V, 4, y) for _, y in GI._EDIT_XY])
    lat = GI._pack_device(lats, dev)
    a = ops.intersect(lat, narrow)
    _same_product(a, ops.intersect(lat, WideDFA.from_constraint(narrow)))
    _same_product(a, ops.intersect(lat, WideDFA.stack([WideDFA.marked_sequence(V, 4, y) for _, y in GI._EDIT_XY])))  # ragged


# ----------------------------------------------------------------------------- 2: word edges
@pytest.mark.parametrize("Q", [1, 64, 65, 127, 128, 129, 200])
def test_word_edges(dev, Q):
    _, res, refs = _run(f"chain {Q}", GI._lattices("mixed5"), _chain(V, Q, HALF), dev)
    if Q > 1:  # the first count's state is the last bit of the last word
        assert int(res.row_q.max()) == Q - 1 and int(res.arc_q.max()) == Q - 1
        assert all(int(r["row_q"].max()) == Q - 1 for r in refs[:4])
    else:
        assert bool((res.row_q == 0).all())


def test_4096_states_with_the_last_bit_of_the_last_word_live(dev):
    (l,) = GI._lattices("edit63")
    dfa = _chain(V, 4096, (3, 4, 5))
    assert dfa.n_states == 4096
    _, res, refs = _run("chain 4096", [l], dfa, dev)
    assert int(res.row_q.max()) == 4095 and (refs[0]["row_q"] == 4095).any()
    assert int(res.row_q[res.row_q > 0].min()) > 4096 - 64  # every count but zero lies in word 63


# ----------------------------------------------------------------------------- 3: the headline: a numerator inside its denominator
X12 = (10, 11, 12, 13, 14, 15, 10, 12, 14, 11, 13, 15)
SYMBOLS = (20, 21, 22, 23)
Y40 = tuple(SYMBOLS[(5 * j * j + j // 3) % 4] for j in range(40))


@functools.lru_cache(maxsize=None)
def _headline():
    den = RW.edit_denominator(X12, SYMBOLS, 40, V)
    dfa = WideDFA.marked_sequence(V, 4, Y40)
    return den, dfa


def test_numerator_inside_the_denominator(dev):
    den, dfa = _headline()
    assert dfa.n_states == 82 and len(set(Y40)) == 4
    assert den.n_rows == 3467 and den.n_rows <= MAX_ROWS  # (nodes 13 * 41, private states 520 + 492 + 4 * 480, state 0, sink)
    lat, res, refs = _run("headline", [den], dfa, dev)
    num = synth.edit_lattice(list(X12), list(Y40), vocab=V)
    assert refs[0]["n_rows"] == num.n_rows and refs[0]["n_arcs"] == num.n_arcs  # the product IS the numerator's machine
    # theta around -0.5 a label: a path has 118 to 142 arcs, and log Z must stay inside (-128, 128), where half an ulp of
    # the float32 result is 3.8e-6 (at label_scores' default mean of -2.3 log Z is near -270: half an ulp, 1.5e-5, alone
    # exceeds the bound)
    theta_np = synth.label_scores(8, V, mean=-0.5, std=0.5)
    theta = torch.from_numpy(theta_np).to(dev)
    logz = float(ops.log_z(res.lattice, theta)[0])
    o = O.forward_backward(num.n_rows, num.src, num.dst, theta_np[num.label].astype(np.float64))
    assert abs(o["logZ"]) < 128
    print(f"headline: rows {refs[0]['n_rows']}, log Z {logz!r}, oracle {o['logZ']!r}, |error| {abs(logz - o['logZ']):.3g}")
    assert abs(logz - o["logZ"]) <= 1e-5, (logz, o["logZ"])
    # and log p(y | x) from the denominator alone
    lp = float(ops.constraint_log_prob(lat, theta, dfa)[0])
    od = O.forward_backward(den.n_rows, den.src, den.dst, theta_np[den.label].astype(np.float64))
    print(f"headline: log p(y | x) {lp!r}, oracle {o['logZ'] - od['logZ']!r}")
    assert lp <= 0 and abs(lp - (o["logZ"] - od["logZ"])) <= 2e-5


def test_small_numerator_path_for_path(dev):
    x, y = [10, 11], [21, 20, 21]
    den = RW.edit_denominator(x, SYMBOLS, 3, V)
    dfa = WideDFA.marked_sequence(V, 4, y)
    _, res, refs = _run("small numerator", [den], dfa, dev)
    got = {k: v.cpu().numpy() for k, v in zip(("src", "label", "dst"), _outputs(res)[:3])}
    got.update(n_rows=int(res.lattice.n_rows[0]), n_arcs=int(res.lattice.n_arcs[0]), arc_map=res.arc_map.cpu().numpy())
    mine = sorted(p[0] for p in R.product_paths(got))
    num = synth.edit_lattice(x, y, vocab=V)
    want = sorted(tuple(int(a) for a in num.label[p]) for _, p in K.enumerate_paths(num.n_rows, num.src, num.dst, np.zeros(num.n_arcs), num.n_rows - 1))
    assert len(want) > 10 and len(set(want)) == len(want) and mine == want


# ----------------------------------------------------------------------------- 4: the exact string of a drawn path
def test_sequence_of_a_drawn_path_with_and_without_chunked_programs(dev):
    l = GI._lattices("snips4")[1]
    theta_np = synth.label_scores(64, 250, mean=-1.5, std=0.8)
    theta = torch.from_numpy(theta_np).to(dev)
    plain = LatticeBatch.from_synth([l], device=dev)
    s = ops.sample_paths(plain, theta, 1, seed=5)
    n = int(s.lengths[0, 0])
    path = s.paths[0, 0, :n].cpu().numpy()
    assert n > 100 and path[0] == BOS and path[-1] == EOS
    dfa = WideDFA.sequence(250, path)
    assert dfa.n_states == n + 1 > 128
    host = LatticeBatch.from_synth([l])
    assert host.build_chunks(force=True)
    chunked = host.to(dev)
    assert chunked.chunks is not None
    r1, r2 = ops.intersect(plain, dfa), ops.intersect(chunked, dfa)
    GI._check("sequence", r1, plain, [l], _refs([l], dfa))
    _same_product(r1, r2)
    assert int(r1.lattice.n_rows[0]) == n + 1 and int(r1.lattice.n_arcs[0]) == n + 1  # one path and the sink's loop
    # the rows come in the order of the lattice's states; by automaton state -- the position in the string -- they are the path
    lab, arc_q, row_q = r1.lattice.arc_label.cpu().numpy(), r1.arc_q.cpu().numpy(), r1.row_q.cpu().numpy()
    src, dst = r1.lattice._t["arc_src"].cpu().numpy(), r1.lattice._t["arc_dst"].cpu().numpy()
    on = src != dst
    assert on.sum() == n and np.array_equal(np.sort(row_q), np.arange(n + 1)) and np.array_equal(np.sort(arc_q[on]), np.arange(n))
    assert np.array_equal(lab[on], path[arc_q[on]]) and np.array_equal(row_q[dst[on]], arc_q[on] + 1)
    tot, end = ops.score_paths(plain, theta, s.paths[:, :1, :n])
    assert int(end[0, 0]) == l.n_rows - 1
    want64 = float(theta_np[path].astype(np.float64).sum())
    # a float32 sum of n terms, in any order, is within n * 2^-24 * sum |theta_i| of the exact sum
    tol = n * 2.0 ** -24 * float(np.abs(theta_np[path]).astype(np.float64).sum())
    # and the two float32 values against each other: log Z of the one-path product IS the path's score.  The suites
    # hold a log Z to 1e-5 where its ulp is 3.8e-6 (test_gpu_intersect.py) and a path score likewise (test_gpu_paths.py),
    # so each to under three ulps of the truth: six ulps of the value between the two
    ulp = float(np.spacing(np.float32(abs(want64))))
    for r in (r1, r2):
        logz = float(ops.log_z(r.lattice, theta)[0])
        print(f"sequence: n {n}, log Z {logz!r}, score_paths {float(tot[0, 0])!r}, float64 {want64!r}, tol {tol:.3g}, "
              f"|log Z - score_paths| {abs(logz - float(tot[0, 0])) / ulp:.2f} ulp")
        assert abs(logz - want64) <= tol and abs(float(tot[0, 0]) - want64) <= tol
        assert abs(logz - float(tot[0, 0])) <= 6 * ulp


# ----------------------------------------------------------------------------- 5: projected sequences
def test_projected_sequence_on_the_star(dev):
    star = _star()
    keep = range(128)  # half of the labels
    _, res, refs = _run("star projected", [star, star], WideDFA.stack([WideDFA.projected_sequence(256, keep, [BOS, 5, EOS]),
                                                                       WideDFA.projected_sequence(256, keep, [BOS, 7, 5, EOS])]), dev)
    # the spokes with a label >= 128 are invisible to the first automaton: 75 of them; the second one names one spoke
    assert [r["n_rows"] for r in refs] == [75 + 4, 5]


def test_projected_sequence_on_the_few_paths_lattice(dev):
    (l,) = GI._lattices("edit63")
    dfa = _PROJ()
    paths = K.enumerate_paths(l.n_rows, l.src, l.dst, np.zeros(l.n_arcs), l.n_rows - 1)
    n_acc = sum(dfa.accepts(l.label[p]) for _, p in paths)
    assert len(paths) == 63 and 1 < n_acc < 63
    _, res, refs = _run("edit63 projected", [l], dfa, dev)
    assert len(R.product_paths(refs[0])) == n_acc


def _PROJ():
    """Of the marks (half of edit63's labels: 3, 4, 5 of the six and the specials) the insertion and output marks read
    "substitution, insertion, substitution"; the deletion that the three x need besides may come anywhere."""
    return WideDFA.projected_sequence(V, [4, 5], [5, 4, 4, 5, 4])


# ----------------------------------------------------------------------------- 6: one automaton per lattice, ragged
def test_ragged_automata_one_word_beside_many(dev):
    lats = GI._lattices("mixed5")
    # (on the edit lattice of five x and four y "at most nine marks" leaves the paths without a substitution)
    dfa = WideDFA.stack([WideDFA.accept_all(V), _chain(V, 200, HALF), _chain(V, 65, HALF, limit=20), _chain(V, 130, (3, 4, 5), limit=9),
                         WideDFA.accept_all(V)])
    assert dfa.n_lattices == 5 and dfa.n_states == 200 and list(np.diff(dfa.q_off)) == [1, 200, 65, 130, 1]
    lat, res, refs = _run("ragged", lats, dfa, dev)
    off = np.concatenate([[0], np.cumsum([r["n_rows"] for r in refs])])
    row_q = res.row_q.cpu().numpy()
    assert not row_q[off[0]:off[1]].any() and not row_q[off[4]:off[5]].any()
    assert [int(row_q[off[b]:off[b + 1]].max()) for b in (1, 2, 3)] == [199, 64, 129]
    assert refs[3]["n_rows"] < lats[3].n_rows  # (the limit binds)


# ----------------------------------------------------------------------------- 7: a bigram model as an automaton
def test_bigram_log_z_and_gradients_against_enumeration(dev):
    (l,) = GI._lattices("edit63")
    rng = np.random.default_rng(9)
    theta_np = synth.label_scores(8, V)
    logp_np, start_np = rng.normal(0.0, 0.3, (V, V)).astype(np.float32), rng.normal(0.0, 0.3, V).astype(np.float32)
    asc_np = rng.normal(0.0, 0.3, l.n_arcs).astype(np.float32)
    lat = LatticeBatch.from_synth([l], device=dev)
    logp = torch.from_numpy(logp_np).to(dev).requires_grad_(True)
    start = torch.from_numpy(start_np).to(dev).requires_grad_(True)
    asc = torch.from_numpy(asc_np).to(dev).requires_grad_(True)
    dfa = WideDFA.bigram(logp, start)
    assert dfa.n_states == V + 1
    res = ops.intersect(lat, dfa)
    GI._check("bigram", res, lat, [l], _refs([l], dfa))
    logz = ops.log_z(res.lattice, torch.from_numpy(theta_np).to(dev), res.scores(asc))
    logz.sum().backward()
    # float64, path by path
    t64 = torch.from_numpy(theta_np).double()
    logp64, start64, asc64 = (torch.from_numpy(a).double().requires_grad_(True) for a in (logp_np, start_np, asc_np))
    paths = K.enumerate_paths(l.n_rows, l.src, l.dst, np.zeros(l.n_arcs), l.n_rows - 1)
    assert len(paths) == 63
    tot = []
    for _, p in paths:
        lab = torch.from_numpy(l.label[np.asarray(p)].astype(np.int64))
        tot.append(t64[lab].sum() + asc64[torch.as_tensor(np.asarray(p), dtype=torch.int64)].sum() + start64[lab[0]] + logp64[lab[:-1], lab[1:]].sum())
    want = torch.logsumexp(torch.stack(tot), 0)
    want.backward()
    print(f"bigram: log Z {float(logz.detach()[0])!r}, float64 {float(want.detach())!r}")
    assert abs(float(logz.detach()[0]) - float(want.detach())) <= 1e-5
    # an entry's gradient sums the posteriors of n product arcs, each held to 1e-5 (test_gpu_intersect.py)
    lab, q = res.lattice.arc_label.cpu().numpy(), res.arc_q.cpu().numpy()
    loop = (res.lattice._t["arc_src"] == res.lattice._t["arc_dst"]).cpu().numpy()
    n_asc, n_logp, n_start = np.zeros(l.n_arcs), np.zeros((V, V)), np.zeros(V)
    np.add.at(n_asc, res.arc_map.cpu().numpy(), 1)
    np.add.at(n_logp, (q[(q > 0) & ~loop] - 1, lab[(q > 0) & ~loop]), 1)
    np.add.at(n_start, lab[(q == 0) & ~loop], 1)
    on = np.asarray(l.src != l.dst)  # (a self loop lies on no path; its gradient is the engine's convention)
    assert np.all(np.abs(asc.grad.cpu().numpy() - asc64.grad.numpy())[on] <= 1e-5 * np.maximum(n_asc, 1)[on])
    assert np.all(np.abs(logp.grad.cpu().numpy() - logp64.grad.numpy()) <= 1e-5 * np.maximum(n_logp, 1))
    assert np.all(np.abs(start.grad.cpu().numpy() - start64.grad.numpy()) <= 1e-5 * np.maximum(n_start, 1))
    assert float(logp.grad.sum()) > 1 and abs(float(start.grad.sum()) - 1) <= 1e-4


# ----------------------------------------------------------------------------- 8, 9: k best and samples
def test_k_best_of_the_product_is_the_filtered_k_best_of_the_input(dev):
    """test_gpu_intersect.py's argument, with the sparse automaton: neither list is truncated (63 paths, k = 64)."""
    (l,) = GI._lattices("edit63")
    dfa = _PROJ()
    lat = LatticeBatch.from_synth([l], device=dev)
    theta = torch.from_numpy(synth.label_scores(8, V)).to(dev)
    T = int(lat.depth.max()) + 1
    k0 = ops.k_best(lat, theta, 64, max_len=T)
    assert int(k0.n_paths[0]) == 63
    res = ops.intersect(lat, dfa)
    k1 = ops.k_best(res.lattice, theta, 64, max_len=T)
    paths0, len0, best0 = k0.paths.cpu().numpy()[0], k0.lengths.cpu().numpy()[0], k0.best.cpu().numpy()[0]
    keep = [j for j in range(63) if dfa.accepts(paths0[j, :len0[j]])]
    n = len(keep)
    assert 1 < n < 63 and int(k1.n_paths[0]) == n
    paths1, len1, best1 = k1.paths.cpu().numpy()[0], k1.lengths.cpu().numpy()[0], k1.best.cpu().numpy()[0]
    assert np.array_equal(paths1[:n], paths0[keep]) and np.array_equal(len1[:n], len0[keep])
    assert np.array_equal(best1[:n].view(np.int32), best0[keep].view(np.int32))
    arcs1 = k1.arcs.cpu().numpy()[0][:n]
    mapped = np.where(arcs1 >= 0, res.arc_map.cpu().numpy()[np.maximum(arcs1, 0)], -1)
    assert np.array_equal(mapped, k0.arcs.cpu().numpy()[0][keep])


def test_samples_of_the_product_are_accepted(dev):
    lats = GI._lattices("mixed")
    dfa = _chain(V, 130, (5,), limit=1)  # count51's language on the states 0, 129, 128
    narrow = GI._dfa("count51")
    lat = LatticeBatch.from_synth(lats, device=dev)
    res = ops.intersect(lat, dfa)
    assert np.array_equal(res.lattice.n_rows, [r["n_rows"] for r in GI._refs("mixed", "count51")])
    s = ops.sample_paths(res.lattice, torch.from_numpy(synth.label_scores(8, V)).to(dev), 32, seed=11)
    paths, lens = s.paths.cpu().numpy(), s.lengths.cpu().numpy()
    n5 = 0
    for b in range(len(lats)):
        for k in range(32):
            p = paths[b, k, :lens[b, k]]
            assert lens[b, k] > 0 and dfa.accepts(p) and narrow.accepts(p), (b, k)
            n5 += int((p == 5).sum())
    assert n5 > 0  # (the constraint binds: some samples use their one 5)


# ----------------------------------------------------------------------------- 10: constraint_log_prob
@pytest.mark.parametrize("wide", [True, False])
def test_constraint_log_prob_against_enumeration(dev, wide):
    (l,) = GI._lattices("edit63")
    dfa = _PROJ() if wide else GI._dfa("count51")
    theta_np = synth.label_scores(8, V)
    asc_np = np.random.default_rng(4).normal(0.0, 0.3, l.n_arcs).astype(np.float32)
    lat = LatticeBatch.from_synth([l, l], device=dev)
    theta = torch.from_numpy(theta_np).to(dev).requires_grad_(True)
    asc = torch.from_numpy(np.concatenate([asc_np, np.zeros_like(asc_np)])).to(dev)
    got = ops.constraint_log_prob(lat, theta, dfa, arc_scores=asc)
    paths = K.enumerate_paths(l.n_rows, l.src, l.dst, np.zeros(l.n_arcs), l.n_rows - 1)
    for b, a in enumerate((asc_np, np.zeros_like(asc_np))):
        sc = np.array([theta_np[l.label[np.asarray(p)]].astype(np.float64).sum() + a[np.asarray(p)].astype(np.float64).sum() for _, p in paths])
        acc = np.array([dfa.accepts(l.label[np.asarray(p)]) for _, p in paths])
        want = np.logaddexp.reduce(sc[acc]) - np.logaddexp.reduce(sc)
        print(f"constraint_log_prob lattice {b}: {float(got[b])!r}, float64 {want!r}")
        assert float(got[b]) <= 0 and abs(float(got[b]) - want) <= 2e-5  # (two log Z, each held to 1e-5)
    got.sum().backward()
    assert theta.grad is not None and bool(torch.isfinite(theta.grad).all()) and float(theta.grad.abs().sum()) > 0


# ----------------------------------------------------------------------------- 11: refusals
def test_product_beyond_the_row_limit_is_refused_before_any_packer(dev, monkeypatch):
    lats = GI._lattices("mixed")
    dfa = WideDFA.from_constraint(GI._dfa("count63"))
    live = RW.live_sets(lats[4], *dfa.to_dense())
    assert int(live[:-1].sum()) + 1 == 13293  # (test_gpu_intersect.py's figure)
    lat = LatticeBatch.from_synth(lats, device=dev)

    def no_packer(*a, **k):
        raise AssertionError("a packer was called")

    monkeypatch.setattr(LatticeBatch, "from_arcs_device", no_packer)
    monkeypatch.setattr(LatticeBatch, "from_arcs", no_packer)
    with pytest.raises(_lib.NfstError, match="lattice 4") as e:
        ops.intersect(lat, dfa)
    assert e.value.code == ERR_LIMIT and e.value.lattice == 4


def test_empty_product_names_the_lattice(dev):
    lats = GI._lattices("mixed5")
    lat = LatticeBatch.from_synth(lats, device=dev)
    ok = _chain(V, 70, HALF)
    bad = WideDFA.stack([ok, ok, WideDFA.sequence(V, [BOS, 7, 7, 7, EOS]), ok, ok])
    assert RW.intersect(lats[2], *bad.to_dense()[2])["n_rows"] == 0
    with pytest.raises(ValueError, match="lattice 2"):
        ops.intersect(lat, bad)
    with pytest.raises(ValueError, match="lattice 0"):  # no run survives bos
        ops.intersect(lat, WideDFA([-1], [0, 0], [], [], [1], vocab=V))


# ----------------------------------------------------------------------------- 12: determinism
def test_two_calls_give_equal_tensors(dev):
    lat = LatticeBatch.from_synth(GI._lattices("mixed5"), device=dev)
    dfa = _chain(V, 200, HALF)
    _same_product(ops.intersect(lat, dfa), ops.intersect(lat, dfa))


_STAR_FIRST = {}


@pytest.mark.parametrize("opts", STAR_OPTS)
def test_every_packing_of_the_input_gives_the_same_product(dev, opts):
    lats = [_star(), synth.layered_lattice(4, n_states=300, avg_degree=8.0, vocab=256, width=9, span=5)]
    dfa = _chain(256, 130, tuple(range(3, 100)), limit=25)
    lat = LatticeBatch.from_synth(lats, device=dev, **opts)
    res = ops.intersect(lat, dfa)
    got = [x.cpu() for x in _outputs(res)]
    if not _STAR_FIRST:
        GI._check("star packings", res, lat, lats, _refs(lats, dfa))
    first = _STAR_FIRST.setdefault("first", got)
    for x, y in zip(first, got):
        assert torch.equal(x, y)


# ----------------------------------------------------------------------------- 13: API
def test_lattice_scorer_constrain_and_constraint_log_prob(dev):
    lats = GI._lattices("mixed5")
    lat = LatticeBatch.from_synth(lats, device=dev)
    sc = LatticeScorer(V, pad=PAD, bos=BOS, eos=EOS, theta=torch.from_numpy(synth.label_scores(6, V))).to(dev)
    sc.set_lattice(lat)
    own = sc._lat()
    dfa = _chain(V, 130, (5,), limit=1)
    _same_product(sc.constrain(dfa), ops.intersect(lat, dfa))
    assert sc._lat() is own  # the scorer keeps its own lattice
    lp = sc.constraint_log_prob(dfa)
    assert torch.equal(lp, ops.constraint_log_prob(lat, sc.theta, dfa)) and lp.shape == (5,) and bool((lp <= 0).all())
    assert bool((lp < 0).any()) and lp.requires_grad


def test_bad_arguments_raise(dev):
    lats = GI._lattices("mixed5")
    lat = LatticeBatch.from_synth(lats, device=dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.intersect(LatticeBatch.from_synth(lats), _chain(V, 70, HALF))
    with pytest.raises(ValueError):
        ops.intersect(lat, _chain(V + 1, 70, HALF))  # another vocabulary
    with pytest.raises(ValueError):
        ops.intersect(lat, WideDFA([0], [0, 1], [V], [0], [1]))  # a label the batch does not have
    with pytest.raises(ValueError):
        ops.intersect(lat, WideDFA.stack([_chain(V, 70, HALF)] * 4))  # four automata, five lattices
    with pytest.raises(ValueError):
        ops.intersect(lat, _chain(V, 70, HALF), chunks="yes")

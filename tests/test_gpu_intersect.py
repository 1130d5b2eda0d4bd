"""ops.intersect / LatticeBatch.intersect (nfst_intersect_count / _write: the product of every lattice with a constraint
automaton) against the pure-Python restatement of tests/intersect_ref.py: every integer output bit for bit, the packed
product against the host packer on the reference's arc lists, and the existing ops on the product (log Z, gradients,
k best, sampling) against the oracle on the reference product."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from nfst_amd import _lib, ops, synth
from nfst_amd.constraints import ConstraintDFA
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from oracle import oracle as O
from tests import intersect_ref as R
from tests.test_gpu_slack import STAR_OPTS, _mixed_batch, _same_arrays, _star, _weighted_batch

pytestmark = pytest.mark.gpu
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
V = 64
MAX_ROWS = 8192  # NFST_MAX_ROWS
ERR_LIMIT = -6


# ----------------------------------------------------------------------------- lattices, automata and references, built once
def _commonest(l, k):
    c = np.bincount(l.label[l.src != l.dst], minlength=l.vocab)
    return [int(x) for x in np.lexsort((np.arange(l.vocab), -c))[:k]]


@functools.lru_cache(maxsize=None)
def _lattices(name):
    if name == "mixed":
        return tuple(_mixed_batch())
    if name == "mixed5":  # without the 700-state lattice
        m = _mixed_batch()
        return tuple(m[:4] + m[5:])
    if name == "wide16":
        return (synth.layered_lattice(11, n_states=1500, avg_degree=6.0, vocab=V, width=16, span=4),)
    if name == "wide40":
        return (synth.layered_lattice(12, n_states=2000, avg_degree=4.0, vocab=V, width=40, span=2),)
    if name == "star":
        return (_star(),)
    if name == "snips4":
        return tuple(synth.snips_shaped_batch(4, vocab=250))
    if name == "weighted":
        return tuple(_weighted_batch())
    if name == "edit63":
        return (synth.edit_lattice([10, 11, 12], [20, 21, 20], vocab=V, seed=5),)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _dfa(name, lats=None):
    if name == "accept_all":
        return ConstraintDFA.accept_all(V)
    if name == "count51":
        return ConstraintDFA.count_at_most(V, [5], 1)
    if name == "bigram79":
        return ConstraintDFA.forbid_bigram(V, 7, 9)
    if name == "parity":
        return ConstraintDFA.parity(V, range(3, 34))
    if name == "count63":
        return ConstraintDFA.count_at_most(V, range(3, 64), 63)  # Q = 64
    if name == "count33":
        return ConstraintDFA.count_at_most(V, range(3, 13), 33)  # Q = 34
    if name == "common2":
        return ConstraintDFA.count_at_most(V, _commonest(_lattices(lats)[0], 2), 2)
    if name == "common4":
        return ConstraintDFA.count_at_most(V, _commonest(_lattices(lats)[0], 4), 3)
    if name == "star_count":
        return ConstraintDFA.count_at_most(256, range(3, 100), 1)
    if name == "star_contains":
        return ConstraintDFA.contains(256, [7, 5])
    if name == "snips_parity":
        return ConstraintDFA.parity(250, range(3, 120))
    if name == "parity48":
        return ConstraintDFA.parity(48, range(3, 30))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _refs(lats_name, dfa_name):
    """The reference product of every lattice (read-only, shared by the tests)."""
    d = _dfa(dfa_name, lats_name if dfa_name.startswith("common") else None)
    return tuple(R.intersect(l, d.delta, d.final) for l in _lattices(lats_name))


def _pack_device(lats, dev, **opts):
    """The batch through the device packer: the same route, and so the same options, as the product takes."""
    n_rows, arc_off, src, label, dst, w = synth.batch_arcs(lats)
    return LatticeBatch.from_arcs_device(n_rows, arc_off, src, label, dst, lats[0].vocab, arc_w=w, device=dev, **opts)


def _check(tag, res, lat, lats, refs):
    """Every integer output equals the reference; the packed product is what the host packer makes of the reference's
    arc lists."""
    new, arc_map, arc_q, row_state, row_q = res
    assert arc_map.dtype == torch.int64 and arc_q.dtype == torch.int32
    assert row_state.dtype == torch.int32 and row_q.dtype == torch.int32
    assert new.n_lattices == len(lats) and new.vocab == lat.vocab
    rows = np.array([r["n_rows"] for r in refs])
    arcs = np.array([r["n_arcs"] for r in refs])
    assert np.array_equal(new.n_rows, rows), (tag, new.n_rows, rows)  # counts: rows
    assert np.array_equal(new.n_arcs, arcs), (tag, new.n_arcs, arcs)  # counts: arcs
    assert np.array_equal(new.meta_host[:, _lib.META_N_REACH], rows) and np.array_equal(new.sink, rows - 1)  # (every row kept)
    a_in = np.asarray(lat.arc_off, np.int64)
    cat = lambda k, off=None: np.concatenate([r[k] + (0 if off is None else off[b]) for b, r in enumerate(refs)])
    assert np.array_equal(arc_map.cpu().numpy(), cat("arc_map", a_in)), tag
    assert np.array_equal(arc_q.cpu().numpy(), cat("arc_q")), tag
    assert np.array_equal(row_state.cpu().numpy(), cat("row_state")), tag
    assert np.array_equal(row_q.cpu().numpy(), cat("row_q")), tag
    for k in ("src", "label", "dst"):
        assert np.array_equal(new._t["arc_" + k].cpu().numpy(), cat(k)), (tag, k)
    if lat.weighted:
        assert torch.equal(new.arc_w, lat.arc_w[arc_map])
    arc_off = np.zeros(len(refs) + 1, np.int64)
    np.cumsum(arcs, out=arc_off[1:])
    host = LatticeBatch.from_arcs(rows.astype(np.int32), arc_off, cat("src"), cat("label"), cat("dst"), lat.vocab,
                                  arc_w=None if not lat.weighted else lat.arc_w.cpu().numpy()[cat("arc_map", a_in)])
    _same_arrays(new, host)


def _run(lats_name, dfa_name, dev, **opts):
    lats, refs = _lattices(lats_name), _refs(lats_name, dfa_name)
    assert all(0 < r["n_rows"] <= MAX_ROWS for r in refs), [r["n_rows"] for r in refs]  # (a wrong shape is an error, not a skip)
    dfa = _dfa(dfa_name, lats_name if dfa_name.startswith("common") else None)
    lat = LatticeBatch.from_synth(lats, device=dev)
    res = ops.intersect(lat, dfa, **opts)
    _check(f"{lats_name} x {dfa_name}", res, lat, lats, refs)
    return lat, res, refs, dfa


# ----------------------------------------------------------------------------- 1, 2: against the reference
def test_accept_all_gives_the_input(dev):
    lat, res, refs, _ = _run("mixed", "accept_all", dev)
    new = res.lattice
    assert np.array_equal(new.n_rows, lat.meta_host[:, _lib.META_N_REACH])
    for k in ("arc_src", "arc_label", "arc_dst"):
        assert torch.equal(new._t[k], lat._t[k]), k
    assert torch.equal(res.arc_map, torch.arange(lat.total_arcs, device=dev))
    assert bool((res.arc_q == 0).all()) and bool((res.row_q == 0).all())


@pytest.mark.parametrize("dfa", ["count51", "bigram79", "parity"])
def test_mixed_batch(dev, dfa):
    _, res, refs, _ = _run("mixed", dfa, dev)
    assert max(r["n_rows"] for r in refs) <= 1363 and max(r["n_arcs"] for r in refs) <= 13340
    if dfa == "count51":
        assert refs[4]["n_rows"] == 1363 and refs[4]["n_arcs"] == 13340


# ----------------------------------------------------------------------------- 3: the upper half of the masks
@pytest.mark.parametrize("dfa,rows", [("count63", 4126), ("count33", 3658)])
def test_more_than_32_automaton_states(dev, dfa, rows):
    assert _dfa(dfa).n_states > 32
    _, res, refs, _ = _run("mixed5", dfa, dev)
    assert max(r["n_rows"] for r in refs) == rows
    # how far the counts get is the reference's to say: under count33 no path of these lattices carries more than 31 of
    # the ten labels, so its pairs stay below bit 32 although Q = 34; under count63 they go up to bit 63
    assert int(res.row_q.max()) == max(int(r["row_q"].max()) for r in refs)
    assert int(res.arc_q.max()) == max(int(r["arc_q"].max()) for r in refs)
    if dfa == "count63":
        assert refs[1]["n_arcs"] == 32968 and int(res.row_q.max()) == 63


# ----------------------------------------------------------------------------- 4: one automaton per lattice
_EDIT_XY = [([10, 11, 12], [20, 21, 20]), ([10, 11], [22, 23, 24, 25]), ([12, 13, 14, 15], [20]), ([10, 11, 12], [30, 31])]


def test_per_lattice_automata_give_identity_products(dev):
    lats = [synth.edit_lattice(x, y, vocab=V, seed=7 + i) for i, (x, y) in enumerate(_EDIT_XY)]
    dfa = ConstraintDFA.stack([ConstraintDFA.marked_sequence(V, 4, y) for _, y in _EDIT_XY])
    assert dfa.n_lattices == 4 and dfa.n_states == 10
    lat = _pack_device(lats, dev)
    res = ops.intersect(lat, dfa)
    refs = [R.intersect(l, dfa.delta[b], dfa.final[b]) for b, l in enumerate(lats)]
    _check("per-lattice", res, lat, lats, refs)
    _same_arrays(res.lattice, lat)  # identical arc lists, packed with the same options: identical batches
    assert torch.equal(res.arc_map, torch.arange(lat.total_arcs, device=dev))
    theta = torch.from_numpy(synth.label_scores(8, V)).to(dev)
    assert torch.equal(ops.log_z(res.lattice, theta), ops.log_z(lat, theta))  # bit for bit
    # one y changed: that lattice's product is empty
    ys = [y for _, y in _EDIT_XY]
    ys[2] = [21]
    bad = ConstraintDFA.stack([ConstraintDFA.marked_sequence(V, 4, y) for y in ys])
    assert R.intersect(lats[2], bad.delta[2], bad.final[2])["n_rows"] == 0
    with pytest.raises(ValueError, match="lattice 2"):
        ops.intersect(lat, bad)


# ----------------------------------------------------------------------------- 5: more states than threads, wide levels, a heavy state
@pytest.mark.parametrize("lats,dfa,rows", [("wide16", "common2", 4385), ("wide16", "common4", 5806), ("wide40", "common2", 5702),
                                           ("wide40", "common4", 7538)])
def test_more_rows_than_threads_and_wide_levels(dev, lats, dfa, rows):
    _, _, refs, _ = _run(lats, dfa, dev)
    assert refs[0]["n_rows"] == rows and _lattices(lats)[0].n_rows > 1024


@pytest.mark.parametrize("dfa,rows,arcs", [("star_count", 107, 209), ("star_contains", 5, 5)])
def test_star(dev, dfa, rows, arcs):
    _, _, refs, _ = _run("star", dfa, dev)
    assert (refs[0]["n_rows"], refs[0]["n_arcs"]) == (rows, arcs)


def test_snips_shaped_with_and_without_chunked_programs(dev):
    lats, refs = _lattices("snips4"), _refs("snips4", "snips_parity")
    assert all(0 < r["n_rows"] <= MAX_ROWS for r in refs)
    dfa = _dfa("snips_parity")
    plain = LatticeBatch.from_synth(lats, device=dev)
    host = LatticeBatch.from_synth(lats)
    assert host.build_chunks(force=True)
    chunked = host.to(dev)
    assert chunked.chunks is not None
    r1 = ops.intersect(plain, dfa)
    _check("snips", r1, plain, lats, refs)
    r2 = ops.intersect(chunked, dfa)
    assert r2.lattice.chunks is None
    _same_arrays(r1.lattice, r2.lattice)
    for x, y in zip(list(r1)[1:], list(r2)[1:]):
        assert torch.equal(x, y)
    r3 = ops.intersect(plain, dfa, chunks="force", group_mode=1)  # (passed through to the packer)
    assert r3.lattice.chunks is not None
    r4 = ops.intersect(plain, dfa, group_mode=1)
    _same_arrays(r3.lattice, r4.lattice)
    assert torch.equal(r3.arc_map, r1.arc_map)
    theta = torch.from_numpy(synth.label_scores(64, 250, mean=-1.5, std=0.8)).to(dev)
    assert torch.allclose(ops.log_z(r3.lattice, theta), ops.log_z(r1.lattice, theta), rtol=0, atol=1e-5)


# ----------------------------------------------------------------------------- 6: limits
def test_product_beyond_the_row_limit_is_refused_before_any_packer(dev, monkeypatch):
    lats = _lattices("mixed")
    dfa = _dfa("count63")
    live = R.masks(lats[4], dfa.delta, dfa.final)[2]
    assert sum(bin(m).count("1") for m in live[:-1]) + 1 == 13293  # (every pair of the other states, one row for the sink)
    lat = LatticeBatch.from_synth(lats, device=dev)

    def no_packer(*a, **k):
        raise AssertionError("a packer was called")

    monkeypatch.setattr(LatticeBatch, "from_arcs_device", no_packer)
    monkeypatch.setattr(LatticeBatch, "from_arcs", no_packer)
    with pytest.raises(_lib.NfstError, match="lattice 4") as e:
        ops.intersect(lat, dfa)
    assert e.value.code == ERR_LIMIT and e.value.lattice == 4


def test_more_than_64_automaton_states_are_refused_on_the_host(dev):
    with pytest.raises(ValueError):
        ConstraintDFA(np.zeros((65, V), np.int64), np.ones(65))
    lat = LatticeBatch.from_synth(_lattices("mixed"), device=dev)
    bs = C.byref(lat.c_struct())
    assert _lib.lib.nfst_intersect_ws_bytes(bs, 65) == ERR_LIMIT
    ws_bytes = int(_lib.lib.nfst_intersect_ws_bytes(bs, 64))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    delta_t = torch.full((V, 64), -1, dtype=torch.int8, device=dev)
    fin = torch.ones(1, dtype=torch.int64, device=dev)
    cs = torch.full((3 * lat.n_lattices,), 77, dtype=torch.int32, device=dev)
    assert _lib.lib.nfst_intersect_count(bs, delta_t.data_ptr(), 0, fin.data_ptr(), 0, 65, ws.data_ptr(), ws_bytes, cs.data_ptr(),
                                         cs[2 * lat.n_lattices:].data_ptr(), None) == ERR_LIMIT
    assert bool((cs == 77).all())  # nothing was launched


# ----------------------------------------------------------------------------- 7: numbers on the product
@pytest.mark.parametrize("lats,dfa", [("mixed", "count51"), ("mixed", "bigram79"), ("mixed", "parity"), ("mixed5", "count63"),
                                      ("mixed5", "count33")])
def test_log_z_of_the_product_against_the_oracle(dev, lats, dfa):
    refs = _refs(lats, dfa)
    assert all(0 < r["n_rows"] <= MAX_ROWS for r in refs)
    theta_np = synth.label_scores(8, V)
    lat = LatticeBatch.from_synth(_lattices(lats), device=dev)
    res = ops.intersect(lat, _dfa(dfa))
    logz = ops.log_z(res.lattice, torch.from_numpy(theta_np).to(dev)).cpu().numpy().astype(np.float64)
    for b, r in enumerate(refs):
        o = O.forward_backward(r["n_rows"], r["src"], r["dst"], theta_np[r["label"]].astype(np.float64))
        print(f"{lats} x {dfa} lattice {b}: rows {r['n_rows']}, |log Z error| {abs(logz[b] - o['logZ']):.3g}")
        assert abs(logz[b] - o["logZ"]) <= 1e-5, (b, logz[b], o["logZ"])


def test_scores_and_gradients_through_arc_map_and_the_automaton_weights(dev):
    lats, refs = _lattices("weighted"), _refs("weighted", "parity48")
    assert all(0 < r["n_rows"] <= MAX_ROWS for r in refs)
    base = _dfa("parity48")
    rng = np.random.default_rng(3)
    theta_np = rng.normal(-2.0, 0.7, size=48).astype(np.float32)
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert lat.weighted == 1
    asc_np = rng.normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32)
    w_np = rng.normal(0.0, 0.3, size=(2, 48)).astype(np.float32)
    asc = torch.from_numpy(asc_np).to(dev).requires_grad_(True)
    weight = torch.from_numpy(w_np).to(dev).requires_grad_(True)
    dfa = ConstraintDFA(base.delta, base.final, weight)
    res = ops.intersect(lat, dfa)
    _check("weighted", res, lat, lats, refs)
    sc = res.scores(asc)
    assert sc.dtype == torch.float32 and sc.shape == (res.lattice.total_arcs,) and bool(torch.isfinite(sc).all())
    theta = torch.from_numpy(theta_np).to(dev)
    logz = ops.log_z(res.lattice, theta, sc)
    logz.sum().backward()
    g_asc, g_w = asc.grad.cpu().numpy().astype(np.float64), weight.grad.cpu().numpy().astype(np.float64)
    want_asc, want_w = np.zeros(lat.total_arcs), np.zeros((2, 48))
    n_asc, n_w = np.zeros(lat.total_arcs), np.zeros((2, 48))
    for b, (l, r) in enumerate(zip(lats, refs)):
        a0 = int(lat.arc_off[b])
        am = r["arc_map"]
        s64 = (theta_np[r["label"]].astype(np.float64) + l.weight[am].astype(np.float64) + asc_np[a0 + am].astype(np.float64)
               + w_np[r["arc_q"], r["label"]].astype(np.float64))
        o = O.forward_backward(r["n_rows"], r["src"], r["dst"], s64)
        assert abs(float(logz[b]) - o["logZ"]) <= 1e-5, (b, float(logz[b]), o["logZ"])
        on = np.ones(r["n_arcs"], bool)  # (every arc, as test_autograd_gives_posteriors compares them: the oracle's posterior of a self loop included)
        np.add.at(want_asc, a0 + am[on], o["posterior"][on])
        np.add.at(n_asc, a0 + am[on], 1)
        np.add.at(want_w, (r["arc_q"][on], r["label"][on]), o["posterior"][on])
        np.add.at(n_w, (r["arc_q"][on], r["label"][on]), 1)
    # test_gpu_slack.py::test_gradient_flows_through_arc_map: arcs outside arc_map get exactly zero, the rest is positive
    outside = torch.ones(lat.total_arcs, dtype=torch.bool, device=dev)
    outside[res.arc_map] = False
    assert bool((asc.grad[outside] == 0).all()) and float(asc.grad.sum()) > 0
    # and the values: one product arc's gradient is its posterior, which the engine holds to 1e-5 of the oracle
    # (test_gpu_parity.py::test_autograd_gives_posteriors); an entry that sums n product arcs is held to n times that
    assert np.all(np.abs(g_asc - want_asc) <= 1e-5 * np.maximum(n_asc, 1))
    assert np.all(np.abs(g_w - want_w) <= 1e-5 * np.maximum(n_w, 1))
    assert g_w[:, 3:30].sum() > 0


# ----------------------------------------------------------------------------- 8: k best
def test_k_best_of_the_product_is_the_filtered_k_best_of_the_input(dev):
    """The 63-path lattice has fewer than 64 paths, so neither list is truncated: the product's paths are the accepted
    paths of the input over the same arcs in the same float32 adds, and the order argument of DESIGN.md section 4.6
    (score desc, then canonical arc, then rank -- which the product keeps, its arcs being in the input's order per
    row) carries over: the filtered list is the product's list, bit for bit."""
    (l,) = _lattices("edit63")
    dfa = _dfa("count51")
    lat = LatticeBatch.from_synth([l], device=dev)
    theta = torch.from_numpy(synth.label_scores(8, V)).to(dev)
    T = int(lat.depth.max()) + 1
    k0 = ops.k_best(lat, theta, 64, max_len=T)
    assert int(k0.n_paths[0]) == 63
    res = ops.intersect(lat, dfa)
    k1 = ops.k_best(res.lattice, theta, 64, max_len=T)
    paths0, len0, best0 = k0.paths.cpu().numpy()[0], k0.lengths.cpu().numpy()[0], k0.best.cpu().numpy()[0]
    keep = [j for j in range(63) if dfa.accepts(paths0[j, :len0[j]])]
    assert len(keep) == 50 and int(k1.n_paths[0]) == 50
    paths1, len1, best1 = k1.paths.cpu().numpy()[0], k1.lengths.cpu().numpy()[0], k1.best.cpu().numpy()[0]
    assert np.array_equal(paths1[:50], paths0[keep]) and np.array_equal(len1[:50], len0[keep])
    assert np.array_equal(best1[:50].view(np.int32), best0[keep].view(np.int32))
    arcs1 = k1.arcs.cpu().numpy()[0][:50]
    mapped = np.where(arcs1 >= 0, res.arc_map.cpu().numpy()[np.maximum(arcs1, 0)], -1)
    assert np.array_equal(mapped, k0.arcs.cpu().numpy()[0][keep])


# ----------------------------------------------------------------------------- 9: sampling
@pytest.mark.parametrize("dfa", ["count51", "bigram79", "parity"])
def test_samples_of_the_product_are_accepted(dev, dfa):
    lats, refs = _lattices("mixed"), _refs("mixed", dfa)
    d = _dfa(dfa)
    lat = LatticeBatch.from_synth(lats, device=dev)
    res = ops.intersect(lat, d)
    theta_np = synth.label_scores(8, V)
    theta = torch.from_numpy(theta_np).to(dev)
    s = ops.sample_paths(res.lattice, theta, 32, seed=11)
    paths, lens, logq = s.paths.cpu().numpy(), s.lengths.cpu().numpy(), s.logq.cpu().numpy()
    for b, r in enumerate(refs):
        sc = theta_np[r["label"]].astype(np.float64)
        o = O.forward_backward(r["n_rows"], r["src"], r["dst"], sc)
        tot, end = O.score_paths(r["n_rows"], r["src"], r["label"], r["dst"], sc, paths[b])
        assert np.all(end == r["n_rows"] - 1) and np.all(lens[b] > 0)
        for k in range(32):
            assert d.accepts(paths[b, k, :lens[b, k]]), (b, k)
        # log q = path score - log Z of the product, at the existing sampler tests' bound (test_gpu_paths.py: TOL)
        assert np.max(np.abs(tot - o["logZ"] - logq[b])) <= 2e-5, b


# ----------------------------------------------------------------------------- 10: determinism
def test_two_calls_give_equal_tensors(dev):
    lat = LatticeBatch.from_synth(_lattices("mixed"), device=dev)
    a, b = ops.intersect(lat, _dfa("parity")), ops.intersect(lat, _dfa("parity"))
    _same_arrays(a.lattice, b.lattice)
    for x, y in zip(list(a)[1:], list(b)[1:]):
        assert torch.equal(x, y)


_STAR_FIRST = {}


@pytest.mark.parametrize("opts", STAR_OPTS)
def test_every_packing_of_the_input_gives_the_same_product(dev, opts):
    star = _star()
    lats = [star, synth.layered_lattice(4, n_states=300, avg_degree=8.0, vocab=256, width=9, span=5)]
    lat = LatticeBatch.from_synth(lats, device=dev, **opts)
    res = ops.intersect(lat, _dfa("star_count"))
    got = [x.cpu() for x in list(res)[1:]] + [res.lattice._t[k].cpu() for k in ("arc_src", "arc_label", "arc_dst")]
    if not _STAR_FIRST:
        refs = [R.intersect(l, _dfa("star_count").delta, _dfa("star_count").final) for l in lats]
        _check("star packings", res, lat, lats, refs)
    first = _STAR_FIRST.setdefault("first", got)
    for x, y in zip(first, got):
        assert torch.equal(x, y)


# ----------------------------------------------------------------------------- 11: API
def test_lattice_scorer_constrain(dev):
    lats = _lattices("mixed")
    lat = LatticeBatch.from_synth(lats, device=dev)
    sc = LatticeScorer(V, pad=PAD, bos=BOS, eos=EOS, theta=torch.from_numpy(synth.label_scores(6, V))).to(dev)
    sc.set_lattice(lat)
    own = sc._lat()
    p1, p2 = sc.constrain(_dfa("count51")), ops.intersect(lat, _dfa("count51"))
    _same_arrays(p1.lattice, p2.lattice)
    for x, y in zip(list(p1)[1:], list(p2)[1:]):
        assert torch.equal(x, y)
    assert sc._lat() is own  # the scorer keeps its own lattice


def test_bad_arguments_raise(dev):
    lats = _lattices("mixed")
    lat = LatticeBatch.from_synth(lats, device=dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.intersect(LatticeBatch.from_synth(lats), _dfa("parity"))
    with pytest.raises(ValueError):
        ops.intersect(lat, ConstraintDFA.parity(V + 1, [5]))  # another vocabulary
    with pytest.raises(ValueError):
        ops.intersect(lat, ConstraintDFA.stack([_dfa("parity")] * 5))  # five automata, six lattices
    with pytest.raises(ValueError):
        ops.intersect(lat, _dfa("parity"), chunks="yes")
    with pytest.raises(ValueError, match="lattice 0"):  # nothing is accepted: no run survives bos
        ops.intersect(lat, ConstraintDFA(np.full((1, V), -1, np.int64), [1]))

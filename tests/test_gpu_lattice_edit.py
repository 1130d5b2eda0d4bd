"""ops.lattice_edit_distance (nfst_lattice_edit: the edit distance between a reference and a whole lattice, with the
oracle path) against the NumPy restatement of tests/lattice_edit_ref.py: integers exactly, scores and paths bit for bit.
tests/test_lattice_edit_cpu.py holds that restatement to brute force over every path and proves that the inputs of the
tie and dead-label cases are what those cases need."""
import numpy as np
import pytest
import torch

from nfst_amd import _lib, ops, synth
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from tests import edge_cases as E
from tests import kbest_ref
from tests import lattice_edit_ref as LR

pytestmark = pytest.mark.gpu
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
V = E.V_MIXED


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _ref_rows(refs, R=None, tail=EOS):
    """(ref [B, R] int32 with every row's tail filled with ``tail``, lengths [B] int32)"""
    n = np.array([len(r) for r in refs], np.int32)
    out = np.full((len(refs), max(1, int(n.max()) + 2) if R is None else R), tail, np.int32)
    for b, r in enumerate(refs):
        out[b, :len(r)] = r
    return out, n


def _path_labels(l, theta_b=None, k=1):
    """The labels of the best path of l (under zero scores without theta_b: the first path in arc order)."""
    th, e = kbest_ref.arc_terms(l, np.zeros(l.vocab, np.float32) if theta_b is None else theta_b)
    return l.label[kbest_ref.k_best(l.n_rows, l.src, l.dst, th, e, k, l.n_rows - 1)["arcs"][k - 1]].astype(np.int64)


def _stretched(y, n):
    """y stretched or cut to n tokens with every third token replaced"""
    r = np.resize(y, n).astype(np.int64) if n else np.zeros(0, np.int64)
    r[2::3] = synth.N_SPECIAL + (r[2::3] + 7) % 11
    return r


def _check(tag, lat, lats, r, want, ref, ref_len, scored):
    """Every output of the op against the restatement's results ``want``, and the op's own distance against
    ops.edit_distance of its path."""
    dist, lens = r.distance.cpu().numpy(), r.lengths.cpu().numpy()
    paths, arcs, align, counts = (x.cpu().numpy() for x in (r.paths, r.path_arcs, r.align, r.counts))
    assert (r.score is not None) == scored
    score = r.score.detach().cpu().numpy() if scored else None
    for b, (l, w) in enumerate(zip(lats, want)):
        a0, m = int(lat.arc_off[b]), len(w["arcs"])
        assert dist[b] == w["distance"], (tag, b, dist[b], w["distance"])
        assert lens[b] == m, (tag, b)
        assert np.array_equal(arcs[b, :m] - a0, w["arcs"]), (tag, b)
        assert np.array_equal(paths[b, :m], l.label[w["arcs"]]), (tag, b)
        assert np.array_equal(align[b, :m], w["align"]), (tag, b)
        assert tuple(counts[b]) == tuple(w["counts"]), (tag, b)
        assert np.all(paths[b, m:] == PAD) and np.all(arcs[b, m:] == -1) and np.all(align[b, m:] == -1), (tag, b)
        if scored:
            assert score[b:b + 1].view(np.int32)[0] == np.asarray([w["score"]], np.float32).view(np.int32)[0], (tag, b, score[b], w["score"])
    has = r.distance >= 0
    if bool(has.any()):
        d = ops.edit_distance(r.paths[has], r.lengths[has], ref[has], ref_len[has])
        assert torch.equal(d, r.distance[has]), tag


def _run(tag, lat, lats, refs, dev, theta_np=None, asc_np=None, tails=(EOS,)):
    want = LR.of_batch(lats, refs, theta_np, asc_np)
    out = None
    for tail in tails:
        rows, n = _ref_rows(refs, tail=tail)
        ref, ref_len = _t(rows, dev), _t(n, dev)
        r = ops.lattice_edit_distance(lat, ref, ref_len, _t(theta_np, dev), _t(asc_np, dev), pad=PAD)
        _check(f"{tag} tail {tail}", lat, lats, r, want, ref, ref_len, theta_np is not None)
        out = out or r
    return out, want


# ----------------------------------------------------------------------------- 1: strip boundaries
@pytest.fixture(scope="module")
def deep_pair():
    lats = [E.mixed_batch()[2], E.mixed_batch()[4]]
    theta = np.stack([synth.label_scores(60 + b, V) for b in range(2)])
    return lats, theta, [_path_labels(l, theta[b]) for b, l in enumerate(lats)]


@pytest.mark.parametrize("n", [0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 200])
def test_strip_boundaries(dev, deep_pair, n):
    """References of every length around the 64-column strips, on a deep lattice of width 1 (90 states) and a wide one;
    the rows carry a tail behind n -- the path's own next label, which would shorten the distance, then another one --
    that must not be read."""
    lats, theta, ys = deep_pair
    lat = LatticeBatch.from_synth(lats, device=dev)
    refs = [_stretched(y, n) for y in ys]
    tail = int(np.resize(ys[0], n + 1)[n])
    _run(f"strips n={n}", lat, lats, refs, dev, theta, tails=(tail, 17))
    _run(f"strips n={n} unscored", lat, lats, refs, dev, tails=(tail,))


# ----------------------------------------------------------------------------- 2: the mixed batch
def test_mixed_batch_in_one_launch(dev):
    lats = E.mixed_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = np.stack([synth.label_scores(70 + b, V) for b in range(len(lats))])
    asc = np.random.default_rng(2).normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32)
    refs = [_stretched(_path_labels(l, theta[b]), (0, 9, 40, 12, 33, 1)[b]) for b, l in enumerate(lats)]
    _run("mixed", lat, lats, refs, dev, theta, asc)
    _run("mixed shared theta", lat, lats, refs, dev, theta[0])
    _run("mixed unscored", lat, lats, refs, dev)


@pytest.mark.parametrize("weighted", [False, True])
def test_weighted_lattices(dev, weighted):
    lats = E.weighted_lats(weighted)
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert lat.weighted == int(weighted)
    rng = np.random.default_rng(3)
    theta = rng.normal(-2.0, 0.7, size=(len(lats), E.V_WEIGHTED)).astype(np.float32)
    asc = rng.normal(0.0, 0.3, size=lat.total_arcs).astype(np.float32)
    refs = [_stretched(_path_labels(l, theta[b]), 20 + 9 * b) for b, l in enumerate(lats)]
    _run("weighted", lat, lats, refs, dev, theta, asc)
    _run("weighted unscored", lat, lats, refs, dev)  # (arc_w is not read either)


# ----------------------------------------------------------------------------- 3: fan-out and packings
def test_fan_out_under_two_packings(dev):
    """The star and the double funnel (200 out-arcs: four chunks of 64), a layer of 24 states (more states per level
    than waves), and the tie of the star against a label that no arc carries: the same bits under both packings."""
    lats = E.packing_lattices()
    theta = synth.label_scores(4, 256)
    refs = [np.array([250]), _stretched(_path_labels(lats[1], theta), 7), _stretched(_path_labels(lats[2], theta), 70)]
    results = []
    for opts in (E.STAR_PACKINGS[0], E.STAR_PACKINGS[-1]):
        lat = LatticeBatch.from_synth(lats, device=dev, **opts)
        r, want = _run(f"packing {opts}", lat, lats, refs, dev, theta)
        results.append((r, _run(f"packing {opts} unscored", lat, lats, refs, dev)[0]))
    assert want[0]["distance"] == 4 and want[0]["arcs"][1] != 1  # (the score decided the star's tie, not the arc order)
    for x, y in zip(results[0][0] + results[0][1], results[1][0] + results[1][1]):
        assert (x is None and y is None) or torch.equal(x, y)


# ----------------------------------------------------------------------------- 4: more lattices than compute units
def test_more_lattices_than_compute_units(dev):
    lats, theta, asc = E.many_small()
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert lat.n_lattices == 330
    rng = np.random.default_rng(8)
    refs = [rng.integers(synth.N_SPECIAL, 40, size=int(rng.integers(0, 41))) for _ in lats]
    for b in range(0, 330, 3):  # (a third of them near a path, so that matches occur)
        refs[b] = _stretched(_path_labels(lats[b], theta[b]), len(refs[b]))
    assert {0, 40} <= {len(r) for r in refs}
    _run("330 lattices", lat, lats, refs, dev, theta, asc)


# ----------------------------------------------------------------------------- 5: identities
def test_the_viterbi_path_is_at_distance_zero(dev):
    lats = E.mixed_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = _t(np.stack([synth.label_scores(80 + b, V) for b in range(len(lats))]), dev)
    v = ops.viterbi(lat, theta, pad=PAD)
    r = ops.lattice_edit_distance(lat, v.paths, v.lengths, theta, pad=PAD)
    assert bool((r.distance == 0).all()) and bool((r.counts == 0).all())
    assert torch.equal(r.paths, v.paths) and torch.equal(r.path_arcs, v.arcs) and torch.equal(r.lengths, v.lengths)
    assert torch.equal(r.score, ops.k_best(lat, theta, 1, pad=PAD).best[:, 0])
    steps = torch.arange(v.paths.shape[1], device=dev)[None, :]
    assert torch.equal(r.align, torch.where(steps < v.lengths[:, None], steps, -1).to(torch.int32))


def _shortest_path(l):
    """arcs of the shortest path from state 0 to the sink (self loops are on no path)"""
    best = np.full(l.n_rows, 10 ** 9)
    best[0] = 0
    for _ in range(l.n_rows):  # (Bellman-Ford over the arcs: the lattices here are small)
        new = best.copy()
        ok = l.src != l.dst
        np.minimum.at(new, l.dst[ok], best[l.src[ok]] + 1)
        if np.array_equal(new, best):
            break
        best = new
    return int(best[l.n_rows - 1])


def test_the_empty_reference_finds_the_shortest_path(dev):
    lats = E.mixed_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    ref = torch.full((len(lats), 3), 9, dtype=torch.int64, device=dev)
    r = ops.lattice_edit_distance(lat, ref, torch.zeros(len(lats), dtype=torch.int64, device=dev))
    assert r.score is None
    assert r.distance.tolist() == [_shortest_path(l) for l in lats] == r.lengths.tolist()
    assert bool((r.align == -1).all()) and r.counts[:, 1].tolist() == r.distance.tolist()
    empty = ops.lattice_edit_distance(lat, ref[:, :0], torch.zeros(len(lats), dtype=torch.int32, device=dev))
    for x, y in zip(r, empty):
        assert (x is None and y is None) or torch.equal(x, y)


def test_against_the_minimum_over_all_paths_of_a_short_list(dev):
    """A lattice that keeps n < 64 finite paths: the 64-best list holds them all, so the least ops.edit_distance over
    the list is the exact answer; on the other lattices the list only bounds it from above."""
    lats, theta_np, b, n = E.few_paths_case()
    assert 0 < n < 64
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = _t(theta_np, dev)
    kb = ops.k_best(lat, theta, 64, pad=PAD)
    assert int(kb.n_paths[b]) == n
    refs = [_stretched(_path_labels(l, theta_np[i], k=2 if i < 5 else 1), (11, 30, 50, 9, 25, 2)[i]) for i, l in enumerate(lats)]
    rows, ref_len = _ref_rows(refs)
    ref, ref_len = _t(rows, dev), _t(ref_len, dev)
    r = ops.lattice_edit_distance(lat, ref, ref_len, theta, pad=PAD)
    d = ops.edit_distance(kb.paths, kb.lengths, ref, ref_len)  # [B, 64]
    live = torch.arange(64, device=dev)[None, :] < kb.n_paths[:, None]
    upper = torch.where(live, d, torch.full_like(d, 10 ** 6)).min(dim=1).values
    assert int(upper[b]) == int(r.distance[b])
    assert bool((r.distance <= upper).all()) and bool((r.distance >= 0).all())


# ----------------------------------------------------------------------------- 6: dead labels, no path
def test_dead_labels(dev):
    lats, theta, refs = LR.dead_label_case()
    lat = LatticeBatch.from_synth(lats, device=dev)
    r, _ = _run("dead labels", lat, lats, refs, dev, theta)
    free, _ = _run("dead labels unscored", lat, lats, refs, dev)
    assert bool((r.distance >= free.distance).all()) and bool((r.distance > free.distance).any())
    paths, lens = r.paths.cpu().numpy(), r.lengths.cpu().numpy()
    for b in range(len(lats)):
        assert not np.isin(paths[b, :lens[b]], E.DEAD).any()


@pytest.mark.parametrize("weighted", [False, True])
def test_lattices_without_a_path(dev, weighted):
    lats, theta = E.no_path_case(weighted)
    lat = LatticeBatch.from_synth(lats, device=dev)
    refs = [_stretched(_path_labels(l), 15) for l in lats]
    r, want = _run("no path", lat, lats, refs, dev, theta)
    assert [w["distance"] < 0 for w in want] == [False, True, False, True, False]
    for b in (1, 3):
        assert int(r.distance[b]) == -1 and bool(torch.isneginf(r.score[b])) and int(r.lengths[b]) == 0
        assert bool((r.paths[b] == PAD).all()) and bool((r.path_arcs[b] == -1).all()) and bool((r.align[b] == -1).all())
        assert r.counts[b].tolist() == [0, 0, 0]


# ----------------------------------------------------------------------------- 7: status words
def _raw(lat, ref, ref_len, theta, max_len):
    """nfst_lattice_edit without the wrapper's read-back of the status: (result, status)"""
    B, dev = lat.n_lattices, lat.device
    sc, keep = ops._scores(lat, theta, None)
    best, paths, arcs, lens, _, _ = ops._path_outputs(lat, (B,), max_len, best=True)
    dist, align = torch.empty(B, dtype=torch.int32, device=dev), torch.empty((B, max_len), dtype=torch.int32, device=dev)
    counts, status = torch.empty((B, 3), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ws, ws_bytes = ops._workspace(lat, "nfst_lattice_edit_ws_bytes", ref.shape[1])
    ops._call("nfst_lattice_edit", lat, sc, ref, ref_len, ref.shape[1], ws, ws_bytes, dist, best, paths, arcs, align, lens, counts,
              max_len, PAD, status)
    return ops.LatticeEditResult(dist, best, paths, arcs, align, lens, counts), int(status.item())


def test_reference_lengths_outside_their_rows(dev):
    lats = E.mixed_batch()[:4]
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta_np = synth.label_scores(5, V)
    theta = _t(theta_np, dev)
    refs = [_stretched(_path_labels(l, theta_np), 8) for l in lats]
    rows, n = _ref_rows(refs)
    R = rows.shape[1]
    bad = n.copy()
    bad[1], bad[2] = R + 1, -1
    ref = _t(rows, dev)
    for b in (1, 2):
        one = n.copy()
        one[b] = bad[b]
        with pytest.raises(_lib.NfstError) as e:
            ops.lattice_edit_distance(lat, ref, _t(one, dev), theta, pad=PAD)
        assert e.value.code == _lib.ERR_LENGTH
    r, status = _raw(lat, ref, _t(bad, dev), theta, int(lat.depth.max()) + 1)
    assert status == _lib.ERR_LENGTH
    want = LR.of_batch(lats, refs, theta_np)
    for b in (1, 2):
        want[b] = {"distance": -1, "score": np.float32(-np.inf), "arcs": [], "align": [], "counts": (0, 0, 0)}
    _check("bad lengths", lat, lats, r, want, ref, _t(n, dev), True)  # (the others hold the restatement's values)
    assert r.distance.tolist() == [want[0]["distance"], -1, -1, want[3]["distance"]]


def test_max_len_too_small_cuts_the_path(dev):
    lats = E.mixed_batch()[:4]
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta_np = synth.label_scores(5, V)
    theta = _t(theta_np, dev)
    refs = [_stretched(_path_labels(l, theta_np), 8) for l in lats]
    rows, n = _ref_rows(refs)
    ref, ref_len = _t(rows, dev), _t(n, dev)
    with pytest.raises(_lib.NfstError) as e:
        ops.lattice_edit_distance(lat, ref, ref_len, theta, max_len=3, pad=PAD)
    assert e.value.code == _lib.ERR_LENGTH
    r, status = _raw(lat, ref, ref_len, theta, 3)
    assert status == _lib.ERR_LENGTH
    want = LR.of_batch(lats, refs, theta_np)
    assert max(len(w["arcs"]) for w in want) > 3
    arcs, lens = r.path_arcs.cpu().numpy(), r.lengths.cpu().numpy()
    for b, w in enumerate(want):
        m = min(3, len(w["arcs"]))
        assert lens[b] == m and np.array_equal(arcs[b, :m] - int(lat.arc_off[b]), w["arcs"][:m])
        assert int(r.distance[b]) == w["distance"] and tuple(r.counts[b].tolist()) == tuple(w["counts"])


# ----------------------------------------------------------------------------- 8: repeatability, gradient
def test_repeated_launches_and_gradient(dev):
    lats = E.mixed_batch()[:5]
    lat = LatticeBatch.from_synth(lats, device=dev)
    rng = np.random.default_rng(4)
    refs = [_stretched(_path_labels(l), 6 + 5 * b) for b, l in enumerate(lats)]
    rows, n = _ref_rows(refs)
    ref, ref_len = _t(rows, dev), _t(n, dev)
    labels = lat.arc_label.cpu().numpy()
    for per_lattice in (False, True):
        th_np = np.stack([synth.label_scores(30 + b, V) for b in range(len(lats))]) if per_lattice else synth.label_scores(30, V)
        theta = _t(th_np, dev).requires_grad_()
        asc = _t(rng.normal(0, 0.2, size=lat.total_arcs).astype(np.float32), dev).requires_grad_()
        r1 = ops.lattice_edit_distance(lat, ref, ref_len, theta, asc, pad=PAD)
        r2 = ops.lattice_edit_distance(lat, ref, ref_len, theta, asc, pad=PAD)
        for x, y in zip(r1, r2):
            assert torch.equal(x.detach(), y.detach())
        r1.score.sum().backward()
        arcs, lens = r1.path_arcs.cpu().numpy(), r1.lengths.cpu().numpy()
        ref_arc, ref_th = np.zeros(lat.total_arcs, np.float32), np.zeros((len(lats), V), np.float32)
        for b in range(len(lats)):
            p = arcs[b, :lens[b]]
            np.add.at(ref_arc, p, 1.0)
            np.add.at(ref_th[b], labels[p], 1.0)
        assert np.array_equal(asc.grad.cpu().numpy(), ref_arc)  # (counts: exact small integers)
        assert np.array_equal(theta.grad.cpu().numpy(), ref_th if per_lattice else ref_th.sum(axis=0))


# ----------------------------------------------------------------------------- 9: the scorer's entry points
def test_lattice_scorer_oracle(dev):
    lats = E.mixed_batch()[:4] + [E.mixed_batch()[5]]
    em, tr = synth.collate_dense([l.dense() for l in lats])
    theta_np = synth.label_scores(6, V)
    sc = LatticeScorer(V, pad=PAD, bos=BOS, eos=EOS, theta=torch.from_numpy(theta_np)).to(dev)
    sc.set_masks(torch.as_tensor(em).to(dev), torch.as_tensor(tr).to(dev))
    refs = [_stretched(_path_labels(l, theta_np), (7, 20, 33, 10, 1)[b]) for b, l in enumerate(lats)]
    rows, n = _ref_rows(refs, tail=PAD)
    ref, ref_len = _t(rows, dev), _t(n, dev)
    r = ops.lattice_edit_distance(sc._lat(), ref, ref_len, _t(theta_np, dev), pad=PAD)
    want = [(int(r.distance[b]), r.paths[b, :int(r.lengths[b])].tolist()) for b in range(len(lats))]
    assert sc.oracle(ref, ref_len) == want
    assert sc.oracle(ref) == want  # (trailing pads do not count)
    assert [w[0] for w in want] == [w["distance"] for w in LR.of_batch(lats, refs, theta_np)]
    rate = sc.oracle_error_rate(ref)
    assert rate == sc.oracle_error_rate(ref, ref_len) == sum(w[0] for w in want) / int(n.sum())
    assert rate > 0.0

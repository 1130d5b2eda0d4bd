"""ops.positional_k_best (nfst_positional_kbest: the k best paths under position-dependent scores and a length budget)
against the NumPy restatement of tests/positional_kbest_ref.py, which tests/test_positional_kbest_cpu.py proves against
path enumeration.  Every output is held to the restatement bit for bit.

The restatement runs once per case at k = 64; the kernel is held to its first k entries for k in {1, 2, 7, 20, 64} (the top
k' of a list is the first k' of its top k: tests/test_positional_kbest_cpu.py asserts it on the restatement).  The op
has one launch flavour, so "every launch branch" is one small and one large lattice (states of up to 123 out-arcs: two
merge chunks; the star of the tie cases takes four)."""
import dataclasses

import numpy as np
import pytest
import torch

from nfst_amd import ops, synth
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from tests import edge_cases as E
from tests import positional_kbest_ref as PK
from tests import positional_ref as R
from tests.test_positional_cpu import N_PATHS, small_lattices, truncations
from tests.test_positional_kbest_cpu import TIE_CASES, tie_reference, tie_truncations

pytestmark = pytest.mark.gpu
PAD = synth.PAD
NEG = -np.inf
F32 = np.float32
KS = (1, 2, 7, 20, 64)
EPS = 2.0 ** -24

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def small6():
    def make():
        V = max(l.vocab for l in small_lattices())
        return [dataclasses.replace(l, vocab=V) for l in small_lattices()]
    return list(cached("small6", make))


def _inputs(lats, seed, T, shared_pos=False, shared_theta=True):
    rng = np.random.default_rng(seed)
    B, V = len(lats), lats[0].vocab
    theta = rng.normal(-1.0, 0.8, size=(V,) if shared_theta else (B, V)).astype(F32)
    pos = rng.normal(0.0, 1.0, size=(T, V) if shared_pos else (B, T, V)).astype(F32)
    pos[..., PAD] = np.nan  # the pad column enters no output
    return theta, pos


def _per(x, b, shared_ndim):
    return None if x is None else (x if x.ndim == shared_ndim else x[b])


def reference(lats, theta, pos, T, asc=None, k=64):
    return [PK.k_best(l, _per(theta, b, 1), _per(pos, b, 2), T, k, None if asc is None else asc[sl])
            for b, (l, sl) in enumerate(zip(lats, E.arc_slices(lats)))]


def run(lat, theta, pos, T, k, dev, asc=None):
    t = lambda x: None if x is None else torch.from_numpy(x).to(dev)
    return ops.positional_k_best_terms(lat, t(theta), k, t(pos), T=T, arc_scores=t(asc), pad=PAD)


def check(tag, lat, lats, r, refs, T, k):
    """Every output against the first k entries of the restatement's lists."""
    best, paths, arcs, lens, n_paths = (x.cpu().numpy() for x in r)
    B = len(lats)
    assert best.shape == (B, k) and paths.shape == (B, k, T) and arcs.shape == (B, k, T) and lens.shape == (B, k) and n_paths.shape == (B,)
    for b, ref in enumerate(refs):
        a0 = int(lat.arc_off[b])
        n = min(k, ref["n_paths"])
        assert n_paths[b] == n, (tag, b, n_paths[b], n)
        want = np.full(k, NEG, F32)
        want[:n] = ref["best"][:n]
        assert np.array_equal(best[b].view(np.int32), want.view(np.int32)), (tag, b, best[b], want)
        for j in range(k):
            L = len(ref["arcs"][j]) if j < n else 0
            assert lens[b, j] == L, (tag, b, j)
            if j < n:
                assert np.array_equal(arcs[b, j, :L] - a0, ref["arcs"][j]) and np.array_equal(paths[b, j, :L], ref["labels"][j]), (tag, b, j)
            assert np.all(paths[b, j, L:] == PAD) and np.all(arcs[b, j, L:] == -1), (tag, b, j)


def run_and_check(tag, lat, lats, theta, pos, T, dev, asc=None, refs=None, ks=KS):
    refs = reference(lats, theta, pos, T, asc) if refs is None else refs
    for k in ks:
        check(f"{tag}.k{k}", lat, lats, run(lat, theta, pos, T, k, dev, asc), refs, T, k)
    return refs


def out_bits(lat, lats, r):
    """Per lattice, every output as raw bytes (arcs relative to the lattice)."""
    best, paths, arcs, lens, n_paths = (x.cpu().numpy() for x in r)
    out = []
    for b in range(len(lats)):
        rel = np.where(arcs[b] >= 0, arcs[b] - int(lat.arc_off[b]), -1).astype(np.int32)
        per = dict(best=best[b], paths=paths[b], arcs=rel, lengths=lens[b], n_paths=n_paths[b:b + 1])
        out.append({key: np.ascontiguousarray(x).view(np.uint8).copy() for key, x in per.items()})
    return out


def same_bits(x, y, where):
    assert x.keys() == y.keys(), where
    for key in x:
        assert np.array_equal(x[key], y[key]), (where, key)


def _all_T(lats):
    return sorted({T for l in lats for _, T in truncations(l)})


# ----------------------------------------------------------------------------- six small lattices, every truncation
@pytest.mark.parametrize("shared_theta", [True, False])
@pytest.mark.parametrize("shared_pos", [False, True])
def test_small_batch_at_every_truncation(dev, shared_pos, shared_theta):
    lats = small6()
    lat = LatticeBatch.from_synth(lats, device=dev)
    seen = set()
    for T in _all_T(lats):
        theta, pos = _inputs(lats, 2000 + T, T, shared_pos=shared_pos, shared_theta=shared_theta)
        refs = run_and_check(f"small.{int(shared_pos)}{int(shared_theta)}.T{T}", lat, lats, theta, pos, T, dev)
        seen |= {("none" if x["n_paths"] == 0 else "fewer" if x["n_paths"] < 64 else "full") for x in refs}
        if any(x["n_paths"] == 0 for x in refs):
            seen.add("dead beside live" if any(x["n_paths"] for x in refs) else "all dead")
    assert {"none", "fewer", "full", "dead beside live"} <= seen


def test_without_positions(dev):
    lats = small6()
    lat = LatticeBatch.from_synth(lats, device=dev)
    for T in (5, 9, int(lat.depth.max())):
        theta, _ = _inputs(lats, 2100 + T, T, shared_theta=False)
        run_and_check(f"nopos.T{T}", lat, lats, theta, None, T, dev)
    r = ops.positional_k_best_terms(lat, torch.from_numpy(theta).to(dev), 7)  # T defaults to the longest path
    assert r.paths.shape[-1] == int(lat.depth.max())


# ----------------------------------------------------------------------------- per-arc extras
def _weighted_case():
    lats = E.weighted_batch()
    T = max(R.min_max_len(l)[1] for l in lats)
    theta, pos = _inputs(lats, 2200, T)
    asc = np.random.default_rng(2201).normal(0.0, 0.3, size=sum(l.n_arcs for l in lats)).astype(F32)
    return lats, theta, pos, asc, T, reference(lats, theta, pos, T, asc)


def test_weighted_lattices_with_arc_scores(dev):
    lats, theta, pos, asc, T, refs = cached("weighted", _weighted_case)
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert lat.weighted and all(x["n_paths"] == 64 for x in refs)
    run_and_check("weighted", lat, lats, theta, pos, T, dev, asc, refs)


def test_forced_scores_of_the_returned_paths(dev):
    """ops.positional_score_paths sums a path's terms in float64 and rounds once; best nests at most 3 L float32 adds,
    each rounded relative to a partial sum of magnitude <= M = the sum of the absolute values of the path's terms:
    |best - forced| <= 3 L 2^-24 M + 2^-24 |score|.  (Lattices without table weights: an arc's terms are theta, pos and
    arc_scores, three rounded adds per arc.)"""
    lats = E.weighted_lats(False)[:3]
    T = max(R.min_max_len(l)[1] for l in lats)
    theta, pos = _inputs(lats, 2250, T)
    asc = np.random.default_rng(2251).normal(0.0, 0.3, size=sum(l.n_arcs for l in lats)).astype(F32)
    lat = LatticeBatch.from_synth(lats, device=dev)
    k = 20
    r = run(lat, theta, pos, T, k, dev, asc)
    t = lambda x: torch.from_numpy(x).to(dev)
    forced, end, lens = ops.positional_score_paths(lat, t(theta), r.paths, t(pos), arc_scores=t(asc))
    assert torch.equal(lens, r.lengths)
    best, forced, arcs, n = r.best.cpu().numpy(), forced.cpu().numpy(), r.arcs.cpu().numpy(), r.lengths.cpu().numpy()
    for b, (l, sl) in enumerate(zip(lats, E.arc_slices(lats))):
        assert np.all(end.cpu().numpy()[b] == l.n_rows - 1) and int(r.n_paths[b]) == k
        for j in range(k):
            p = arcs[b, j, :n[b, j]] - sl.start
            score, M, _ = PK.path_terms64(l, theta, pos[b], p, asc[sl])
            L = len(p)
            assert abs(float(forced[b, j]) - score) <= EPS * abs(score), (b, j)
            assert abs(float(best[b, j]) - float(forced[b, j])) <= 3 * L * EPS * M + EPS * abs(score), (b, j, best[b, j], forced[b, j])


# ----------------------------------------------------------------------------- exact ties
@pytest.mark.parametrize("which", [0, 1], ids=["longest", "halfway"])
@pytest.mark.parametrize("name", TIE_CASES)
def test_exact_ties(dev, name, which):
    """Scores on the 0.25 grid: whole paths tie inside the top 64 (tests/test_positional_kbest_cpu.py: 41 to 61 equal
    neighbours per list), so (canonical arc, rank) decides the order.  The star's 200 out-arcs take four merge chunks."""
    lats, theta, asc, pos, _ = E.pos_tie_inputs(name)
    T = tie_truncations(lats)[which]
    refs = cached(("ties", name, T), lambda: tie_reference(name, T))
    lat = LatticeBatch.from_synth(lats, device=dev, **E.tie_cases()[name][3])
    run_and_check(f"ties.{name}.T{T}", lat, lats, theta, np.ascontiguousarray(pos[:, :T]), T, dev, asc, refs)


# ----------------------------------------------------------------------------- -inf entries, lattices without a path
def test_minus_infinity_entries_force_and_forbid_marks(dev):
    lats = small6()[:3]
    T = 6
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta, pos = _inputs(lats, 2300, T)
    # lattice 0: exactly one path left alive (forced marks); lattice 1: a position at which every label is -inf; lattice 2:
    # the best path's second mark is forbidden at its position
    keep = R.enumerate_paths(lats[0])[5]
    one = np.full((T, lat.vocab), NEG, F32)
    for t, a in enumerate(keep):
        one[t, lats[0].label[a]] = pos[0, t, lats[0].label[a]]
    pos[0] = one
    pos[1, 1, :] = NEG
    before = PK.k_best(lats[2], theta, pos[2], T, 64)
    pos[2, 1, before["labels"][0][1]] = NEG
    refs = run_and_check("neginf", lat, lats, theta, pos, T, dev)
    assert refs[0]["n_paths"] == 1 and refs[0]["arcs"][0] == keep and refs[1]["n_paths"] == 0
    assert 0 < refs[2]["n_paths"] < before["n_paths"] and all(p[1] != before["labels"][0][1] for p in refs[2]["labels"])
    # a label at -inf in theta
    theta2 = theta.copy()
    theta2[before["labels"][0][2]] = NEG
    run_and_check("neginf.theta", lat, lats, theta2, pos, T, dev)


@pytest.mark.parametrize("weighted", [False, True])
def test_lattices_without_a_path_beside_live_neighbours(dev, weighted):
    lats, theta = E.no_path_case(weighted)
    T = 40
    assert all(R.min_max_len(l)[0] <= T < R.min_max_len(lats[-1])[1] for l in lats)
    _, pos = _inputs(lats, 2400, T)
    lat = LatticeBatch.from_synth(lats, device=dev)
    refs = run_and_check(f"nopath.{int(weighted)}", lat, lats, theta, pos, T, dev, ks=(1, 7, 64))
    assert [x["n_paths"] > 0 for x in refs] == [True, False, True, False, True]


def test_none_fewer_and_all_paths(dev):
    l = E.pos_neighbour()
    lat = LatticeBatch.from_synth([l], device=dev)
    for T, n in ((3, 0), (4, 3), (6, 23)):
        theta, pos = _inputs([l], 2500 + T, T)
        refs = run_and_check(f"neighbour.T{T}", lat, [l], theta, pos, T, dev)
        assert refs[0]["n_paths"] == n


# ----------------------------------------------------------------------------- a large lattice beside a small one
def test_large_lattice_beside_a_small_one(dev):
    """`big` of tests/edge_cases.py (481 rows, states of up to 123 out-arcs, 41 path lengths) beside the 13-row neighbour
    at k = 7: the op's single launch flavour at both ends of its shapes."""
    def make():
        big = E.pos_large("big")
        lats = [big, E.pos_neighbour()]
        T = R.min_max_len(big)[1]
        theta, pos = _inputs(lats, 2600, T)
        return lats, theta, pos, T, reference(lats, theta, pos, T, k=7)
    lats, theta, pos, T, refs = cached("large", make)
    assert T == 62 and np.bincount(lats[0].src[lats[0].src != lats[0].dst]).max() > 64
    lat = LatticeBatch.from_synth(lats, device=dev)
    run_and_check("large", lat, lats, theta, pos, T, dev, refs=refs, ks=(7,))


# ----------------------------------------------------------------------------- repeatability, packings, chunked programs
def test_two_launches_and_another_batch_order_give_the_same_bits(dev):
    lats = small6()
    T = 9
    theta, pos = _inputs(lats, 2700, T)
    lat = LatticeBatch.from_synth(lats, device=dev)
    a = out_bits(lat, lats, run(lat, theta, pos, T, 20, dev))
    for x, y in zip(a, out_bits(lat, lats, run(lat, theta, pos, T, 20, dev))):
        same_bits(x, y, "again")
    order = [4, 2, 5, 0, 3, 1]
    other = [lats[i] for i in order]
    lat_p = LatticeBatch.from_synth(other, device=dev)
    p = out_bits(lat_p, other, run(lat_p, theta, np.ascontiguousarray(pos[order]), T, 20, dev))
    for j, i in enumerate(order):
        same_bits(a[i], p[j], (i, j))


def test_every_packing_gives_the_same_bits(dev):
    lats = E.packing_lattices()
    T = max(R.min_max_len(l)[1] for l in lats)
    theta, pos = _inputs(lats, 2800, T)
    refs = reference(lats, theta, pos, T, k=7)
    first = None
    rows = set()
    for opts in (E.STAR_PACKINGS[0], E.STAR_PACKINGS[3], E.STAR_PACKINGS[9]):
        lat = LatticeBatch.from_synth(lats, device=dev, **opts)
        rows.add(int(lat.max_rows))
        r = run(lat, theta, pos, T, 7, dev)
        check(f"packing.{opts}", lat, lats, r, refs, T, 7)
        mine = out_bits(lat, lats, r)
        first = first or mine
        for b in range(len(lats)):
            same_bits(first[b], mine[b], (opts, b))
    assert len(rows) >= 2


def test_with_and_without_chunked_programs(dev):
    lats = synth.snips_shaped_batch(2, vocab=250)
    T = max(R.min_max_len(l)[1] for l in lats)
    assert T == 337 and R.min_max_len(lats[0])[1] < T
    theta, pos = _inputs(lats, 2900, T)
    plain = LatticeBatch.from_synth(lats).to(dev, auto_chunks=False)
    host = LatticeBatch.from_synth(lats)
    assert host.build_chunks(force=True)
    chunked = host.to(dev)
    assert chunked.chunks is not None and plain.chunks is None
    r1, r2 = run(plain, theta, pos, T, 7, dev), run(chunked, theta, pos, T, 7, dev)
    for b, (x, y) in enumerate(zip(out_bits(plain, lats, r1), out_bits(chunked, lats, r2))):
        same_bits(x, y, b)
    assert int(r1.n_paths.min()) >= 1
    t = lambda x: torch.from_numpy(x).to(dev)
    v = ops.positional_viterbi(plain, t(theta), t(pos), T=T, pad=PAD)
    assert torch.equal(r1.best[:, 0].view(torch.int32), v.best.view(torch.int32)) and torch.equal(r1.arcs[:, 0], v.path_arcs)


# ----------------------------------------------------------------------------- the three consequences, on the GPU
def test_entry_zero_is_positional_viterbi(dev):
    lats = small6() + [E.pos_neighbour(vocab=small6()[0].vocab)]
    lat = LatticeBatch.from_synth(lats, device=dev)
    for T in (5, 9, 13):
        theta, pos = _inputs(lats, 3000 + T, T)
        t = lambda x: torch.from_numpy(x).to(dev)
        v = ops.positional_viterbi(lat, t(theta), t(pos), T=T, pad=PAD)
        for k in (1, 20):
            r = run(lat, theta, pos, T, k, dev)
            assert torch.equal(r.best[:, 0].view(torch.int32), v.best.view(torch.int32))
            assert torch.equal(r.paths[:, 0], v.paths) and torch.equal(r.arcs[:, 0], v.path_arcs) and torch.equal(r.lengths[:, 0], v.lengths)


@pytest.mark.parametrize("which", ["small", "mixed"])
def test_without_positions_and_full_length_it_is_k_best(dev, which):
    lats = small6() if which == "small" else E.mixed_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = torch.from_numpy(synth.label_scores(5, lat.vocab)).to(dev)
    for extra in (0, 3):
        T = int(lat.depth.max()) + extra
        for k in KS:
            r = ops.positional_k_best_terms(lat, theta, k, None, T=T, pad=PAD)
            kb = ops.k_best_terms(lat, theta, k, max_len=T, pad=PAD)
            for x, y in zip(r, kb):
                assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), (extra, k)


def test_below_the_depth_it_is_k_best_without_the_longer_paths(dev):
    """The four small lattices with fewer than 64 paths: neither list is truncated at k = 64."""
    idx = [i for i, n in enumerate(N_PATHS) if n < 64]
    lats = [small6()[i] for i in idx]
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = torch.from_numpy(synth.label_scores(6, lat.vocab)).to(dev)
    depth = int(lat.depth.max())
    kb = [x.cpu().numpy() for x in ops.k_best_terms(lat, theta, 64, max_len=depth, pad=PAD)]
    cut = 0
    for T in range(3, depth):
        r = [x.cpu().numpy() for x in ops.positional_k_best_terms(lat, theta, 64, None, T=T, pad=PAD)]
        for b in range(len(lats)):
            keep = [j for j in range(kb[4][b]) if kb[3][b, j] <= T]
            n = len(keep)
            cut += n < kb[4][b]
            assert r[4][b] == n and np.array_equal(r[3][b, :n], kb[3][b, keep])
            assert np.array_equal(r[0][b, :n].view(np.int32), kb[0][b, keep].view(np.int32))
            assert np.array_equal(r[1][b, :n], kb[1][b, keep][:, :T]) and np.array_equal(r[2][b, :n], kb[2][b, keep][:, :T])
            assert np.all(r[0][b, n:] == NEG) and np.all(r[3][b, n:] == 0)
    assert cut >= 4


# ----------------------------------------------------------------------------- the reranker's list
def test_nbest_probabilities_sum_to_one_when_every_path_is_listed(dev):
    l = E.pos_neighbour()
    lat = LatticeBatch.from_synth([l], device=dev)
    T = 6
    theta, pos = _inputs([l], 3100, T)
    pos[..., PAD] = 0.0
    sc = LatticeScorer(lat.vocab, theta=theta).to(dev).set_lattice(lat)
    pos_t = torch.from_numpy(pos).to(dev)
    (nbest,) = sc.positional_nbest(pos_t, 64)
    assert len(nbest) == 23
    logz = float(ops.positional_forward_backward(lat, torch.from_numpy(theta).to(dev), pos_t, want_pos_posterior=False).logz64[0])
    tol = 1e-5 * max(1.0, abs(logz))
    logp = np.array([x[0] for x in nbest])
    assert np.all(logp <= tol) and np.all(np.diff(logp) <= 0)
    assert abs(R.logsumexp(logp)) <= tol
    ref = PK.k_best(l, theta, pos[0], T, 64)
    assert [x[1] for x in nbest] == ref["labels"]
    r = sc.positional_k_best(pos_t, 5)
    assert torch.equal(r.best.detach(), ops.positional_k_best_terms(lat, sc.theta.detach(), 5, pos_t, pad=PAD).best) and r.best.requires_grad


# ----------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("shared", [True, False])
def test_gradients_count_labels_arcs_and_positions(dev, shared):
    """d (sum_j g_j best_j): theta counts a path's labels, arc_scores marks its arcs, pos_scores marks (t, label) of its
    positions, each weighted by g_j and summed over the lattices for a shared tensor.  An entry sums n float32 terms:
    it is held to n 2^-24 sum |g| over those terms.  Entries beyond n_paths (-inf) contribute nothing, whatever their g."""
    lats = small6()
    T, k = 9, 64
    lat = LatticeBatch.from_synth(lats, device=dev)
    B, V = len(lats), lat.vocab
    theta_np, pos_np = _inputs(lats, 3200, T, shared_pos=shared, shared_theta=shared)
    pos_np[..., PAD] = 0.0
    asc_np = np.random.default_rng(3201).normal(0.0, 0.3, size=lat.total_arcs).astype(F32)
    g_np = np.random.default_rng(3202).normal(0.0, 1.0, size=(B, k)).astype(F32)
    theta, pos, asc = (torch.from_numpy(x).to(dev).requires_grad_(True) for x in (theta_np, pos_np, asc_np))
    r = ops.positional_k_best(lat, theta, k, pos, arc_scores=asc, pad=PAD)
    refs = reference(lats, theta_np, pos_np, T, asc_np)
    check("grad.forward", lat, lats, ops.PositionalKBestResult(*(x.detach() for x in r)), refs, T, k)
    assert any(x["n_paths"] < k for x in refs) and not r.paths.requires_grad
    r.best.backward(torch.from_numpy(g_np).to(dev))
    want = {"theta": np.zeros((B, V)), "pos": np.zeros((B, T, V)), "arc": np.zeros(lat.total_arcs)}
    mag = {key: np.zeros_like(x) for key, x in want.items()}
    cnt = {key: np.zeros_like(x) for key, x in want.items()}
    for b, (l, ref, sl) in enumerate(zip(lats, refs, E.arc_slices(lats))):
        for j, p in enumerate(ref["arcs"]):
            g = float(g_np[b, j])
            for t, a in enumerate(p):
                for key, at in (("theta", (b, l.label[a])), ("pos", (b, t, l.label[a])), ("arc", (sl.start + a,))):
                    want[key][at] += g
                    mag[key][at] += abs(g)
                    cnt[key][at] += 1
    if shared:
        for d in (want, mag, cnt):
            d["theta"], d["pos"] = d["theta"].sum(axis=0), d["pos"].sum(axis=0)
    for key, got in (("theta", theta.grad), ("pos", pos.grad), ("arc", asc.grad)):
        got = got.cpu().numpy()
        assert got.shape == want[key].shape and np.isfinite(got).all(), key
        assert np.all(np.abs(got - want[key]) <= cnt[key] * EPS * mag[key]), key
        assert np.all(got[cnt[key] == 0] == 0.0), key
    with pytest.raises(RuntimeError):  # once_differentiable, as ops.k_best
        theta2 = torch.from_numpy(theta_np).to(dev).requires_grad_(True)
        b2 = ops.positional_k_best(lat, theta2, 2, pos.detach(), pad=PAD).best
        (g2,) = torch.autograd.grad(b2[torch.isfinite(b2)].sum(), theta2, create_graph=True)
        g2.sum().backward()


# ----------------------------------------------------------------------------- wrappers
def test_wrapper_errors_raise(dev):
    lats = small6()[:3]
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = torch.zeros(lat.vocab, device=dev)
    good = torch.zeros(3, 6, lat.vocab, device=dev)
    for fn in (ops.positional_k_best, ops.positional_k_best_terms):
        for k in (0, 65, -1, True, 2.0):
            with pytest.raises(ValueError):
                fn(lat, theta, k, good)
        with pytest.raises(ValueError):
            fn(lat, theta, 5, good, T=5)
        with pytest.raises(ValueError):
            fn(lat, theta, 5, None, T=0)
        for bad in (torch.zeros(3, 6, lat.vocab + 1, device=dev), torch.zeros(2, 6, lat.vocab, device=dev), good.cpu()):
            with pytest.raises(ValueError):
                fn(lat, theta, 5, bad)
    assert ops.positional_k_best_terms(lat, theta, 5, good, T=6).best.shape == (3, 5)

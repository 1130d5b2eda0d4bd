"""The path-side kernels (nfst_amd/csrc/path_kernels.h) against exact references at every launch branch (``-m gpu``):

* Viterbi, both flavours (``tuning(tw=1)`` / ``tw=0``), bit for bit against ``paths_ref.viterbi_ref`` in the add order
  each flavour documents: best, labels, arcs, lengths and the pad / -1 tails;
* the posterior sampler against ``oracle.sample_paths`` (walks whose uniforms stay clear of a CDF boundary exactly);
* ``score_paths`` against ``oracle.score_paths``;
* the walker kernels (step, emission mask, beta-logit gather: bit-exact; the fused proposal step and its backward);
* IWAE and the launchers' size limits.

Tolerances: indices, paths, arcs, lengths, states, masks and Viterbi's best are exact.  log q / log z of a proposal step
are held to max(2e-5, 4 E32(V)), E32 the error of the float32 restatement of tests/paths_ref.py against the float64
oracle on the same inputs (never the kernel's): the factor 4 covers __expf / logf and another summation order.  E32 and
the GPU's worst errors go to path_errors.json beside parity_errors.json of test_gpu_parity.py.  The caps on the share of walks left out of the exact
comparison are proved on the oracle alone in tests/test_paths_ref_cpu.py.
"""
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest
import torch

from nfst_amd import _lib, ops, synth
from nfst_amd.lattice import LatticeBatch
from nfst_amd.ops import BackwardResult, _ptr, _stream
from oracle import oracle as O
from tests import edge_cases as E
from tests import paths_ref as P
from tests.test_gpu_fuzz import _draw_batch

pytestmark = pytest.mark.gpu
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
F32 = np.float32
TOL = 2e-5  # the project's bound on log q / log z against the float64 oracle
ERR_LIMIT = -6

_ERR = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    # the directory of run outputs at the repository's root that test_gpu_parity.py and test_gpu_fuzz.py write their
    # largest errors to (a run that wants the figures creates it; nothing is written without it)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for out in sorted(glob.glob(os.path.join(root, "*_out"))):
        if _ERR and os.path.isdir(out):
            with open(os.path.join(out, "path_errors.json"), "w") as f:
                json.dump(dict(sorted(_ERR.items())), f, indent=1)


def rec(tag, err):
    _ERR[tag] = max(_ERR.get(tag, 0.0), float(err))
    return float(err)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ============================================================================= Viterbi
def _theta_of(theta, b):
    return theta[b] if theta.ndim == 2 else theta


def _viterbi_miss(lat, lats, got, refs):
    """None when every output of the batch is the reference's, bit for bit; else the first difference."""
    best, paths, arcs, lens = got
    for b, (l, r) in enumerate(zip(lats, refs)):
        a0, n = int(lat.arc_off[b]), r["length"]
        if best[b:b + 1].view(np.int32)[0] != r["best"].view(np.int32):
            return (b, "best", float(best[b]), float(r["best"]))
        if lens[b] != n:
            return (b, "length", int(lens[b]), n)
        if not np.array_equal(arcs[b, :n] - a0, r["arcs"]):
            return (b, "arcs")
        if not np.array_equal(paths[b, :n], r["labels"]):
            return (b, "labels")
        if not (np.all(paths[b, n:] == PAD) and np.all(arcs[b, n:] == -1)):
            return (b, "tail")
    return None


def _viterbi_case(tag, dev, lats, theta_np, asc_np=None, tw_order=None, guard_every=1, **opts):
    """Both flavours of one batch against the reference.  ``tw=0`` runs the general kernel: the "general" order.
    ``tw=1`` runs the tile-wave kernel on all-compact batches whose records leave it eight ring slots, else the general
    one; no public call tells which ran, so the batch must be one of the two references as a whole (``tw_order``: the
    one it must be, where the batch is known to be all-compact and small).  Returns the references of the general
    order."""
    lat = LatticeBatch.from_synth(lats, device=dev, **opts)
    theta, asc = _t(theta_np, dev), _t(asc_np, dev)
    refs = {}
    for order in ("general", "tile_waves"):
        refs[order] = []
        for b, l in enumerate(lats):
            a0 = int(lat.arc_off[b])
            refs[order].append(P.viterbi_ref(l, _theta_of(theta_np, b), l.weight, None if asc_np is None else asc_np[a0:a0 + l.n_arcs], order))
    for tw in (1, 0):
        with _lib.tuning(tw=tw):
            r = ops.viterbi(lat, theta, arc_scores=asc, pad=PAD)
            got = tuple(x.cpu().numpy() for x in (r.best, r.paths, r.arcs, r.lengths))
        orders = ("general",) if tw == 0 else ((tw_order,) if tw_order else ("tile_waves", "general"))
        miss = {o: _viterbi_miss(lat, lats, got, refs[o]) for o in orders}
        assert any(m is None for m in miss.values()), (tag, tw, miss)
        # independent of any add order: the returned path against the float64 optimum
        for b in range(0, len(lats), guard_every):
            l, a0, n = lats[b], int(lat.arc_off[b]), int(got[3][b])
            sc = P.score64(l, _theta_of(theta_np, b), l.weight, None if asc_np is None else asc_np[a0:a0 + l.n_arcs])
            if n > 0:
                gap, bound = P.path_guard(l, sc, got[2][b, :n] - a0)
                assert -bound <= gap <= bound, (tag, tw, b, gap, bound)
                rec("viterbi_gap_over_bound", gap / bound if bound > 0 else 0.0)
    return refs["general"]


_weighted_lats = E.weighted_lats  # (one definition: tests/edge_cases.py)


def _asc(lats, seed, std=0.3):
    return np.random.default_rng(seed).normal(0.0, std, size=sum(l.n_arcs for l in lats)).astype(F32)


@pytest.mark.parametrize("per_lattice", [False, True])
@pytest.mark.parametrize("extras", ["none", "weights", "arc_scores", "both"])
def test_viterbi_per_arc_extras(dev, extras, per_lattice):
    """No extras, one array of extras (table weights, or caller scores on unweighted tables) and both: the three
    instantiations of k_viterbi_tw and the general kernel's sums, with shared and per-lattice label scores."""
    lats = _weighted_lats(extras in ("weights", "both"))
    rng = np.random.default_rng(0)
    theta = rng.normal(-2.0, 0.7, size=(len(lats), 48) if per_lattice else 48).astype(F32)
    asc = _asc(lats, 1) if extras in ("arc_scores", "both") else None
    _viterbi_case(f"extras {extras}", dev, lats, theta, asc, tw_order="tile_waves")


@pytest.mark.parametrize("opts", [dict(group_mode=1), dict(group_mode=2), dict(slots_per_lane=1), dict(slots_per_lane=2),
                                  dict(slots_per_lane=4), dict(group_mode=1, slots_per_lane=1), dict(group_mode=2, slots_per_lane=2),
                                  dict(no_compact=True), dict(group_mode=1, slots_per_lane=4, no_compact=True)])
def test_viterbi_with_extras_under_every_packing(dev, opts):
    lats = _weighted_lats(True)
    theta = np.random.default_rng(2).normal(-2.0, 0.7, size=48).astype(F32)
    _viterbi_case(f"packing {opts}", dev, lats, theta, _asc(lats, 3), **opts)


def _star(weighted_seed):  # a state with 200 out-arcs (test_gpu_parity.py), here with table weights
    src = [0] + [1] * 200 + list(range(2, 202)) + [202]
    lab = [BOS] + list(range(3, 203)) + [5] * 200 + [EOS]
    dst = [1] + list(range(2, 202)) + [202] * 200 + [203]
    w = np.random.default_rng(weighted_seed).normal(-0.5, 0.8, size=len(src)).astype(F32)
    return synth._finish(204, 256, src, lab, dst, w)


@pytest.mark.parametrize("opts", [dict(), dict(group_mode=1), dict(group_mode=2), dict(group_mode=1, slots_per_lane=1),
                                  dict(group_mode=2, slots_per_lane=1), dict(group_mode=1, slots_per_lane=4, no_compact=True)])
def test_viterbi_star_with_extras(dev, opts):
    """200 out-arcs of one state with table weights and caller scores: the best arc is handed through unit-label
    records (combine pieces of narrow groups, continuation pieces of wide groups) while the real arcs carry extras."""
    for seed in range(3):  # (the best arc falls into different pieces)
        star = _star(seed)
        theta = synth.label_scores(4 + seed, 256)
        _viterbi_case(f"star {opts}", dev, [star], theta, _asc([star], 10 + seed, std=1.0), **opts)


def test_viterbi_deep_chain(dev):
    lats = [synth.layered_lattice(900 + i, n_states=n, avg_degree=2.5, vocab=40, width=1, span=1 + i, max_degree=6, weighted=True)
            for i, n in enumerate((1000, 1450))]
    lat = LatticeBatch.from_synth(lats)
    assert 900 <= int(lat.depth.min()) and int(lat.depth.max()) <= 1500
    _viterbi_case("deep chain", dev, lats, synth.label_scores(5, 40, mean=-1.0, std=1.0), _asc(lats, 4))


@pytest.mark.parametrize("n_states", [7800, 8150])
def test_viterbi_large_lattice(dev, n_states):
    """7800 states leave the tile-wave kernel its smallest ring (eight slots beside 16 bytes per row); 8150 leave fewer
    and the launcher falls back to the general kernel.  No public call tells which kernel ran: the bits are held to the
    references under both tunings."""
    big, small = E.large_pair(n_states)
    lat = LatticeBatch.from_synth([big, small])
    assert (lat.max_rows * 16 + 1024 > 160 * 1024 - 8 * 4096) == (n_states == 8150)
    _viterbi_case(f"large {n_states}", dev, [big, small], synth.label_scores(6, 64), _asc([big, small], 5))


def test_viterbi_more_lattices_than_compute_units(dev):
    lats, theta, asc = E.many_small()
    _viterbi_case("330 lattices", dev, lats, theta, asc, tw_order="tile_waves", guard_every=7)


@pytest.mark.parametrize("extras", [False, True])
def test_viterbi_exact_ties(dev, extras):
    """Scores on a grid of 0.25: every float32 sum is exact, whole paths tie, and the smaller canonical arc must win at
    every tied state -- in both flavours, whose sums coincide here."""
    lats = _weighted_lats(extras) + [synth.edit_lattice([10, 11, 12, 13, 14], [20, 21, 22, 23], vocab=48, seed=2)]
    if extras:
        for l in lats[:-1]:
            l.weight = (np.round(l.weight * 4) / 4).astype(F32)
        lats[-1].weight = np.zeros(lats[-1].n_arcs, F32)
    q = lambda x: (np.round(x * 4) / 4).astype(F32)
    theta = q(np.random.default_rng(8).normal(-2.0, 0.7, size=48))
    asc = q(_asc(lats, 9, std=0.5)) if extras else None
    refs = _viterbi_case("ties", dev, lats, theta, asc)
    assert sum(r["ties"] for r in refs) >= 3
    a0 = 0
    for l, r in zip(lats, refs):  # (exact sums: the float32 optimum is the float64 optimum)
        sc = P.score64(l, theta, l.weight, None if asc is None else asc[a0:a0 + l.n_arcs])
        assert float(r["best"]) == P.viterbi_f64(l, sc)["best"]
        a0 += l.n_arcs


@pytest.mark.parametrize("extras", [False, True])
def test_viterbi_labels_at_minus_infinity(dev, extras):
    lats = _weighted_lats(extras)
    theta = np.random.default_rng(10).normal(-2.0, 0.7, size=48).astype(F32)
    dead = E.DEAD
    theta[dead] = -np.inf
    refs = _viterbi_case("dead labels", dev, lats, theta, _asc(lats, 11) if extras else None, tw_order="tile_waves")
    for l, r in zip(lats, refs):
        assert np.isfinite(r["best"]) and not np.isin(r["labels"], dead).any() and np.isin(l.label, dead).sum() > 20


@pytest.mark.parametrize("extras", [False, True])
def test_viterbi_without_a_finite_path(dev, extras):
    """The convention of include/nfst_hip.h: a lattice all of whose paths cross a label at -inf gets best = -inf,
    length 0, labels all pad and arcs all -1 (entry 0 of nfst_kbest), from both kernels; its neighbours in the batch
    are not disturbed."""
    lats, theta = E.no_path_case(extras)  # (eos at -inf for lattice 1, bos at -inf for lattice 3)
    asc = _asc(lats, 13) if extras else None
    refs = _viterbi_case("no finite path", dev, lats, theta, asc, tw_order="tile_waves")
    assert [bool(np.isneginf(r["best"])) for r in refs] == [False, True, False, True, False]
    assert refs[1]["length"] == 0 and refs[3]["length"] == 0
    lat = LatticeBatch.from_synth(lats, device=dev)
    for tw in (1, 0):
        with _lib.tuning(tw=tw):
            r = ops.viterbi(lat, _t(theta, dev), arc_scores=_t(asc, dev), pad=PAD)
            k = ops.k_best(lat, _t(theta, dev), 2, arc_scores=_t(asc, dev), pad=PAD)
        for b in (1, 3):
            assert float(r.best[b]) == -np.inf and int(r.lengths[b]) == 0
            assert bool((r.paths[b] == PAD).all()) and bool((r.arcs[b] == -1).all())
            assert int(k.n_paths[b]) == 0 and int(k.lengths[b, 0]) == 0 and float(k.best[b, 0]) == -np.inf


@pytest.mark.parametrize("seed", list(range(12)))
def test_viterbi_fuzz(dev, seed):
    """The shapes of test_gpu_fuzz._draw_batch (batch sizes, 4 .. 1500 states, widths, spans, degrees, vocabularies up to
    700, table weights), label scores shared or per lattice, caller scores on or off, every group mode."""
    rng = np.random.default_rng(5000 + seed)
    lats, V, weighted = _draw_batch(rng)
    gm = int(rng.choice([0, 0, 1, 2]))
    shape = (len(lats), V) if rng.integers(0, 2) else (V,)
    theta = rng.normal(float(rng.choice([-2.3, 0.0, -8.0])), float(rng.choice([0.5, 2.0])), size=shape).astype(F32)
    asc = _asc(lats, 6000 + seed, std=0.5) if rng.integers(0, 2) else None
    _viterbi_case(f"fuzz {seed}", dev, lats, theta, asc, guard_every=5, group_mode=gm)


def test_viterbi_general_kernel_beyond_lds_is_refused(dev):
    """4000 states over 30000 labels: 32-bit records (not all-compact), so the general kernel, which would need
    12 * 4001 + 4 * 30000 + 16 bytes of LDS > 160 KiB: NFST_ERR_LIMIT from the host, no launch.  (check_batch and the
    packer take this batch: max_rows <= 8192, vocab <= 32767.)"""
    l = synth.layered_lattice(78, n_states=4000, avg_degree=3.0, vocab=P.BIG_V, width=8, span=3)
    lat = LatticeBatch.from_synth([l], device=dev)
    assert lat.max_rows * 12 + P.BIG_V * 4 + 16 > 160 * 1024
    theta = _t(synth.label_scores(1, P.BIG_V), dev)
    for tw in (1, 0):
        with _lib.tuning(tw=tw):
            with pytest.raises(_lib.NfstError) as e:
                ops.viterbi(lat, theta, pad=PAD)
        assert e.value.code == ERR_LIMIT
    # a smaller lattice over the same vocabulary runs, and is the oracle's path
    s = synth.layered_lattice(79, n_states=300, avg_degree=3.0, vocab=P.BIG_V, width=8, span=3)
    _viterbi_case("big vocabulary", dev, [s], synth.label_scores(1, P.BIG_V), None)


# ============================================================================= posterior sampler
def _check_walks(tag, c, lat, s, refs, want_arcs):
    paths, lens, logq = s.paths.cpu().numpy(), s.lengths.cpu().numpy(), s.logq.cpu().numpy()
    arcs = s.arcs.cpu().numpy() if want_arcs else None
    for b, (l, (ref, logz, sc, _)) in enumerate(zip(c["lats"], refs)):
        a0 = int(lat.arc_off[b])
        safe = ref["margin"] > P.MARGIN
        assert safe.mean() > P.CAP
        assert np.array_equal(paths[b][safe], ref["paths"][safe]), (tag, b)
        assert np.array_equal(lens[b][safe], ref["lengths"][safe]), (tag, b)
        if want_arcs:
            assert np.array_equal((arcs[b] - np.where(arcs[b] >= 0, a0, 0))[safe], ref["arcs"][safe]), (tag, b)
            for k in range(paths.shape[1]):
                assert np.array_equal(paths[b, k, :lens[b, k]], l.label[arcs[b, k, :lens[b, k]] - a0]), (tag, b, k)
        # every walk, safe or not: an accepting path (the forced walk of its labels ends in the sink) with
        # log q = score - log Z
        tot, end = O.score_paths(l.n_rows, l.src, l.label, l.dst, sc, paths[b])
        assert np.all(end == l.n_rows - 1) and np.all(lens[b] > 0), (tag, b)
        assert np.all(paths[b][np.arange(paths.shape[2])[None, :] >= lens[b][:, None]] == PAD)
        assert rec(f"sampler_logq_{tag}", np.max(np.abs(tot - logz - logq[b]))) <= TOL, (tag, b)
        assert np.max(np.abs(logq[b][safe] - ref["logq"][safe])) <= TOL
        if c["dead"] is not None:
            assert not np.isin(paths[b], c["dead"]).any()


@pytest.mark.parametrize("name,want_arcs", [("big_vocab", True), ("big_vocab", False), ("big_vocab_big_lattice", True),
                                            ("big_vocab_big_lattice", False)])
def test_sampler_with_label_scores_in_global_memory(dev, name, want_arcs):
    """30000 labels: max_rows * 8 + vocab * 4 > 96 KiB, so k_sample reads the label scores from global memory
    (stage_theta = 0), in its three ways of reading a lattice: cumulative probabilities precomputed in LDS (arcs wanted),
    CSR staged in LDS (no arcs), and a 3000-state lattice whose CSR does not fit.  The sweeps keep the label weights in
    LDS and do not take such a vocabulary, so beta comes from the caller (``beta=``), here the oracle's in float64
    rounded to the engine's (mantissa, exponent) pairs."""
    c = P.sampler_case(name)
    u = P.sampler_uniforms(c, name)
    refs = P.sampler_refs(c, u)
    lat = LatticeBatch.from_synth(c["lats"], device=dev)
    assert lat.max_rows * 8 + lat.vocab * 4 > 96 * 1024
    me = torch.from_numpy(np.concatenate([P.beta_me(r[3]) for r in refs])).to(dev).view(torch.float32)
    z = np.array([r[1] for r in refs])
    beta = BackwardResult(None, _t(z.astype(F32), dev), _t(z, dev), me)
    s = ops.sample_paths(lat, _t(c["theta"], dev), c["K"], max_len=u.shape[2], uniforms=_t(u, dev), pad=PAD, beta=beta, want_arcs=want_arcs)
    _check_walks(name, c, lat, s, refs, want_arcs)


@pytest.mark.parametrize("K", [1, 5, 17, 100])
@pytest.mark.parametrize("want_arcs", [True, False])
def test_sampler_per_lattice_scores_and_walk_counts(dev, K, want_arcs):
    name = f"per_lattice_k{K}"
    c = P.sampler_case(name)
    u = P.sampler_uniforms(c, name)
    refs = P.sampler_refs(c, u)
    lat = LatticeBatch.from_synth(c["lats"], device=dev)
    s = ops.sample_paths(lat, _t(c["theta"], dev), K, arc_scores=_t(c["asc"], dev), max_len=u.shape[2], uniforms=_t(u, dev), pad=PAD,
                         want_arcs=want_arcs)
    _check_walks("per_lattice", c, lat, s, refs, want_arcs)


@pytest.mark.parametrize("want_arcs", [True, False])
def test_sampler_never_draws_a_label_at_minus_infinity(dev, want_arcs):
    c = P.sampler_case("dead_labels")
    u = P.sampler_uniforms(c, "dead_labels")
    refs = P.sampler_refs(c, u)
    lat = LatticeBatch.from_synth(c["lats"], device=dev)
    theta = _t(c["theta"], dev)
    s = ops.sample_paths(lat, theta, c["K"], max_len=u.shape[2], uniforms=_t(u, dev), pad=PAD, want_arcs=want_arcs)
    _check_walks("dead_labels", c, lat, s, refs, want_arcs)
    # ... nor with uniforms on the boundaries (0, and the largest float32 below 1), nor from the Philox stream
    for fill in (0.0, float(np.nextafter(F32(1), F32(0)))):
        e = ops.sample_paths(lat, theta, 16, max_len=u.shape[2], uniforms=torch.full((len(c["lats"]), 16, u.shape[2]), fill), pad=PAD,
                             want_arcs=want_arcs)
        assert not np.isin(e.paths.cpu().numpy(), c["dead"]).any() and int(e.lengths.min()) > 0
    p = ops.sample_paths(lat, theta, 512, seed=5, pad=PAD, want_arcs=want_arcs)
    assert not np.isin(p.paths.cpu().numpy(), c["dead"]).any() and bool(torch.isfinite(p.logq).all())


# ============================================================================= score_paths
def _score_paths_case(tag, dev, lats, theta, asc, marks):
    lat = LatticeBatch.from_synth(lats, device=dev)
    tot, end = ops.score_paths(lat, _t(theta, dev), _t(marks, dev), arc_scores=_t(asc, dev))
    tot, end = tot.cpu().numpy(), end.cpu().numpy()
    a0 = 0
    for b, l in enumerate(lats):
        a = None if asc is None else asc[a0:a0 + l.n_arcs]
        sc = P.score64(l, _theta_of(theta, b), l.weight, a)
        ref, ref_end = O.score_paths(l.n_rows, l.src, l.label, l.dst, sc, marks[b])
        assert np.array_equal(end[b], ref_end), (tag, b)
        off = np.isneginf(ref)
        assert np.all(np.isneginf(tot[b][off])) and np.all(ref_end[off] == 0)
        # the kernel adds an arc's float32 terms in float32 (at most two adds, each within 2^-24 of the sum of the terms'
        # magnitudes), sums the arcs in float64 and rounds the total once
        mag, _ = O.score_paths(l.n_rows, l.src, l.label, l.dst, P.score64(l, np.abs(_theta_of(theta, b)), None if l.weight is None else np.abs(l.weight),
                                                                          None if a is None else np.abs(a)), marks[b])
        bound = 2.0 ** -24 * np.abs(ref[~off]) + 2 * 2.0 ** -24 * mag[~off] + 1e-12
        err = np.abs(tot[b][~off].astype(np.float64) - ref[~off])
        assert np.all(err <= bound), (tag, b, float(err.max()))
        rec(f"score_paths_{tag}", err.max() if err.size else 0.0)
        a0 += l.n_arcs
    return tot, end


def test_score_paths_weighted_per_lattice_and_broken_marks(dev):
    """65 walks per lattice (a second block in y), table weights + caller scores + per-lattice label scores; marks out
    of range, marks off the lattice (-inf, end state 0) and pad after eos."""
    c = P.sampler_case("per_lattice_k17")
    K = 65
    c["K"] = K
    u = P.sampler_uniforms(c, "score_paths")
    marks = np.stack([r[0]["paths"] for r in P.sampler_refs(c, u)]).astype(np.int32)  # valid walks, pad after eos
    assert (marks[:, :, -1] == PAD).all() or (marks == PAD).any()
    V = c["lats"][0].vocab
    for b, l in enumerate(c["lats"]):
        marks[b, 3, 2] = V + 5          # beyond the vocabulary
        marks[b, 4, 1] = -1             # negative
        marks[b, 64, 0] = V             # ... in the second block
        free = np.setdiff1d(np.arange(3, V), l.label[l.src == 1])  # a label state 1 does not carry
        marks[b, 5, 1] = free[0]
        marks[b, 6, 0] = EOS            # no eos arc out of state 0
    tot, end = _score_paths_case("weighted_per_lattice", dev, c["lats"], c["theta"], c["asc"], marks)
    for b, l in enumerate(c["lats"]):
        assert np.all(np.isneginf(tot[b, [3, 4, 5, 6, 64]])) and np.all(end[b, [3, 4, 5, 6, 64]] == 0)
        keep = np.setdiff1d(np.arange(K), [3, 4, 5, 6, 64])
        assert np.all(np.isfinite(tot[b, keep])) and np.all(end[b, keep] == l.n_rows - 1)


def test_score_paths_big_vocabulary(dev):
    c = P.sampler_case("big_vocab")
    c["K"] = 5
    u = P.sampler_uniforms(c, "score_paths_big")
    marks = np.stack([r[0]["paths"] for r in P.sampler_refs(c, u)]).astype(np.int32)
    marks[0, 1, 1] = P.BIG_V - 1
    marks[1, 2, 0] = P.BIG_V
    _score_paths_case("big_vocab", dev, c["lats"], c["theta"], None, marks)


# ============================================================================= walker kernels: gathers
def _gather_states(lats, k, seed):
    """Walker states and labels with the edges in: the hub, the sink, random rows, rows out of range (beyond the
    lattice, negative) and labels out of range."""
    rng = np.random.default_rng(seed)
    _, inp, state = P.walker_positions(lats, k, seed)
    N = len(state)
    label = np.zeros(N, np.int64)
    for n in range(N):
        l = lats[n // k]
        out = l.label[l.src == state[n]]
        label[n] = rng.choice(out) if (n % 2 == 0 and out.size) else rng.integers(0, l.vocab)
    state[N - 1] = lats[-1].n_rows + 5
    if N > 3:
        state[4], label[5], label[6] = -1, lats[0].vocab, -3
    else:
        label[1] = lats[0].vocab
    return state, inp, label


def _in_range(l, s):
    return 0 <= s < l.n_rows


@pytest.mark.parametrize("k", P.WALKER_KS)
@pytest.mark.parametrize("V", P.WALKER_VOCABS)
def test_step_mask_and_value_gather_bit_exact(dev, V, k):
    """nfst_step, nfst_emission_mask (with and without the previous symbols, weighted and not, forced end) and
    nfst_beta_logits against the oracle on the dense tables; states and labels out of range give 0, an empty row and
    row 0's value like the dense gather."""
    for weighted in (False, True):
        lats = P.walker_lattices(V, weighted)
        lat = LatticeBatch.from_synth(lats, device=dev)
        assert bool(lat.weighted) == weighted
        state, inp, label = _gather_states(lats, k, 300 + V)
        N = len(state)
        values = np.random.default_rng(V).normal(0, 1, size=lat.total_rows).astype(F32)
        st, ip, lb = _t(state, dev), _t(inp, dev), _t(label, dev)
        nxt = ops.step(lat, st, lb, k=k).cpu().numpy()
        plain = ops.emission_mask(lat, st, k=k).cpu().numpy()
        legal = ops.emission_mask(lat, st, k=k, inp=ip, pad=PAD, bos=BOS, eos=EOS).cpu().numpy()
        forced = ops.emission_mask(lat, st, k=k, inp=ip, pad=PAD, bos=BOS, eos=EOS, has_to_end=True).cpu().numpy()
        gathered = ops.beta_logits(lat, _t(values, dev), st, k=k).cpu().numpy()
        dense = [tuple(x[None] for x in l.dense(weighted=weighted)) for l in lats]
        for n in range(N):
            l = lats[n // k]
            r0 = int(lat.row_off[n // k])
            ok = _in_range(l, state[n])
            em, tr = P.dense_rows(l, [state[n]], weighted) if not ok else dense[n // k]
            s = np.array([state[n] if ok else 0])
            ref_next = int(tr[0, s[0], label[n]]) if (ok and 0 <= label[n] < V) else 0
            assert nxt[n] == ref_next, (V, k, weighted, n)
            row = em[0, s[0]]
            ref_plain = row.astype(F32) if weighted else np.where(row, F32(0), F32(-np.inf))
            assert np.array_equal(plain[n], ref_plain), (V, k, weighted, n)
            one = np.array([inp[n]])
            assert np.array_equal(legal[n], O.mask_out_invalid(em, one, s, 2, 300, PAD, BOS, EOS)[0]), (V, k, weighted, n)
            assert np.array_equal(forced[n], O.mask_out_invalid(em, one, s, 5, 3, PAD, BOS, EOS)[0]), (V, k, weighted, n)
            beta = values[r0:r0 + l.n_rows][None]
            assert np.array_equal(gathered[n], O.beta_logits(tr, beta, s)[0]), (V, k, weighted, n)
            if not ok:
                assert np.all(np.isneginf(plain[n])) and np.all(gathered[n] == values[r0])


@pytest.mark.parametrize("weighted", [False, True])
def test_mask_and_value_gather_big_vocabulary(dev, weighted):
    """30000 labels: a row of 120 KB, beyond the 64 KiB of LDS a kernel gets without asking.  The dense tables are not
    built: the reference reads the arc-list form of the rows the walkers sit on."""
    V, k = P.BIG_V, 3
    lats = [P.hub_lattice(9500 + b, V, hub_degree=300, weighted=weighted) for b in range(P.WALKER_B)]
    lat = LatticeBatch.from_synth(lats, device=dev)
    state, inp, label = _gather_states(lats, k, 17)
    values = np.random.default_rng(3).normal(0, 1, size=lat.total_rows).astype(F32)
    st, ip = _t(state, dev), _t(inp, dev)
    nxt = ops.step(lat, st, _t(label, dev), k=k).cpu().numpy()
    plain = ops.emission_mask(lat, st, k=k).cpu().numpy()
    legal = ops.emission_mask(lat, st, k=k, inp=ip, pad=PAD, bos=BOS, eos=EOS).cpu().numpy()
    gathered = ops.beta_logits(lat, _t(values, dev), st, k=k).cpu().numpy()
    zero = np.zeros(1, np.int64)
    for n in range(len(state)):
        l, r0 = lats[n // k], int(lat.row_off[n // k])
        em, tr = P.dense_rows(l, [state[n]], weighted)
        assert nxt[n] == (int(tr[0, 0, label[n]]) if 0 <= label[n] < V else 0)
        assert np.array_equal(plain[n], em[0, 0].astype(F32) if weighted else np.where(em[0, 0], F32(0), F32(-np.inf)))
        assert np.array_equal(legal[n], O.mask_out_invalid(em, np.array([inp[n]]), zero, 2, 300, PAD, BOS, EOS)[0])
        assert np.array_equal(gathered[n], O.beta_logits(tr, values[r0:r0 + l.n_rows][None], zero)[0])


# ============================================================================= walker kernels: the fused proposal step
def _step_tol(tag, V, outs):
    """max(2e-5, 4 E32(V)) over the oracle's results ``outs`` of one case: from the references alone."""
    e32 = max(P.e32(o) for o in outs)
    rec(f"{tag}_E32_V{V}", e32)
    return max(TOL, 4.0 * e32)


def _check_step(tag, V, r, o, tol):
    sym, logq, logz, nxt = (x.detach().cpu().numpy() for x in r)
    finite = np.isfinite(o["logz"])
    assert np.all(np.isneginf(logz[~finite])) and np.all(np.isneginf(logq[~finite])) and np.all(sym[~finite] == PAD)
    assert np.all(nxt[~finite] == 0)
    safe, share = P.safe_share(o)
    assert share > P.CAP
    if finite.any():
        assert rec(f"{tag}_gpu_logz_V{V}", np.max(np.abs(logz[finite] - o["logz"][finite]))) <= tol, (tag, V)
    assert np.array_equal(sym[safe], o["symbol"][safe]) and np.array_equal(nxt[safe], o["next_state"][safe]), (tag, V)
    if safe.any():
        assert rec(f"{tag}_gpu_logq_V{V}", np.max(np.abs(logq[safe] - o["logq"][safe]))) <= tol, (tag, V)
    return sym


@pytest.mark.parametrize("k", P.WALKER_KS)
@pytest.mark.parametrize("V", P.WALKER_VOCABS)
def test_proposal_step_every_vocabulary(dev, V, k):
    """nfst_proposal_step against oracle.proposal_step: free sampling and forced, temperature != 1, values out of the
    walker's own state and out of a value state (V = 3413 is the largest vocabulary that fits with one), forced end;
    N = 3 or 9 walkers (a partly filled block), a hub whose legal marks span the 64-wide chunks of the CDF scan."""
    for weighted in (False, True):
        d = P.walker_inputs(V, k, weighted)
        lat = LatticeBatch.from_synth(d["lats"], device=dev)
        st, ip, sc, uu, vl, vs = (_t(d[key], dev) for key in ("state", "inp", "scores", "u", "values", "vstate"))
        configs = P.step_configs(V)
        assert len(configs) == (4 if V <= 3413 else 3)
        free = [P.oracle_step(d, k, weighted, cfg) for cfg in configs]
        forced = [P.oracle_step(d, k, weighted, cfg, forced=o["symbol"]) for cfg, o in zip(configs, free)]
        tol = _step_tol("proposal", V, free + forced)
        for cfg, o, of in zip(configs, free, forced):
            _, temperature, use_values, own, has_to_end = cfg
            not_pad = torch.zeros(1, dtype=torch.int32, device=dev)
            kw = dict(k=k, inp=ip, values=vl if use_values else None, pad=PAD, bos=BOS, eos=EOS, has_to_end=has_to_end,
                      temperature=temperature, value_state=vs if own else None)
            r = ops.proposal_step(lat, st, sc, uniforms=uu, not_pad=not_pad, **kw)
            sym = _check_step("proposal", V, r, o, tol)
            assert int(not_pad.item()) == int((sym != PAD).sum())
            # forced along the oracle's symbols
            f = ops.proposal_step(lat, st, sc, forced=_t(o["symbol"], dev), **kw)
            _check_step("proposal_forced", V, f, of, tol)


@pytest.mark.parametrize("V", P.CHAIN_VOCABS)
def test_proposal_steps_chained_with_penalties_while_sampling(dev, V):
    """Five chained steps, sampling freely, with the insertion and length penalties on: the counters ``accumulated`` and
    ``vocab_use`` carry from step to step and are the oracle's after every step.  Both sides take the oracle's symbols
    and states into the next step, so that a walker on a CDF boundary cannot part the two chains."""
    k = 3
    d = P.chain_inputs(V, k)
    N = d["N"]
    lat = LatticeBatch.from_synth(d["lats"], device=dev)
    pen_o = dict(P.CHAIN_PEN, insertion_mark=d["mark"], accumulated=d["accumulated"].copy(), vocab_use=np.zeros((N, V), F32))
    pen_g = ops.StepPenalties(N, V, dev, insertion_mark=d["mark"], **P.CHAIN_PEN)
    pen_g.accumulated.copy_(_t(d["accumulated"], dev))
    state, inp, vstate = d["state"].copy(), d["inp"].copy(), d["vstate"].copy()
    cfg = ("chain", 1.0, True, True, False)
    in_force, steps = 0, []
    for t in range(P.CHAIN_STEPS):  # the oracle's chain: it does not depend on the GPU's
        o = P.oracle_step(d, k, True, cfg, penalties=pen_o, length=t + 2, scores=d["scores"][t], inp=inp, state=state, vstate=vstate,
                          u=d["u"][t])
        steps.append((o, state, inp, vstate, pen_o["accumulated"].copy(), pen_o["vocab_use"].copy()))
        in_force += int((pen_o["accumulated"] > P.CHAIN_PEN["insert_threshold"]).sum())
        vstate, state, inp = state, o["next_state"], o["symbol"]
    assert in_force > 0 and pen_o["vocab_use"].sum() == P.CHAIN_STEPS * N
    tol = _step_tol("chain", V, [x[0] for x in steps])
    for t, (o, state, inp, vstate, acc, use) in enumerate(steps):
        not_pad = torch.zeros(1, dtype=torch.int32, device=dev)
        r = ops.proposal_step(lat, _t(state, dev), _t(d["scores"][t], dev), k=k, inp=_t(inp, dev), values=_t(d["values"], dev), pad=PAD,
                              bos=BOS, eos=EOS, temperature=1.0, uniforms=_t(d["u"][t], dev), value_state=_t(vstate, dev),
                              penalties=pen_g, length=t + 2, not_pad=not_pad)
        sym = _check_step("chain", V, r, o, tol)
        assert int(not_pad.item()) == int((sym != PAD).sum())
        assert np.array_equal(pen_g.accumulated.cpu().numpy(), acc), t
        assert np.array_equal(pen_g.vocab_use.cpu().numpy(), use), t


# ----------------------------------------------------------------------------- backward, through the C ABI
def _raw_step(lat, dev, k, state, inp, scores, values, vstate, u, temperature):
    N, V = scores.shape
    sym = torch.empty(N, dtype=torch.int64, device=dev)
    nxt = torch.empty(N, dtype=torch.int64, device=dev)
    logq = torch.empty(N, dtype=torch.float32, device=dev)
    logz = torch.empty(N, dtype=torch.float32, device=dev)
    logits = torch.empty(N, V, dtype=torch.float32, device=dev)
    extras = None
    if vstate is not None:
        extras = _lib.StepExtras()
        extras.value_state = vstate.data_ptr()
    _lib.check(_lib.lib.nfst_proposal_step(C.byref(lat.c_struct()), _ptr(state), _ptr(inp), _ptr(scores), _ptr(values), PAD, BOS, EOS, 0,
                                           float(temperature), _ptr(u), None, None if extras is None else C.byref(extras), _ptr(sym),
                                           _ptr(logq), _ptr(logz), _ptr(nxt), _ptr(logits), k, _stream()), "nfst_proposal_step")
    return sym, logq, logz, logits


@pytest.mark.parametrize("V,own", [(65, True), (65, False), (700, True), (700, False), (3413, True), (4096, False)])
def test_proposal_step_backward_every_vocabulary(dev, V, own):
    """nfst_proposal_step_backward against torch float64 autograd of the dense restatement
    logits = ((scores + values[next state]) * padmask + masks) / T, with g_logq only, g_logz only and both (a null
    pointer for the one that is absent), the value gather out of the walker's own state and out of a value state
    (with one, V <= 3413).  grad_values: row 0 of a lattice receives exactly the marks without an arc out of the value
    state -- nothing at all when the values are gathered out of the masks' own state."""
    k, weighted, T = 3, True, 0.8
    d = P.walker_inputs(V, k, weighted)
    N = d["N"]
    lat = LatticeBatch.from_synth(d["lats"], device=dev)
    st, ip, sc, uu, vl, vs = (_t(d[key], dev) for key in ("state", "inp", "scores", "u", "values", "vstate"))
    sym_t, logq_t, logz_t, logits = _raw_step(lat, dev, k, st, ip, sc, vl, vs if own else None, uu, T)
    sym = sym_t.cpu().numpy()
    o = P.oracle_step(d, k, weighted, ("bwd", T, True, own, False), forced=sym)
    tol = _step_tol("backward", V, [o])
    # the dense restatement, lattice by lattice
    mask, idx = [], []
    for b, l in enumerate(d["lats"]):
        sl = slice(b * k, (b + 1) * k)
        em, tr = l.dense(weighted=weighted)
        em_k, tr_k = np.broadcast_to(em[None], (k,) + em.shape), np.broadcast_to(tr[None], (k,) + tr.shape)
        mask.append(O.mask_out_invalid(em_k, d["inp"][sl], d["state"][sl], 2, 300, PAD, BOS, EOS).astype(np.float64))
        idx.append(tr[(d["vstate"] if own else d["state"])[sl]] + int(d["row_off"][b]))
    mask, idx = torch.from_numpy(np.concatenate(mask)), torch.from_numpy(np.concatenate(idx))
    rng = np.random.default_rng(V)
    gq_np, gz_np = rng.normal(size=N).astype(F32), rng.normal(size=N).astype(F32)
    pz = torch.ones(V, dtype=torch.float64)
    pz[PAD] = 0
    for use_q, use_z in ((True, False), (False, True), (True, True)):
        tsc = torch.from_numpy(d["scores"].astype(np.float64)).requires_grad_(True)
        tvl = torch.from_numpy(d["values"].astype(np.float64)).requires_grad_(True)
        x = ((tsc + tvl[idx]) * pz + mask) / T
        lq = torch.log_softmax(x, dim=1)[torch.arange(N), torch.from_numpy(sym)]
        lz = torch.logsumexp(x, dim=1)
        loss = torch.zeros((), dtype=torch.float64)
        if use_q:
            loss = loss + (lq * torch.from_numpy(gq_np.astype(np.float64))).sum()
        if use_z:
            loss = loss + (lz * torch.from_numpy(gz_np.astype(np.float64))).sum()
        loss.backward()
        gs = torch.empty(N, V, dtype=torch.float32, device=dev)
        gv = torch.zeros(lat.total_rows, dtype=torch.float32, device=dev)
        gq, gz = (_t(gq_np, dev) if use_q else None), (_t(gz_np, dev) if use_z else None)
        _lib.check(_lib.lib.nfst_proposal_step_backward(C.byref(lat.c_struct()), _ptr(vs if own else st), _ptr(logits), _ptr(sym_t), _ptr(logz_t),
                                                        _ptr(gq), _ptr(gz), PAD, float(T), _ptr(gs), _ptr(gv), k, _stream()),
                   "nfst_proposal_step_backward")
        tag = f"backward_{'q' if use_q else ''}{'z' if use_z else ''}"
        assert rec(f"{tag}_scores_V{V}", np.max(np.abs(gs.cpu().numpy() - tsc.grad.numpy()))) <= tol, (V, own, use_q, use_z)
        assert rec(f"{tag}_values_V{V}", np.max(np.abs(gv.cpu().numpy() - tvl.grad.numpy()))) <= max(5e-5, tol), (V, own, use_q, use_z)
        row0 = gv.cpu().numpy()[d["row_off"]]
        if own:
            assert np.any(row0 != 0.0) and np.any(tvl.grad.numpy()[d["row_off"]] != 0.0)
        else:
            assert np.all(row0 == 0.0) and np.all(tvl.grad.numpy()[d["row_off"]] == 0.0)
    assert np.max(np.abs(logq_t.cpu().numpy() - o["logq"])[np.isfinite(o["logq"])]) <= tol


# ============================================================================= IWAE
def test_iwae_rows_of_minus_infinity_and_large_values(dev):
    ninf = -np.inf
    log_p = np.array([[ninf, ninf, ninf, ninf],          # every sample off p's support
                      [-3.0, ninf, -1.0, ninf],          # some
                      [1e30, 2e30, -1e30, 3e29],         # large finite values: no overflow
                      [-1e30, -2e30, -3e30, -1.5e30],
                      [-2.0, -1.0, -0.5, -4.0]], F32)
    log_q = np.array([[-1.0, -2.0, -0.5, -3.0], [-1.5, -0.7, -2.0, -0.1], [1.0, -2.0, 3.0, 0.5], [0.5, 1.0, -1.0, 2.0],
                      [-1.0, -1.5, -2.5, -0.3]], F32)
    lm, log_w = ops.iwae(_t(log_p, dev), _t(log_q, dev))
    lm, log_w = lm.cpu().numpy(), log_w.cpu().numpy()
    ref, ref_w = O.iwae(log_p, log_q)
    t = (torch.logsumexp(torch.from_numpy((log_p - log_q).astype(np.float64)), dim=1) - np.log(4.0)).numpy()
    assert np.isneginf(lm[0]) and np.isneginf(ref[0]) and np.isneginf(t[0])
    assert np.array_equal(log_w, ref_w)
    assert np.all(np.isfinite(lm[1:])) and np.all(np.isfinite(ref[1:]))
    for got in (lm, ref):  # float32 values: within two roundings of the float64 logsumexp
        assert np.all(np.abs(got[1:].astype(np.float64) - t[1:]) <= 2 * 2.0 ** -23 * np.maximum(1.0, np.abs(t[1:])))


# ============================================================================= limits
def test_proposal_step_with_a_value_state_beyond_lds_is_refused(dev):
    """values + a value state keep three rows per walker in LDS, four walkers per block: 4 * 3 * V * 4 bytes fit
    160 KiB up to V = 3413 (the 3413 case of the tests above).  3414 and 4096 return NFST_ERR_LIMIT from the host;
    4096 without a value state runs."""
    for V in (3414, 4096):
        lats = [P.hub_lattice(9700 + V, V, hub_degree=50)]
        lat = LatticeBatch.from_synth(lats, device=dev)
        state = torch.ones(3, dtype=torch.int64, device=dev)
        scores = torch.zeros(3, V, device=dev)
        values = torch.zeros(lat.total_rows, device=dev)
        u = torch.full((3,), 0.5, device=dev)
        with pytest.raises(_lib.NfstError) as e:
            ops.proposal_step(lat, state, scores, k=3, inp=torch.full((3,), BOS, dtype=torch.int64), values=values, pad=PAD, bos=BOS,
                              eos=EOS, uniforms=u, value_state=torch.zeros(3, dtype=torch.int64))
        assert e.value.code == ERR_LIMIT
        r = ops.proposal_step(lat, state, scores, k=3, inp=torch.full((3,), BOS, dtype=torch.int64), values=values, pad=PAD, bos=BOS,
                              eos=EOS, uniforms=u)
        legal = lats[0].label[lats[0].src == 1]
        assert bool(torch.isfinite(r.logz).all()) and np.isin(r.symbol.cpu().numpy(), legal).all()
        assert abs(float(r.logz[0]) - np.log(50.0)) <= TOL

"""The path-side ops on the structural corpus of tests/structure_cases.py (``-m gpu``): a sink that is not the last row,
reachable states above it, self loops at inner states, at state 0 and at the edges of a state's 64-arc chunks,
unreachable rows below and above reachable ones (canonical arc ids differ from the caller's), members whose state 0 is
the sink.  One test per op over the whole corpus, dealt into four batches (``structure_cases.batches``), packed by both
packers and, for the ops that read the tile programs, under the three group modes.

Every packed batch is first held to the arc numbering (``arc_src / arc_dst / arc_label / arc_w`` are the concatenated
``pack_cases.reachable_arcs``, ``sink`` is ``expectation_ref.sink_of``); after that every arc-valued output is compared
in that numbering, against the reference that the op's own test module uses and with that module's checker or constants
(named where they are used): no new tolerance.  tests/test_structure_cpu.py holds those references to plain enumeration
on the same lattices.  The largest error of every kind goes to structure_errors.json in the directory of run outputs
(profiles/README.md)."""
import contextlib
import glob
import json
import os

import numpy as np
import pytest
import torch

from nfst_amd import _lib, ops, swor
from nfst_amd.constraints import ConstraintDFA, WideDFA
from nfst_amd.lattice import LatticeBatch
from oracle import oracle as O
from tests import edge_cases as E, expectation_ref as X, intersect_ref, intersect_wide_ref, kbest_ref, lattice_edit_ref
from tests import pack_cases as PC
from tests import paths_ref, positional_ref as P, positional_sample_ref as PS, positional_swor_ref as PW
from tests import structure_cases as S, swor_ref
from tests import test_gpu_expectation as GX, test_gpu_kbest as GK, test_gpu_lattice_edit as GL, test_gpu_parity as GP
from tests import test_gpu_paths as GV, test_gpu_positional as GPOS, test_gpu_positional_expectation as GPE
from tests import test_gpu_positional_kbest as GPK, test_gpu_positional_sample as GPS, test_gpu_positional_swor as GPW
from tests import test_gpu_slack as GS, test_gpu_swor as GW

pytestmark = pytest.mark.gpu
F32 = np.float32
PAD, HI = S.PAD, S.HI
NEG = -np.inf
BATCHES = S.batches()
CANON = {name: [S.canonical(l) for l in lats] for name, lats in BATCHES.items()}
NAMES = tuple(BATCHES)
EVERY_PACKING = [(route, gm) for route in ("host", "device") for gm in (0, 1, 2)]  # for the ops that read the tile programs
BOTH_PACKERS = [("host", 0), ("device", 0)]  # for the ops that read the canonical arrays only

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
            with open(os.path.join(out, "structure_errors.json"), "w") as f:
                json.dump(dict(sorted(_ERR.items())), f, indent=1)


@contextlib.contextmanager
def recorded_here(module, prefix):
    """What the checkers of another test module record while the block runs ("<their tag> <what>") goes into this
    module's record as "<prefix> <what>", and the other module's record is left as it was."""
    before = dict(module._ERR)
    try:
        yield
    finally:
        for k, v in module._ERR.items():
            if before.get(k) != v:
                rec(f"{prefix} {k.split(' ', 1)[-1]}", v)
        module._ERR.clear()
        module._ERR.update(before)


def t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def theta_of(name):
    return S.theta(BATCHES[name][0].vocab)


def asc_of(name, seed=3):
    """per-arc scores over the batch's canonical arcs (None for the batch without arcs)"""
    A = sum(l.n_arcs for l in CANON[name])
    return np.random.default_rng(seed).normal(0.0, 0.4, size=A).astype(F32) if A else None


def slices(name):
    return E.arc_slices(CANON[name])


def per_lattice(name, x):
    return [None if x is None else x[sl] for sl in slices(name)]


def degenerate(name):
    return [b for b, l in enumerate(CANON[name]) if l.n_arcs == 0]


# ----------------------------------------------------------------------------- packing, and the arc numbering first
_PACKED = {}


def numbering(lat, lats, tag):
    """The batch's canonical arcs are the reachable arcs of the caller's lists, in their order, and its sink is the
    state the arcs say."""
    can = [S.canonical(l) for l in lats]
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if sum(len(x) for x in xs) else np.zeros(0, dt)
    for key, field in (("arc_src", "src"), ("arc_dst", "dst"), ("arc_label", "label")):
        assert np.array_equal(lat._t[key].cpu().numpy(), cat([getattr(c, field) for c in can], np.int32)), (tag, key)
    assert bool(lat.weighted) == (can[0].weight is not None), tag
    if lat.weighted:
        assert np.array_equal(lat.arc_w.cpu().numpy().view(np.int32), cat([c.weight for c in can], F32).view(np.int32)), tag
    assert np.array_equal(lat.n_arcs, [c.n_arcs for c in can]) and np.array_equal(lat.n_rows, [c.n_rows for c in can]), tag
    assert np.array_equal(lat.sink, [S.sink(c) for c in can]), (tag, lat.sink)
    assert np.array_equal(lat.meta_host[:, _lib.META_N_REACH], [int((X.levels(c.n_rows, c.src, c.dst) >= 0).sum()) for c in can]), tag


def pack(name, dev, route="host", gm=0):
    key = (name, route, gm)
    if key not in _PACKED:
        lats = BATCHES[name]
        n_rows, arc_off, src, label, dst, w = PC.batch_arcs(lats)
        if route == "host":
            lat = LatticeBatch.from_arcs(n_rows, arc_off, src, label, dst, lats[0].vocab, arc_w=w, group_mode=gm).to(dev, auto_chunks=False)
        else:
            lat = LatticeBatch.from_arcs_device(n_rows, arc_off, src, label, dst, lats[0].vocab, arc_w=w, device=dev, group_mode=gm)
        numbering(lat, lats, key)
        _PACKED[key] = lat
    return _PACKED[key]


def test_arc_numbering_of_every_packing_and_the_dense_route(dev):
    for name in NAMES:
        for route, gm in EVERY_PACKING:
            lat = pack(name, dev, route, gm)
            GS._same_arrays(lat, pack(name, dev, "host", gm))
            lat.validate()
    # pad_rows_behind_sink: the collated tables through from_dense, on the host and on the device, are the batch of the
    # arc lists that the tables spell out (mixed_with_junk)
    for entry in ("pad_rows_behind_sink", "pad_rows_behind_sink_weighted"):
        e = S.entries()[entry]
        em, tr = e.dense
        n_rows, arc_off, src, label, dst, w = PC.batch_arcs(e.lats)
        arcs = LatticeBatch.from_arcs(n_rows, arc_off, src, label, dst, S.V, arc_w=w)
        host = LatticeBatch.from_dense(em, tr)
        devb = LatticeBatch.from_dense(t(em, dev), t(tr, dev))
        assert devb.device.type == "cuda"
        for lat in (host, devb):
            numbering(lat, e.lats, entry)
            GS._same_arrays(lat, arcs)
        assert list(host.sink) == [3, 4] and list(host.n_rows) == [7, 7]


# ----------------------------------------------------------------------------- forward-backward, backward, log Z
def _oracle_fb(l, sc):
    if l.n_arcs == 0:  # state 0 is the sink: the empty path, of weight 1
        la = np.full(l.n_rows, NEG)
        la[0] = 0.0
        return {"logZ": 0.0, "logalpha": la, "logbeta": la.copy(), "posterior": np.zeros(0)}
    return O.forward_backward(l.n_rows, l.src, l.dst, sc)


@pytest.mark.parametrize("name", NAMES)
def test_forward_backward(dev, name):
    """Against the float64 oracle with the constants of tests/test_gpu_parity.py (TOL = 1e-5 on log Z, ``cmp_rows`` on
    the rows, 2e-6 on posteriors, 1e-4 on grad_theta, 1e-5 on the gradient in arc_scores); the same bits from both
    packers (tests/test_gpu_pack.py)."""
    lats, theta, asc = CANON[name], theta_of(name), asc_of(name)
    V = lats[0].vocab
    refs = [_oracle_fb(l, E.score64(l, theta, a)) for l, a in zip(lats, per_lattice(name, asc))]
    depth = [X.levels(l.n_rows, l.src, l.dst) for l in lats]
    first = {}
    for route, gm in EVERY_PACKING:
        lat = pack(name, dev, route, gm)
        r = ops.forward_backward(lat, t(theta, dev), t(asc, dev), want_grad_theta=True)
        rb = ops.backward(lat, t(theta, dev), t(asc, dev))
        assert torch.equal(rb.logbeta, r.logbeta) and torch.equal(rb.logz64, r.logz64)
        z = ops.log_z(lat, t(theta, dev), t(asc, dev))
        assert torch.equal(z, r.logz)
        if gm in first:  # the device packer's batch has the host packer's bits
            assert all(torch.equal(x, y) for x, y in zip(first[gm], (r.logz64, r.logalpha, r.logbeta, r.posterior, r.grad_theta)))
        first.setdefault(gm, (r.logz64, r.logalpha, r.logbeta, r.posterior, r.grad_theta))
        la, lb, post, gth = (x.cpu().numpy() for x in (r.logalpha, r.logbeta, r.posterior, r.grad_theta))
        if asc is not None and (route, gm) in BOTH_PACKERS:  # the per-arc gradient of sum_b log Z[b] is the posterior, in canonical numbering
            a = t(asc, dev).requires_grad_()
            ops.log_z(lat, t(theta, dev), a).sum().backward()
            g = a.grad.cpu().numpy()
            loops = np.concatenate([l.src == l.dst for l in lats])
            assert np.all(g[loops] == 0.0) and rec("fb d log Z / d arc_scores", np.max(np.abs(g - np.concatenate([o["posterior"] for o in refs])))) <= 1e-5, (name, route)
        for b, (l, o) in enumerate(zip(lats, refs)):
            r0, a0 = int(lat.row_off[b]), int(lat.arc_off[b])
            assert rec("fb logz64", abs(float(r.logz64[b]) - o["logZ"])) <= GP.TOL, (name, route, gm, b)
            assert rec("fb logz32", abs(float(r.logz[b]) - o["logZ"])) <= GP.TOL, (name, route, gm, b)
            GP.cmp_rows(la[r0:r0 + l.n_rows], o["logalpha"])
            GP.cmp_rows(lb[r0:r0 + l.n_rows], o["logbeta"])
            off = depth[b] < 0  # rows that state 0 does not reach
            assert np.all(np.isneginf(la[r0:r0 + l.n_rows][off])) and np.all(np.isneginf(lb[r0:r0 + l.n_rows][off])), (name, b)
            p = post[a0:a0 + l.n_arcs]
            loop = l.src == l.dst
            assert np.all(p[loop] == 0.0), (name, route, gm, b)  # exactly 0 on every self loop
            if l.n_arcs:
                assert rec("fb posterior", np.max(np.abs(p - o["posterior"]))) <= 2e-6, (name, route, gm, b)
            ref_g = np.bincount(l.label[~loop], weights=o["posterior"][~loop], minlength=V)  # self-loop labels are not counted
            assert rec("fb grad_theta", np.max(np.abs(gth[b] - ref_g))) <= 1e-4, (name, route, gm, b)
            assert np.all(gth[b][np.setdiff1d(np.arange(V), l.label[~loop])] == 0.0), (name, b)


# ----------------------------------------------------------------------------- Viterbi, sampling, score_paths
@pytest.mark.parametrize("name", NAMES)
def test_viterbi_both_kernels(dev, name):
    """Bit for bit against ``paths_ref.viterbi_ref`` in the add order of each kernel, with the checker of
    tests/test_gpu_paths.py (``_viterbi_miss``, ``path_guard``)."""
    lats, theta, asc = CANON[name], theta_of(name), asc_of(name)
    for extras in (None, asc):
        refs = {o: [paths_ref.viterbi_ref(l, theta, l.weight, a, o) for l, a in zip(lats, per_lattice(name, extras))] for o in ("general", "tile_waves")}
        for route, gm in EVERY_PACKING:
            lat = pack(name, dev, route, gm)
            for tw in (1, 0):
                with _lib.tuning(tw=tw):
                    r = ops.viterbi(lat, t(theta, dev), arc_scores=t(extras, dev), pad=PAD)
                    got = tuple(x.cpu().numpy() for x in (r.best, r.paths, r.arcs, r.lengths))
                orders = ("general",) if tw == 0 else ("tile_waves", "general")
                miss = {o: GV._viterbi_miss(lat, lats, got, refs[o]) for o in orders}
                assert any(m is None for m in miss.values()), (name, route, gm, tw, miss)
                for b, l in enumerate(lats):
                    a0, n = int(lat.arc_off[b]), int(got[3][b])
                    arcs = got[2][b, :n] - a0
                    assert not np.any(l.src[arcs] == l.dst[arcs]), (name, b)  # never a self loop
                    if n:
                        gap, bound = paths_ref.path_guard(l, paths_ref.score64(l, theta, l.weight, per_lattice(name, extras)[b]), arcs)
                        assert -bound <= gap <= bound, (name, route, gm, tw, b, gap, bound)
                    else:  # state 0 is the sink: the empty path, of score 0.0
                        assert l.n_arcs == 0 and got[0][b] == 0.0 and np.all(got[1][b] == PAD) and np.all(got[2][b] == -1)


@pytest.mark.parametrize("name", NAMES)
def test_sample_paths_and_score_paths(dev, name):
    """Given uniforms against the oracle's walks where the uniform stays clear of every CDF boundary (paths_ref.MARGIN,
    which holds for every walk here: none is left out), log q within tests/test_gpu_paths.py's TOL; every walk ends in
    ``lat.sink``."""
    lats, theta, asc = CANON[name], theta_of(name), asc_of(name)
    K = 24 if name != "many_with_junk" else 5
    L = max(int(X.levels(l.n_rows, l.src, l.dst).max()) for l in lats) + 1
    u = np.random.default_rng(7).random((len(lats), K, L)).astype(F32)
    refs = []
    for b, (l, a) in enumerate(zip(lats, per_lattice(name, asc))):
        sc = paths_ref.score64(l, theta, l.weight, a)
        refs.append((paths_ref.oracle_walks(l, sc, u[b]) if l.n_arcs else None, sc))
    for route, gm in BOTH_PACKERS:
        lat = pack(name, dev, route, gm)
        for want_arcs in (True, False):
            s = ops.sample_paths(lat, t(theta, dev), K, arc_scores=t(asc, dev), max_len=L, uniforms=t(u, dev), pad=PAD, want_arcs=want_arcs)
            paths, lens, logq = s.paths.cpu().numpy(), s.lengths.cpu().numpy(), s.logq.cpu().numpy()
            arcs = s.arcs.cpu().numpy() if want_arcs else None
            tot, end = (x.cpu().numpy() for x in ops.score_paths(lat, t(theta, dev), s.paths, arc_scores=t(asc, dev)))
            for b, (l, (ref, sc)) in enumerate(zip(lats, refs)):
                a0 = int(lat.arc_off[b])
                assert np.all(paths[b][np.arange(L)[None, :] >= lens[b][:, None]] == PAD)
                if ref is None:  # state 0 is the sink: the empty path, log q = 0; its marks are all pad, and without a
                    # pad loop at state 0 the forced walk of them finds no arc: -inf and end state 0 (nfst_score_paths)
                    assert np.all(lens[b] == 0) and np.all(np.abs(logq[b]) <= GV.TOL) and (arcs is None or np.all(arcs[b] == -1)), (name, b)
                    assert np.all(np.isneginf(tot[b])) and np.all(end[b] == 0) and lat.sink[b] == 0
                    continue
                walks, logz, _ = ref
                safe = walks["margin"] > paths_ref.MARGIN
                rec("sample walks left undecided", (~safe).sum())
                assert safe.all(), (name, b)  # every walk is compared: the uniforms were chosen clear of every CDF boundary
                assert np.array_equal(paths[b][safe], walks["paths"][safe]) and np.array_equal(lens[b][safe], walks["lengths"][safe]), (name, b)
                if want_arcs:
                    rel = arcs[b] - np.where(arcs[b] >= 0, a0, 0)
                    assert np.array_equal(rel[safe], walks["arcs"][safe]), (name, b)
                    for k in range(K):
                        p = rel[k, :lens[b, k]]
                        assert np.array_equal(paths[b, k, :lens[b, k]], l.label[p]) and not np.any(l.src[p] == l.dst[p]), (name, b, k)
                assert np.all(end[b] == lat.sink[b]) and np.all(lens[b] > 0), (name, b)  # the end state is the sink
                o_tot, o_end = O.score_paths(l.n_rows, l.src, l.label, l.dst, sc, paths[b])
                assert np.all(o_end == lat.sink[b])
                assert rec("sample logq", np.max(np.abs(o_tot - logz - logq[b]))) <= GV.TOL, (name, b)
                assert np.max(np.abs(logq[b][safe] - walks["logq"][safe])) <= GV.TOL
                # (the bound of tests/test_gpu_paths.py's _score_paths_case: two float32 adds per arc, one rounding of the total)
                mag, _ = O.score_paths(l.n_rows, l.src, l.label, l.dst, paths_ref.score64(l, np.abs(theta), None if l.weight is None else np.abs(l.weight),
                                                                                          None if asc is None else np.abs(per_lattice(name, asc)[b])), paths[b])
                err = np.abs(tot[b].astype(np.float64) - o_tot)
                assert np.all(err <= 2.0 ** -24 * np.abs(o_tot) + 2 * 2.0 ** -24 * mag + 1e-12), (name, b, float(err.max()))
                rec("score_paths", err.max())


# ----------------------------------------------------------------------------- k best
def _kbest_refs(lats, theta, asc_parts):
    out = []
    for l, a in zip(lats, asc_parts):
        th, e = kbest_ref.arc_terms(l, theta, a)
        out.append(kbest_ref.k_best(l.n_rows, l.src, l.dst, th, e, 64, S.sink(l)))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_k_best(dev, name):
    """k = 1 and k = 64 (more than most lattices have paths): bit for bit against ``kbest_ref.k_best`` with the checker
    of tests/test_gpu_kbest.py; entry 0 is Viterbi's general kernel."""
    lats, theta, asc = CANON[name], theta_of(name), asc_of(name)
    refs = _kbest_refs(lats, theta, per_lattice(name, asc))
    assert any(r["n_paths"] < 64 for r in refs)
    for route, gm in EVERY_PACKING:
        lat = pack(name, dev, route, gm)
        for k in (1, 64):
            r = ops.k_best_terms(lat, t(theta, dev), k, arc_scores=t(asc, dev), pad=PAD)
            GK._check(name, lat, lats, r, refs, k)
            arcs, lens = r.arcs.cpu().numpy(), r.lengths.cpu().numpy()
            for b in degenerate(name):  # one path: the empty one, of score 0.0
                assert int(r.n_paths[b]) == 1 and float(r.best[b, 0]) == 0.0 and lens[b, 0] == 0 and np.all(arcs[b] == -1)
            for b, l in enumerate(lats):
                used = arcs[b][arcs[b] >= 0] - int(lat.arc_off[b])
                assert not np.any(l.src[used] == l.dst[used]), (name, b)
        with _lib.tuning(tw=0):
            GK._check_viterbi(lat, ops.k_best_terms(lat, t(theta, dev), 1, arc_scores=t(asc, dev), pad=PAD),
                              ops.viterbi(lat, t(theta, dev), arc_scores=t(asc, dev), pad=PAD, max_len=int(lat.depth.max()) + 1))


# ----------------------------------------------------------------------------- expectation and entropy
@pytest.mark.parametrize("name", NAMES)
def test_expectation_and_entropy(dev, name):
    """Against ``expectation_ref.expectation`` with the checkers of tests/test_gpu_expectation.py (TOL64 on the float64
    outputs, TOL scaled by M on the float32 ones, 2e-6 on posteriors)."""
    lats, theta, asc = CANON[name], theta_of(name), asc_of(name)
    V = lats[0].vocab
    rng = np.random.default_rng(12)
    lv = rng.normal(0.5, 1.0, size=V).astype(F32)
    av = rng.normal(0.0, 1.5, size=sum(l.n_arcs for l in lats)).astype(F32) if asc is not None else None
    refs, ents = [], []
    for l, a, v in zip(lats, per_lattice(name, asc), per_lattice(name, av)):
        if l.n_arcs:
            refs.append(GX._ref(l, theta, a, lv, v, 0.5))
            ents.append(GX._ref(l, theta, a, coef=1.0))
        else:  # the empty path: log Z = 0, E[V] = 0, H = 0
            zero = {"logZ": 0.0, "ev": 0.0, "M": 0.0, "posterior": np.zeros(0), "cov": np.zeros(0)}
            refs.append(zero), ents.append(zero)
    for route, gm in EVERY_PACKING:
        lat = pack(name, dev, route, gm)
        r = ops.expectation_terms(lat, t(theta, dev), t(asc, dev), t(lv, dev), t(av, dev), 0.5, want_posterior=True, want_cov=True,
                                  want_label_cov=True, want_label_post=True)
        cov, post, lc, lp = (x.cpu().numpy() for x in (r.cov, r.posterior, r.label_cov, r.label_post))
        H = ops.entropy(lat, t(theta, dev), t(asc, dev)).cpu().numpy()
        for b, (l, e) in enumerate(zip(lats, refs)):
            with recorded_here(GX, "expectation"):
                GX._check64(f"structure {name}", r, b, e)
                if l.n_arcs:
                    GX._check("structure", l, b, lat, e, cov=cov, post=post, label_cov=lc, label_post=lp)
            a0 = int(lat.arc_off[b])
            loop = l.src == l.dst
            assert np.all(post[a0:a0 + l.n_arcs][loop] == 0.0) and np.all(cov[a0:a0 + l.n_arcs][loop] == 0.0), (name, b)
            if l.n_arcs == 0:
                assert np.all(lc[b] == 0.0) and np.all(lp[b] == 0.0) and float(r.logz64[b]) == 0.0 and float(r.ev64[b]) == 0.0
            h = ents[b]
            assert rec("entropy / M", abs(float(H[b]) - (h["logZ"] - h["ev"])) / max(1.0, h["M"])) <= GX.TOL, (name, route, gm, b)


# ----------------------------------------------------------------------------- arc slack, beam masks, restrict
@pytest.mark.parametrize("name", NAMES)
def test_arc_slack_restrict_and_k_best_again(dev, name):
    """Every output of ``ops.arc_slack`` has the bits of ``slack_ref.arc_slack`` (the checker of tests/test_gpu_slack.py,
    per-lattice beams 0, 0.5, 3, inf taking turns); ``restrict`` of the mask packs the kept arcs, which leaves a second
    layer of unreachable rows, and ``k_best`` on that batch is ``kbest_ref`` on the kept arcs, bit for bit."""
    lats, theta, asc = CANON[name], theta_of(name), asc_of(name)
    for route, gm in EVERY_PACKING:
        lat = pack(name, dev, route, gm)
        r, refs = GS._check(name, lat, lats, theta, dev, asc)
        slack = r.slack.cpu().numpy()
        for b, l in enumerate(lats):
            a0 = int(lat.arc_off[b])
            on = np.asarray(_kbest_refs([l], theta, [per_lattice(name, asc)[b]])[0]["arcs"][0], np.int64)
            assert np.all(slack[a0 + on] == 0.0), (name, b)  # exactly 0 on the best path's arcs
        if (route, gm) not in BOTH_PACKERS:
            continue
        new, arc_map = lat.restrict(r.keep, n_kept=r.n_kept, group_mode=gm)
        am = arc_map.cpu().numpy()
        keep = r.keep.cpu().numpy()
        kept = []
        for b, l in enumerate(lats):
            kb = keep[slices(name)[b]]
            kept.append(PC.Lat(l.n_rows, l.vocab, l.src[kb], l.label[kb], l.dst[kb], None if l.weight is None else l.weight[kb]))
        numbering(new, kept, (name, "restricted"))  # (the kept arcs are trim: all of them are canonical again)
        assert np.array_equal(am, np.flatnonzero(keep)) and np.array_equal(new.sink, lat.sink)
        refs2 = _kbest_refs(kept, theta, [None if asc is None else asc[am][sl] for sl in E.arc_slices(kept)])
        for k in (1, 64):
            GK._check(f"{name} restricted", new, kept, ops.k_best_terms(new, t(theta, dev), k, arc_scores=None if asc is None else t(asc, dev)[arc_map], pad=PAD),
                      refs2, k)
        for b in degenerate(name):
            assert int(r.n_kept[b]) == 0 and float(r.best[b]) == 0.0 and int(new.n_arcs[b]) == 0


# ----------------------------------------------------------------------------- sampling without replacement
def _gumbel_err(got, want):
    """|got - want|, 0 where both are the same infinity: the empty path of a member whose state 0 is the sink keeps the
    root's perturbed score, +inf"""
    return 0.0 if got == want else abs(float(got) - float(want))


def _check_swor(tag, lat, lats, r, refs, k, decided, tol, T=None):
    """``_check`` of tests/test_gpu_swor.py and tests/test_gpu_positional_swor.py (the same body; ``tol`` is their G_TOL;
    their CAP is not used: no lattice of this corpus may be left out as undecided) with a difference of perturbed scores
    that takes equal infinities."""
    o = GW._np(r)
    assert T is None or o["paths"].shape == o["arcs"].shape == (len(lats), k, T)
    left_out = 0
    for b, (l, ref) in enumerate(zip(lats, refs)):
        n = int(o["n_paths"][b])
        assert np.all(o["lengths"][b, n:] == 0) and np.all(o["logp"][b, n:] == NEG) and np.all(o["gumbel"][b, n:] == NEG), (tag, b, k)
        for i in range(k):
            m = int(o["lengths"][b, i])
            assert np.all(o["paths"][b, i, m:] == PAD) and np.all(o["arcs"][b, i, m:] == -1), (tag, b, k, i)
        assert np.all(np.diff(o["gumbel"][b, :n]) <= 0), (tag, b, k)
        assert n == 0 or o["gumbel"][b, n - 1] >= o["kappa"][b]
        assert n > 0 or o["kappa"][b] == NEG
        a0 = int(lat.arc_off[b])
        got = {tuple(o["arcs"][b, i, :o["lengths"][b, i]] - a0): i for i in range(n)}
        assert len(got) == n, (tag, b, k)  # distinct paths
        if not decided(ref):
            left_out += 1
            continue
        assert n == ref["n_paths"], (tag, b, k)
        for j, p in enumerate(ref["arcs"]):
            assert tuple(p) in got, (tag, b, k, j)
            i = got[tuple(p)]
            assert i == j, (tag, b, k, j)  # ranked by gumbel as the reference ranks them
            assert np.array_equal(o["paths"][b, i, :len(p)], l.label[p]), (tag, b, k, j)
            assert abs(float(o["logp"][b, i]) - float(ref["logp"][j])) <= 1e-6, (tag, b, k, j)
            assert rec("swor gumbel", _gumbel_err(o["gumbel"][b, i], ref["gumbel"][j])) <= tol, (tag, b, k, j)
        assert rec("swor gumbel", _gumbel_err(o["kappa"][b], ref["kappa"])) <= tol, (tag, b, k)
    assert left_out == 0, (tag, k, left_out)  # every lattice is compared: the seeds were chosen so that each is decided


@pytest.mark.parametrize("name", NAMES)
def test_swor(dev, name):
    """``swor_ref.search`` on the op's own beta and the reference's uniforms (``swor_ref.uniforms_for``), with the checker
    of tests/test_gpu_swor.py, except that no lattice may be left out as undecided; k = 1 and k = 64 on every batch, and k
    at or above a lattice's number of paths returns every path once."""
    lats, theta, asc = CANON[name], theta_of(name), asc_of(name)
    ks = (1, 64)
    case = swor_ref.Case(name, lats, theta, asc, ks=ks, seed=11)
    counts = [S.n_paths(l) for l in lats]
    for route, gm in BOTH_PACKERS:
        lat = pack(name, dev, route, gm)
        L = int(lat.depth.max()) + 1
        for k in ks:
            u = case.uniforms(k, L) if swor_ref.degree(lats) else np.random.default_rng(1).random((len(lats), L, k, 1), dtype=F32)
            _, r, refs = GW._run(case, dev, k, lat=lat, u=u, max_len=L)
            _check_swor(name, lat, lats, r, refs, k, swor_ref.decided, GW.G_TOL)
            o = GW._np(r)
            for b, l in enumerate(lats):
                n, a0 = int(o["n_paths"][b]), int(lat.arc_off[b])
                assert n == min(k, counts[b]), (name, k, b)
                drawn = {tuple(o["arcs"][b, i, :o["lengths"][b, i]] - a0) for i in range(n)}
                assert len(drawn) == n and all(not np.any(l.src[list(p)] == l.dst[list(p)]) for p in drawn if p)
                if k >= counts[b]:  # every path once
                    assert drawn == {a for a, _ in swor_ref.enumerate_paths(l, np.zeros(l.n_arcs))} and o["kappa"][b] == NEG, (name, k, b)
                if l.n_arcs == 0:  # the empty path: length 0, log p = 0 - log Z, the root's perturbed score
                    assert n == 1 and o["lengths"][b, 0] == 0 and abs(o["logp"][b, 0]) <= 1e-6 and np.all(o["arcs"][b] == -1)
                    assert o["gumbel"][b, 0] == np.inf


# ----------------------------------------------------------------------------- lattice edit distance
@pytest.mark.parametrize("name", NAMES)
def test_lattice_edit_distance(dev, name):
    """Scored and unscored against ``lattice_edit_ref`` with the checker of tests/test_gpu_lattice_edit.py (integers
    exactly, scores and paths bit for bit): the empty reference, one longer than any path made of the labels the self
    loops carry, and a path's own labels with those labels inserted."""
    lats, theta, asc = CANON[name], theta_of(name), asc_of(name)
    longest = max(int(X.levels(l.n_rows, l.src, l.dst).max()) for l in lats)
    worst = []
    for l in lats:
        th, e = kbest_ref.arc_terms(l, theta)
        r = kbest_ref.k_best(l.n_rows, l.src, l.dst, th, e, 64, S.sink(l))
        y = l.label[r["arcs"][-1]].astype(np.int64)
        worst.append(np.concatenate([y[:1], [HI, 8, 7], y[1:]]))
    for tag, refs in (("empty", [np.zeros(0, np.int64)] * len(lats)), ("long", [np.resize([HI, 8, 7, 5], longest + 4).astype(np.int64)] * len(lats)),
                      ("own", worst)):
        for route, gm in BOTH_PACKERS:
            lat = pack(name, dev, route, gm)
            for th_np, a_np in ((theta, asc), (theta, None), (None, None)):
                r, want = GL._run(f"{name} {tag}", lat, lats, refs, dev, th_np, a_np)
                dist, lens, counts = r.distance.cpu().numpy(), r.lengths.cpu().numpy(), r.counts.cpu().numpy()
                arcs = r.path_arcs.cpu().numpy()
                for b, l in enumerate(lats):
                    p = arcs[b, :lens[b]] - int(lat.arc_off[b])
                    assert not np.any(l.src[p] == l.dst[p]), (name, tag, b)
                    if tag == "empty":
                        assert dist[b] == lens[b] and tuple(counts[b]) == (0, int(lens[b]), 0)
                for b in degenerate(name):  # le_fold's sink cell: every reference token is deleted
                    n = len(refs[b])
                    assert dist[b] == n and tuple(counts[b]) == (0, 0, n) and lens[b] == 0, (name, tag, b)
                    assert th_np is None or float(r.score[b]) == 0.0


# ----------------------------------------------------------------------------- intersection
def _automata(V):
    """name -> (delta [Q, V], final [Q]); the self loops of the corpus carry the labels 7, 8, 9 (= HI) and pad"""
    out = {"everything": (np.zeros((1, V), np.int64), np.ones(1, bool))}
    d = np.zeros((1, V), np.int64)
    d[0, [7, 8, HI]] = -1
    out["none of the loops' labels"] = (d, np.ones(1, bool))
    d = np.stack([np.zeros(V, np.int64), np.ones(V, np.int64)])
    d[0, 5], d[1, 5] = 1, 0
    d[:, HI] = -1
    out["parity of 5, no label 9"] = (d, np.ones(2, bool))
    return out


def _check_product(tag, res, lat, lats, refs):
    """tests/test_gpu_intersect.py's ``_check`` with the product's sink read from the reference (the product's rows are in
    the order of the lattice's states, so its sink is wherever the lattice's is): every integer output exactly, and the
    packed product is what the host packer makes of the reference's arc lists."""
    new, arc_map, arc_q, row_state, row_q = res
    rows = np.array([r["n_rows"] for r in refs])
    arcs = np.array([r["n_arcs"] for r in refs])
    assert np.array_equal(new.n_rows, rows) and np.array_equal(new.n_arcs, arcs), (tag, new.n_rows, rows)
    assert np.array_equal(new.meta_host[:, _lib.META_N_REACH], rows), tag  # (every row of a product is reachable)
    sinks = [int(np.flatnonzero(r["row_state"] == S.sink(l))[0]) for l, r in zip(lats, refs)]
    assert np.array_equal(new.sink, sinks), (tag, new.sink, sinks)
    a_in = np.asarray(lat.arc_off, np.int64)
    cat = lambda k, off=None: np.concatenate([r[k] + (0 if off is None else off[b]) for b, r in enumerate(refs)])
    assert np.array_equal(arc_map.cpu().numpy(), cat("arc_map", a_in)), tag
    assert np.array_equal(arc_q.cpu().numpy(), cat("arc_q")) and np.array_equal(row_state.cpu().numpy(), cat("row_state")), tag
    assert np.array_equal(row_q.cpu().numpy(), cat("row_q")), tag
    for k in ("src", "label", "dst"):
        assert np.array_equal(new._t["arc_" + k].cpu().numpy(), cat(k)), (tag, k)
    if lat.weighted:
        assert torch.equal(new.arc_w, lat.arc_w[arc_map])
    arc_off = np.zeros(len(refs) + 1, np.int64)
    np.cumsum(arcs, out=arc_off[1:])
    host = LatticeBatch.from_arcs(rows.astype(np.int32), arc_off, cat("src"), cat("label"), cat("dst"), lat.vocab,
                                  arc_w=None if not lat.weighted else lat.arc_w.cpu().numpy()[cat("arc_map", a_in)])
    GS._same_arrays(new, host)


@pytest.mark.parametrize("name", NAMES)
def test_intersect_narrow_and_wide(dev, name):
    """``intersect_ref.intersect`` for a ConstraintDFA, ``intersect_wide_ref.intersect`` for a WideDFA: arc_map, arc_q,
    row_state and row_q exactly.  An automaton that accepts nothing leaves every product empty, which the op refuses with
    a ValueError that names the first lattice."""
    lats = CANON[name]
    V = lats[0].vocab
    for route, gm in BOTH_PACKERS:
        lat = pack(name, dev, route, gm)
        for tag, (delta, final) in _automata(V).items():
            narrow = [intersect_ref.intersect(l, delta, final) for l in lats]
            wide = [intersect_wide_ref.intersect(l, delta, final) for l in lats]
            assert all(r["n_rows"] > 0 for r in narrow), (name, tag)
            _check_product(f"{name} x {tag}", ops.intersect(lat, ConstraintDFA(delta, final)), lat, lats, narrow)
            _check_product(f"{name} x {tag} (wide)", ops.intersect(lat, WideDFA.from_dense(delta, final)), lat, lats, wide)
            if tag == "everything":  # every reachable state at q = 0, every canonical arc: self loops included
                res = ops.intersect(lat, ConstraintDFA.accept_all(V))
                assert torch.equal(res.arc_map, torch.arange(lat.total_arcs, device=dev)) and np.array_equal(res.lattice.n_rows, lat.meta_host[:, _lib.META_N_REACH])
        for dfa in (ConstraintDFA(np.zeros((1, V), np.int64), np.zeros(1, bool)), WideDFA.from_dense(np.zeros((1, V), np.int64), np.zeros(1, bool))):
            with pytest.raises(ValueError, match="lattice 0: the automaton accepts none of its paths"):
                ops.intersect(lat, dfa)


# ----------------------------------------------------------------------------- the positional ops
def _budgets(lats):
    hi = max(P.min_max_len(l)[1] for l in lats)
    return sorted({max(hi - 1, 1), max(hi, 1), hi + 1})  # one below, one at, one above the longest path (T >= 1)


def _pos_inputs(lats, T, seed=21):
    rng = np.random.default_rng([seed, T])
    pos = rng.normal(0.0, 1.0, size=(len(lats), T, lats[0].vocab)).astype(F32)
    pos[..., PAD] = np.nan  # the pad column enters no output
    return pos


def _amax(x):
    """the largest |x|, 0 for a member without arcs"""
    return float(np.abs(x).max()) if np.size(x) else 0.0


def _check_positional_sum(tag, lat, lats, r, refs, T):
    """``check_sum`` of tests/test_gpu_positional.py with its bounds (TOL64, TOL32, TOLP), for batches that hold members
    without arcs (the largest error over no arcs is 0)."""
    z64, z32 = r.logz64.cpu().numpy(), r.logz.cpu().numpy()
    ll, pp, ap = r.len_logz.cpu().numpy(), r.pos_posterior.cpu().numpy(), r.arc_posterior.cpu().numpy()
    assert pp.shape == (len(lats), T, lat.vocab) and ll.shape == (len(lats), T + 1)
    assert not any(np.isnan(x).any() for x in (z64, z32, ll, pp, ap))
    for b, (l, ref) in enumerate(zip(lats, refs)):
        a0 = int(lat.arc_off[b])
        if np.isfinite(ref["logz"]):
            scale = max(1.0, abs(ref["logz"]))
            assert rec("positional logz64", abs(z64[b] - ref["logz"]) / scale) <= GPOS.TOL64, (tag, b, z64[b], ref["logz"])
            assert rec("positional logz32", abs(float(z32[b]) - ref["logz"]) / scale) <= GPOS.TOL32, (tag, b)
        else:
            assert z64[b] == NEG and z32[b] == NEG, (tag, b)
        fin = np.isfinite(ref["len_logz"])
        assert np.all(ll[b][~fin] == NEG), (tag, b)
        if fin.any():
            e = np.abs(ll[b][fin] - ref["len_logz"][fin]) / np.maximum(1.0, np.abs(ref["len_logz"][fin]))
            assert rec("positional len_logz", e.max()) <= GPOS.TOL64, (tag, b)
        assert rec("positional pos_post", _amax(pp[b] - ref["pos_post"])) <= GPOS.TOLP, (tag, b)
        assert rec("positional arc_post", _amax(ap[a0:a0 + l.n_arcs] - ref["arc_post"])) <= GPOS.TOLP, (tag, b)


def _check_positional_expectation(tag, lat, c, r, refs, dev):
    """``check`` of tests/test_gpu_positional_expectation.py with its bounds (TOL64, TOL32, TOLP, scaled by M as there),
    for batches that hold members without arcs; the masses bit for bit against ``ops.positional_forward_backward``."""
    for x in r:
        assert x is None or not torch.isnan(x).any(), tag
    z64, z32, e64, e32 = (x.cpu().numpy() for x in (r.logz64, r.logz, r.ev64, r.ev))
    pp, ap, pc, ac = (x.cpu().numpy() for x in (r.pos_posterior, r.arc_posterior, r.pos_cov, r.arc_cov))
    for b, (l, ref, sl) in enumerate(zip(c.lats, refs, E.arc_slices(c.lats))):
        M = max(1.0, ref["M"])
        if np.isfinite(ref["logz"]):
            assert rec("positional expectation logz64", abs(z64[b] - ref["logz"]) / max(1.0, abs(ref["logz"]))) <= GPE.TOL64, (tag, b)
        else:
            assert z64[b] == NEG and z32[b] == NEG and e64[b] == 0.0 and e32[b] == 0.0, (tag, b)
        assert rec("positional expectation ev64 / M", abs(e64[b] - ref["ev"]) / M) <= GPE.TOL64, (tag, b, e64[b], ref["ev"])
        assert rec("positional expectation ev32 / M", abs(float(e32[b]) - ref["ev"]) / M) <= GPE.TOL32, (tag, b)
        assert rec("positional expectation pos_post", _amax(pp[b] - ref["pos_post"])) <= GPE.TOLP, (tag, b)
        assert rec("positional expectation arc_post", _amax(ap[sl] - ref["arc_post"])) <= GPE.TOLP, (tag, b)
        assert rec("positional expectation pos_cov / M", _amax(pc[b] - ref["pos_cov"]) / M) <= GPE.TOL32, (tag, b)
        assert rec("positional expectation arc_cov / M", _amax(ac[sl] - ref["arc_cov"]) / M) <= GPE.TOL32, (tag, b)
    f = ops.positional_forward_backward(lat, t(c.theta, dev), t(c.pos, dev), c.T, t(c.asc, dev), want_pos_posterior=True, want_arc_posterior=True)
    assert GPE.eq(r.logz64, f.logz64) and GPE.eq(r.logz, f.logz) and GPE.eq(r.pos_posterior, f.pos_posterior), tag
    assert GPE.eq(r.arc_posterior, f.arc_posterior), tag


@pytest.mark.parametrize("name", NAMES)
def test_positional_forward_backward_and_viterbi(dev, name):
    """``positional_ref.sum_product`` / ``max_plus`` with the checker and the bounds of tests/test_gpu_positional.py."""
    lats, theta, asc = CANON[name], theta_of(name), asc_of(name)
    for T in _budgets(lats):
        pos = _pos_inputs(lats, T)
        for route, gm in BOTH_PACKERS:
            lat = pack(name, dev, route, gm)
            refs = GPOS.reference(lat, lats, theta, pos, T, asc)
            r, v = GPOS.run(lat, theta, pos, T, dev, asc)
            _check_positional_sum(f"{name} T={T}", lat, lats, r, refs, T)
            GPOS.check_vit(f"{name} T={T}", lat, lats, v, refs, T)
            ap, ll = r.arc_posterior.cpu().numpy(), r.len_logz.cpu().numpy()
            for b, l in enumerate(lats):
                assert np.all(ap[slices(name)[b]][l.src == l.dst] == 0.0), (name, T, b)
            for b in degenerate(name):  # the empty path: log Z = 0, all of it at length 0; Viterbi's score 0.0, length 0
                assert float(r.logz64[b]) == 0.0 and ll[b, 0] == 0.0 and np.all(np.isneginf(ll[b, 1:])), (name, T, b)
                assert float(v.best[b]) == 0.0 and int(v.lengths[b]) == 0


@pytest.mark.parametrize("name", NAMES)
def test_positional_k_best(dev, name):
    """``positional_kbest_ref.k_best`` bit for bit, with the checker of tests/test_gpu_positional_kbest.py."""
    lats, theta, asc = CANON[name], theta_of(name), asc_of(name)
    for T in _budgets(lats):
        pos = _pos_inputs(lats, T)
        refs = GPK.reference(lats, theta, pos, T, asc)
        for route, gm in BOTH_PACKERS:
            lat = pack(name, dev, route, gm)
            for k in (1, 64):
                r = GPK.run(lat, theta, pos, T, k, dev, asc)
                GPK.check(f"{name}.T{T}.k{k}", lat, lats, r, refs, T, k)
                for b in degenerate(name):
                    assert int(r.n_paths[b]) == 1 and float(r.best[b, 0]) == 0.0 and int(r.lengths[b, 0]) == 0


@pytest.mark.parametrize("name", NAMES)
def test_positional_expectation(dev, name):
    """``positional_expectation_ref.expectation`` with the checker and the bounds of
    tests/test_gpu_positional_expectation.py (values of every kind, the score coefficient on)."""
    lats = CANON[name]
    for T in _budgets(lats):
        c = GPE.make_case(lats, 40 + T, T, kind="all", shared=False, extras=bool(sum(l.n_arcs for l in lats)))
        c.theta = np.broadcast_to(theta_of(name), c.theta.shape).copy()
        refs = GPE.reference(c)
        for route, gm in BOTH_PACKERS:
            lat = pack(name, dev, route, gm)
            r = GPE.launch(lat, c, dev)
            _check_positional_expectation(f"{name} T={T}", lat, c, r, refs, dev)
            ac = r.arc_cov.cpu().numpy()
            for b, l in enumerate(lats):
                assert np.all(ac[slices(name)[b]][l.src == l.dst] == 0.0), (name, T, b)
            for b in degenerate(name):
                assert float(r.logz64[b]) == 0.0 and float(r.ev64[b]) == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_positional_sample(dev, name):
    """``positional_sample_ref.Sampler`` on given uniforms: the contract of tests/test_gpu_positional_sample.py's ``check``
    (decided walks equal, log q within TOLQ of the walk's own rescored arcs; every walk here is decided) with the end state
    read from the arcs' sink."""
    lats, theta, asc = CANON[name], theta_of(name), asc_of(name)
    K = 16 if name != "many_with_junk" else 4
    for T in _budgets(lats):
        pos = _pos_inputs(lats, T)
        U = np.stack([PS.uniforms(100 * T + b, K, T) for b in range(len(lats))])
        smp = [PS.Sampler(l, P.arc_score64(l, theta, a), pos[b], T) for b, (l, a) in enumerate(zip(lats, per_lattice(name, asc)))]
        walks = [s.walks(U[b]) if l.n_arcs else None for b, (l, s) in enumerate(zip(lats, smp))]
        for route, gm in BOTH_PACKERS:
            lat = pack(name, dev, route, gm)
            r = ops.positional_sample_paths(lat, t(theta, dev), K, t(pos, dev), T=T, arc_scores=t(asc, dev), uniforms=t(U, dev), pad=PAD)
            h = GPS.host(r)
            arcs = GPS.rel_arcs(lat, h["arcs"])
            skipped = 0
            for b, (l, s) in enumerate(zip(lats, smp)):
                if not np.isfinite(s.logz) or l.n_arcs == 0:  # no path within T; or the empty path: log Z = 0, log q = 0
                    assert h["logz64"][b] == (0.0 if l.n_arcs == 0 else NEG), (name, T, b)
                    assert np.all(h["lengths"][b] == 0) and np.all(h["paths"][b] == PAD) and np.all(arcs[b] == -1) and np.all(h["logq"][b] == 0.0)
                    continue
                assert abs(h["logz64"][b] - s.logz) <= 1e-9 * max(1.0, abs(s.logz)), (name, T, b)
                for k in range(K):
                    n = int(h["lengths"][b, k])
                    got = [int(a) for a in arcs[b, k, :n]]
                    assert 1 <= n <= T and np.all(h["paths"][b, k, n:] == PAD) and np.all(arcs[b, k, n:] == -1), (name, T, b, k)
                    st = 0
                    for a in got:
                        assert 0 <= a < l.n_arcs and l.src[a] == st and l.dst[a] != st, (name, T, b, k)
                        st = int(l.dst[a])
                    assert st == lat.sink[b], (name, T, b, k)
                    assert [int(x) for x in h["paths"][b, k, :n]] == [int(l.label[a]) for a in got]
                    own = s.path_score(got) - s.logz
                    assert rec("positional sample logq", abs(float(h["logq"][b, k]) - own) / max(1.0, abs(own))) <= GPS.TOLQ, (name, T, b, k)
                    ref = walks[b][k]
                    if ref["margin"] <= PS.DECIDED:
                        skipped += 1
                        continue
                    assert got == ref["arcs"] and n == ref["length"], (name, T, b, k, ref["margin"])
            rec("positional sample walks left undecided", skipped)
            assert skipped == 0, (name, T, skipped)  # every walk is compared


@pytest.mark.parametrize("name", NAMES)
def test_positional_swor(dev, name):
    """``positional_swor_ref.search`` on float64 beta rows and seeded uniforms, with the checker of
    tests/test_gpu_positional_swor.py, except that no lattice may be left out as undecided; k = 1 and k = 64 on every
    batch, and k at or above the number of paths that fit returns each of them once."""
    lats, theta, asc = CANON[name], theta_of(name), asc_of(name)
    ks = (1, 64)
    case = swor_ref.Case(name, lats, theta, asc, ks=ks, seed=13)
    es = case.scores()
    D = max(swor_ref.degree(lats), 1)
    for T in _budgets(lats):
        pos = _pos_inputs(lats, T)
        pos[..., PAD] = 0.0
        betas = PW.beta_rows(case, T, pos)
        fit = [[p for p in P.enumerate_paths(l) if len(p) <= T] for l in lats]
        for k in ks:
            u = np.stack([np.random.default_rng([13, b, T]).random((T, k, D), dtype=F32) for b in range(len(lats))])
            refs = [PW.search(l, es[b], pos[b], betas[b][0], betas[b][1], k, T, u[b]) for b, l in enumerate(lats)]
            for route, gm in BOTH_PACKERS:
                lat = pack(name, dev, route, gm)
                r = GPW._sample(case, dev, lat, k, pos, u, T=T)
                _check_swor(name, lat, lats, r, refs, k, PW.decided, GPW.G_TOL, T)
                o = GPW._np(r)
                for b, l in enumerate(lats):
                    n, a0 = int(o["n_paths"][b]), int(lat.arc_off[b])
                    assert n == min(k, len(fit[b])), (name, T, k, b)
                    if k >= len(fit[b]):
                        assert {tuple(o["arcs"][b, i, :o["lengths"][b, i]] - a0) for i in range(n)} == {tuple(p) for p in fit[b]}, (name, T, k, b)
                    if l.n_arcs == 0:
                        assert n == 1 and o["lengths"][b, 0] == 0 and o["logp"][b, 0] == 0.0 and o["gumbel"][b, 0] == np.inf

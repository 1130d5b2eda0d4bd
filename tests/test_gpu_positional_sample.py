"""ops.positional_sample_paths / ops.positional_score_paths (nfst_positional_sample, nfst_positional_score_paths: exact
draws under position-dependent scores and a length budget, and forced scores) against the NumPy restatement of
tests/positional_sample_ref.py, which tests/test_positional_sample_cpu.py proves against path enumeration.

Bounds.  The engine's walk works in (float64 mantissa, int32 exponent) and reads float32 uniforms, so a walk whose
uniforms stay 1e-6 clear of every CDF boundary (its ``margin``) must be the restatement's walk arc for arc; at most 1 %
of the walks of a comparison may be closer (tests/test_positional_sample_cpu.py holds every case of ``COMPARED`` below
to that cap on the reference alone).  logq: 2e-6 * max(1, |ref|), one float32 rounding of the output; logz64: the bits
of ops.positional_forward_backward.  Every walk, decided or not, must be an accepting path of at most T arcs whose logq
is its own rescored arcs."""
import dataclasses
from typing import Optional

import numpy as np
import pytest
import torch

from nfst_amd import ops, synth
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from tests import edge_cases as E
from tests import positional_ref as R
from tests import positional_sample_ref as S
from tests.test_positional_cpu import small_lattices, truncations

pytestmark = pytest.mark.gpu
PAD = synth.PAD
NEG = -np.inf
TOLQ = 2e-6


@dataclasses.dataclass
class Case:
    tag: str
    lats: list
    theta: np.ndarray  # [V] or [B, V]
    pos: Optional[np.ndarray]  # [T, V], [B, T, V] or None
    asc: Optional[np.ndarray]  # [total_arcs] or None
    T: int
    U: np.ndarray  # [B, K, T] float32
    thresholds: tuple = (S.DECIDED,)  # the margins at which this case's walks are compared
    opts: dict = dataclasses.field(default_factory=dict)


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _same_vocab(lats, V=None):
    V = max(l.vocab for l in lats) if V is None else V
    return [dataclasses.replace(l, vocab=V) for l in lats]


def small6():
    return list(cached("small6", lambda: _same_vocab(small_lattices())))


def _inputs(lats, seed, T, shared_pos=False, shared_theta=True):
    rng = np.random.default_rng(seed)
    B, V = len(lats), lats[0].vocab
    theta = rng.normal(-1.0, 0.8, size=(V,) if shared_theta else (B, V)).astype(np.float32)
    pos = rng.normal(0.0, 1.0, size=(T, V) if shared_pos else (B, T, V)).astype(np.float32)
    pos[..., PAD] = np.nan  # the pad column enters no output
    return theta, pos


def _per(x, b, shared_ndim):
    return None if x is None else (x if x.ndim == shared_ndim else x[b])


def samplers(case):
    def make():
        out = []
        for b, (l, sl) in enumerate(zip(case.lats, E.arc_slices(case.lats))):
            asc_b = None if case.asc is None else case.asc[sl]
            out.append(S.Sampler(l, R.arc_score64(l, _per(case.theta, b, 1), asc_b), _per(case.pos, b, 2), case.T))
        return out
    return cached(("samplers", case.tag), make)


def reference_walks(case):
    """Per lattice, the restatement's walks under the case's uniforms (once per process)."""
    return cached(("walks", case.tag), lambda: [smp.walks(case.U[b]) for b, smp in enumerate(samplers(case))])


# ----------------------------------------------------------------------------- the cases compared with the restatement
def _all_T(lats):
    return sorted({T for l in lats for _, T in truncations(l)})


def small_cases():
    lats = small6()
    out = []
    for T in _all_T(lats):
        for shared in (False, True):
            theta, pos = _inputs(lats, 1000 + T, T, shared_pos=shared)
            U = np.stack([S.small_uniforms(b, T) for b in range(6)])
            out.append(Case(f"small.{T}.{int(shared)}", lats, theta, pos, None, T, U))
    return out


def high_degree_pair():
    def make():
        l = synth.layered_lattice(24, n_states=200, avg_degree=90.0, vocab=140, width=8, span=3, max_degree=130)
        chain = synth.layered_lattice(5, n_states=20, avg_degree=1.0, vocab=140, width=1, span=1, max_degree=1)
        return [l, chain]
    return list(cached("high degree", make))


def big_pair():
    def make():
        big = synth.layered_lattice(22, n_states=1100, avg_degree=6.0, vocab=70, width=24, span=4, max_degree=24)
        tiny = synth.layered_lattice(3, n_states=12, avg_degree=2.0, vocab=70, width=3, span=3, max_degree=4)
        return [big, tiny]
    return list(cached("big pair", make))


def wave_cases():
    out = []
    for tag, lats, T, seed in (("degree119", high_degree_pair(), 27, 24), ("rows1101", big_pair(), 48, 22)):
        theta, pos = _inputs(lats, seed, T)
        U = np.stack([S.uniforms(100 * seed + b, 8, T) for b in range(len(lats))])
        out.append(Case(f"waves.{tag}", lats, theta, pos, None, T, U))
    return out


K_WORKGROUP = (17, 5, 1)  # neither multiples of the walks of a workgroup (4) nor all above it


def workgroup_cases():
    lats = small6()
    T = 13
    theta, pos = _inputs(lats, 77, T)
    U = np.stack([S.uniforms(770 + b, max(K_WORKGROUP), T) for b in range(6)])
    return [Case(f"workgroup.{K}", lats, theta, pos, None, T, np.ascontiguousarray(U[:, :K])) for K in K_WORKGROUP]


def weighted_lattices():
    return list(cached("weighted", lambda: [synth.layered_lattice(s, n_states=12, avg_degree=2.0, vocab=12, width=3, span=3, max_degree=4,
                                                                  weighted=True) for s in (11, 12, 13)]))


def extras_cases():
    lats = weighted_lattices()
    T = max(R.min_max_len(l)[1] for l in lats)
    theta, pos = _inputs(lats, 88, T, shared_theta=False)
    asc = np.random.default_rng(89).normal(0.0, 0.3, size=sum(l.n_arcs for l in lats)).astype(np.float32)
    U = np.stack([S.uniforms(880 + b, 16, T) for b in range(len(lats))])
    plain = _same_vocab(small_lattices()[:3])
    theta0, pos0 = _inputs(plain, 90, T, shared_theta=False)
    asc0 = np.random.default_rng(91).normal(0.0, 0.3, size=sum(l.n_arcs for l in plain)).astype(np.float32)
    return [Case("extras.weights+arc_scores", lats, theta, pos, asc, T, U), Case("extras.arc_scores", plain, theta0, pos0, asc0, T, U),
            Case("extras.none", plain, theta0, pos0, None, T, U)]


def no_position_cases():
    lats = small6()
    T = max(R.min_max_len(l)[1] for l in lats) + 1
    theta = synth.label_scores(5, lats[0].vocab)
    U = np.stack([S.uniforms(990 + b, 64, T) for b in range(6)])
    return [Case("no positions", lats, theta, None, None, T, U, thresholds=(S.DECIDED, 1e-5))]


RANGE = "shift"


def range_cases():
    lats, theta, asc, pos, T = E.pos_range_inputs(RANGE)
    U = np.stack([S.uniforms(660 + b, 8, T) for b in range(len(lats))])
    return [Case("range." + RANGE, lats, theta, pos, asc, T, U)]


def single_position_cases():
    lats = E.mixed_batch()
    theta, pos = _inputs(lats, 351, 1)
    U = np.stack([S.uniforms(550 + b, 4, 1) for b in range(len(lats))])
    return [Case("T1", lats, theta, pos, None, 1, U)]


COMPARED = {"small": small_cases, "waves": wave_cases, "workgroup": workgroup_cases, "extras": extras_cases,
            "no positions": no_position_cases, "range": range_cases, "T1": single_position_cases}


# ----------------------------------------------------------------------------- running and checking
def t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def run(case, dev, lat=None, **kw):
    lat = LatticeBatch.from_synth(case.lats, device=dev, **case.opts) if lat is None else lat
    K = case.U.shape[1]
    r = ops.positional_sample_paths(lat, t(case.theta, dev), K, t(case.pos, dev), T=case.T, arc_scores=t(case.asc, dev),
                                    uniforms=t(case.U, dev), pad=PAD, **kw)
    return lat, r


def host(r):
    return {k: None if v is None else v.cpu().numpy() for k, v in r._asdict().items()}


def rel_arcs(lat, arcs):
    off = np.asarray([int(lat.arc_off[b]) for b in range(arcs.shape[0])], np.int64)[:, None, None]
    return np.where(arcs >= 0, arcs - off, -1).astype(np.int32)


def check(case, lat, r, threshold=S.DECIDED):
    """The whole contract of one launch against the restatement; returns (walks, undecided)."""
    h = host(r)
    B, K, T = case.U.shape
    assert h["paths"].shape == (B, K, T) and h["arcs"].shape == (B, K, T) and h["lengths"].shape == (B, K) and h["logq"].shape == (B, K)
    assert not np.isnan(h["logq"]).any()
    arcs = rel_arcs(lat, h["arcs"])
    refs = reference_walks(case)
    fb = ops.positional_forward_backward(lat, t(case.theta, lat.device), t(case.pos, lat.device), T=case.T,
                                         arc_scores=t(case.asc, lat.device), want_pos_posterior=False)
    assert np.array_equal(h["logz64"].view(np.int64), fb.logz64.cpu().numpy().view(np.int64)), case.tag
    assert np.array_equal(h["logz"].view(np.int32), fb.logz.cpu().numpy().view(np.int32)), case.tag
    skipped = 0
    for b, (l, smp) in enumerate(zip(case.lats, samplers(case))):
        if not np.isfinite(smp.logz):  # the empty result
            assert h["logz64"][b] == NEG
            assert np.all(h["lengths"][b] == 0) and np.all(h["paths"][b] == PAD) and np.all(arcs[b] == -1) and np.all(h["logq"][b] == 0.0)
            continue
        assert abs(h["logz64"][b] - smp.logz) <= 1e-9 * max(1.0, abs(smp.logz)), (case.tag, b)
        for k in range(K):
            n = int(h["lengths"][b, k])
            got = [int(a) for a in arcs[b, k, :n]]
            # an accepting path of at most T arcs, padded, whose logq is its own rescored arcs
            assert 1 <= n <= T and np.all(h["paths"][b, k, n:] == PAD) and np.all(arcs[b, k, n:] == -1), (case.tag, b, k)
            s = 0
            for a in got:
                assert 0 <= a < l.n_arcs and l.src[a] == s and l.dst[a] != s, (case.tag, b, k)
                s = int(l.dst[a])
            assert s == l.n_rows - 1, (case.tag, b, k)
            assert [int(x) for x in h["paths"][b, k, :n]] == [int(l.label[a]) for a in got], (case.tag, b, k)
            own = smp.path_score(got) - smp.logz
            assert abs(float(h["logq"][b, k]) - own) <= TOLQ * max(1.0, abs(own)), (case.tag, b, k, h["logq"][b, k], own)
            ref = refs[b][k]
            if ref["margin"] <= threshold:
                skipped += 1
                continue
            assert got == ref["arcs"] and n == ref["length"], (case.tag, b, k, ref["margin"])
            assert abs(float(h["logq"][b, k]) - ref["logq"]) <= TOLQ * max(1.0, abs(ref["logq"])), (case.tag, b, k)
    assert skipped <= S.CAP * B * K, (case.tag, skipped)
    return B * K, skipped


# ----------------------------------------------------------------------------- small batch at every truncation
@pytest.mark.parametrize("shared_pos", [False, True])
def test_small_batch_at_every_truncation(dev, shared_pos):
    lat = LatticeBatch.from_synth(small6(), device=dev)
    seen = set()
    for case in small_cases():
        if (case.pos.ndim == 2) != shared_pos:
            continue
        _, r = run(case, dev, lat)
        check(case, lat, r)
        lens = r.lengths.cpu().numpy()
        for b, l in enumerate(case.lats):
            for name, Tb in truncations(l):
                if Tb == case.T:
                    seen.add((b, name))
                    if name == "below":
                        assert np.all(lens[b] == 0) and torch.all(r.logq[b] == 0) and torch.all(r.paths[b] == PAD) and torch.all(r.arcs[b] == -1)
                    else:
                        assert np.all(lens[b] >= 1)
    assert all((b, name) in seen for b in range(6) for name in ("below", "shortest", "between", "depth", "beyond"))


# ----------------------------------------------------------------------------- wave rounds
@pytest.mark.parametrize("i", [0, 1])
def test_wave_rounds(dev, i):
    """Out-degree 119 (two rounds of 64 lanes, the running sum carried over) beside a chain of out-degree 1; a lattice of
    1101 rows beside one of 13."""
    case = wave_cases()[i]
    if i == 0:
        deg = [np.bincount(l.src[l.src != l.dst]) for l in case.lats]
        assert deg[0].max() == 119 and deg[1].max() == 1 and R.min_max_len(case.lats[0])[1] <= case.T
        taken = np.concatenate([w["arcs"] for w in reference_walks(case)[0]])
        first = np.searchsorted(case.lats[0].src, case.lats[0].src[taken])
        assert (taken - first >= 64).any()  # some walk takes an arc of a second round
    else:
        assert case.lats[0].n_rows > 1024 and case.lats[1].n_rows == 13 and R.min_max_len(case.lats[0])[1] == case.T
    lat, r = run(case, dev)
    check(case, lat, r)


# ----------------------------------------------------------------------------- K against the workgroup
def test_k_against_the_workgroup(dev):
    lat = LatticeBatch.from_synth(small6(), device=dev)
    got = {}
    for case in workgroup_cases():
        _, r = run(case, dev, lat)
        check(case, lat, r)
        got[case.U.shape[1]] = host(r)
    for K in (5, 1):  # walk k of a larger launch is walk k of a smaller one given the same uniform rows
        for name in ("paths", "arcs", "lengths", "logq"):
            assert np.array_equal(got[17][name][:, :K].view(np.uint8), got[K][name].view(np.uint8)), (K, name)


# ----------------------------------------------------------------------------- extras
def test_extras(dev):
    """Weighted tables, arc_scores and per-lattice theta: k_positional_walk<true> with both extras and with one, and
    k_positional_walk<false>."""
    for case in extras_cases():
        lat, r = run(case, dev)
        assert (lat.weighted != 0) == (case.tag == "extras.weights+arc_scores")
        check(case, lat, r)


def test_staged_and_unstaged_give_the_same_bits(dev):
    lats = [dataclasses.replace(l, vocab=E.POS_V) for l in small_lattices()] + E.pos_degree_classes()
    big = E.pos_large("big")
    T = max(R.min_max_len(l)[1] for l in lats)
    theta, pos = _inputs(lats + [big], 280, T)
    U = np.stack([S.uniforms(2800 + b, 8, T) for b in range(len(lats) + 1)])
    staged = Case("staged", lats, theta, pos[:-1], None, T, U[:-1])
    both = Case("unstaged", lats + [big], theta, pos, None, T, U)
    lat_s, rs = run(staged, dev)
    lat_u, ru = run(both, dev)
    assert ops.positional_plan(lat_s)[1] is True and ops.positional_plan(lat_u)[1] is False
    check(staged, lat_s, rs)
    hs, hu = host(rs), host(ru)
    n = len(lats)
    assert np.isfinite(hs["logz64"]).all()
    for name in ("paths", "lengths", "logq", "logz", "logz64"):
        assert np.array_equal(hs[name].view(np.uint8), hu[name][:n].view(np.uint8)), name
    assert np.array_equal(rel_arcs(lat_s, hs["arcs"]), rel_arcs(lat_u, hu["arcs"])[:n])


# ----------------------------------------------------------------------------- forcing
def test_forcing(dev):
    """pos is -inf everywhere except along one accepting mark sequence per lattice: every walk is that path and logq is
    0; one -inf entry on the only path gives the empty result for that lattice alone."""
    lats = small6()[:3]
    T = 6
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta, pos = _inputs(lats, 41, T)
    keep = []
    for b, l in enumerate(lats):
        p = [q for q in R.enumerate_paths(l) if len(q) <= T][3 + b]
        one = np.full((T, lat.vocab), NEG, np.float32)
        for i, a in enumerate(p):
            one[i, l.label[a]] = pos[b, i, l.label[a]]
        pos[b] = one
        keep.append(p)
    U = np.stack([S.uniforms(410 + b, 16, T) for b in range(3)])
    case = Case("forcing", lats, theta, pos, None, T, U)
    _, r = run(case, dev, lat)
    h = host(r)
    arcs = rel_arcs(lat, h["arcs"])
    for b, p in enumerate(keep):
        assert np.all(h["lengths"][b] == len(p)) and np.all(arcs[b, :, :len(p)] == np.asarray(p)[None, :]), b
        assert np.abs(h["logq"][b]).max() <= 1e-6, b
    dead = pos.copy()
    dead[1, 2, lats[1].label[keep[1][2]]] = NEG
    case = Case("forcing.dead", lats, theta, dead, None, T, U)
    _, r2 = run(case, dev, lat)
    h2 = host(r2)
    assert h2["logz64"][1] == NEG and np.all(h2["lengths"][1] == 0) and np.all(h2["paths"][1] == PAD) and np.all(h2["logq"][1] == 0.0)
    assert np.all(h2["arcs"][1] == -1)
    for b in (0, 2):
        for name in ("paths", "arcs", "lengths", "logq", "logz64"):
            assert np.array_equal(h[name][b:b + 1].view(np.uint8), h2[name][b:b + 1].view(np.uint8)), (b, name)


# ----------------------------------------------------------------------------- without positions: the float32 sampler
def test_without_positions_it_is_sample_paths(dev):
    (case,) = no_position_cases()
    lat, r = run(case, dev)
    check(case, lat, r)
    check(case, lat, r, threshold=1e-5)
    s = ops.sample_paths(lat, t(case.theta, dev), case.U.shape[1], max_len=case.T, uniforms=t(case.U, dev), pad=PAD)
    margin = np.asarray([[w["margin"] for w in per] for per in reference_walks(case)])
    safe = torch.from_numpy(margin > 1e-5).to(dev)  # the float32 sampler's own rule
    assert int((~safe).sum()) <= S.CAP * safe.numel()
    assert torch.equal(r.paths[safe], s.paths[safe]) and torch.equal(r.arcs[safe], s.arcs[safe])
    assert torch.equal(r.lengths[safe], s.lengths[safe])
    assert float((r.logq[safe] - s.logq[safe]).abs().max()) <= 2e-5


# ----------------------------------------------------------------------------- zero-variance IWAE, forced scoring
def test_zero_variance_iwae(dev):
    case = small_cases()[-2]  # the largest truncation, a table per lattice
    lat, r = run(case, dev)
    score, end, lens = ops.positional_score_paths(lat, t(case.theta, dev), r.paths, t(case.pos, dev))
    live = torch.isfinite(r.logz64)
    assert bool(live.all())
    assert torch.equal(lens, r.lengths)
    sink = torch.tensor([l.n_rows - 1 for l in case.lats], dtype=torch.int32, device=dev)
    assert torch.equal(end, sink[:, None].expand_as(end))
    z = r.logz.cpu().numpy()
    assert np.abs((score - r.logq).cpu().numpy() - z[:, None]).max() <= 5e-5
    lm, log_w = ops.iwae(score, r.logq)
    assert np.abs(lm.cpu().numpy() - z).max() <= 5e-5 and np.abs(log_w.cpu().numpy() - z[:, None]).max() <= 5e-5
    sc = LatticeScorer(lat.vocab, theta=case.theta).to(dev).set_lattice(lat)
    rs = sc.positional_sample(t(case.pos, dev), case.U.shape[1], uniforms=t(case.U, dev))
    assert torch.equal(rs.paths, r.paths) and torch.equal(rs.logq, r.logq)
    assert torch.equal(sc.positional_score(t(case.pos, dev), r.paths)[0], score)


def test_forced_scoring(dev):
    lats = small6()[:3]
    T = 7
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta, pos = _inputs(lats, 45, T)
    pos[0, 2, :] = NEG  # lattice 0: every path longer than 2 arcs scores -inf
    per = [[p for p in R.enumerate_paths(l) if len(p) <= T][:18] for l in lats]
    K = 18 + 2
    marks = np.full((3, K, T), PAD, np.int32)
    for b, (l, ps) in enumerate(zip(lats, per)):
        assert len(ps) == 18
        for k, p in enumerate(ps):
            marks[b, k, :len(p)] = l.label[p]
        marks[b, 18] = marks[b, 0]
        marks[b, 18, 1] = lat.vocab - 1 if marks[b, 0, 1] != lat.vocab - 1 else lat.vocab - 2  # leaves the lattice at mark 1
        marks[b, 19] = marks[b, 0]
        marks[b, 19, T - 1] = marks[b, 0, 0]  # a mark after the pad
    score, end, lens = (x.cpu().numpy() for x in ops.positional_score_paths(lat, t(theta, dev), t(marks, dev), t(pos, dev)))
    for b, l in enumerate(lats):
        sc64 = R.arc_score64(l, theta)
        for k in range(K):
            fs, fe, fn = S.forced_score(l, sc64, pos[b], marks[b, k])
            assert end[b, k] == fe and lens[b, k] == fn, (b, k)
            if np.isfinite(fs):
                assert abs(float(score[b, k]) - fs) <= TOLQ * max(1.0, abs(fs)), (b, k)
            else:
                assert score[b, k] == NEG, (b, k)
        assert score[b, 18] == NEG and end[b, 18] == 0 and score[b, 19] == NEG and end[b, 19] == 0
    assert np.isinf(score[0]).sum() > 2 and np.isfinite(score[1][:18]).all()
    # without positions: nfst_score_paths
    s2, e2, _ = ops.positional_score_paths(lat, t(theta, dev), t(marks, dev))
    s1, e1 = ops.score_paths(lat, t(theta, dev), t(marks, dev))
    assert torch.equal(e1, e2) and torch.equal(torch.isinf(s1), torch.isinf(s2))
    fin = torch.isfinite(s1)
    assert float(((s1[fin] - s2[fin]).abs() / s1[fin].abs().clamp(min=1.0)).max()) <= 2e-7


# ----------------------------------------------------------------------------- Philox
def test_philox(dev):
    lats = small6()[:2]
    T = 8
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta, pos = _inputs(lats, 47, T)
    K = 4096
    a = ops.positional_sample_paths(lat, t(theta, dev), K, t(pos, dev), seed=5, pad=PAD)
    b = ops.positional_sample_paths(lat, t(theta, dev), K, t(pos, dev), seed=5, pad=PAD)
    c = ops.positional_sample_paths(lat, t(theta, dev), K, t(pos, dev), seed=6, pad=PAD, want_arcs=False)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert c.arcs is None and not torch.equal(a.paths, c.paths)
    pp = ops.positional_forward_backward(lat, t(theta, dev), t(pos, dev)).pos_posterior.cpu().numpy()
    paths, lens = a.paths.cpu().numpy(), a.lengths.cpu().numpy()
    for r in (a, c):
        z = r.logz64.cpu().numpy()
        assert np.isfinite(z).all() and abs(np.exp(r.logq.double().cpu().numpy()).max()) <= 1.0 + 1e-6
    for bi in range(2):
        freq = np.zeros((T, lat.vocab))
        for ti in range(T):
            on = lens[bi] > ti
            freq[ti] = np.bincount(paths[bi, on, ti], minlength=lat.vocab) / K
        assert np.abs(freq - pp[bi]).max() <= 0.05, bi  # (binomial sd <= 0.0078 at 4096 draws)


# ----------------------------------------------------------------------------- bits
def _bits(lat, r):
    h = host(r)
    h["arcs"] = rel_arcs(lat, h["arcs"])
    return h


def _same_per_lattice(x, y, pairs):
    for i, j in pairs:
        for name in x:
            assert np.array_equal(np.ascontiguousarray(x[name][i:i + 1]).view(np.uint8), np.ascontiguousarray(y[name][j:j + 1]).view(np.uint8)), (i, j, name)


def test_two_launches_another_order_and_packings_give_the_same_bits(dev):
    lats = _same_vocab(small6() + big_pair())
    T = 30
    theta, pos = _inputs(lats, 71, T)
    U = np.stack([S.uniforms(710 + b, 8, T) for b in range(len(lats))])
    case = Case("bits", lats, theta, pos, None, T, U)
    lat, r1 = run(case, dev)
    _, r2 = run(case, dev, lat)
    b1 = _bits(lat, r1)
    _same_per_lattice(b1, _bits(lat, r2), [(i, i) for i in range(len(lats))])
    order = [7, 2, 5, 0, 6, 3, 1, 4]
    other = Case("bits.order", [lats[i] for i in order], theta, pos[order], None, T, U[order])
    lat_p, rp = run(other, dev)
    _same_per_lattice(b1, _bits(lat_p, rp), [(i, j) for j, i in enumerate(order)])
    # two packings with different scratch rows (max_rows is the stride of the backward pass's LDS rows)
    star = E.packing_lattices()
    Ts = max(R.min_max_len(l)[1] for l in star)
    theta, pos = _inputs(star, 310, Ts)
    U = np.stack([S.uniforms(3100 + b, 8, Ts) for b in range(len(star))])
    got = []
    for i in (0, 3):
        case = Case(f"bits.packing{i}", star, theta, pos, None, Ts, U, opts=E.STAR_PACKINGS[i])
        lat_i, ri = run(case, dev)
        got.append((int(lat_i.max_rows), _bits(lat_i, ri)))
    assert got[0][0] != got[1][0]
    _same_per_lattice(got[0][1], got[1][1], [(i, i) for i in range(len(star))])
    assert np.isfinite(got[0][1]["logz64"]).all() and (got[0][1]["lengths"] >= 1).all()


def test_snips_shaped_batch_with_and_without_chunked_programs(dev):
    lats = synth.snips_shaped_batch(4, vocab=250)
    T = max(R.min_max_len(l)[1] for l in lats)
    theta, pos = _inputs(lats, 320, T)
    U = np.stack([S.uniforms(3200 + b, 4, T) for b in range(4)])
    case = Case("snips", lats, theta, pos, None, T, U)
    plain = LatticeBatch.from_synth(lats).to(dev, auto_chunks=False)
    host_lat = LatticeBatch.from_synth(lats)
    assert host_lat.build_chunks(force=True)
    chunked = host_lat.to(dev)
    assert chunked.chunks is not None and plain.chunks is None
    _, r1 = run(case, dev, plain)
    _, r2 = run(case, dev, chunked)
    b1 = _bits(plain, r1)
    _same_per_lattice(b1, _bits(chunked, r2), [(i, i) for i in range(4)])
    assert np.isfinite(b1["logz64"]).all() and (b1["lengths"] >= 1).all() and np.isfinite(b1["logq"]).all()


# ----------------------------------------------------------------------------- exponent range, T = 1
def test_exponent_range(dev):
    """|log Z| of 1e5 and more: the ratios of the walk must neither overflow nor collapse."""
    (case,) = range_cases()
    assert max(abs(smp.logz) for smp in samplers(case)) > E.RANGE_LOGZ[RANGE]
    lat, r = run(case, dev)
    assert torch.isfinite(r.logq).all() and torch.isfinite(r.logz64).all()
    check(case, lat, r)
    assert len({tuple(w["arcs"]) for per in reference_walks(case) for w in per}) > len(case.lats)  # the draws differ


def test_single_position(dev):
    (case,) = single_position_cases()
    live = [bool(np.isfinite(smp.logz)) for smp in samplers(case)]
    assert live == [False] * 5 + [True]
    lat, r = run(case, dev)
    check(case, lat, r)
    assert torch.all(r.lengths[-1] == 1)


# ----------------------------------------------------------------------------- wrappers
def test_wrapper_errors_raise_before_any_launch(dev):
    lats = small6()[:3]
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = torch.zeros(lat.vocab, device=dev)
    good = torch.zeros(3, 6, lat.vocab, device=dev)
    for bad in (torch.zeros(3, 4, 7, device=dev), torch.zeros(3, 6, device=dev), torch.zeros(2, 4, 6, device=dev), np.zeros((3, 4, 6), np.float32)):
        with pytest.raises(ValueError):
            ops.positional_sample_paths(lat, theta, 4, good, uniforms=bad)
    for k in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            ops.positional_sample_paths(lat, theta, k, good)
    with pytest.raises(ValueError):
        ops.positional_sample_paths(lat, theta, 4, good.cpu())
    with pytest.raises(ValueError):
        ops.positional_sample_paths(lat, theta.cpu(), 4, good)
    with pytest.raises(ValueError):
        ops.positional_sample_paths(lat, theta, 4, good, T=5)
    marks = torch.zeros(3, 4, 6, dtype=torch.int32, device=dev)
    for bad in (marks[:2], marks[:, :, :5], marks[0], marks.float(), marks[:, :0]):
        with pytest.raises(ValueError):
            ops.positional_score_paths(lat, theta, bad, good)
    with pytest.raises(ValueError):
        ops.positional_score_paths(lat, theta, marks, good.cpu())
    r = ops.positional_sample_paths(lat, theta, 4, good, want_arcs=False)
    assert r.arcs is None and r.paths.shape == (3, 4, 6) and r.logz64.dtype == torch.float64

"""swor.positional_sample (nfst_positional_swor: k distinct paths per lattice drawn without replacement under positional
scores and a length budget) against the float64 NumPy restatement of tests/positional_swor_ref.py, which is fed NumPy
beta rows of its own, not the kernel's.

Lattices whose reference margin exceeds positional_swor_ref.DECIDED are compared as a map from path to (length, marks,
arcs, logp, gumbel), with kappa, n_paths and the output order; tests/test_positional_swor_cpu.py proves on the reference
alone that no comparison leaves out more than 1 % of its lattices and that the cases are what they claim to be."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from nfst_amd import _lib, ops, swor, synth
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from tests import edge_cases as E
from tests import positional_ref as P
from tests import positional_swor_ref as Q
from tests import swor_ref as R

pytestmark = pytest.mark.gpu
PAD = synth.PAD
NEG = -np.inf
G_TOL = Q.DECIDED / 10
TOLQ = 2e-6  # the project's tolerance on a float32 log-probability, times max(1, |.|)
ERRORS = {"gumbel": 0.0}  # the largest |G_gpu - G_ref| over decided lattices seen by this module


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _sample(case, dev, lat, k, pos, u=None, T=None, **kw):
    return swor.positional_sample(lat, _t(case.theta, dev), k, _t(pos, dev), T=T, arc_scores=_t(case.asc, dev), uniforms=_t(u, dev), pad=PAD,
                                  **kw)


def _run(name, T, k, dev, lat=None, **kw):
    """(case, lat, result, references) of a case of swor_ref.cases() at budget T."""
    case, pos, u, refs = Q.references(name, T, k)
    lat = lat or LatticeBatch.from_synth(case.lats, device=dev, **case.opts)
    return case, lat, _sample(case, dev, lat, k, pos, u, **kw), refs


def _np(r):
    return {f: (None if v is None else v.cpu().numpy()) for f, v in r._asdict().items()}


def _check(tag, lat, lats, r, refs, k, T):
    o = _np(r)
    assert o["paths"].shape == o["arcs"].shape == (len(lats), k, T)
    left_out = 0
    for b, (l, ref) in enumerate(zip(lats, refs)):
        n = int(o["n_paths"][b])
        # the layout holds for every lattice, decided or not
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
        if not Q.decided(ref):
            left_out += 1
            continue
        assert n == ref["n_paths"], (tag, b, k)
        for j, p in enumerate(ref["arcs"]):
            assert tuple(p) in got, (tag, b, k, j)
            i = got[tuple(p)]
            assert i == j, (tag, b, k, j)  # ranked by gumbel as the reference ranks them
            assert np.array_equal(o["paths"][b, i, :len(p)], l.label[p]), (tag, b, k, j)
            assert abs(float(o["logp"][b, i]) - float(ref["logp"][j])) <= 1e-6, (tag, b, k, j)
            err = abs(float(o["gumbel"][b, i]) - float(ref["gumbel"][j]))
            ERRORS["gumbel"] = max(ERRORS["gumbel"], err)
            assert err <= G_TOL, (tag, b, k, j, err)
        if ref["kappa"] == NEG:
            assert o["kappa"][b] == NEG, (tag, b, k)
        else:
            err = abs(float(o["kappa"][b]) - ref["kappa"])
            ERRORS["gumbel"] = max(ERRORS["gumbel"], err)
            assert err <= G_TOL, (tag, b, k, err)
    assert left_out <= Q.CAP * len(lats), (tag, k, left_out)
    print(f"{tag} T={T} k={k}: largest |G_gpu - G_ref| so far {ERRORS['gumbel']:.3e}")


# ----------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("name", list(R.cases()))
def test_against_the_reference(dev, name):
    """Every case of swor_ref.cases() under per-lattice position scores with entries at -inf, at the longest, a middle
    and the shortest path length of the batch, at each of the case's ks."""
    lat = None
    for T in Q.case_budgets(name):
        for k in R.cases()[name]().ks:
            case, lat, r, refs = _run(name, T, k, dev, lat=lat)
            _check(case.tag, lat, case.lats, r, refs, k, T)
            logz = r.logz.cpu().numpy()
            assert all((ref["n_paths"] > 0) == bool(np.isfinite(logz[b])) for b, ref in enumerate(refs))


def test_candidates_beyond_the_lds_cap_use_the_workspace(dev):
    """The over-cap lattice lists 7744 candidates in a step at k = 64, more than the keys LDS holds, and is decided."""
    case, lat, r, refs = _run("star", 5, 64, dev)
    assert refs[1]["max_candidates"] > ops.beam_lds_candidates() and Q.decided(refs[1]) and int(r.n_paths[1]) == 64
    assert 64 * lat.vocab > ops.beam_lds_candidates()  # (the workspace has the spill part)


def test_shared_table_and_no_table(dev):
    """One [T, V] table for the batch gives the bits of the same table repeated per lattice and what the restatement
    gives; pos = None with T >= the longest path and with a T that cuts paths off follow the restatement too."""
    case = R.cases()["mixed"]()
    lat = LatticeBatch.from_synth(case.lats, device=dev)
    es = case.scores()
    k = 7
    for T, with_pos in ((45, True), (90, False), (22, False)):
        table = Q.pos_for(case, T)[2] if with_pos else None
        pos = None if table is None else np.stack([table] * len(case.lats))
        u = case.uniforms(k, T)
        betas = Q.beta_rows(case, T, pos, with_pos=with_pos)
        refs = [Q.search(l, es[b], table, betas[b][0], betas[b][1], k, T, u[b]) for b, l in enumerate(case.lats)]
        r = _sample(case, dev, lat, k, table, u, T=T)
        _check(f"mixed shared={with_pos}", lat, case.lats, r, refs, k, T)
        if with_pos:
            r2 = _sample(case, dev, lat, k, pos, u)
            _same(_bits(r), _bits(r2))
        else:  # (without -inf scores only the budget drops candidates: lattice 2 has paths of 20 to 90 arcs and draws
            # some of 27 when nothing holds it back; T = 22 cuts those off)
            assert all(ref["n_paths"] == 7 for ref in refs[:5]) and all((ref["dropped"] > 0) == (T == 22 and b == 2) for b, ref in enumerate(refs))
            assert max(len(a) for a in refs[2]["arcs"]) == (27 if T == 90 else 22)


def test_budget_at_and_below_the_shortest_path(dev):
    """T is lattice 0's shortest path and below that of the other three: lattice 0 draws paths of exactly T arcs after T
    steps, dropping the candidates that cannot finish; the others are empty and disturb nobody."""
    case0 = R.cases()["weighted"]()
    T = Q.budgets(case0.lats)[2]
    case, lat, r, refs = _run("weighted", T, 64, dev)
    o = _np(r)
    assert Q.decided(refs[0]) and refs[0]["dropped"] > 0 and refs[0]["steps"] == T
    assert o["n_paths"].tolist() == [64, 0, 0, 0] and np.all(o["lengths"][0] == T)
    for b in (1, 2, 3):
        assert o["kappa"][b] == NEG and np.all(o["lengths"][b] == 0) and np.all(o["paths"][b] == PAD) and np.all(o["arcs"][b] == -1)
        assert np.all(o["logp"][b] == NEG) and np.all(o["gumbel"][b] == NEG) and r.logz[b] == NEG
    lw = swor.log_weights(r).cpu().numpy()
    assert np.all(lw[1:] == NEG) and np.all(np.isfinite(lw[0]))
    _check(case.tag, lat, case.lats, r, refs, 64, T)


def test_finished_slots_wait_at_the_sink(dev):
    """The edit lattice's paths differ in length: a slot that reached the sink is carried through the later steps."""
    T = Q.case_budgets("mixed")[0]
    case, lat, r, refs = _run("mixed", T, 20, dev)
    lens = r.lengths.cpu().numpy()[3]
    assert len(set(lens[:int(r.n_paths[3])].tolist())) > 1
    assert Q.decided(refs[3]) and refs[3]["steps"] == lens.max() < T


def test_exact_ties_go_to_the_earlier_flat_index(dev):
    """Every label at -0.25, every position score at -0.5 and every uniform 0.5: states that look alike carry the same
    beta bits in either backward pass, whole steps tie, below and above 256 candidates and beyond the LDS cap, and the op
    keeps what the restatement keeps: the first k of the flat index, ranked by slot."""
    case = R.tie_case()
    lat = LatticeBatch.from_synth(case.lats, device=dev)
    T = 5
    pos = np.full((len(case.lats), T, 256), -0.5, np.float32)
    betas = Q.beta_rows(case, T, pos)
    es = case.scores()
    for k in case.ks:
        u = case.uniforms(k, T)
        r = _sample(case, dev, lat, k, pos, u)
        o = _np(r)
        for b, l in enumerate(case.lats):
            ref = Q.search(l, es[b], pos[b], betas[b][0], betas[b][1], k, T, u[b])
            assert ref["margin"] == 0.0 and o["n_paths"][b] == ref["n_paths"] == k
            a0 = int(lat.arc_off[b])
            for j, p in enumerate(ref["arcs"]):
                assert o["lengths"][b, j] == len(p) and np.array_equal(o["arcs"][b, j, :len(p)] - a0, p), (k, b, j)
            assert np.max(np.abs(o["gumbel"][b] - ref["gumbel"])) <= G_TOL and abs(o["kappa"][b] - ref["kappa"]) <= G_TOL


@pytest.mark.parametrize("value", [0.0, float(np.nextafter(np.float32(1), np.float32(0)))])
def test_uniforms_all_on_a_boundary(dev, value):
    """Every uniform 0, or the largest float32 below 1: the noise stays finite (x = u + 2^-25 lies inside (0, 1))."""
    case = R.cases()["weighted"]()
    T, k = Q.budgets(case.lats)[1], 20
    pos = Q.pos_for(case, T)
    lat = LatticeBatch.from_synth(case.lats, device=dev)
    u = np.full((len(case.lats), T, k, R.degree(case.lats)), value, np.float32)
    r = _sample(case, dev, lat, k, pos, u)
    o = _np(r)
    assert np.all(o["n_paths"] == k) and np.all(np.isfinite(o["gumbel"])) and np.all(np.isfinite(o["kappa"]))
    betas = Q.beta_rows(case, T, pos)
    refs = [Q.search(l, e, pos[b], betas[b][0], betas[b][1], k, T, u[b]) for b, (l, e) in enumerate(zip(case.lats, case.scores()))]
    if all(Q.decided(x) for x in refs):  # (equal uniforms tie candidates of equal phi only)
        _check(f"all {value}", lat, case.lats, r, refs, k, T)
    for b in range(len(case.lats)):
        assert len({tuple(o["arcs"][b, i, :o["lengths"][b, i]]) for i in range(k)}) == k
        assert np.all(np.diff(o["gumbel"][b]) <= 0) and o["gumbel"][b, -1] >= o["kappa"][b]


def test_errors(dev):
    """Uniforms narrower than an out-degree set the status word; k, T and the workspace are checked on the host."""
    T = Q.case_budgets("mixed")[1]
    case, pos, u, _ = Q.references("mixed", T, 7)
    lat = LatticeBatch.from_synth(case.lats, device=dev)
    with pytest.raises(_lib.NfstError) as ei:
        _sample(case, dev, lat, 7, pos, u[:, :, :, :2].copy())
    assert ei.value.code == Q.ERR_ARG
    theta = _t(case.theta, dev)
    for k in (0, 65, True, 2.0):
        with pytest.raises(ValueError):
            swor.positional_sample(lat, theta, k, _t(pos, dev))
    for bad_T in (0, T + 1):
        with pytest.raises(ValueError):
            swor.positional_sample(lat, theta, 7, _t(pos, dev), T=bad_T)
    with pytest.raises(ValueError):
        swor.positional_sample(lat, theta, 7, T=0)
    with pytest.raises(ValueError):
        swor.positional_sample(lat, theta, 7, _t(pos, dev), uniforms=_t(u[:, :-1], dev))
    # the C entry point on device pointers: every refusal comes back before a launch and leaves the outputs alone
    B, K = lat.n_lattices, 7
    sc, keep = ops._scores(lat, theta, None)
    bs = C.byref(lat.c_struct())
    full = _lib.lib.nfst_positional_swor_ws_bytes(bs, T, K)
    ws = torch.empty(full, dtype=torch.uint8, device=dev)
    pt = _t(pos, dev)
    z = torch.full((B,), 7.0, dtype=torch.float64, device=dev)
    paths = torch.full((B, K, T), -7, dtype=torch.int32, device=dev)
    lens, npt = torch.full((B, K), -7, dtype=torch.int32, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev)
    logp = torch.zeros((B, K), dtype=torch.float32, device=dev)
    gum, kappa = torch.zeros((B, K), dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def call(k=K, T=T, wsb=full):
        return _lib.lib.nfst_positional_swor(bs, C.byref(sc), pt.data_ptr(), T * lat.vocab, T, k, None, 0, 0, PAD, ws.data_ptr(), wsb,
                                             z.data_ptr(), None, paths.data_ptr(), None, lens.data_ptr(), logp.data_ptr(), gum.data_ptr(),
                                             kappa.data_ptr(), npt.data_ptr(), status.data_ptr(), ops._stream())

    assert call(k=0) == -1 and call(k=65) == -6 and call(T=0) == -1 and call(wsb=full - 1) == -1
    torch.cuda.synchronize()
    assert bool((paths == -7).all()) and bool((npt == -7).all()) and bool((z == 7.0).all()) and int(status) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((npt >= 0).all()) and int(status) == 0


# ----------------------------------------------------------------------------- identities
def test_logp_is_the_forced_score_minus_log_z(dev):
    for name in ("mixed_per_lattice", "weighted"):
        T = Q.case_budgets(name)[1]
        case, lat, r, _ = _run(name, T, 7, dev)
        pos = _t(Q.references(name, T, 7)[1], dev)
        score, _, lens = ops.positional_score_paths(lat, _t(case.theta, dev), r.paths, pos, arc_scores=_t(case.asc, dev))
        ok = (torch.arange(7, device=dev)[None, :] < r.n_paths[:, None]).cpu().numpy()
        assert ok.any() and torch.equal(lens[torch.from_numpy(ok).to(dev)], r.lengths[torch.from_numpy(ok).to(dev)])
        want = (score.double() - r.logz.double()[:, None]).cpu().numpy()
        got = r.logp.double().cpu().numpy()
        assert np.all(np.abs(got - want)[ok] <= TOLQ * np.maximum(1.0, np.abs(want[ok])))


def test_every_admitted_path_drawn_is_exact(dev):
    """k at least the number of admitted paths: kappa = -inf, the probabilities sum to 1 and the Horvitz-Thompson
    estimate of a cost summed over (position, label) is ops.positional_expectation's."""
    l = R.small_lattice()
    lats = [l] * 3
    theta = R.small_theta()
    lat = LatticeBatch.from_synth(lats, device=dev)
    for T, n in ((4, 2), (5, 4), (6, 6)):
        rng = np.random.default_rng([41, T])
        pos = rng.normal(0.0, 1.0, size=(3, T, 16)).astype(np.float32)
        cost = rng.normal(0.0, 1.0, size=(3, T, 16)).astype(np.float32)
        r = swor.positional_sample(lat, _t(theta, dev), 8, _t(pos, dev), seed=T, pad=PAD)
        assert r.n_paths.tolist() == [n] * 3 and bool(torch.all(r.kappa == NEG))
        assert float((torch.exp(r.logp.double()).sum(dim=1) - 1.0).abs().max()) <= 1e-5
        t_idx = torch.arange(T, device=dev)[None, None, :].expand(3, 8, T)
        b_idx = torch.arange(3, device=dev)[:, None, None].expand(3, 8, T)
        on = r.arcs >= 0
        per = torch.where(on, _t(cost, dev)[b_idx, t_idx, r.paths.long().clamp(0, 15)], torch.zeros((), device=dev)).double().sum(dim=2)
        est = swor.expectation(r, per).cpu().numpy()
        want = ops.positional_expectation(lat, _t(theta, dev), _t(pos, dev), pos_values=_t(cost, dev)).double().cpu().numpy()
        assert np.all(np.abs(est - want) <= 1e-5 * np.maximum(1.0, np.abs(want))), (T, est, want)


# ----------------------------------------------------------------------------- determinism
def _bits(r):
    return [None if v is None else v.cpu().numpy().copy() for v in r[:8]]


def _same(x, y, rows=None, arc_shift=None):
    for i, (a, b) in enumerate(zip(x, y)):
        if rows is not None:
            a, b = a[:rows], b[:rows]
        if i == 1 and arc_shift is not None:  # arc ids are canonical in the batch: they move with the lattice
            a, b = np.where(a >= 0, a - arc_shift[0][:len(a), None, None], -1), np.where(b >= 0, b - arc_shift[1][:len(b), None, None], -1)
        assert np.array_equal(a, b, equal_nan=True), i


def test_two_launches_and_a_permuted_batch(dev):
    T, k = Q.case_budgets("mixed")[1], 20
    case, lat, r, _ = _run("mixed", T, k, dev)
    _, _, r2, _ = _run("mixed", T, k, dev, lat=lat)
    _same(_bits(r), _bits(r2))
    perm = [4, 0, 5, 2, 1, 3]
    _, pos, u, _ = Q.references("mixed", T, k)
    lat_p = LatticeBatch.from_synth([case.lats[i] for i in perm], device=dev)
    rp = _sample(case, dev, lat_p, k, pos[perm], u[perm])
    off, off_p = np.asarray(lat.arc_off)[perm], np.asarray(lat_p.arc_off)
    _same([x[perm] for x in _bits(r)], _bits(rp), arc_shift=(off, off_p))


def test_packings_give_the_same_bits(dev):
    """Philox noise is keyed by (lattice, step, slot, arc rank): a lattice draws the same paths under every packing of
    the tile programs, with its arc records staged in LDS or not, and with or without chunked programs."""
    case, lat, r, _ = _run("star", 5, 64, dev, seed=3)
    base = None
    pos = Q.references("star", 5, 64)[1]
    for opts in (E.STAR_PACKINGS[0], E.STAR_PACKINGS[2], E.STAR_PACKINGS[8]):
        lat = LatticeBatch.from_synth(case.lats, device=dev, **opts)
        got = _bits(_sample(case, dev, lat, 64, pos, seed=3))
        base = base or got
        _same(base, got)
    assert base[6].tolist() == [64, 64]
    # staged and unstaged: the small lattices alone, and beside one whose arc records do not fit in LDS
    lats = [dataclasses.replace(R.small_lattice(), vocab=E.POS_V), E.pos_neighbour()]
    big = E.pos_large("big")
    T = 12
    rng = np.random.default_rng(61)
    theta = rng.normal(-1.0, 0.8, size=E.POS_V).astype(np.float32)
    pos = rng.normal(0.0, 1.0, size=(3, T, E.POS_V)).astype(np.float32)
    lat_s = LatticeBatch.from_synth(lats, device=dev)
    lat_u = LatticeBatch.from_synth(lats + [big], device=dev)
    assert ops.positional_plan(lat_s)[1] is True and ops.positional_plan(lat_u)[1] is False
    rs = swor.positional_sample(lat_s, _t(theta, dev), 5, _t(pos[:2], dev), seed=8, pad=PAD)
    ru = swor.positional_sample(lat_u, _t(theta, dev), 5, _t(pos, dev), seed=8, pad=PAD)
    assert int(rs.n_paths.min()) >= 1
    _same(_bits(rs), _bits(ru), rows=2, arc_shift=(np.asarray(lat_s.arc_off), np.asarray(lat_u.arc_off)))
    # with and without chunked programs
    snips = synth.snips_shaped_batch(4, vocab=250)
    T = max(P.min_max_len(l)[1] for l in snips)
    theta = rng.normal(-1.0, 0.8, size=250).astype(np.float32)
    pos = rng.normal(0.0, 1.0, size=(T, 250)).astype(np.float32)
    plain = LatticeBatch.from_synth(snips).to(dev, auto_chunks=False)
    host_lat = LatticeBatch.from_synth(snips)
    assert host_lat.build_chunks(force=True)
    chunked = host_lat.to(dev)
    assert chunked.chunks is not None and plain.chunks is None
    r1 = swor.positional_sample(plain, _t(theta, dev), 4, _t(pos, dev), seed=9, pad=PAD)
    r2 = swor.positional_sample(chunked, _t(theta, dev), 4, _t(pos, dev), seed=9, pad=PAD)
    assert int(r1.n_paths.min()) >= 1
    _same(_bits(r1), _bits(r2))


def test_philox(dev):
    T = Q.case_budgets("mixed")[1]
    case, pos, _, _ = Q.references("mixed", T, 7)
    lat = LatticeBatch.from_synth(case.lats, device=dev)
    a, b, c = (_sample(case, dev, lat, 7, pos, seed=s) for s in (5, 5, 6))
    _same(_bits(a), _bits(b))
    assert not torch.equal(a.paths, c.paths)
    o = _np(a)
    for bb in range(lat.n_lattices):
        n = int(o["n_paths"][bb])
        assert len({tuple(o["arcs"][bb, i, :o["lengths"][bb, i]]) for i in range(n)}) == n
        assert np.all(np.diff(o["gumbel"][bb, :n]) <= 0) and (n == 0 or o["gumbel"][bb, n - 1] >= o["kappa"][bb])


@pytest.mark.parametrize("k", [1, 3])
def test_philox_frequencies(dev, k):
    """The small lattice 2048 times in one batch at T = 5 under one [T, V] table: the frequency of every admitted path
    among the drawn sets against its exact inclusion probability (0.05 is 4.5 binomial standard deviations), and the
    Horvitz-Thompson estimate of a value that does not decompose within 5 of its own standard errors."""
    T = 5
    l = R.small_lattice()
    e = R.arc_score32(l, R.small_theta())
    pos = Q.small_pos(T)
    probs = Q.path_probs(l, e, pos, T)
    keys = list(probs)
    p = np.array([probs[a] for a in keys])
    want = p if k == 1 else R.inclusion_probs(p, k)
    lat = LatticeBatch.from_synth([l] * R.SMALL_COPIES, device=dev)
    r = swor.positional_sample(lat, _t(R.small_theta(), dev), k, _t(pos, dev), seed=17, pad=PAD)
    o = _np(r)
    assert np.all(o["n_paths"] == k) and len(keys) == 4
    rel = o["arcs"] - np.asarray(lat.arc_off)[:, None, None]
    count = {a: 0 for a in keys}
    vals = np.zeros((R.SMALL_COPIES, k))
    for b in range(R.SMALL_COPIES):
        for i in range(k):
            a = tuple(rel[b, i, :o["lengths"][b, i]])
            count[a] += 1  # (a path beyond the budget would be a KeyError)
            vals[b, i] = Q.small_value(l, a)
    freq = np.array([count[a] for a in keys]) / R.SMALL_COPIES
    assert np.max(np.abs(freq - want)) <= 0.05, (freq, want)
    est = swor.expectation(r, torch.from_numpy(vals)).cpu().numpy()
    exact = sum(Q.small_value(l, a) * q for a, q in probs.items())
    assert abs(est.mean() - exact) <= 5 * est.std(ddof=1) / np.sqrt(len(est))


# ----------------------------------------------------------------------------- log-probabilities and their gradient
@pytest.mark.parametrize("name,shared", [("mixed_per_lattice", False), ("weighted", True)])
def test_log_prob_and_its_gradient(dev, name, shared):
    """swor.positional_log_prob repeats r.logp (to float32 rounding of the path score and of log Z_T) and its gradient
    is the path's (position, label) / arc / label counts minus pos_post / arc_post / sum_t pos_post of
    ops.positional_forward_backward."""
    k, T = 7, Q.case_budgets(name)[1]
    case, pos_np, u, _ = Q.references(name, T, k)
    pos_np = pos_np[0] if shared else pos_np
    lat = LatticeBatch.from_synth(case.lats, device=dev)
    r = _sample(case, dev, lat, k, pos_np, u)
    B, V = lat.n_lattices, lat.vocab
    theta = _t(case.theta, dev).requires_grad_(True)
    pos = _t(pos_np, dev).requires_grad_(True)
    asc0 = case.asc if case.asc is not None else np.zeros(lat.total_arcs, np.float32)
    asc = _t(asc0, dev).requires_grad_(True)
    lp = swor.positional_log_prob(lat, theta, r, pos, arc_scores=asc)
    ok = torch.arange(k, device=dev)[None, :] < r.n_paths[:, None]
    assert bool(ok.any()) and bool(torch.all(lp.detach()[~ok] == NEG)) and bool(torch.all(r.logp[~ok] == NEG))
    score = ops.positional_score_paths(lat, theta.detach(), r.paths, pos.detach(), arc_scores=asc.detach())[0]
    size = float(score[ok].abs().max()) + float(r.logz[torch.isfinite(r.logz)].abs().max())
    assert float((lp.detach() - r.logp)[ok].abs().max()) <= 4 * size * 2.0 ** -23
    g = torch.from_numpy(np.random.default_rng(3).normal(size=(B, k)).astype(np.float32)).to(dev) * ok
    (torch.where(ok, lp, torch.zeros_like(lp)) * g).sum().backward()
    fb = ops.positional_forward_backward(lat, theta.detach(), pos.detach(), arc_scores=asc.detach(), want_arc_posterior=True)
    arcs, gn = r.arcs.cpu().numpy(), g.cpu().numpy().astype(np.float64)
    gsum = gn.sum(axis=1)
    pp = fb.pos_posterior.double().cpu().numpy()
    want_pos = -pp * gsum[:, None, None]
    want_theta = -pp.sum(axis=1) * gsum[:, None]
    want_arc = -fb.arc_posterior.double().cpu().numpy() * gsum[lat.arc_lattice().cpu().numpy()]
    label = lat.arc_label.cpu().numpy()
    for b in range(B):
        for i in range(k):
            for t, a in enumerate(arcs[b, i]):
                if a >= 0:
                    want_arc[a] += gn[b, i]
                    want_theta[b, label[a]] += gn[b, i]
                    want_pos[b, t, label[a]] += gn[b, i]
    if case.theta.ndim == 1:
        want_theta = want_theta.sum(axis=0)
    if shared:
        want_pos = want_pos.sum(axis=0)
    assert np.max(np.abs(asc.grad.double().cpu().numpy() - want_arc)) <= 1e-5
    assert np.max(np.abs(theta.grad.double().cpu().numpy() - want_theta)) <= 1e-5
    assert np.max(np.abs(pos.grad.double().cpu().numpy() - want_pos)) <= 1e-5
    # without pos_scores: T comes from the paths, the gradient reaches theta
    r0 = swor.positional_sample(lat, theta.detach(), 3, T=T, arc_scores=asc.detach(), seed=2, pad=PAD)
    lp0 = swor.positional_log_prob(lat, theta, r0, arc_scores=asc.detach())
    ok0 = torch.arange(3, device=dev)[None, :] < r0.n_paths[:, None]
    assert float((lp0.detach() - r0.logp)[ok0].abs().max()) <= 4 * size * 2.0 ** -23


def test_scorer_entry_point(dev):
    T = Q.case_budgets("mixed")[1]
    case, pos, _, _ = Q.references("mixed", T, 7)
    lat = LatticeBatch.from_synth(case.lats, device=dev)
    scorer = LatticeScorer(E.V_MIXED, theta=torch.from_numpy(case.theta)).to(dev).set_lattice(lat)
    a = scorer.positional_sample_without_replacement(_t(pos, dev), 7, seed=9)
    b = _sample(case, dev, lat, 7, pos, seed=9)
    _same(_bits(a), _bits(b))

"""The NumPy restatement of the draws without replacement under positional scores (tests/positional_swor_ref.py), which
the GPU tests of ``swor.positional_sample`` rely on: the distribution of the drawn sets against path enumeration under
the budget, that no search outruns T, that the restatement is ``swor_ref.search`` where the two ops coincide, the cap on
undecided lattices for every comparison of tests/test_gpu_positional_swor.py (a condition on the inputs, held on the
reference alone), and the C entry points' host-side checks, exports and workspace formula."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import edge_cases as E
from tests import positional_ref as P
from tests import positional_sample_ref as PS
from tests import positional_swor_ref as Q
from tests import swor_ref as R

NEG = -np.inf
ERR_ARG, ERR_LIMIT = -1, -6  # (include/nfst_hip.h)
NAMES = list(R.cases())


def _as_result(refs, k):
    from nfst_amd import swor

    B = len(refs)
    logp, gum = np.full((B, k), NEG, np.float32), np.full((B, k), NEG)
    for b, r in enumerate(refs):
        logp[b, :r["n_paths"]], gum[b, :r["n_paths"]] = r["logp"], r["gumbel"]
    t = torch.from_numpy
    return swor.SworResult(None, None, None, t(logp), t(gum), t(np.array([r["kappa"] for r in refs])),
                           t(np.array([r["n_paths"] for r in refs], np.int32)), None)


# ----------------------------------------------------------------------------- the cases of the GPU tests
@pytest.mark.parametrize("name", NAMES)
def test_every_gpu_comparison_stays_within_the_cap(name):
    """Every case of the GPU file (the star and the boundary uniforms included) at each of its budgets and ks: at most
    1 % of the lattices undecided, no status, and no search of more than T steps."""
    ks = R.cases()[name]().ks
    for T in Q.case_budgets(name):
        for k in ks:
            _, _, _, refs = Q.references(name, T, k)
            assert sum(not Q.decided(r) for r in refs) <= Q.CAP * len(refs), (name, T, k)
            assert all(r["status"] == 0 and r["steps"] <= T for r in refs), (name, T, k)
            assert all(len(a) <= T for r in refs for a in r["arcs"])


def test_the_cases_are_what_they_claim():
    from nfst_amd import _lib

    cap = _lib.lib.nfst_beam_lds_candidates()
    # the over-cap lattice lists more candidates than LDS holds in some step at k = 64; the star does not
    assert Q.case_budgets("star") == (5, 4)  # (the over-cap lattice's paths have 5 arcs, the star's 4)
    star = Q.references("star", 5, 64)[3]
    assert star[1]["max_candidates"] > cap >= star[0]["max_candidates"] >= 200
    # the budgets of the mixed batch: the longest path, the single-arc lattice's one arc, and one in between
    hi, mid, lo = Q.case_budgets("mixed")
    lens = [P.min_max_len(l) for l in E.mixed_batch()]
    assert hi == max(m[1] for m in lens) and lo == 1 and lo < mid < hi
    # the weighted batch at its smallest budget: T is lattice 0's shortest path, so every drawn path has exactly T arcs and
    # most candidates are dropped; T is below the shortest path of the other three: the empty result beside a neighbour
    case = R.cases()["weighted"]()
    wl = [P.min_max_len(l) for l in case.lats]
    lo = Q.budgets(case.lats)[2]
    assert wl[0][0] == lo and all(m[0] > lo for m in wl[1:])
    at_lo = Q.references("weighted", lo, 64)[3]
    assert [r["n_paths"] for r in at_lo] == [64, 0, 0, 0] and {len(a) for a in at_lo[0]["arcs"]} == {lo} and at_lo[0]["steps"] == lo
    at_hi = Q.references("weighted", Q.budgets(case.lats)[0], 64)[3]
    assert at_lo[0]["dropped"] > 4 * at_hi[0]["dropped"] > 0
    # the edit lattice's paths differ in length: finished slots wait at the sink
    edit = Q.references("mixed", hi, 20)[3][3]
    assert len({len(a) for a in edit["arcs"]}) > 1 and edit["steps"] == max(len(a) for a in edit["arcs"])
    assert len(Q.references("many_small", Q.case_budgets("many_small")[0], 4)[3]) == 330 > 256


# ----------------------------------------------------------------------------- where the two ops coincide
@pytest.mark.parametrize("name,k", [("mixed", 7), ("weighted", 20)])
def test_without_pos_and_budget_it_is_the_plain_search(name, k):
    """Without pos and with T >= the longest path every beta row a search reads is the row of position 0: the
    restatement gives what swor_ref.search gives on that row."""
    case = R.cases()[name]()
    T = Q.budgets(case.lats)[0] + 1
    betas = Q.beta_rows(case, T, with_pos=False)
    u = case.uniforms(k, T)
    es = case.scores()
    for b, l in enumerate(case.lats):
        rows, z = betas[b]
        got = Q.search(l, es[b], None, rows, z, k, T, u[b])
        want = R.search(l, es[b], rows[0], z, k, T, u[b])
        assert got["arcs"] == want["arcs"] and got["n_paths"] == want["n_paths"] > 0
        assert np.array_equal(got["gumbel"], want["gumbel"]) and got["kappa"] == want["kappa"]
        assert np.array_equal(got["logp"], want["logp"]) and got["steps"] == want["steps"]


# ----------------------------------------------------------------------------- the distribution of the drawn set
_SMALL = {}


def _small(T):
    """(lattice, e, pos, {arcs: p_T}, beta rows, log Z_T) of the small lattice at budget T."""
    if T not in _SMALL:
        l = R.small_lattice()
        e = R.arc_score32(l, R.small_theta())
        pos = Q.small_pos(T)
        rows = PS.beta_rows(l, e.astype(np.float64), pos, T)
        _SMALL[T] = (l, e, pos, Q.path_probs(l, e, pos, T), rows, float(rows[0, 0]))
    return _SMALL[T]


_DRAWS = {}


def _small_draws(T, k):
    if (T, k) not in _DRAWS:
        l, e, pos, _, rows, z = _small(T)
        u = R.uniforms_for([l] * R.SMALL_COPIES, k, 13 + T, T)
        _DRAWS[(T, k)] = [Q.search(l, e, pos, rows, z, k, T, u[b]) for b in range(R.SMALL_COPIES)]
    return _DRAWS[(T, k)]


def test_the_budget_admits_four_and_six_paths():
    for T, n in ((4, 2), (5, 4), (6, 6)):
        l, e, pos, probs, rows, z = _small(T)
        assert len(probs) == n and all(len(a) <= T for a in probs) and abs(sum(probs.values()) - 1.0) <= 1e-12
        # log Z_T of the beta rows is the enumeration's
        sc = [sum(float(e[a]) + float(pos[t, l.label[a]]) for t, a in enumerate(p)) for p in probs]
        assert abs(z - P.logsumexp(sc)) <= 1e-12


@pytest.mark.parametrize("T", [5, 6])
@pytest.mark.parametrize("k", [1, 3])
def test_frequencies_follow_the_inclusion_probabilities(T, k):
    l, _, _, probs, _, _ = _small(T)
    keys = list(probs)
    p = np.array([probs[a] for a in keys])
    want = p if k == 1 else R.inclusion_probs(p, k)
    assert abs(want.sum() - k) <= 1e-12
    draws = _small_draws(T, k)
    assert all(r["n_paths"] == k and len({tuple(a) for a in r["arcs"]}) == k and r["steps"] <= T for r in draws)
    assert all(tuple(a) in probs for r in draws for a in r["arcs"])  # nothing beyond the budget is ever drawn
    freq = np.array([sum(tuple(a) == key for r in draws for a in r["arcs"]) for key in keys]) / len(draws)
    assert np.max(np.sqrt(want * (1 - want) / len(draws))) <= 0.0112  # (0.05 is 4.5 binomial standard deviations)
    assert np.max(np.abs(freq - want)) <= 0.05, (freq, want)


@pytest.mark.parametrize("T", [5, 6])
@pytest.mark.parametrize("k", [1, 3])
def test_estimate_of_a_value_that_does_not_decompose_is_unbiased(T, k):
    from nfst_amd import swor

    l, _, _, probs, _, _ = _small(T)
    exact = sum(Q.small_value(l, a) * p for a, p in probs.items())
    draws = _small_draws(T, k)
    vals = np.zeros((len(draws), k))
    for b, r in enumerate(draws):
        vals[b, :r["n_paths"]] = [Q.small_value(l, a) for a in r["arcs"]]
    est = swor.expectation(_as_result(draws, k), torch.from_numpy(vals)).numpy()
    se = est.std(ddof=1) / np.sqrt(len(est))
    assert se > 0 and abs(est.mean() - exact) <= 5 * se, (est.mean(), exact, se)


@pytest.mark.parametrize("T", [5, 6])
def test_k_at_least_the_admitted_paths_is_exact(T):
    from nfst_amd import swor

    l, e, pos, probs, rows, z = _small(T)
    for k in (len(probs), 10):
        u = R.uniforms_for([l], k, 12, T)
        r = Q.search(l, e, pos, rows, z, k, T, u[0])
        assert sorted(tuple(a) for a in r["arcs"]) == sorted(probs) and r["n_paths"] == len(probs)
        assert r["kappa"] == NEG and r["steps"] <= T
        w64 = np.exp(r["logp64"])
        p64 = np.array([probs[tuple(a)] for a in r["arcs"]])
        assert np.max(np.abs(w64 - p64)) <= 1e-12 and abs(w64.sum() - 1.0) <= 1e-12
        vals = np.zeros((1, k))
        vals[0, :r["n_paths"]] = [Q.small_value(l, a) for a in r["arcs"]]
        exact = sum(Q.small_value(l, a) * q for a, q in probs.items())
        assert abs(float((w64 * vals[0, :r["n_paths"]]).sum()) - exact) <= 1e-12
        assert abs(float(swor.expectation(_as_result([r], k), torch.from_numpy(vals))[0]) - exact) <= 1e-5


def test_budget_below_the_shortest_path_is_the_empty_result():
    l = R.small_lattice()
    e = R.arc_score32(l, R.small_theta())
    rows = PS.beta_rows(l, e.astype(np.float64), None, 3)
    assert rows[0, 0] == NEG
    r = Q.search(l, e, None, rows, rows[0, 0], 3, 3, np.zeros((3, 3, 3), np.float32))
    assert r["n_paths"] == 0 and r["kappa"] == NEG and r["arcs"] == []


# ----------------------------------------------------------------------------- the C entry points
def test_exports_are_declared():
    from nfst_amd import _lib

    assert {"nfst_positional_swor", "nfst_positional_swor_ws_bytes"} <= set(_lib.EXPORTS)
    with open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "nfst_hip.h")) as f:
        h = f.read()
    assert int(re.search(r"#define\s+NFST_ABI_VERSION\s+(\d+)", h).group(1)) == 7  # functions only added
    assert re.search(r"\bint\s+nfst_positional_swor\s*\(", h) and re.search(r"\bint64_t\s+nfst_positional_swor_ws_bytes\s*\(", h)


def test_workspace_formula():
    """The NFST_POS_WS_SAMPLE part of nfst_positional_ws_bytes, then nfst_swor's parts with max_len = T."""
    from nfst_amd import _lib
    from nfst_amd.lattice import LatticeBatch

    for lats in (E.mixed_batch()[:3], [E.star(), R.over_cap_lattice()]):
        lat = LatticeBatch.from_synth(lats)
        bs = C.byref(lat.c_struct())
        for k, T in ((1, 1), (7, 13), (64, 40)):
            want = _lib.lib.nfst_positional_ws_bytes(bs, T, _lib.POS_WS_SAMPLE) + _lib.lib.nfst_swor_ws_bytes(bs, k, T)
            assert want % 256 == 0 and _lib.lib.nfst_positional_swor_ws_bytes(bs, T, k) == want, (k, T)
        assert _lib.lib.nfst_positional_swor_ws_bytes(bs, 4, 0) == ERR_ARG
        assert _lib.lib.nfst_positional_swor_ws_bytes(bs, 4, 65) == ERR_LIMIT
        assert _lib.lib.nfst_positional_swor_ws_bytes(bs, 0, 4) == ERR_ARG


def test_argument_checks_return_before_any_launch():
    from nfst_amd import _lib
    from nfst_amd.lattice import LatticeBatch

    lat = LatticeBatch.from_synth(E.mixed_batch()[:3])  # host-packed: the checks run before anything touches a device
    assert lat.device.type == "cpu"
    V, B, T, K, D = lat.vocab, lat.n_lattices, 6, 4, 8
    theta = np.zeros(V, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    lib = _lib.lib
    bs = C.byref(lat.c_struct())
    full = lib.nfst_positional_swor_ws_bytes(bs, T, K)
    ws = np.zeros(full // 8 + 2, np.float64)
    pos = np.zeros((B, T, V), np.float32)
    u = np.zeros((B, T, K, D), np.float32)
    z = np.zeros(B, np.float64)
    paths, arcs = np.zeros((B, K, T), np.int32), np.zeros((B, K, T), np.int32)
    lens, logp, gum = np.zeros((B, K), np.int32), np.zeros((B, K), np.float32), np.zeros((B, K), np.float64)
    kappa, npt, status = np.zeros(B, np.float64), np.zeros(B, np.int32), np.zeros(1, np.int32)
    p = lambda a: None if a is None else a.ctypes.data

    def call(k=K, T=T, pos=pos, stride=T * V, u=None, D=0, ws=ws, wsb=full, scores=C.byref(sc), z=z, paths=paths, arcs=arcs, lens=lens,
             logp=logp, gum=gum, kappa=kappa, npt=npt, status=status):
        return lib.nfst_positional_swor(bs, scores, p(pos), stride, T, k, p(u), D, 0, 0, p(ws), wsb, p(z), None, p(paths), p(arcs),
                                        p(lens), p(logp), p(gum), p(kappa), p(npt), p(status), None)

    assert call(k=0) == ERR_ARG
    assert call(k=-2) == ERR_ARG
    assert call(k=65) == ERR_LIMIT
    assert call(T=0, stride=0) == ERR_ARG
    assert call(stride=T * V - 1) == ERR_ARG
    assert call(ws=None) == ERR_ARG
    assert call(wsb=full - 1) == ERR_ARG
    assert call(k=2 * K) == ERR_ARG  # the workspace of k = 4 is short for k = 8
    assert call(T=T + 1, stride=0) == ERR_ARG  # ... and that of T = 6 for T = 7
    assert call(u=u, D=0) == ERR_ARG
    assert call(u=u, D=-1) == ERR_ARG
    assert call(scores=None) == ERR_ARG
    for name in ("z", "paths", "lens", "logp", "gum", "kappa", "npt", "status"):
        assert call(**{name: None}) == ERR_ARG, name
    assert status[0] == 0 and not paths.any()  # nothing ran


def test_wrappers_validate_before_any_launch():
    from nfst_amd import swor
    from nfst_amd.lattice import LatticeBatch
    from nfst_amd.scorers import LatticeScorer

    lat = LatticeBatch.from_synth(E.mixed_batch()[:3])
    theta = torch.zeros(lat.vocab)
    with pytest.raises(RuntimeError):  # a host batch: no CPU fallback
        swor.positional_sample(lat, theta, 4)
    assert hasattr(LatticeScorer, "positional_sample_without_replacement")
    for name in ("positional_sample", "positional_log_prob"):
        assert hasattr(swor, name)

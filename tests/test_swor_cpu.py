"""The NumPy restatement of the draws without replacement (tests/swor_ref.py), which the GPU tests of nfst_amd.swor rely
on: the cap on undecided lattices for every case of tests/test_gpu_swor.py (a condition on the inputs, held on the
reference alone), that the cases are what they claim to be, the distribution of the drawn sets against exact inclusion
probabilities, the Horvitz-Thompson weights, and the C entry points' host-side checks, exports and workspace formula."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import edge_cases as E
from tests import swor_ref as R

NEG = -np.inf
ERR_ARG, ERR_LIMIT = -1, -6  # (include/nfst_hip.h)

_REFS = {}


def _refs(name, k):
    """The references of a case at k, computed once."""
    if (name, k) not in _REFS:
        _REFS[(name, k)] = R.cases()[name]().references(k)
    return _REFS[(name, k)]


def _as_result(refs, k):
    """A swor.SworResult on the host from reference results (the weights and estimates are torch arithmetic)."""
    from nfst_amd import swor

    B = len(refs)
    logp, gum = np.full((B, k), NEG, np.float32), np.full((B, k), NEG)
    for b, r in enumerate(refs):
        logp[b, :r["n_paths"]], gum[b, :r["n_paths"]] = r["logp"], r["gumbel"]
    t = torch.from_numpy
    return swor.SworResult(None, None, None, t(logp), t(gum), t(np.array([r["kappa"] for r in refs])),
                           t(np.array([r["n_paths"] for r in refs], np.int32)), None)


# ----------------------------------------------------------------------------- the cases of the GPU tests
@pytest.mark.parametrize("name", list(R.cases()))
def test_every_gpu_comparison_stays_within_the_cap(name):
    case = R.cases()[name]()
    for k in case.ks:
        refs = _refs(name, k)
        assert sum(not R.decided(r) for r in refs) <= R.CAP * len(refs), (name, k)
        assert all(r["status"] == 0 for r in refs)


def test_the_cases_are_what_they_claim():
    from nfst_amd import _lib

    cap = _lib.lib.nfst_beam_lds_candidates()
    # the over-cap lattice lists more candidates than LDS holds in some step at k = 64, the star and the mixed batch do not
    star = _refs("star", 64)
    assert star[1]["max_candidates"] > cap >= star[0]["max_candidates"] >= 200
    assert 64 * 256 > cap  # (the workspace has room for the keys)
    assert max(r["max_candidates"] for r in _refs("mixed", 64)) <= cap
    # paths of different lengths in one lattice: the edit lattice's finished slots wait at the sink
    edit = _refs("mixed", 20)[3]
    assert len({len(a) for a in edit["arcs"]}) > 1 and edit["steps"] == max(len(a) for a in edit["arcs"])
    # labels at -inf drop candidates; lattices 1 and 3 of the no-path case have no finite path
    assert all(r["dropped"] > 0 for r in _refs("dead_labels", 64))
    nop = _refs("no_path", 7)
    assert [r["n_paths"] for r in nop] == [7, 0, 7, 0, 7]
    # fewer paths than k: everything is drawn, nothing dropped
    _, _, b, n = E.few_paths_case()
    few = _refs("few_paths", 64)[b]
    assert 0 < n < 64 and few["n_paths"] == n and few["kappa"] == NEG
    # more lattices than compute units
    assert len(_refs("many_small", 4)) == 330 > 256


def test_margin_reports_the_smallest_gap():
    """A uniform tensor of one value ties every noise of equal phi: the star's 200 equal arcs are undecided."""
    l = E.star()
    e = R.arc_score32(l, np.full(256, -0.25, np.float32))
    lb, z = R.rounded_beta(l, e)
    r = R.search(l, e, lb, z, 4, 4, np.full((4, 4, 200), 0.5, np.float32))
    assert r["margin"] == 0.0 and not R.decided(r)
    assert [a[1] for a in r["arcs"]] == [1, 2, 3, 4]  # ties go to the earlier flat index


def test_tie_case_ties_and_keeps_the_first_in_flat_order():
    """Every candidate of a step of the tie case has the same perturbed score: the survivors are the first k of the
    flat index, across the 7744 candidates of the over-cap lattice too."""
    case = R.tie_case()
    for k in case.ks:
        star, over = case.references(k)
        assert star["margin"] == 0.0 and over["margin"] == 0.0
        assert [a[1] for a in star["arcs"]] == list(range(1, k + 1))  # the hub's first k arcs
        assert len(set(star["gumbel"])) == 1 and star["kappa"] == star["gumbel"][0]
        rp = R.out_arcs(case.lats[1])
        first_mid = int(case.lats[1].dst[rp[1]])
        assert all(a[1] == rp[1] for a in over["arcs"][:min(k, 121)])  # all through the hub's first arc ...
        assert [a[2] for a in over["arcs"][:min(k, 121)]] == list(range(rp[first_mid], rp[first_mid] + min(k, 121)))  # ... in arc order
        assert over["max_candidates"] == (7744 if k == 64 else k * 121)


# ----------------------------------------------------------------------------- the distribution of the drawn set
def _small():
    l = R.small_lattice()
    e = R.arc_score32(l, R.small_theta())
    probs = R.path_probs(l, e)
    return l, e, probs


_DRAWS = {}


def _small_draws(k):
    if k not in _DRAWS:
        l, e, _ = _small()
        lb, z = R.rounded_beta(l, e)
        u = R.uniforms_for([l] * R.SMALL_COPIES, k, 11)
        _DRAWS[k] = [R.search(l, e, lb, z, k, u.shape[1], u[b]) for b in range(R.SMALL_COPIES)]
    return _DRAWS[k]


def test_small_lattice_has_six_to_ten_paths():
    _, _, probs = _small()
    assert 6 <= len(probs) <= 10 and abs(sum(probs.values()) - 1.0) <= 1e-12
    # the binomial standard deviation of every frequency the tests below compare: the bound of 0.05 is 4.5 of them
    p = np.array(list(probs.values()))
    for q in (p, R.inclusion_probs(p, 3)):
        assert np.max(np.sqrt(q * (1 - q) / R.SMALL_COPIES)) <= 0.011


@pytest.mark.parametrize("k", [1, 3])
def test_frequencies_follow_the_inclusion_probabilities(k):
    _, _, probs = _small()
    keys = list(probs)
    p = np.array([probs[a] for a in keys])
    want = p if k == 1 else R.inclusion_probs(p, k)
    assert abs(want.sum() - k) <= 1e-12
    draws = _small_draws(k)
    freq = np.array([sum(tuple(a) == key for r in draws for a in r["arcs"]) for key in keys]) / len(draws)
    assert all(r["n_paths"] == k and len({tuple(a) for a in r["arcs"]}) == k for r in draws)
    assert np.max(np.abs(freq - want)) <= 0.05, (freq, want)


@pytest.mark.parametrize("k", [1, 3])
def test_expectation_of_the_length_is_unbiased(k):
    from nfst_amd import swor

    _, _, probs = _small()
    exact = sum(len(a) * p for a, p in probs.items())
    draws = _small_draws(k)
    lens = np.zeros((len(draws), k))
    for b, r in enumerate(draws):
        lens[b, :r["n_paths"]] = [len(a) for a in r["arcs"]]
    est = swor.expectation(_as_result(draws, k), torch.from_numpy(lens)).numpy()
    se = est.std(ddof=1) / np.sqrt(len(est))
    assert abs(est.mean() - exact) <= 5 * se, (est.mean(), exact, se)
    norm = swor.expectation(_as_result(draws, k), torch.from_numpy(lens), normalize=True).numpy()
    assert np.all((norm >= 4 - 1e-12) & (norm <= 6 + 1e-12))  # a weighted mean of path lengths


def test_k_at_least_the_number_of_paths_is_exact():
    from nfst_amd import swor

    l, e, probs = _small()
    lb, z = R.rounded_beta(l, e)
    for k in (len(probs), 10):
        u = R.uniforms_for([l], k, 12)
        r = R.search(l, e, lb, z, k, u.shape[1], u[0])
        assert sorted(tuple(a) for a in r["arcs"]) == sorted(probs) and r["n_paths"] == len(probs)
        assert r["kappa"] == NEG
        res = _as_result([r], k)
        w = torch.exp(swor.log_weights(res))[0].numpy()
        assert np.array_equal(w[:r["n_paths"]], np.exp(r["logp"].astype(np.float64))) and np.all(w[r["n_paths"]:] == 0)
        # before logp's rounding to float32 the weights are the enumeration's probabilities and sum to 1
        w64 = np.exp(r["logp64"])
        p64 = np.array([probs[tuple(a)] for a in r["arcs"]])
        assert np.max(np.abs(w64 - p64)) <= 1e-12 and abs(w64.sum() - 1.0) <= 1e-12
        assert np.max(np.abs(w[:r["n_paths"]] - p64)) <= 1e-6
        vals = np.zeros((1, k))
        vals[0, :r["n_paths"]] = [len(a) for a in r["arcs"]]
        exact = sum(len(a) * q for a, q in probs.items())
        assert abs(float((w64 * vals[0, :r["n_paths"]]).sum()) - exact) <= 1e-12
        got = float(swor.expectation(res, torch.from_numpy(vals))[0])
        assert abs(got - exact) <= 1e-5


def test_log_weights_against_the_definition():
    from nfst_amd import swor

    for k in (1, 3):
        draws = _small_draws(k)[:64]
        lw = swor.log_weights(_as_result(draws, k)).numpy()
        for b, r in enumerate(draws):
            assert np.allclose(lw[b, :r["n_paths"]], R.log_weights(r), rtol=0, atol=1e-12)
            # w = p / q with q = 1 - exp(-exp(logp - kappa)) in (0, 1]: never below p
            assert np.all(lw[b, :r["n_paths"]] >= r["logp"].astype(np.float64) - 1e-12)
    # far below the threshold q -> exp(logp - kappa): log w -> kappa, with no cancellation
    res = swor.SworResult(None, None, None, torch.tensor([[-80.0, NEG]]), torch.tensor([[1.0, NEG]], dtype=torch.float64),
                          torch.tensor([-3.0], dtype=torch.float64), torch.tensor([1], dtype=torch.int32), None)
    lw = swor.log_weights(res)
    assert abs(float(lw[0, 0]) - (-3.0)) <= 1e-12 and float(lw[0, 1]) == NEG


@pytest.mark.parametrize("name,k", [("mixed", 20), ("weighted", 64), ("few_paths", 64), ("many_small", 4)])
def test_gumbels_are_ranked_and_above_the_threshold(name, k):
    for r in _refs(name, k):
        g = r["gumbel"]
        assert np.all(np.diff(g) <= 0)
        if r["n_paths"]:
            assert g.min() >= r["kappa"]


# ----------------------------------------------------------------------------- the C entry points
def test_exports_are_declared():
    from nfst_amd import _lib

    assert {"nfst_swor", "nfst_swor_ws_bytes"} <= set(_lib.EXPORTS)
    with open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "nfst_hip.h")) as f:
        h = f.read()
    assert int(re.search(r"#define\s+NFST_ABI_VERSION\s+(\d+)", h).group(1)) == 7
    assert re.search(r"\bint\s+nfst_swor\s*\(", h) and re.search(r"\bint64_t\s+nfst_swor_ws_bytes\s*\(", h)


def test_workspace_formula():
    """8 bytes per (lattice, step, slot); 8 k vocab per lattice more when k * vocab exceeds the keys LDS holds; each
    part rounded up to 256 bytes."""
    from nfst_amd import _lib
    from nfst_amd.lattice import LatticeBatch

    up = lambda x: (x + 255) & ~255
    cap = _lib.lib.nfst_beam_lds_candidates()
    for lats in (E.mixed_batch()[:3], [E.star(), R.over_cap_lattice()]):
        lat = LatticeBatch.from_synth(lats)
        bs, B, V = C.byref(lat.c_struct()), lat.n_lattices, lat.vocab
        for k, L in ((1, 1), (7, 13), (64, 40)):
            want = up(8 * B * L * k) + (up(8 * B * k * V) if k * V > cap else 0)
            assert _lib.lib.nfst_swor_ws_bytes(bs, k, L) == want, (k, L)
        assert _lib.lib.nfst_swor_ws_bytes(bs, 0, 4) == ERR_ARG
        assert _lib.lib.nfst_swor_ws_bytes(bs, 65, 4) == ERR_LIMIT
        assert _lib.lib.nfst_swor_ws_bytes(bs, 4, 0) == ERR_ARG
    assert 64 * 64 <= cap < 64 * 256  # the mixed batch never spills at k = 64, the star's batch may


def test_argument_checks_return_before_any_launch():
    from nfst_amd import _lib
    from nfst_amd.lattice import LatticeBatch

    lat = LatticeBatch.from_synth(E.mixed_batch()[:3])  # host-packed: the checks run before anything touches a device
    assert lat.device.type == "cpu"
    V, B, L, K, D = lat.vocab, lat.n_lattices, 6, 4, 8
    theta = np.zeros(V, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    lib = _lib.lib
    bs = C.byref(lat.c_struct())
    full = lib.nfst_swor_ws_bytes(bs, K, L)
    ws = np.zeros(full // 8 + 2, np.float64)
    lb, z = np.zeros(lat.total_rows, np.float32), np.zeros(B, np.float64)
    u = np.zeros((B, L, K, D), np.float32)
    paths, arcs = np.zeros((B, K, L), np.int32), np.zeros((B, K, L), np.int32)
    lens, logp, gum = np.zeros((B, K), np.int32), np.zeros((B, K), np.float32), np.zeros((B, K), np.float64)
    kappa, npt, status = np.zeros(B, np.float64), np.zeros(B, np.int32), np.zeros(1, np.int32)
    p = lambda a: None if a is None else a.ctypes.data

    def call(k=K, L=L, u=None, D=0, ws=ws, wsb=full, scores=C.byref(sc), lb=lb, z=z, paths=paths, arcs=arcs, lens=lens, logp=logp,
             gum=gum, kappa=kappa, npt=npt, status=status):
        return lib.nfst_swor(bs, scores, p(lb), p(z), k, L, p(u), D, 0, 0, p(ws), wsb, p(paths), p(arcs), p(lens), p(logp), p(gum),
                             p(kappa), p(npt), p(status), None)

    assert call(k=0) == ERR_ARG
    assert call(k=-2) == ERR_ARG
    assert call(k=65) == ERR_LIMIT
    assert call(L=0) == ERR_ARG
    assert call(ws=None) == ERR_ARG
    assert call(wsb=full - 1) == ERR_ARG
    assert call(k=2 * K) == ERR_ARG  # the workspace of k = 4 is short for k = 8
    assert call(u=u, D=0) == ERR_ARG
    assert call(u=u, D=-1) == ERR_ARG
    assert call(scores=None) == ERR_ARG
    for name in ("lb", "z", "paths", "lens", "logp", "gum", "kappa", "npt", "status"):
        assert call(**{name: None}) == ERR_ARG, name
    assert status[0] == 0 and not paths.any()  # nothing ran


def test_wrappers_validate_before_any_launch():
    from nfst_amd import swor
    from nfst_amd.lattice import LatticeBatch
    from nfst_amd.scorers import LatticeScorer

    lat = LatticeBatch.from_synth(E.mixed_batch()[:3])
    theta = torch.zeros(lat.vocab)
    with pytest.raises(RuntimeError):  # a host batch: no CPU fallback
        swor.sample(lat, theta, 4)
    assert swor.max_degree(lat) == R.degree(E.mixed_batch()[:3])
    assert hasattr(LatticeScorer, "sample_without_replacement")
    for name in ("sample", "log_weights", "expectation", "log_prob", "SworResult"):
        assert hasattr(swor, name)

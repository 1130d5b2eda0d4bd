"""The float32 NumPy reference of the k-best recursion (tests/kbest_ref.py) that the GPU tests of ops.k_best rely on,
checked against path enumeration and the oracle's Viterbi; the C entry point's argument checks (host side, before any
launch) and the register guard of its sweep kernel."""
import ctypes as C

import numpy as np
import pytest

from nfst_amd import synth
from oracle import oracle as O
from tests import edge_cases as E
from tests import kbest_ref as R

V = 16
NEG = -np.inf
ERR_ARG, ERR_LIMIT = -1, -6  # (include/nfst_hip.h)


def _small_lattices():
    return [
        synth.layered_lattice(11, n_states=10, avg_degree=2.5, vocab=V, width=3, span=2),
        synth.layered_lattice(12, n_states=12, avg_degree=3.0, vocab=V, width=4, span=3),
        synth.layered_lattice(13, n_states=9, avg_degree=2.0, vocab=V, width=1, span=4, weighted=True),
        synth.edit_lattice([6, 7], [8, 9], vocab=V, seed=3),
    ]


def _theta(seed):
    return np.random.default_rng(seed).normal(-1.0, 0.8, size=V).astype(np.float32)


def _check_against_enumeration(l, theta, k, arc_scores=None):
    th, e = R.arc_terms(l, theta, arc_scores)
    sink = l.n_rows - 1
    got = R.k_best(l.n_rows, l.src, l.dst, th, e, k, sink)
    score64 = th.astype(np.float64) + e.astype(np.float64)
    ref = R.enumerate_paths(l.n_rows, l.src, l.dst, score64, sink)
    n = min(k, len(ref))
    assert got["n_paths"] == n == min(k, R.count_finite_paths(l.n_rows, l.src, l.dst, score64, sink))
    assert np.all(got["best"][n:] == NEG)
    ref_scores = np.array([s for s, _ in ref[:n]])
    tol = 1e-5 * np.maximum(1.0, np.abs(ref_scores))
    assert np.all(np.abs(got["best"][:n].astype(np.float64) - ref_scores) <= tol)
    assert np.all(np.diff(got["best"][:n]) <= 0)
    assert len({tuple(p) for p in got["arcs"]}) == n  # distinct
    for j, p in enumerate(got["arcs"]):
        # a real path whose float64 score is the reported one; where it is not the enumeration's j-th path, the two
        # scores lie within 1e-5 (a near tie decided by float32 rounding)
        assert abs(float(score64[p].sum()) - float(got["best"][j])) <= tol[j]
        if p != ref[j][1]:
            assert abs(ref[j][0] - float(score64[p].sum())) <= 2 * tol[j]
    return got


@pytest.mark.parametrize("i", range(4))
@pytest.mark.parametrize("k", [1, 3, 7, 64])
def test_reference_equals_path_enumeration(i, k):
    l = _small_lattices()[i]
    _check_against_enumeration(l, _theta(i), k)


def test_reference_with_arc_scores():
    l = _small_lattices()[2]
    asc = np.random.default_rng(4).normal(0, 0.5, size=l.n_arcs).astype(np.float32)
    _check_against_enumeration(l, _theta(9), 10, asc)


def test_single_path():
    l = synth._finish(4, V, [0, 1, 2], [3, 4, 5], [1, 2, 3])
    got = _check_against_enumeration(l, _theta(1), 5)
    assert got["n_paths"] == 1 and got["arcs"][0] == [0, 1, 2]


def test_diamond_with_exactly_tied_scores_takes_the_smaller_first_label():
    # 0 -5-> 1 -7-> 3 and 0 -4-> 2 -8-> 3 (sink 3): theta equal on all labels, both paths score the same bits
    l = synth._finish(4, V, [0, 0, 1, 2], [5, 4, 7, 8], [1, 2, 3, 3])
    theta = np.full(V, -0.75, np.float32)
    th, e = R.arc_terms(l, theta)
    got = R.k_best(l.n_rows, l.src, l.dst, th, e, 4, 3)
    assert got["n_paths"] == 2 and got["best"][0] == got["best"][1]
    assert [l.label[a] for a in got["arcs"][0]] == [4, 8]  # the smaller first mark wins
    assert [l.label[a] for a in got["arcs"][1]] == [5, 7]


def test_minus_infinity_arcs_and_fewer_paths_than_k():
    l = synth.layered_lattice(12, n_states=12, avg_degree=3.0, vocab=V, width=4, span=3)
    theta = _theta(2)
    theta[l.label[np.nonzero(l.src == 0)[0][0]]] = -np.inf  # one arc out of state 0 is gone
    got = _check_against_enumeration(l, theta, 64)
    total = R.count_finite_paths(l.n_rows, l.src, l.dst, theta[l.label].astype(np.float64), l.n_rows - 1)
    assert got["n_paths"] == min(64, total)
    none = np.full(V, -np.inf, np.float32)
    th, e = R.arc_terms(l, none)
    assert R.k_best(l.n_rows, l.src, l.dst, th, e, 3, l.n_rows - 1)["n_paths"] == 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reference_k1_equals_oracle_viterbi_bit_for_bit(seed):
    for l in [synth.layered_lattice(seed, n_states=300, avg_degree=6.0, vocab=64, width=9, span=4),
              synth.edit_lattice([10, 11, 12, 13], [20, 21, 22], vocab=64, seed=seed)]:
        theta = synth.label_scores(seed, 64)
        th, e = R.arc_terms(l, theta)
        got = R.k_best(l.n_rows, l.src, l.dst, th, e, 1, l.n_rows - 1)
        best, path, arcs = O.viterbi(l.n_rows, l.src, l.label, l.dst, theta[l.label], 4000)
        assert np.float32(best) == got["best"][0]
        assert got["arcs"][0] == list(arcs)


# ----------------------------------------------------------------------------- ties, dead labels: the edges the GPU tests lean on
def _canonical_order(l, score64, sink):
    """Every finite path by (score desc, arcs in lexicographic order): the order of nfst_kbest where sums are exact."""
    paths = R.enumerate_paths(l.n_rows, l.src, l.dst, score64, sink)
    return sorted(paths, key=lambda x: (-x[0], x[1]))


@pytest.mark.parametrize("i", range(4))
@pytest.mark.parametrize("dead_label", [False, True])
def test_scores_on_a_grid_tie_and_are_ordered_by_arc(i, dead_label):
    """Scores on a grid of 0.25: float32 sums are exact, so the reference's list must be the enumeration's in the order
    (score desc, then the smaller canonical arc at the first state where two paths part) -- with one label at -inf too."""
    l = _small_lattices()[i]
    theta = E.quarter(_theta(20 + i))
    if l.weight is not None:
        l.weight = E.quarter(l.weight)
    sink = l.n_rows - 1
    if dead_label:
        total = R.count_finite_paths(l.n_rows, l.src, l.dst, np.zeros(l.n_arcs), sink)
        for lab in np.argsort(-np.bincount(l.label, minlength=V), kind="stable"):
            t = theta.copy()
            t[lab] = -np.inf
            if 0 < R.count_finite_paths(l.n_rows, l.src, l.dst, t[l.label].astype(np.float64), sink) < total:
                break
        else:
            pytest.fail("no label kills some paths and not all")
        theta = t
    th, e = R.arc_terms(l, theta)
    ref = _canonical_order(l, th.astype(np.float64) + e.astype(np.float64), sink)
    for k in (1, 3, 7, 64):
        got = R.k_best(l.n_rows, l.src, l.dst, th, e, k, sink)
        n = min(k, len(ref))
        assert got["n_paths"] == n and np.all(got["best"][n:] == NEG)
        assert [float(x) for x in got["best"][:n]] == [s for s, _ in ref[:n]]
        assert got["arcs"] == [p for _, p in ref[:n]]
        if dead_label:
            assert not any(np.isneginf(theta[l.label[p]]).any() for p in got["arcs"])
    assert len({s for s, _ in ref[:64]}) < min(64, len(ref))  # (there are ties among the listed paths)


def test_plus_infinity_on_a_dead_arc_is_no_candidate():
    l = _small_lattices()[1]
    theta = _theta(3)
    a = int(np.nonzero(l.src == 0)[0][0])
    nxt = np.nonzero(l.src == l.dst[a])[0]
    theta[l.label[nxt[0]]] = -np.inf
    asc = np.zeros(l.n_arcs, np.float32)
    asc[nxt[0]] = np.inf  # +inf + -inf = NaN
    th, e = R.arc_terms(l, theta, asc)
    with np.errstate(invalid="ignore"):
        got = R.k_best(l.n_rows, l.src, l.dst, th, e, 64, l.n_rows - 1)
    assert np.all(np.isfinite(got["best"][:got["n_paths"]])) and not np.isnan(got["best"]).any()
    assert not any(int(nxt[0]) in p for p in got["arcs"])
    asc[nxt[0]] = 0.0
    th, e = R.arc_terms(l, theta, asc)
    same = R.k_best(l.n_rows, l.src, l.dst, th, e, 64, l.n_rows - 1)
    assert same["arcs"] == got["arcs"] and np.array_equal(same["best"], got["best"])


def test_tie_cases_really_tie():
    """The conditions of test_gpu_kbest.test_exact_ties, on the reference alone."""
    for name, (lats, theta, asc, _) in E.tie_cases().items():
        refs = E.kbest_refs(lats, theta, asc)
        for l, sl, ref in zip(lats, E.arc_slices(lats), refs):
            assert E.tied_entries(ref) >= 2, name
            # exact sums: the float32 scores are the float64 ones
            s64 = E.score64(l, theta, None if asc is None else asc[sl])
            assert [float(x) for x in ref["best"][:ref["n_paths"]]] == [float(s64[p].sum()) for p in ref["arcs"]]
        if name.startswith("star"):
            assert np.all(refs[0]["best"] == np.float32(-1.0))
            assert [p[1] for p in refs[0]["arcs"]] == list(range(1, 65))
        if name == "funnel":
            for pos in (1, 3):
                assert len({E.sweep_chunk(lats[0], p[pos]) for p in refs[0]["arcs"]}) >= 2


def test_sweep_chunk():
    l = E.star()
    assert [E.sweep_chunk(l, a) for a in (1, 64, 65, 127, 128, 190, 191, 200)] == [0, 0, 1, 1, 2, 2, 3, 3]


def test_few_paths_case_has_between_one_and_63_finite_paths():
    lats, theta, b, n = E.few_paths_case()
    assert 0 < n < 20 and n == 14
    for i, l in enumerate(lats):
        if i != b:
            full = R.count_finite_paths(l.n_rows, l.src, l.dst, E.score64(l, theta[i]), l.n_rows - 1)
            assert full == R.count_finite_paths(l.n_rows, l.src, l.dst, np.zeros(l.n_arcs), l.n_rows - 1)


def test_dead_label_and_no_path_cases_on_the_reference():
    lats = E.weighted_batch()
    theta = E.dead_label_theta()
    for l, ref in zip(lats, E.kbest_refs(lats, theta)):
        assert np.isin(l.label, E.DEAD).sum() > 120 and ref["n_paths"] == 64
        assert not any(np.isin(l.label[p], E.DEAD).any() for p in ref["arcs"])
        assert l.label[E.reachable_dead_arc(l)] in E.DEAD
    lats, theta = E.no_path_case(True)
    assert [r["n_paths"] == 0 for r in E.kbest_refs(lats, theta, k=7)] == [False, True, False, True, False]


# ----------------------------------------------------------------------------- the C entry point
def test_lib_declares_and_exports_the_new_symbols():
    from nfst_amd import _lib

    for name in ("nfst_kbest_ws_bytes", "nfst_kbest"):
        assert hasattr(_lib.lib, name)
        assert getattr(_lib.lib, name).argtypes is not None


def test_argument_checks_return_before_any_launch():
    from nfst_amd import _lib
    from nfst_amd.lattice import LatticeBatch

    lats = _small_lattices()
    lat = LatticeBatch.from_synth(lats)  # host-packed: the checks run before anything touches a device
    assert lat.device.type == "cpu"
    theta = np.zeros(V, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    lib = _lib.lib
    bs = C.byref(lat.c_struct())
    assert lib.nfst_kbest_ws_bytes(bs, 0) == ERR_ARG
    assert lib.nfst_kbest_ws_bytes(bs, 65) == ERR_LIMIT
    k = 5
    ws_bytes = lib.nfst_kbest_ws_bytes(bs, k)
    assert ws_bytes >= lat.total_rows * k * 8
    B, T = lat.n_lattices, 8
    ws = np.zeros(ws_bytes // 8 + 2, np.float64)  # (16-byte aligned by numpy)
    best = np.zeros((B, k), np.float32)
    paths = np.zeros((B, k, T), np.int32)
    lens = np.zeros((B, k), np.int32)
    n_paths = np.zeros(B, np.int32)
    status = np.zeros(1, np.int32)
    p = lambda a: None if a is None else a.ctypes.data

    def call(k, ws=ws, wsb=ws_bytes, best=best, paths=paths, lens=lens, n_paths=n_paths, status=status, T=T):
        return lib.nfst_kbest(bs, C.byref(sc), k, p(ws), wsb, p(best), p(paths), None, p(lens), p(n_paths), T, 0,
                              p(status), None)

    assert call(0) == ERR_ARG
    assert call(-3) == ERR_ARG
    assert call(65) == ERR_LIMIT
    assert call(k, best=None) == ERR_ARG
    assert call(k, paths=None) == ERR_ARG
    assert call(k, lens=None) == ERR_ARG
    assert call(k, n_paths=None) == ERR_ARG
    assert call(k, status=None) == ERR_ARG
    assert call(k, ws=None) == ERR_ARG
    assert call(k, wsb=ws_bytes - 1) == ERR_ARG
    assert call(k, T=0) == ERR_ARG
    assert lib.nfst_kbest(None, C.byref(sc), k, p(ws), ws_bytes, p(best), p(paths), None, p(lens), p(n_paths), T, 0,
                          p(status), None) == ERR_ARG


def test_ops_k_best_rejects_a_bad_k():
    import torch

    from nfst_amd import ops

    class Dev:  # (the check on k comes before anything looks at the batch)
        pass

    for k in (0, 65, 2.0, True):
        with pytest.raises(ValueError):
            ops.k_best(Dev(), torch.zeros(V), k)


def test_build_guard_covers_the_kbest_sweep():
    from nfst_amd.build import check_resources

    assert check_resources({"k_kbest_sweep": {"vgpr_spill": 4, "agprs": 0}})
    assert not check_resources({"k_kbest_sweep": {"vgpr_spill": 0, "agprs": 0}})

"""The NumPy restatement of the time-synchronous sweeps (tests/positional_ref.py), which the GPU tests of
ops.positional_* rely on: against path enumeration, against finite differences of its own log Z, the identities of the
semantics at every truncation case, and -- without position scores and with T >= depth -- against
the oracle's forward-backward and the k-best reference bit for bit.  Then the C entry points' argument checks (host side,
before any launch) and the register guard of the new kernels."""
import ctypes as C

import numpy as np
import pytest

from nfst_amd import synth
from oracle import oracle as O
from tests import kbest_ref as K
from tests import positional_ref as R

NEG = -np.inf
ERR_ARG, ERR_LIMIT = -1, -6  # (include/nfst_hip.h)
N_PATHS = (18, 28, 28, 6063, 25, 681)  # (the enumeration and kbest_ref.count_finite_paths agree on every one)
N_LENGTHS = (3, 2, 3, 6, 3, 5)


def small_lattices():
    return [synth.layered_lattice(s, n_states=12, avg_degree=2.0, vocab=12, width=3, span=3, max_degree=4) for s in (11, 12, 13)] + [
        synth.layered_lattice(21, n_states=40, avg_degree=3.0, vocab=16, width=4, span=3, max_degree=6),
        synth.edit_lattice([6, 7, 8], [9, 10], vocab=12, seed=1),
        synth.edit_lattice([6, 7, 8, 6, 7], [9, 10, 9, 11], vocab=12, seed=2),
    ]


_PATHS = {}


def _paths(i):
    if i not in _PATHS:
        _PATHS[i] = R.enumerate_paths(small_lattices()[i])
    return _PATHS[i]


def _inputs(l, seed, T):
    rng = np.random.default_rng(seed)
    theta = rng.normal(-1.0, 0.8, size=l.vocab).astype(np.float32)
    pos = rng.normal(0.0, 1.0, size=(T, l.vocab)).astype(np.float32)
    return theta, pos


def truncations(l):
    """(name, T): below the shortest path, at it, between it and the depth, at the depth, beyond it."""
    lo, hi = R.min_max_len(l)
    assert lo < hi and lo >= 2
    return [("below", lo - 1), ("shortest", lo), ("between", (lo + hi) // 2 if hi - lo > 1 else lo), ("depth", hi), ("beyond", hi + 3)]


def _close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    inf = ~np.isfinite(b)
    assert np.array_equal(a[inf], b[inf])
    assert np.all(np.abs(a[~inf] - b[~inf]) <= tol * np.maximum(1.0, np.abs(b[~inf])))


@pytest.mark.parametrize("i", range(6))
def test_lattices_have_the_path_counts_and_lengths_the_cases_rely_on(i):
    l = small_lattices()[i]
    paths = _paths(i)
    assert len(paths) == N_PATHS[i] < 10000
    assert len(paths) == K.count_finite_paths(l.n_rows, l.src, l.dst, np.zeros(l.n_arcs), l.n_rows - 1)
    lens = sorted({len(p) for p in paths})
    assert len(lens) == N_LENGTHS[i]
    assert (lens[0], lens[-1]) == R.min_max_len(l)


@pytest.mark.parametrize("i", range(6))
@pytest.mark.parametrize("with_pos", [True, False])
def test_reference_equals_path_enumeration(i, with_pos):
    l = small_lattices()[i]
    for name, T in truncations(l):
        theta, pos = _inputs(l, 100 + i, T)
        if not with_pos:
            pos = None
        score = R.arc_score64(l, theta)
        ref = R.sum_product(l, score, pos, T)
        bf = R.brute_force(l, score, pos, T, _paths(i))
        _close(ref["logz"], bf["logz"], 1e-12)
        _close(ref["len_logz"], bf["len_logz"], 1e-12)
        assert np.abs(ref["pos_post"] - bf["pos_post"]).max() <= 1e-12, name
        assert np.abs(ref["arc_post"] - bf["arc_post"]).max() <= 1e-12, name
        mp = R.max_plus(l, theta, pos, T)
        if name == "below":
            assert ref["logz"] == NEG and mp["best"] == NEG and mp["arcs"] == []
            continue
        # a real path of at most T arcs whose float64 score is the reported one and the enumeration's best; the same
        # path wherever the runner-up is not a near tie (edit lattices have paths with the same labels in another order)
        tol = 1e-5 * max(1.0, abs(bf["best"]))
        assert mp["arcs"] in _paths(i) and len(mp["arcs"]) <= T
        s64 = score[mp["arcs"]].sum() + (0.0 if pos is None else sum(float(pos[t, l.label[a]]) for t, a in enumerate(mp["arcs"])))
        assert abs(float(mp["best"]) - s64) <= tol and abs(s64 - bf["best"]) <= tol, name
        if bf["best"] - bf["runner_up"] > 2 * tol:
            assert mp["arcs"] == bf["best_arcs"], name


@pytest.mark.parametrize("i", [0, 4])
def test_reference_posteriors_are_the_gradient_of_its_log_z(i):
    l = small_lattices()[i]
    T = R.min_max_len(l)[1]
    theta, pos = _inputs(l, 200 + i, T)
    pos = pos.astype(np.float64)
    score = R.arc_score64(l, theta)
    ref = R.sum_product(l, score, pos, T)
    h = 1e-4
    for t in range(T):
        for lab in range(l.vocab):
            up, dn = pos.copy(), pos.copy()
            up[t, lab] += h
            dn[t, lab] -= h
            fd = (R.sum_product(l, score, up, T)["logz"] - R.sum_product(l, score, dn, T)["logz"]) / (2 * h)
            assert abs(fd - ref["pos_post"][t, lab]) <= 1e-6, (t, lab)
    for a in range(l.n_arcs):
        up, dn = score.copy(), score.copy()
        up[a] += h
        dn[a] -= h
        fd = (R.sum_product(l, up, pos, T)["logz"] - R.sum_product(l, dn, pos, T)["logz"]) / (2 * h)
        assert abs(fd - ref["arc_post"][a]) <= 1e-6, a


def check_identities(l, ref, T, bos=synth.BOS):
    """The identities of the semantics on one lattice's outputs (float64 arrays); returns the largest violation."""
    worst = 0.0
    if not np.isfinite(ref["logz"]):
        assert np.all(ref["len_logz"] == NEG) and not ref["pos_post"].any() and not ref["arc_post"].any()
        return worst
    worst = max(worst, abs(R.logsumexp(ref["len_logz"]) - ref["logz"]))
    p_len = np.exp(ref["len_logz"] - ref["logz"])  # P(L = k)
    longer = 1.0 - np.cumsum(p_len)[:T]  # P(L > t), t = 0 .. T - 1
    worst = max(worst, np.abs(ref["pos_post"].sum(axis=1) - longer).max())
    worst = max(worst, abs(ref["pos_post"][0, bos] - 1.0))
    per_label = np.bincount(l.label, weights=ref["arc_post"], minlength=l.vocab)
    worst = max(worst, np.abs(ref["pos_post"].sum(axis=0) - per_label).max())
    assert ref["len_logz"][0] == NEG
    return worst


@pytest.mark.parametrize("i", range(6))
def test_identities_at_every_truncation(i):
    l = small_lattices()[i]
    for name, T in truncations(l):
        theta, pos = _inputs(l, 300 + i, T)
        ref = R.sum_product(l, R.arc_score64(l, theta), pos, T)
        assert (ref["logz"] == NEG) == (name == "below")
        assert check_identities(l, ref, T) <= 1e-12, name


def _oracle_posterior(l, score):
    o = O.forward_backward(l.n_rows, l.src.astype(np.int32), l.dst.astype(np.int32), score)
    la, lb, lz = np.asarray(o["logalpha"], np.float64), np.asarray(o["logbeta"], np.float64), float(o["logZ"])
    with np.errstate(invalid="ignore"):
        post = np.where(l.src != l.dst, np.exp(la[l.src] + score + lb[l.dst] - lz), 0.0)
    return lz, np.nan_to_num(post)


@pytest.mark.parametrize("i", range(6))
@pytest.mark.parametrize("extra", [0, 3])
def test_without_positions_and_full_length_it_is_forward_backward_and_k_best(i, extra):
    l = small_lattices()[i]
    T = R.min_max_len(l)[1] + extra
    theta, _ = _inputs(l, 400 + i, T)
    score = R.arc_score64(l, theta)
    ref = R.sum_product(l, score, None, T)
    lz, post = _oracle_posterior(l, score)
    assert abs(ref["logz"] - lz) <= 1e-12 * max(1.0, abs(lz))
    assert np.abs(ref["arc_post"] - post).max() <= 1e-12
    th, e = K.arc_terms(l, theta)
    kb = K.k_best(l.n_rows, l.src, l.dst, th, e, 1, l.n_rows - 1)
    mp = R.max_plus(l, theta, None, T)
    assert mp["best"].view(np.int32) == kb["best"][:1].view(np.int32)[0]
    assert mp["arcs"] == kb["arcs"][0]


def test_forbidden_positions_and_dead_labels_on_the_reference():
    l = small_lattices()[0]
    paths = _paths(0)
    T = R.min_max_len(l)[1]
    theta, pos = _inputs(l, 7, T)
    score = R.arc_score64(l, theta)
    keep = paths[5]
    one = np.full((T, l.vocab), NEG, np.float32)
    for t, a in enumerate(keep):
        one[t, l.label[a]] = pos[t, l.label[a]]
    ref = R.sum_product(l, score, one, T)
    alive = [p for p in paths if all(np.isfinite(one[t, l.label[a]]) for t, a in enumerate(p))]
    assert alive == [keep]  # (lattices are deterministic: the labels of a path determine it)
    assert set(np.unique(np.round(ref["pos_post"], 12))) <= {0.0, 1.0}
    assert R.max_plus(l, theta, one, T)["arcs"] == keep
    dead = pos.copy()
    dead[1, :] = NEG
    ref = R.sum_product(l, score, dead, T)
    assert ref["logz"] == NEG and not ref["pos_post"].any() and np.all(ref["len_logz"] == NEG)
    assert R.max_plus(l, theta, dead, T)["best"] == NEG


# ----------------------------------------------------------------------------- the C entry points
def test_argument_checks_return_before_any_launch():
    from nfst_amd import _lib
    from nfst_amd.lattice import LatticeBatch

    lats = small_lattices()[:3]
    lat = LatticeBatch.from_synth(lats)  # host-packed: the checks run before anything touches a device
    assert lat.device.type == "cpu"
    V, B, T = lat.vocab, lat.n_lattices, 6
    theta = np.zeros(V, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    lib = _lib.lib
    bs = C.byref(lat.c_struct())
    assert lib.nfst_positional_ws_bytes(bs, 0, 0) == ERR_ARG
    assert lib.nfst_positional_ws_bytes(bs, T, 4) == ERR_ARG
    assert lib.nfst_positional_ws_bytes(None, T, 0) == ERR_ARG
    small, full, vit = (lib.nfst_positional_ws_bytes(bs, T, f) for f in (0, 1, 2))
    assert full >= small + 12 * (T + 1) * lat.total_rows  # every beta row of every position
    assert vit >= 4 * (T + 1) * lat.total_rows
    ws = np.zeros(full // 8 + 2, np.float64)  # (16-byte aligned by numpy)
    pos = np.zeros((B, T, V), np.float32)
    z64, z32 = np.zeros(B, np.float64), np.zeros(B, np.float32)
    pp = np.zeros((B, T, V), np.float32)
    p = lambda a: None if a is None else a.ctypes.data

    def call(T=T, stride=T * V, ws=ws, wsb=full, z64=z64, pp=pp, scores=C.byref(sc)):
        return lib.nfst_positional(bs, scores, p(pos), stride, T, p(ws), wsb, p(z64), p(z32), None, p(pp), None, None)

    assert call(T=0, stride=0) == ERR_ARG
    assert call(stride=V) == ERR_ARG
    assert call(stride=T * V + 1) == ERR_ARG
    assert call(z64=None) == ERR_ARG
    assert call(ws=None) == ERR_ARG
    assert call(wsb=full - 1) == ERR_ARG
    assert call(wsb=small) == ERR_ARG  # a posterior needs the stored rows
    assert call(scores=None) == ERR_ARG
    best, paths, lens = np.zeros(B, np.float32), np.zeros((B, T), np.int32), np.zeros(B, np.int32)

    def vcall(T=T, stride=T * V, ws=ws, wsb=vit, best=best, paths=paths, lens=lens):
        return lib.nfst_positional_viterbi(bs, C.byref(sc), p(pos), stride, T, p(ws), wsb, p(best), p(paths), None, p(lens), 0, None)

    assert vcall(T=-1) == ERR_ARG
    assert vcall(stride=3) == ERR_ARG
    assert vcall(best=None) == ERR_ARG
    assert vcall(paths=None) == ERR_ARG
    assert vcall(lens=None) == ERR_ARG
    assert vcall(ws=None) == ERR_ARG
    assert vcall(wsb=vit - 1) == ERR_ARG


def test_lds_limit_is_checked_on_the_host():
    """24 max_rows + 20 vocab + 4112 bytes must fit in 160 KiB: a 7000-row lattice does not (NFST_ERR_LIMIT), while the
    max-plus kernel (8 max_rows + 4 vocab + 16) takes it."""
    from nfst_amd import _lib
    from nfst_amd.lattice import LatticeBatch

    l = synth.layered_lattice(5, n_states=7000, avg_degree=2.0, vocab=16, width=8, span=2, max_degree=4)
    lat = LatticeBatch.from_synth([l])
    assert 24 * lat.max_rows + 20 * lat.vocab + 4112 > 160 * 1024
    theta = np.zeros(lat.vocab, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    bs = C.byref(lat.c_struct())
    T = 4
    n = _lib.lib.nfst_positional_ws_bytes(bs, T, 0)
    ws = np.zeros(n // 8 + 2, np.float64)
    z = np.zeros(1, np.float64)
    assert _lib.lib.nfst_positional(bs, C.byref(sc), None, 0, T, ws.ctypes.data, n, z.ctypes.data, None, None, None, None, None) == ERR_LIMIT


def test_wrappers_validate_before_any_launch():
    import torch

    from nfst_amd import ops
    from nfst_amd.lattice import LatticeBatch

    lat = LatticeBatch.from_synth(small_lattices()[:3])
    theta = torch.zeros(lat.vocab)
    with pytest.raises(RuntimeError):  # a host batch: no CPU fallback
        ops.positional_forward_backward(lat, theta, torch.zeros(4, lat.vocab))
    for bad in (torch.zeros(4, lat.vocab + 1), torch.zeros(2, 4, lat.vocab), torch.zeros(lat.vocab), torch.zeros(0, lat.vocab),
                torch.zeros(4, lat.vocab, dtype=torch.int64)):
        with pytest.raises(ValueError):
            ops._positions(lat, bad, None)
    for T in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            ops._positions(lat, None, T)
    with pytest.raises(ValueError):
        ops._positions(lat, torch.zeros(4, lat.vocab), 5)
    assert ops._positions(lat, None, None)[2] == int(lat.depth.max())
    pos, stride, T = ops._positions(lat, torch.zeros(3, 4, lat.vocab, dtype=torch.float64), None)
    assert pos.dtype == torch.float32 and stride == 4 * lat.vocab and T == 4


def test_build_guard_covers_the_positional_kernels():
    from nfst_amd.build import check_resources

    for name in ("k_positional<true>", "k_positional<false>", "k_positional_viterbi"):
        assert check_resources({name: {"vgpr_spill": 4, "agprs": 0}})
        assert not check_resources({name: {"vgpr_spill": 0, "agprs": 0}})

"""The NumPy restatement of the time-synchronous sweeps (tests/positional_ref.py), which the GPU tests of
ops.positional_* rely on: against path enumeration, against finite differences of its own log Z, the identities of the
semantics at every truncation case, and -- without position scores and with T >= depth -- against
the oracle's forward-backward and the k-best reference bit for bit.  Then the C entry points' argument checks (host side,
before any launch), the register guard of the new kernels, the plan query the launchers share (nfst_positional_plan)
against the formulas of include/nfst_hip.h, and the proofs that the inputs of tests/edge_cases.py are what the cases of
tests/test_gpu_positional.py need: which flavour a batch takes, the group sizes, the exponent range with posteriors that
have not collapsed, the limits, and scores that tie on the walked path."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from nfst_amd import synth
from oracle import oracle as O
from tests import edge_cases as E
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


# ----------------------------------------------------------------------------- the plan query and the inputs of the GPU cases
LDS_LIMIT = 160 * 1024


def _pack(lats, **opts):
    from nfst_amd.lattice import LatticeBatch

    return LatticeBatch.from_synth(lats, **opts)  # host-packed: nothing here touches a device


def _plan(lat, viterbi):
    """(lds_bytes, staged) of ops.positional_plan, or the error code."""
    from nfst_amd import _lib, ops

    try:
        return ops.positional_plan(lat, viterbi)
    except _lib.NfstError as e:
        return e.code


def _plan_by_the_header(lat, lats, viterbi):
    """The two expressions of include/nfst_hip.h, restated."""
    R_, V = int(lat.max_rows), int(lat.vocab)
    lds = 8 * R_ + 4 * V + 16 if viterbi else 24 * R_ + 20 * V + 4112
    if lds > LDS_LIMIT:
        return ERR_LIMIT
    more = 4 * (R_ + 1 + max(l.n_arcs for l in lats)) + 16
    return (lds + more, True) if lds + more <= LDS_LIMIT else (lds, False)


def test_plan_query_is_the_rule_of_the_header():
    from nfst_amd import _lib

    batches = {"small": small_lattices()[:3], "mixed": E.mixed_batch(), "big": [E.pos_large("big"), E.pos_neighbour()],
               "mid": [E.pos_large("mid")], "degrees": E.pos_degree_classes(), "rowmax": E.pos_rowmax_batch(),
               "rowmax + 1": E.pos_rowmax_batch(1), "wide": [E.pos_wide()], "7000 rows": [
                   synth.layered_lattice(5, n_states=7000, avg_degree=2.0, vocab=16, width=8, span=2, max_degree=4)]}
    seen = set()
    for name, lats in batches.items():
        lat = _pack(lats)
        for viterbi in (False, True):
            got = _plan(lat, viterbi)
            assert got == _plan_by_the_header(lat, lats, viterbi), (name, viterbi, got)
            seen.add((viterbi, got if got == ERR_LIMIT else got[1]))
    assert seen == {(False, True), (False, False), (False, ERR_LIMIT), (True, True), (True, False)}
    # either output may be null; a null batch is an argument error
    lat = _pack(batches["small"])
    bs = C.byref(lat.c_struct())
    lds, staged = C.c_int64(-1), C.c_int32(-1)
    assert _lib.lib.nfst_positional_plan(bs, 0, None, None) == 0
    assert _lib.lib.nfst_positional_plan(bs, 0, C.byref(lds), None) == 0 and lds.value == _plan(lat, False)[0]
    assert _lib.lib.nfst_positional_plan(bs, 7, None, C.byref(staged)) == 0 and staged.value == 1
    assert _lib.lib.nfst_positional_plan(None, 0, C.byref(lds), C.byref(staged)) == ERR_ARG


def test_large_lattices_take_the_unstaged_flavours():
    """big: neither kernel stages its arcs; mid: the sum-product does not, max-plus does.  With table weights (the
    EXTRA flavours) the same."""
    for weighted in (False, True):
        big, mid = E.pos_large("big", weighted), E.pos_large("mid", weighted)
        assert (big.n_rows, big.n_arcs, R.min_max_len(big)) == (481, 42718, (22, 62))
        assert (mid.n_rows, mid.n_arcs, R.min_max_len(mid)[1]) == (441, 39105, 57)
        assert (big.weight is not None) == weighted
        lat = _pack([big, E.pos_neighbour(weighted=weighted)])
        assert E.pos_neighbour().n_rows == 13 and bool(lat.weighted) == weighted
        assert _plan(lat, False)[1] is False and _plan(lat, True)[1] is False
        assert R.batch_groups(lat) == [64, 2]
        lat = _pack([mid])
        assert _plan(lat, False)[1] is False and _plan(lat, True)[1] is True


def test_big_has_many_path_lengths():
    big = E.pos_large("big")
    T = 62
    theta, pos = _inputs(big, 27, T)
    ref = R.sum_product(big, R.arc_score64(big, theta), pos, T)
    assert np.isfinite(ref["len_logz"]).sum() == 41 and np.isfinite(ref["logz"])


def test_pos_group_restatement_and_the_degree_classes():
    """Every width of the butterfly, 8, 16 and 32 both by the mean degree alone and through the widening loop; with the
    other inputs of tests/test_gpu_positional.py every G of the kernel."""
    from nfst_amd import _lib

    assert [R.pos_group(d * 100, 100, 5000) for d in (0, 1, 2, 3, 4, 7, 8, 31, 32, 63, 64, 1000)] == [1, 1, 2, 2, 4, 4, 8, 16, 32, 32, 64, 64]
    assert R.pos_group(500, 100, 200) == 4 and R.pos_group(500, 100, 128) == 8  # 5 arcs per state: widened while 2 G rows <= 1024
    assert R.pos_group(300, 100, 10) == 4 and R.pos_group(100, 0, 1) == 64
    lats = E.pos_degree_classes()
    lat = _pack(lats)
    m = lat.meta_host
    for b, ((n, d), (g_mean, g)) in enumerate(E.POS_DEGREE_CLASSES.items()):
        avg = int(m[b, _lib.META_N_DP]) // int(m[b, _lib.META_N_REACH])
        assert lats[b].n_rows == n + 1 == m[b, _lib.META_N_ROWS]
        assert g_mean <= avg < 2 * g_mean, (n, d, avg)
        assert R.batch_groups(lat)[b] == g, (n, d)
    got = set(E.POS_DEGREE_CLASSES.values())
    assert {8, 16, 32} <= {g for g0, g in got if g0 == g} and {8, 16, 32} <= {g for g0, g in got if g0 < g}
    assert _plan(lat, False)[1] is True and _plan(lat, True)[1] is True
    everything = set(R.batch_groups(lat))
    small = [dataclasses.replace(l, vocab=E.POS_V) for l in small_lattices()]
    for other in (small, E.mixed_batch(), [E.pos_large("big")], E.packing_lattices()):
        everything |= set(R.batch_groups(_pack(other)))
    assert everything == {1, 2, 4, 8, 16, 32, 64}
    # fan-out 200 and fan-in 200 at one lane per state
    star, funnel = E.packing_lattices()[:2]
    assert R.batch_groups(_pack([star, funnel])) == [1, 1]
    assert np.bincount(star.src).max() == 200 and np.bincount(funnel.dst).max() == 200


def test_staged_and_unstaged_batches_of_the_bit_comparison():
    shared = [dataclasses.replace(l, vocab=E.POS_V) for l in small_lattices()] + E.pos_degree_classes()
    lat = _pack(shared)
    assert _plan(lat, False)[1] is True and _plan(lat, True)[1] is True
    lat = _pack(shared + [E.pos_large("big")])
    assert _plan(lat, False)[1] is False and _plan(lat, True)[1] is False


def test_row_and_vocabulary_limits():
    lats = E.pos_rowmax_batch()
    lat = _pack(lats)
    assert E.pos_sum_lds(lat.max_rows, lat.vocab) == LDS_LIMIT and lat.vocab == 256  # the last byte
    assert _plan(lat, False) == (LDS_LIMIT, False) and _plan(lat, True)[1] is False
    assert R.min_max_len(lats[0]) == (16, 53)
    over = _pack(E.pos_rowmax_batch(1))
    assert over.max_rows == lat.max_rows + 1
    assert _plan(over, False) == ERR_LIMIT and _plan(over, True)[1] is False
    l = E.pos_wide(64)
    V = E.pos_vocab_limit(_pack([l]).max_rows)
    assert l.n_rows == 13 and V == 7970
    lat = _pack([E.pos_wide(V)])
    assert lat.max_rows == 13 and E.pos_sum_lds(13, V) <= LDS_LIMIT < E.pos_sum_lds(13, V + 1)
    assert _plan(lat, False)[1] is False and _plan(lat, True)[1] is True
    lat = _pack([E.pos_wide(V + 1)])
    assert lat.max_rows == 13 and _plan(lat, False) == ERR_LIMIT and _plan(lat, True)[1] is True
    w = E.pos_wide()
    assert (w.vocab, w.n_rows, w.n_arcs, int(w.label.max()), R.min_max_len(w)) == (32767, 13, 28, 30650, (4, 6))
    assert w.label.max() >= 1 << 14  # bit 30 of a staged record
    lat = _pack([w])
    assert _plan(lat, False) == ERR_LIMIT and _plan(lat, True)[1] is True


@pytest.mark.parametrize("name", E.RANGE_CASES)
def test_range_inputs_reach_the_exponents_without_collapsing(name):
    lats, theta, asc, pos, T = E.pos_range_inputs(name)
    assert T == max(R.min_max_len(l)[1] for l in lats) and pos.shape == (len(lats), T, lats[0].vocab)
    big = 0.0
    for b, (l, sl) in enumerate(zip(lats, E.arc_slices(lats))):
        ref = R.sum_product(l, R.arc_score64(l, theta, asc[sl]), pos[b], T)
        assert np.isfinite(ref["logz"])
        big = max(big, abs(ref["logz"]))
        for p in (ref["arc_post"], ref["pos_post"]):
            assert np.sum((p > 0.01) & (p < 0.99)) >= E.SPREAD_MIN, (name, b)
        assert check_identities(l, ref, T) <= 1e-9
    assert big > E.RANGE_LOGZ[name]


@pytest.mark.parametrize("name", sorted(E.POS_TIE_SEED))
def test_tie_inputs_tie_on_the_walked_path(name):
    """At some step of the reference's walk at least two live arcs of the walked state attain vb_t(state): the rule
    "the smallest canonical arc" decides the path."""
    lats, theta, asc, pos, T = E.pos_tie_inputs(name)
    assert np.array_equal(pos, E.quarter(pos)) and np.array_equal(theta, E.quarter(theta))
    tied = 0
    for b, (l, sl) in enumerate(zip(lats, E.arc_slices(lats))):
        mp = R.max_plus(l, theta, pos[b], T, None if asc is None else asc[sl])
        assert np.isfinite(mp["best"]) and len(mp["ties"]) == len(mp["arcs"])
        if max(mp["ties"]) >= 2:
            tied += 1
            t = int(np.argmax(np.asarray(mp["ties"]) >= 2))  # the walk took the smallest of the tied arcs
            st = int(l.src[mp["arcs"][t]])
            c = {a: _candidate(l, theta, pos[b], None if asc is None else asc[sl], mp["vb"], t, a)
                 for a in np.nonzero((l.src == st) & (l.dst != st))[0]}
            top = [a for a, x in c.items() if x == mp["vb"][t, st]]
            assert len(top) == mp["ties"][t] and mp["arcs"][t] == min(top)
    assert tied >= E.POS_TIE_LATTICES[name] >= 1


def _candidate(l, theta, pos, asc, vb, t, a):
    e = np.float32(0.0)
    if l.weight is not None:
        e = np.float32(e + np.float32(l.weight[a]))
    if asc is not None:
        e = np.float32(e + np.float32(asc[a]))
    return np.float32(e + np.float32(np.float32(theta[l.label[a]] + pos[t, l.label[a]]) + vb[t + 1, l.dst[a]]))


def test_packings_change_the_scratch_rows():
    assert len(E.STAR_PACKINGS) == 10
    rows = [int(_pack(E.packing_lattices(), **opts).max_rows) for opts in E.STAR_PACKINGS]
    assert len(set(rows)) >= 2 and max(rows) > min(rows) >= max(l.n_rows for l in E.packing_lattices())


def test_mixed_batch_has_the_truncation_extremes():
    lens = [R.min_max_len(l) for l in E.mixed_batch()]
    assert min(lo for lo, _ in lens) == 1 and max(hi for _, hi in lens) == 90
    assert E.mixed_batch()[-1].n_arcs - 1 == 1  # one arc and the sink's pad loop

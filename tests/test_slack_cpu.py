"""The float32 NumPy restatement of the arc slack semantics (tests/slack_ref.py) that the GPU tests of ops.arc_slack
rely on: against path enumeration on small lattices, its invariants on random lattices, the exports of the library and
LatticeBatch.restrict on host batches."""
import numpy as np
import pytest
import torch

from nfst_amd import synth
from nfst_amd.lattice import LatticeBatch
from tests import kbest_ref as K
from tests import slack_ref as R

V = 16
INF = np.inf


def _bound(l, ref, theta, arc_scores=None):
    """8 * depth * 2^-24 * max(1, max |vbeta| + max |s_a|): a generous worst case of two roundings per level in each of
    the two passes (not a measurement)."""
    th, e = K.arc_terms(l, theta, arc_scores)
    s = th.astype(np.float64) + e.astype(np.float64)
    vb = ref["vbeta"].astype(np.float64)
    mv = np.max(np.abs(vb[np.isfinite(vb)]), initial=0.0)
    ms = np.max(np.abs(s[np.isfinite(s)]), initial=0.0)
    return 8.0 * max(ref["depth"], 1) * 2.0 ** -24 * max(1.0, mv + ms)


def _small():
    out = []
    for seed in (1, 2, 3):
        for weighted in (False, True):
            out.append((synth.layered_lattice(seed, n_states=12, avg_degree=2.5, vocab=V, width=3, span=2, weighted=weighted), seed))
    out.append((synth.edit_lattice([6, 7, 8], [9, 10, 11], vocab=V, seed=4), 7))
    return out


@pytest.mark.parametrize("i", range(7))
def test_reference_equals_path_enumeration(i):
    l, seed = _small()[i]
    theta = np.random.default_rng(seed).normal(-1.0, 0.8, size=V).astype(np.float32)
    ref = R.arc_slack(l, theta)
    mm = R.max_marginals64(l, theta)
    got = (ref["best"] - ref["slack"]).astype(np.float64)  # the derived max-marginal: one more rounding
    fin = np.isfinite(mm)
    assert fin.any()
    assert np.array_equal(fin, np.isfinite(ref["slack"]) & (np.asarray(l.src) != np.asarray(l.dst)))
    tol = _bound(l, ref, theta)
    err = float(np.max(np.abs(got[fin] - mm[fin])))
    print(f"lattice {i}: largest |max-marginal error| {err:.3g} (bound {tol:.3g})")
    assert err <= tol
    assert np.all(ref["slack"][~fin & (np.asarray(l.src) != np.asarray(l.dst))] == INF)


def _random_case(seed):
    rng = np.random.default_rng(9000 + seed)
    l = synth.layered_lattice(500 + seed, n_states=int(rng.integers(8, 401)), avg_degree=float(rng.uniform(1.5, 6.0)), vocab=V,
                              width=int(rng.integers(1, 12)), span=int(rng.integers(1, 6)), weighted=seed % 2 == 1)
    theta = rng.normal(-1.0, 0.8, size=V).astype(np.float32)
    if seed % 3 == 2:
        theta[rng.choice(np.arange(3, V), size=5, replace=False)] = -INF
    asc = rng.normal(0.0, 0.5, size=l.n_arcs).astype(np.float32) if seed % 4 == 3 else None
    return l, theta, asc


N_SEEDS = 40


def test_invariants_on_random_lattices():
    no_path = 0
    for seed in range(N_SEEDS):
        l, theta, asc = _random_case(seed)
        src, dst = np.asarray(l.src), np.asarray(l.dst)
        ref = R.arc_slack(l, theta, asc)
        th, e = K.arc_terms(l, theta, asc)
        kb = K.k_best(l.n_rows, src, dst, th, e, 8, l.n_rows - 1)
        # beta*(0) has the bits of the k-best reference's entry 0
        assert np.array_equal(np.asarray([ref["best"]], np.float32).view(np.int32), kb["best"][:1].view(np.int32)), seed
        if kb["n_paths"] == 0:
            no_path += 1
            assert ref["best"] == -INF and np.all(ref["slack"] == INF), seed
            assert R.arc_slack(l, theta, asc, beam=INF)["n_kept"] == 0
            continue
        slack = ref["slack"]
        assert np.all(slack >= 0), seed
        assert np.all(slack[kb["arcs"][0]] == 0), seed  # exactly 0 on the best path
        assert slack[-1] == 0 and src[-1] == dst[-1]  # the sink's pad loop
        for beam in (0.0, 0.5, 2.0, INF):
            r = R.arc_slack(l, theta, asc, beam=beam)
            assert R.is_trim(l, r["keep"]), (seed, beam)
            assert np.all(r["keep"][kb["arcs"][0]]) and r["keep"][-1], (seed, beam)
        tol = _bound(l, ref, theta, asc)
        for j in range(kb["n_paths"]):
            short = float(kb["best"][0]) - float(kb["best"][j])
            assert np.all(slack[kb["arcs"][j]].astype(np.float64) <= short + tol), (seed, j)
    assert no_path <= 3  # (lattices without a path of finite score stay a small minority of the cases)


def test_lib_declares_and_exports_the_new_symbols():
    from nfst_amd import _lib

    for name in ("nfst_arc_slack_ws_bytes", "nfst_arc_slack"):
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib, name)
        assert getattr(_lib.lib, name).argtypes is not None


# ----------------------------------------------------------------------------- LatticeBatch.restrict on host batches
def _host_batch():
    lats = [synth.layered_lattice(3, n_states=30, avg_degree=3.0, vocab=V, width=4, span=2, weighted=True),
            synth.layered_lattice(4, n_states=120, avg_degree=6.0, vocab=V, width=7, span=3, weighted=True),
            synth.layered_lattice(5, n_states=60, avg_degree=4.0, vocab=V, width=1, span=4, weighted=True)]
    return lats, LatticeBatch.from_synth(lats)


def _same_arrays(x: LatticeBatch, y: LatticeBatch):
    assert x._h == y._h
    for k in LatticeBatch._FIELDS:
        a, b = x._t[k], y._t[k]
        assert (a is None) == (b is None), k
        if a is not None:
            assert a.dtype == b.dtype and torch.equal(a, b), k


def test_restrict_everything_gives_the_same_batch():
    lats, lat = _host_batch()
    new, arc_map = lat.restrict(np.ones(lat.total_arcs, bool))
    assert arc_map.dtype == torch.int64 and torch.equal(arc_map, torch.arange(lat.total_arcs))
    _same_arrays(new, lat)


def test_restrict_equals_packing_the_filtered_arc_lists():
    lats, lat = _host_batch()
    theta = np.random.default_rng(5).normal(-1.0, 0.8, size=V).astype(np.float32)
    keeps = [R.arc_slack(l, theta, beam=1.0)["keep"] for l in lats]
    keep = np.concatenate(keeps)
    assert 0 < keep.sum() < keep.size
    new, arc_map = lat.restrict(torch.from_numpy(keep))
    assert np.array_equal(arc_map.numpy(), np.nonzero(keep)[0])
    n_rows, _, src, label, dst, w = synth.batch_arcs(lats)
    arc_off = np.concatenate([[0], np.cumsum([k.sum() for k in keeps])]).astype(np.int64)
    ref = LatticeBatch.from_arcs(n_rows, arc_off, src[keep], label[keep], dst[keep], V, arc_w=w[keep])
    _same_arrays(new, ref)
    assert np.array_equal(new.n_rows, lat.n_rows) and new.vocab == lat.vocab
    # the counts may be handed in instead of being counted
    again, _ = lat.restrict(keep, n_kept=np.array([k.sum() for k in keeps]))
    _same_arrays(again, ref)


def test_restrict_refuses_a_lattice_without_arcs():
    lats, lat = _host_batch()
    keep = np.ones(lat.total_arcs, bool)
    keep[lat.arc_off[1]:lat.arc_off[1] + lat.n_arcs[1]] = False
    with pytest.raises(ValueError, match="lattice 1"):
        lat.restrict(keep)
    with pytest.raises(ValueError):
        lat.restrict(keep[:-1])


# ----------------------------------------------------------------------------- the C entry point's checks, the guard
def test_argument_checks_return_before_any_launch():
    import ctypes as C

    from nfst_amd import _lib

    ERR_ARG = -1  # (include/nfst_hip.h)
    _, lat = _host_batch()  # host-packed: the checks run before anything touches a device
    theta = np.zeros(V, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    lib = _lib.lib
    bs = C.byref(lat.c_struct())
    ws_bytes = lib.nfst_arc_slack_ws_bytes(bs)
    assert ws_bytes >= 4 * lat.total_arcs + 8 * lat.total_rows
    assert lib.nfst_arc_slack_ws_bytes(None) == ERR_ARG
    ws = np.zeros(ws_bytes // 8 + 2, np.float64)  # (16-byte aligned by numpy)
    B, A = lat.n_lattices, lat.total_arcs
    best, slack, beam = np.zeros(B, np.float32), np.zeros(A, np.float32), np.zeros(B, np.float32)
    keep, n_kept = np.zeros(A, np.uint8), np.zeros(B, np.int32)
    p = lambda a: None if a is None else a.ctypes.data

    def call(beam=beam, ws=ws, wsb=ws_bytes, best=best, slack=slack, keep=keep, n_kept=n_kept, scores=C.byref(sc)):
        return lib.nfst_arc_slack(bs, scores, p(beam), p(ws), wsb, p(best), None, None, p(slack), p(keep), p(n_kept), None)

    assert call(best=None) == ERR_ARG
    assert call(slack=None) == ERR_ARG
    assert call(keep=None) == ERR_ARG  # a beam needs both mask outputs
    assert call(n_kept=None) == ERR_ARG
    assert call(beam=None) == ERR_ARG  # ... and they need a beam
    assert call(ws=None) == ERR_ARG
    assert call(wsb=ws_bytes - 1) == ERR_ARG
    assert call(scores=None) == ERR_ARG


def test_ops_arc_slack_rejects_a_bad_beam():
    from nfst_amd import ops

    _, lat = _host_batch()
    for beam in (-1.0, float("nan"), True, "wide", torch.tensor([0.0, -0.5, 1.0]), torch.tensor([0.0, float("nan"), 1.0]),
                 torch.zeros(2), torch.zeros(3, 1)):
        with pytest.raises(ValueError):
            ops._beam(lat, beam)
    assert torch.equal(ops._beam(lat, float("inf")), torch.full((3,), float("inf")))
    assert torch.equal(ops._beam(lat, torch.tensor([0.0, 0.5, float("inf")])), torch.tensor([0.0, 0.5, float("inf")]))


def test_build_guard_covers_the_slack_kernel():
    from nfst_amd.build import check_resources

    assert check_resources({"k_arc_slack": {"vgpr_spill": 4, "agprs": 0}})
    assert not check_resources({"k_arc_slack": {"vgpr_spill": 0, "agprs": 0}})

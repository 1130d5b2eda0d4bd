"""The yardstick of ``nfst_lattice_edit`` (tests/lattice_edit_ref.py) against brute force over every path, the inputs the
GPU tests lean on (a tie that really is one, dead labels that really cost edits), and the C entry point's host-side
checks on host pointers.  Runs without a GPU; tests/test_gpu_lattice_edit.py holds the kernels to the same restatement."""
import ctypes as C

import numpy as np
import pytest

from nfst_amd import synth
from tests import edge_cases as E
from tests import edit_ref
from tests import kbest_ref
from tests import lattice_edit_ref as LR

ERR_ARG, ERR_LIMIT = -1, -6


def small_lattices():
    """The four lattices whose every path a test can enumerate (3267, 681, 1654 and 200 paths)."""
    mixed = E.mixed_batch()
    return [mixed[0], mixed[3], synth.layered_lattice(9, n_states=24, avg_degree=2.5, vocab=16, width=3, span=2), E.star()]


def references(l, paths, rng, draws=3):
    """References built from a random path's labels with about 40 % of the tokens replaced, at lengths 0, 1, len - 2,
    len and len + 3 (cut, or stretched with random labels): ``draws`` of each."""
    out = []
    for _ in range(draws):
        y = l.label[paths[int(rng.integers(len(paths)))][1]].astype(np.int64)
        for n in (0, 1, len(y) - 2, len(y), len(y) + 3):
            r = np.concatenate([y, rng.integers(synth.N_SPECIAL, l.vocab, size=3)])[:max(n, 0)]
            swap = rng.random(len(r)) < 0.4
            r[swap] = rng.integers(0, l.vocab, size=int(swap.sum()))
            out.append(r)
    return out


def check_result(l, ref, got):
    """The returned arcs are a path from state 0 to the sink whose labels lie at the returned distance from ref, and
    align and counts describe one optimal alignment."""
    arcs, align = got["arcs"], np.asarray(got["align"], np.int64)
    s = 0
    for a in arcs:
        assert l.src[a] == s and l.dst[a] != s
        s = int(l.dst[a])
    assert s == l.n_rows - 1
    labels = l.label[arcs]
    assert edit_ref.levenshtein(labels, ref) == got["distance"]
    n_sub, n_ins, n_del = got["counts"]
    assert n_sub + n_ins + n_del == got["distance"]
    on = align >= 0
    assert np.all(np.diff(align[on]) > 0) and np.all(align[on] < len(ref))  # positions of ref, in order
    assert n_ins == int((~on).sum()) and n_del == len(ref) - int(on.sum())
    assert n_sub == int((labels[on] != np.asarray(ref)[align[on]]).sum())


@pytest.mark.parametrize("i", range(4))
def test_restatement_equals_brute_force(i):
    l = small_lattices()[i]
    theta = synth.label_scores(50 + i, l.vocab)
    s64 = E.score64(l, theta)
    paths = kbest_ref.enumerate_paths(l.n_rows, l.src, l.dst, s64, l.n_rows - 1)
    assert len(paths) == (3267, 681, 1654, 200)[i]
    by_arcs = {tuple(p): sc for sc, p in paths}
    refs = references(l, paths, np.random.default_rng(100 + i))
    assert len(refs) >= 12
    for ref in refs:
        got, bf = LR.of_lattice(l, ref, theta), LR.brute_force(l, ref, s64)
        assert got["distance"] == bf["distance"] >= 0
        assert LR.of_lattice(l, ref)["distance"] == bf["distance"]  # (no scores: the same distance)
        check_result(l, ref, got)
        # the float64 score of the returned path against the best one at that distance: each of the two float32 sums is
        # within L roundings of 2^-24 sum |terms| of its float64 sum (adding e_a = 0.0 is exact)
        terms = np.abs(s64)
        L = max(len(got["arcs"]), len(bf["best_arcs"]))
        eps = 2 * L * 2.0 ** -24 * max(terms[got["arcs"]].sum(), terms[bf["best_arcs"]].sum())
        mine = by_arcs[tuple(got["arcs"])]
        assert abs(float(got["score"]) - mine) <= eps
        assert bf["best"] - eps <= mine <= bf["best"]


def test_restatement_with_weights_and_arc_scores():
    l = synth.layered_lattice(9, n_states=24, avg_degree=2.5, vocab=16, width=3, span=2, weighted=True)
    rng = np.random.default_rng(5)
    theta, asc = synth.label_scores(3, 16), rng.normal(0, 0.5, size=l.n_arcs).astype(np.float32)
    s64 = E.score64(l, theta, asc)
    paths = kbest_ref.enumerate_paths(l.n_rows, l.src, l.dst, s64, l.n_rows - 1)
    for ref in references(l, paths, rng, draws=1):
        got, bf = LR.of_lattice(l, ref, theta, asc), LR.brute_force(l, ref, s64)
        assert got["distance"] == bf["distance"]
        check_result(l, ref, got)
        terms = np.abs(E.score64(l, theta)) + np.abs(l.weight.astype(np.float64)) + np.abs(asc.astype(np.float64))
        L = max(len(got["arcs"]), len(bf["best_arcs"]))
        eps = 2 * 3 * L * 2.0 ** -24 * max(terms[got["arcs"]].sum(), terms[bf["best_arcs"]].sum())  # (three adds per arc)
        assert bf["best"] - eps <= s64[got["arcs"]].sum() <= bf["best"]


def test_the_tie_case_is_really_a_tie():
    """The star against one label that no arc carries: all 200 paths lie at distance 4 and differ in their scores, so
    the score decides -- and the restatement takes the best of them."""
    l = E.star()
    ref = [250]
    assert 250 not in l.label
    theta = synth.label_scores(4, 256)
    s64 = E.score64(l, theta)
    bf = LR.brute_force(l, ref, s64)
    assert bf["distance"] == 4 and len(bf["ties"]) >= 2
    got = LR.of_lattice(l, ref, theta)
    assert got["distance"] == 4 and got["arcs"] == bf["best_arcs"]
    check_result(l, ref, got)
    # without scores the same tie goes to the first arc in canonical order
    assert LR.of_lattice(l, ref)["arcs"][1] == 1


def test_no_candidate_path():
    l = small_lattices()[2]
    theta = synth.label_scores(1, 16)
    theta[synth.EOS] = -np.inf
    got = LR.of_lattice(l, [5, 6], theta)
    assert got["distance"] == -1 and got["score"] == -np.inf and got["arcs"] == [] and got["counts"] == (0, 0, 0)
    assert LR.of_lattice(l, [5, 6])["distance"] >= 0  # (without scores every path counts)


def test_dead_labels_cost_edits():
    """The condition of test_gpu_lattice_edit.test_dead_labels, on the restatement alone: with the dead labels the
    distance is never smaller and strictly greater on at least one lattice."""
    lats, theta, refs = LR.dead_label_case()
    with_dead, without = LR.of_batch(lats, refs, theta), LR.of_batch(lats, refs)
    assert all(a["distance"] >= b["distance"] >= 0 for a, b in zip(with_dead, without))
    assert any(a["distance"] > b["distance"] for a, b in zip(with_dead, without))
    for l, r in zip(lats, with_dead):
        assert not np.isin(l.label[r["arcs"]], E.DEAD).any()


# ----------------------------------------------------------------------------- the C entry point
def test_exports_are_declared():
    from nfst_amd import _lib, ops

    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "nfst_hip.h")).read()
    for name in ("nfst_lattice_edit_ws_bytes", "nfst_lattice_edit"):
        assert name in _lib.EXPORTS and f" {name}(" in header
    assert _lib.ABI_VERSION == 7 and _lib.lib.nfst_abi_version() == 7  # functions were added, no struct changed
    assert ops.lattice_edit_distance is not None and ops.LatticeEditResult._fields == (
        "distance", "score", "paths", "path_arcs", "align", "lengths", "counts")


def test_argument_checks_return_before_any_launch():
    """Every host-side check of nfst_lattice_edit on host pointers: had anything been launched, the outputs would not be
    untouched (and without a GPU the launch itself would have returned NFST_ERR_HIP)."""
    from nfst_amd import _lib, ops
    from nfst_amd.lattice import LatticeBatch

    lats = small_lattices()[:3]
    lat = LatticeBatch.from_synth([synth.layered_lattice(s, n_states=12, avg_degree=2.5, vocab=16, width=3, span=2) for s in range(3)])
    assert lat.device.type == "cpu"
    lib, bs = _lib.lib, C.byref(lat.c_struct())
    theta = np.zeros(16, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    B, R, T = lat.n_lattices, 9, 8
    assert lib.nfst_lattice_edit_ws_bytes(bs, 0) == ERR_ARG and lib.nfst_lattice_edit_ws_bytes(bs, -4) == ERR_ARG
    assert lib.nfst_lattice_edit_ws_bytes(bs, ops.EDIT_MAX_LEN + 1) == ERR_LIMIT
    assert lib.nfst_lattice_edit_ws_bytes(None, R) == ERR_ARG
    ws_bytes = lib.nfst_lattice_edit_ws_bytes(bs, R)
    assert ws_bytes >= lat.total_rows * (R + 1) * 8
    # the workspace grows with R and with the rows
    assert lib.nfst_lattice_edit_ws_bytes(bs, ops.EDIT_MAX_LEN) > lib.nfst_lattice_edit_ws_bytes(bs, 100) > ws_bytes
    wide = LatticeBatch.from_synth(lats)
    assert wide.total_rows > lat.total_rows and lib.nfst_lattice_edit_ws_bytes(C.byref(wide.c_struct()), R) > ws_bytes
    ws = np.zeros(ws_bytes // 8 + 2, np.float64)  # (16-byte aligned by numpy)
    ref, ref_len = np.zeros((B, R), np.int32), np.zeros(B, np.int32)
    outs = dict(dist=np.full(B, 77, np.int32), score=np.full(B, 77, np.float32), paths=np.full((B, T), 77, np.int32),
                arcs=np.full((B, T), 77, np.int32), align=np.full((B, T), 77, np.int32), lens=np.full(B, 77, np.int32),
                counts=np.full((B, 3), 77, np.int32))
    status = np.zeros(1, np.int32)
    p = lambda a: None if a is None else a.ctypes.data

    def call(lat_=bs, sc_=C.byref(sc), ref=ref, ref_len=ref_len, R=R, ws=ws, wsb=ws_bytes, T=T, status=status, **kw):
        o = {**outs, **kw}
        return lib.nfst_lattice_edit(lat_, sc_, p(ref), p(ref_len), R, p(ws), wsb, p(o["dist"]), p(o["score"]), p(o["paths"]),
                                     p(o["arcs"]), p(o["align"]), p(o["lens"]), p(o["counts"]), T, 0, p(status), None)

    for name in ("ref", "ref_len", "ws", "status", "dist", "paths", "lens"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(lat_=None) == ERR_ARG
    assert call(R=0) == ERR_ARG and call(R=-2) == ERR_ARG and call(T=0) == ERR_ARG and call(T=-1) == ERR_ARG
    assert call(R=ops.EDIT_MAX_LEN + 1) == ERR_LIMIT
    assert call(wsb=ws_bytes - 1) == ERR_ARG
    assert call(ws=ws[1:]) == ERR_ARG  # (not 16-byte aligned)
    assert call(sc_=C.byref(_lib.Scores(None, 0, None, None, 0))) == ERR_ARG  # scores without theta
    # nothing to do is not an error, whatever the data pointers
    empty = lat.c_struct().__class__.from_buffer_copy(lat.c_struct())
    empty.n_lattices = 0
    assert call(lat_=C.byref(empty)) == 0 and call(lat_=C.byref(empty), ref=None, ws=None, dist=None) == 0
    assert lib.nfst_lattice_edit_ws_bytes(C.byref(empty), R) == 0
    assert call(lat_=C.byref(empty), status=None) == ERR_ARG
    assert status[0] == 0 and all(np.all(o == 77) for o in outs.values())  # nothing ran


def test_wrapper_validates_before_any_launch():
    import torch

    from nfst_amd import ops
    from nfst_amd.lattice import LatticeBatch

    lat = LatticeBatch.from_synth(small_lattices()[:2])
    ref, n = torch.zeros((2, 5), dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.lattice_edit_distance(lat, ref, n)


def test_build_guard_covers_the_new_kernels():
    from nfst_amd.build import check_resources

    assert check_resources({"k_lattice_edit_sweep<true>": {"vgpr_spill": 0, "scratch": 8}})
    assert check_resources({"k_lattice_edit_walk<false>": {"vgpr_spill": 2, "scratch": 0}})
    assert not check_resources({"k_lattice_edit_sweep<false>": {"vgpr_spill": 0, "scratch": 0, "agprs": 0}})

"""The yardstick of ``nfst_string_viterbi`` and ``nfst_string_sample`` (tests/strings_align_ref.py) against brute force
over every path of the enumerable lattices in both tape modes: the best alignment is the best enumerated path that spells
the string, ``align`` reproduces ``strings_ref.project``, a draw's ``logq`` is its enumerated score less the string's
enumerated mass, and the draws' frequencies follow the enumerated p(path | x, y).  Also, on the reference alone, the cap
on the undecided walks of every case of tests/test_gpu_strings_align.py, and the host-side checks of the C entry points
and the wrappers.  Runs without a GPU.

Tolerance, from float64 arithmetic only: ``logq`` against enumeration is a difference of two sums of at most 16 scores
and a log-sum of exp over at most 3267 paths; the largest difference measured here is 5.3e-15, and the issue's 1e-12 holds.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from nfst_amd import synth
from tests import edge_cases as E
from tests import strings_align_ref as AR
from tests import strings_ref as SR
from tests.test_lattice_edit_cpu import small_lattices

ERR_ARG, ERR_LIMIT = -1, -6
NEG = -np.inf
K_FREQ, SEED_FREQ = 4096, 11  # (the seed is chosen so that the frequencies pass on the reference alone)


def enumerable():
    out = [(f"small{i}", l, 50 + i) for i, l in enumerate(small_lattices())]
    return out + [("grid2", SR.denominator(SR.SMALL), 2), ("tape", SR.tape_lattice(), 3)]


def tapes(l, step=3):
    """a keep set of every ``step``-th label (the fewer labels, the fewer strings and the more paths under each) and a marker"""
    labels = sorted(set(int(x) for x in l.label))
    return [dict(keep=set(labels[1::step])), dict(marker=SR.MARK if SR.MARK in labels else labels[len(labels) // 2])]


@functools.lru_cache(maxsize=None)
def _case(i):
    """(name, lattice, float64 arc scores without ties)"""
    name, l, seed = enumerable()[i]
    theta = synth.label_scores(seed, l.vocab, mean=-1.0, std=0.5)
    asc = np.random.default_rng(seed).normal(0.0, 0.3, size=l.n_arcs).astype(np.float32)
    return name, l, E.score64(l, theta, asc)


def _by_string(l, s64, tape):
    """{string: [(score, arcs), ...] best first} over every path that spells one"""
    _, _, paths = SR.brute_force(l, s64, **tape)
    by = {}
    for sc, p in paths:
        labs = np.asarray(l.label)[p]
        if "marker" in tape and SR.dangling(labs, tape["marker"]):
            continue
        by.setdefault(SR.project(labs, **tape), []).append((float(sc), [int(a) for a in p]))
    return by


def _check_align(l, y, r, tape):
    """the arcs are a path from state 0 to the sink, and align marks exactly the arcs that emit y, in order"""
    labs = [int(l.label[a]) for a in r["arcs"]]
    assert labs == r["labels"] and SR.project(labs, **tape) == tuple(y)
    emitted = [(p, labs[t]) for t, p in enumerate(r["align"]) if p >= 0]
    assert [p for p, _ in emitted] == list(range(len(y))) and [x for _, x in emitted] == list(y)
    if "keep" in tape:
        assert [p >= 0 for p in r["align"]] == [x in tape["keep"] for x in labs]
    else:  # a symbol directly follows an active marker, which emits nothing itself
        for t, p in enumerate(r["align"]):
            assert p < 0 or (labs[t - 1] == tape["marker"] and r["align"][t - 1] < 0)


@pytest.mark.parametrize("case", range(6))
def test_best_alignment_and_logq_against_enumeration(case):
    name, l, s64 = _case(case)
    worst = 0.0
    for tape in tapes(l):
        by = _by_string(l, s64, tape)
        for y, members in by.items():
            al = AR.Aligner(l, s64, y, **tape)
            num, _ = SR.string_log_prob(l, s64, y, **tape)
            assert np.float64(al.log_num).view(np.int64) == np.float64(num).view(np.int64)  # G0[0][0], bit for bit
            assert len(members) < 2 or members[0][0] > members[1][0]  # (no ties)
            v = al.viterbi()
            assert v["arcs"] == members[0][1] and abs(v["score"] - members[0][0]) <= 1e-12, (name, tape, y)
            _check_align(l, y, v, tape)
            mass = float(SR._lse_rows(np.asarray([m[0] for m in members])[:, None])[0])
            u = AR.uniforms(case * 1000 + len(y), (8, l.n_rows))
            for k in range(8):
                w = al.walk(u[k])
                _check_align(l, y, w, tape)
                want = dict((tuple(p), sc) for sc, p in members)[tuple(w["arcs"])] - mass
                worst = max(worst, abs(w["logq"] - want), abs(al.path_logq(w["arcs"]) - want))
            assert v["score"] <= al.log_num + 1e-12 and (len(members) > 1 or abs(v["score"] - al.log_num) <= 1e-12)
        # strings that no path spells
        y0 = max(by, key=len)
        for y in (tuple(y0) + y0[-1:], tuple(y0) + (int(l.label.max()),) * 2):
            if y not in by:
                al = AR.Aligner(l, s64, y, **tape)
                assert al.viterbi() == dict(arcs=[], labels=[], align=[], length=0, score=NEG)
                assert al.walk(np.zeros(l.n_rows, np.float32))["length"] == 0
    print(f"{name}: logq against enumeration {worst:.3g}")
    assert worst <= 1e-12


@pytest.mark.parametrize("case", range(6))
def test_draw_frequencies_follow_the_enumerated_posterior(case):
    """K = 4096 draws per string: every path of probability >= 0.01 within five binomial standard deviations"""
    name, l, s64 = _case(case)
    for tape in tapes(l, 5):
        for y, members in _by_string(l, s64, tape).items():
            if len(members) < 2:
                continue
            al = AR.Aligner(l, s64, y, **tape)
            mass = float(SR._lse_rows(np.asarray([m[0] for m in members])[:, None])[0])
            u = AR.uniforms(SEED_FREQ + 7 * case + len(y), (K_FREQ, l.n_rows))
            counts = {}
            for k in range(K_FREQ):
                a = tuple(al.walk(u[k])["arcs"])
                counts[a] = counts.get(a, 0) + 1
            for sc, p in members:
                q = float(np.exp(sc - mass))
                if q >= 0.01:
                    sd = np.sqrt(q * (1.0 - q) / K_FREQ)
                    assert abs(counts.get(tuple(p), 0) / K_FREQ - q) <= 5.0 * sd + 1e-12, (name, tape, y, q)


def test_the_gpu_cases_stay_under_the_cap_on_undecided_walks():
    """Every case of the GPU file: the share of walks whose margin is at most DECIDED is at most CAP (float32 uniforms:
    a walk of 140 deciding steps is undecided with probability about 3e-4); the star's draws land in every chunk."""
    for name, case in AR.sample_cases().items():
        al = AR.aligners(case)
        U = case["uniforms"]
        walks = [al[b][m].walk(U[b, m, k]) for b in range(U.shape[0]) for m in range(U.shape[1]) for k in range(U.shape[2])]
        share = sum(w["margin"] <= AR.DECIDED for w in walks) / len(walks)
        print(f"{name}: {len(walks)} walks, undecided share {share:.4f}")
        assert share <= AR.CAP, name
        assert max(w["length"] for w in walks) < case["L"]
        if name == "star keep 5":
            first = al[0][0].out[1][0]
            assert {(w["arcs"][1] - first) // 64 for w in walks} == {0, 1, 2, 3}
        if name == "star keep all":
            assert sorted((w["arcs"][1] - al[0][0].out[1][0]) // 64 for w in walks) == [0, 1, 3]
            assert all(len(al[0][m].step_probs(1, 1, 0)[5]) == 1 for m in range(3))  # one live arc per string


def test_the_register_rule_covers_the_new_kernels():
    from nfst_amd.build import check_resources

    for k in ("k_string_viterbi_sweep<true>", "k_string_viterbi_sweep<false>", "k_string_walk<true, false>", "k_string_walk<false, true>"):
        assert check_resources({k: {"vgpr_spill": 1, "scratch": 0}}) and check_resources({k: {"vgpr_spill": 0, "scratch": 16}})
        assert not check_resources({k: {"vgpr_spill": 0, "scratch": 0, "sgpr_spill": 3}})


def _host_batch():
    from nfst_amd.lattice import LatticeBatch

    lat = LatticeBatch.from_synth([synth.layered_lattice(s, n_states=12, avg_degree=2.5, vocab=16, width=3, span=2) for s in range(3)])
    assert lat.device.type == "cpu"
    return lat


@pytest.mark.parametrize("entry", ["nfst_string_viterbi", "nfst_string_sample"])
def test_argument_checks_return_before_any_launch(entry):
    from nfst_amd import _lib, ops

    lat = _host_batch()
    lib, bs = _lib.lib, C.byref(lat.c_struct())
    theta = np.zeros(16, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    B, M, N, V, K, L = lat.n_lattices, 4, 9, 16, 3, 12
    sample = entry == "nfst_string_sample"
    Q, QF = getattr(lib, entry + "_ws_bytes"), lib.nfst_string_logprob_ws_bytes
    assert Q(bs, M, 0, 0) == ERR_ARG and Q(bs, -1, N, 0) == ERR_ARG and Q(None, M, N, 0) == ERR_ARG
    assert Q(bs, M, ops.EDIT_MAX_LEN + 1, 0) == ERR_LIMIT
    assert all(Q(bs, m, N, mk) == QF(bs, m, N, mk) for m in (0, 1, M) for mk in (0, 1))  # the layout of the sum sweep, nothing more
    ws_bytes = Q(bs, M, N, 0)
    ws = np.zeros(Q(bs, M, N, 1) // 8 + 2, np.float64)  # (16-byte aligned by numpy)
    lead = (B, M, K) if sample else (B, M)
    a = dict(y=np.zeros((B, M, N), np.int32), n=np.zeros((B, M), np.int32), keep=np.ones(V, np.uint8), ws=ws, num=np.full((B, M), 77.0),
             z=np.full(B, 77.0), score=np.full(lead, 77.0), logq=np.full(lead, 77.0), paths=np.full(lead + (L,), 77, np.int32),
             arcs=np.full(lead + (L,), 77, np.int32), align=np.full(lead + (L,), 77, np.int32), lens=np.full(lead, 77, np.int32),
             status=np.zeros(1, np.int32))
    outs = ("num", "z", "score", "logq", "paths", "arcs", "align", "lens") if sample else ("score", "paths", "arcs", "align", "lens")
    p = lambda x: None if x is None else x.ctypes.data

    def call(lat_=bs, sc_=C.byref(sc), M=M, N=N, marker=-1, wsb=ws_bytes, K=K, m0=0, max_len=L, **kw):
        o = {**a, **kw}
        head = (lat_, sc_, p(o["y"]), p(o["n"]), M, N, p(o["keep"]), marker)
        if sample:
            return lib.nfst_string_sample(*head, K, m0, None, 5, max_len, 0, p(o["ws"]), wsb, *(p(o[k]) for k in outs), p(o["status"]), None)
        return lib.nfst_string_viterbi(*head, max_len, 0, p(o["ws"]), wsb, *(p(o[k]) for k in outs), p(o["status"]), None)

    for name in ("y", "n", "ws", "status") + outs:
        assert call(**{name: None}) == ERR_ARG, name
    assert call(lat_=None) == ERR_ARG and call(sc_=None) == ERR_ARG
    assert call(sc_=C.byref(_lib.Scores(None, 0, None, None, 0))) == ERR_ARG
    assert call(marker=4) == ERR_ARG and call(keep=None) == ERR_ARG  # both tapes, neither
    assert call(keep=None, marker=V) == ERR_ARG and call(keep=None, marker=-3) == ERR_ARG
    assert call(N=0) == ERR_ARG and call(M=-1) == ERR_ARG and call(N=ops.EDIT_MAX_LEN + 1) == ERR_LIMIT
    assert call(max_len=0) == ERR_ARG
    if sample:
        assert call(K=0) == ERR_ARG and call(m0=-1) == ERR_ARG
        assert call(K=(2 ** 31 - 1) // (B * M) + 1) == ERR_LIMIT  # more than 2^31 - 1 walks
    assert call(wsb=ws_bytes - 1) == ERR_ARG and call(ws=ws[1:]) == ERR_ARG
    assert call(keep=None, marker=4, wsb=ws_bytes) == ERR_ARG  # (marker mode needs the larger workspace)
    assert call(M=0) == 0 and call(M=0, y=None, n=None, ws=None, **{k: None for k in outs}) == 0  # no candidate: a no-op
    empty = lat.c_struct().__class__.from_buffer_copy(lat.c_struct())
    empty.n_lattices = 0
    assert call(lat_=C.byref(empty)) == 0 and Q(C.byref(empty), M, N, 0) == 0
    assert all(np.all(a[k] == 77) for k in outs) and a["status"][0] == 0  # nothing was launched, nothing written


def test_wrappers_validate_before_any_launch():
    import torch

    from nfst_amd import ops
    from nfst_amd.lattice import LatticeBatch
    from nfst_amd.scorers import LatticeScorer

    lat = LatticeBatch.from_synth(small_lattices()[:2])
    y, n = torch.zeros((2, 1, 5), dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int32)
    th = torch.zeros(lat.vocab)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.string_viterbi(lat, th, y, n, marker=4)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.string_sample_paths(lat, th, y, n, 2, marker=4)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.string_alignment_log_prob(lat, th, y, n, torch.zeros((2, 1, 2, 3), dtype=torch.int32), torch.zeros((2, 1, 2), dtype=torch.int32), marker=4)
    for k in (0, True, 2.0):
        with pytest.raises(ValueError):
            ops.string_sample_paths(lat, th, y, n, k, marker=4)
    for f in (ops.string_viterbi, ops.string_sample_paths, ops.string_alignment_log_prob, LatticeScorer.align, LatticeScorer.sample_alignments):
        assert f.__doc__ and len(f.__doc__) > 200
    assert "NFST_ERR_LENGTH" in ops.string_viterbi.__doc__ and "uniforms" in ops.string_sample_paths.__doc__
    assert ops.StringAlignment._fields == ("score", "paths", "arcs", "align", "lengths")
    assert ops.StringSampleResult._fields == ("paths", "arcs", "align", "lengths", "score", "logq", "log_num", "logz")

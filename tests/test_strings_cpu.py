"""The yardsticks of ``nfst_merge_paths`` and ``nfst_string_logprob`` (tests/strings_ref.py) against brute force over every
path and against ``intersect_wide_ref.live_sets`` on the matching automata, the two facts the GPU tests lean on (the
best string is not the Viterbi path's; a product beyond the row limit), and the C entry points' host-side checks on host
pointers.  Runs without a GPU; tests/test_gpu_strings.py holds the kernels to the same restatements."""
import ctypes as C
import math

import numpy as np
import pytest

from nfst_amd import synth
from nfst_amd.constraints import WideDFA
from tests import edge_cases as E
from tests import intersect_wide_ref as IW
from tests import strings_ref as SR
from tests.test_lattice_edit_cpu import small_lattices

ERR_ARG, ERR_LIMIT = -1, -6
TOL = 1e-12  # float64 round-off between two restatements (tests/test_expectation_cpu.py, tests/test_swor_cpu.py)
NEG = -np.inf


def enumerable():
    """(name, lattice, theta seed, keep, marker): the four small lattices and the two denominator grids"""
    out = [(f"small{i}", l, 50 + i) for i, l in enumerate(small_lattices())]
    out += [("seed1", SR.denominator(SR.SEED1), 1), ("grid2", SR.denominator(SR.SMALL), 2), ("tape", SR.tape_lattice(), 3)]
    return out


def tapes(l):
    labels = sorted(set(int(x) for x in l.label))
    return [dict(keep=set(labels[1::2])), dict(marker=SR.MARK if SR.MARK in labels else labels[len(labels) // 2])]


def test_projection():
    P = SR.project
    assert P([1, 4, 8, 3, 6, 4, 9, 2], marker=4) == (8, 9) and P([1, 4, 8, 3, 6, 4, 9, 2], keep={8, 6, 2}) == (8, 6, 2)
    assert P([4, 4, 4, 4, 7], marker=4) == (4, 4) and P([4, 4, 4, 7], marker=4) == (4, 7)  # a symbol that is the marker
    assert P([3, 4], marker=4) == () and SR.dangling([3, 4], 4) and not SR.dangling([4, 4], 4) and SR.dangling([4, 4, 4], 4)
    assert P([5, 6], None, None) == (5, 6) and P([], marker=4) == ()


def test_the_weight_arithmetic_is_exp_and_log():
    rng = np.random.default_rng(0)
    for x in np.concatenate([-rng.exponential(3.0, 300), [0.0, -1e-300, -699.9, -50.0]]):
        assert abs(SR.sm_exp(x) - math.exp(x)) <= 4e-16 * math.exp(x)
    assert SR.sm_exp(0.0) == 1.0 and SR.sm_exp(-701.0) == 0.0 and SR.sm_exp(-np.inf) == 0.0
    for s in np.concatenate([1.0 + rng.exponential(5.0, 300), [1.0, 2.0, 1024.0, 1.4142135623730951, 1.4142135623730949]]):
        assert abs(SR.sm_log(s) - math.log(s)) <= 4e-16 * max(math.log(s), 1.0)
    assert SR.sm_log(1.0) == 0.0 and SR.merged_weight([-3.25]) == -3.25
    ws = rng.normal(-5, 2, 40)
    assert abs(SR.merged_weight(list(ws)) - float(np.logaddexp.reduce(ws))) <= TOL


@pytest.mark.parametrize("case", range(7))
def test_recurrence_equals_brute_force(case):
    name, l, seed = enumerable()[case]
    theta = synth.label_scores(seed, l.vocab, mean=-1.0, std=0.5)
    s64 = E.score64(l, theta)
    for tape in tapes(l):
        by, logz, paths = SR.brute_force(l, s64, **tape)
        strings = sorted(by, key=lambda y: -by[y])
        some = strings if len(strings) <= 120 else strings[:40] + strings[40::max(1, len(strings) // 60)]
        total = []
        for y in some:
            num, z = SR.string_log_prob(l, s64, y, **tape)
            assert abs(num - by[y]) <= TOL and abs(z - logz) <= TOL, (name, tape, y)
            total.append(num)
        if len(some) == len(strings):  # the per-string sums add up to Z (less the paths that end on a marker)
            lost = [sc for sc, p in paths if "marker" in tape and SR.dangling(l.label[p], tape["marker"])]
            assert abs(np.logaddexp.reduce(total + lost) - logz) <= TOL, (name, tape)
            assert name != "tape" or "keep" in tape or len(lost) > 0
        # strings that no path spells: one symbol more than the longest, one less than the shortest non-empty one, a foreign symbol
        longest = max(strings, key=len)
        for y in (longest + (longest[-1],) if longest else (int(l.label[0]),), (max(l.label) + 0,) * 40):
            if tuple(y) not in by:
                assert SR.string_log_prob(l, s64, y, **tape)[0] == NEG, (name, tape, y)


@pytest.mark.parametrize("case", range(7))
def test_acceptance_is_that_of_the_automata(case):
    """A string has weight > -inf exactly when the product with ``projected_sequence`` / ``marked_sequence`` is not empty."""
    name, l, seed = enumerable()[case]
    s64 = E.score64(l, synth.label_scores(seed, l.vocab))
    rng = np.random.default_rng(case)
    for tape in tapes(l):
        by, _, _ = SR.brute_force(l, s64, **tape)
        ys = list(by)[:: max(1, len(by) // 6)][:6]
        alphabet = sorted(tape["keep"]) if "keep" in tape else sorted(set(int(x) for x in l.label))
        ys += [tuple(rng.choice(alphabet, size=n)) for n in (1, 2, 3)] + [()]
        if ys[0]:
            ys += [ys[0][:-1], ys[0] + ys[0][-1:]]
        hits = 0
        for y in ys:
            y = [int(t) for t in y]
            if "keep" in tape:
                dfa = WideDFA.projected_sequence(l.vocab, tape["keep"], y)
            else:
                dfa = WideDFA.marked_sequence(l.vocab, tape["marker"], y)
            live = bool(IW.live_sets(l, *dfa.to_dense(l.vocab))[0, 0])
            assert live == (SR.string_log_prob(l, s64, y, **tape)[0] > NEG) == (tuple(y) in by), (name, tape, y)
            hits += live
        assert 0 < hits < len(ys) or name == "tape"


def test_the_tape_lattice_has_its_corners():
    l = SR.tape_lattice()
    by, logz, paths = SR.brute_force(l, np.zeros(l.n_arcs), marker=SR.MARK)
    labs = [tuple(int(x) for x in l.label[p]) for _, p in paths]
    assert any(SR.dangling(x, SR.MARK) for x in labs) and any(SR.MARK in SR.project(x, marker=SR.MARK) for x in labs)
    assert (SR.MARK,) in by and (8, 8) in by and sum(len(v) for v in [by]) >= 1
    assert np.logaddexp.reduce(list(by.values())) < logz - 0.1  # the dangling paths' share is missing


def test_merge_restatement():
    paths = np.array([[[1, 4, 8, 2, 0], [1, 4, 8, 3, 2], [1, 3, 2, 0, 0], [1, 4, 9, 2, 0], [1, 4, 8, 2, 0], [4, 4, 4, 4, 4]]])
    lens = np.array([[4, 5, 3, 4, 4, 9]])
    w = np.array([[-1.0, -0.5, -2.0, np.nan, -1.0, 0.0]])
    m = SR.merge(paths, lens, w, marker=4, pad=0)
    assert m["n_strings"][0] == 2 and m["group"][0].tolist() == [0, 0, 1, -1, 0, -1]  # (NaN and the bad length are invalid)
    assert m["strings"][0, 0].tolist() == [8, 0, 0, 0, 0] and m["lengths"][0].tolist() == [1, 0, 0, 0, 0, 0]
    assert m["first"][0].tolist() == [1, 2, -1, -1, -1, -1]
    assert abs(m["log_weights"][0, 0] - np.logaddexp.reduce([-1.0, -0.5, -1.0])) <= TOL and m["log_weights"][0, 1] == -2.0
    ident = SR.merge(paths, lens, w, n_paths=[5])
    assert ident["n_strings"][0] == 3 and ident["group"][0].tolist() == [0, 1, 2, -1, 0, -1]  # weights -0.307, -0.5, -2


# ----------------------------------------------------------------------------- the facts the GPU tests lean on
def test_the_best_string_is_not_the_viterbi_string():
    l = SR.denominator(SR.SEED1)
    assert l.n_rows == 78
    theta = synth.label_scores(1, 12, mean=-1.0, std=0.5)
    by, logz, paths = SR.brute_force(l, E.score64(l, theta), marker=SR.MARK)
    assert len(paths) == 1948 and len(by) == 40
    counts = {}
    for _, p in paths:
        y = SR.project(l.label[p], marker=SR.MARK)
        counts[y] = counts.get(y, 0) + 1
    assert min(counts.values()) == 1 and max(counts.values()) == 63
    top = [(sc, SR.project(l.label[p], marker=SR.MARK)) for sc, p in paths[:64]]
    assert len({y for _, y in top}) == 10
    assert top[0][1] == () and max(by, key=by.get) == (8,)
    mass = {}
    for sc, y in top:
        mass[y] = np.logaddexp(mass.get(y, NEG), sc)
    assert max(mass, key=mass.get) == (8,)  # summing the 64 best paths by string recovers it


def test_the_layered_product_exceeds_the_row_limit():
    l, keep, y = SR.layered_case()
    assert len(y) == 28
    live = IW.live_sets(l, *WideDFA.projected_sequence(12, keep, y).to_dense(12))
    assert int(live.sum()) == 15934 > 8192
    num, z = SR.string_log_prob(l, E.score64(l, synth.label_scores(2, 12)), y, keep=keep)
    assert NEG < num < z


# ----------------------------------------------------------------------------- the C entry points
def test_exports_are_declared():
    from nfst_amd import _lib, decoders, ops

    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "nfst_hip.h")).read()
    for name in ("nfst_merge_paths", "nfst_string_logprob_ws_bytes", "nfst_string_logprob"):
        assert name in _lib.EXPORTS and f" {name}(" in header
    assert _lib.ABI_VERSION == 7 and _lib.lib.nfst_abi_version() == 7  # functions were added, no struct changed
    assert ops.StringSet._fields == ("strings", "lengths", "log_weights", "n_strings", "group", "first")
    assert ops.StringScores._fields == ("log_num", "logz", "log_prob")
    assert decoders.StringDecodeResult._fields == ("strings", "lengths", "log_prob", "n_strings", "path_mass", "first_path")
    assert ops.merge_paths is not None and ops.string_log_prob is not None


def test_build_guard_covers_the_new_kernels():
    from nfst_amd.build import check_resources

    assert check_resources({"k_merge_paths": {"vgpr_spill": 0, "scratch": 8}})
    assert check_resources({"k_string_logprob<true>": {"vgpr_spill": 2, "scratch": 0}})
    assert not check_resources({"k_string_logprob<false>": {"vgpr_spill": 0, "scratch": 0, "sgpr_spill": 5}, "k_merge_paths": {}})


def test_merge_argument_checks_return_before_any_launch():
    from nfst_amd import _lib, ops

    lib = _lib.lib
    B, K, L, V = 2, 3, 5, 12
    a = dict(paths=np.zeros((B, K, L), np.int32), lens=np.zeros((B, K), np.int32), w=np.zeros((B, K)), n=np.full(B, K, np.int32),
             keep=np.ones(V, np.uint8), scratch=np.full((B, K, L), 77, np.int32), strings=np.full((B, K, L), 77, np.int32),
             olen=np.full((B, K), 77, np.int32), ow=np.full((B, K), 77.0), ns=np.full(B, 77, np.int32), group=np.full((B, K), 77, np.int32),
             first=np.full((B, K), 77, np.int32), status=np.zeros(1, np.int32))
    p = lambda x: None if x is None else x.ctypes.data

    def call(B=B, K=K, L=L, V=V, marker=-1, bits=64, **kw):
        o = {**a, **kw}
        return lib.nfst_merge_paths(p(o["paths"]), p(o["lens"]), p(o["w"]), p(o["n"]), B, K, L, p(o["keep"]), V, marker, bits, 0,
                                    p(o["scratch"]), p(o["strings"]), p(o["olen"]), p(o["ow"]), p(o["ns"]), p(o["group"]), p(o["first"]),
                                    p(o["status"]), None)

    for name in ("paths", "lens", "w", "scratch", "strings", "olen", "ow", "ns", "group", "first", "status"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(marker=4) == ERR_ARG  # both tapes
    assert call(keep=None, marker=V) == ERR_ARG and call(keep=None, marker=-2) == ERR_ARG and call(V=0) == ERR_ARG
    assert call(bits=0) == ERR_ARG and call(bits=65) == ERR_ARG and call(L=0) == ERR_ARG and call(K=-1) == ERR_ARG and call(B=-1) == ERR_ARG
    assert call(K=ops.MERGE_MAX_K + 1) == ERR_LIMIT and call(L=ops.EDIT_MAX_LEN + 1) == ERR_LIMIT
    assert call(B=0) == 0 and call(K=0) == 0 and call(K=0, paths=None, strings=None, ns=None) == 0  # nothing to do
    assert call(K=0, status=None) == ERR_ARG
    assert a["status"][0] == 0 and all(np.all(a[k] == 77) for k in ("scratch", "strings", "olen", "ow", "ns", "group", "first"))


def test_string_logprob_argument_checks_return_before_any_launch():
    from nfst_amd import _lib, ops
    from nfst_amd.lattice import LatticeBatch

    lat = LatticeBatch.from_synth([synth.layered_lattice(s, n_states=12, avg_degree=2.5, vocab=16, width=3, span=2) for s in range(3)])
    assert lat.device.type == "cpu"
    lib, bs = _lib.lib, C.byref(lat.c_struct())
    theta = np.zeros(16, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    B, M, N = lat.n_lattices, 4, 9
    Q = lib.nfst_string_logprob_ws_bytes
    assert Q(bs, M, 0, 0) == ERR_ARG and Q(bs, -1, N, 0) == ERR_ARG and Q(None, M, N, 0) == ERR_ARG
    assert Q(bs, M, ops.EDIT_MAX_LEN + 1, 0) == ERR_LIMIT
    ws_bytes = Q(bs, M, N, 0)
    assert ws_bytes >= lat.total_rows * (N + 1) * M * 8
    assert Q(bs, M, N, 1) >= ws_bytes + lat.total_rows * (N + 1) * M * 8  # two rows per state in marker mode
    assert Q(bs, 2 * M, N, 0) > ws_bytes > Q(bs, 0, N, 0) > 0
    ws = np.zeros(Q(bs, M, N, 1) // 8 + 2, np.float64)  # (16-byte aligned by numpy)
    a = dict(y=np.zeros((B, M, N), np.int32), n=np.zeros((B, M), np.int32), keep=np.ones(16, np.uint8), ws=ws,
             num=np.full((B, M), 77.0), z=np.full(B, 77.0), status=np.zeros(1, np.int32))
    p = lambda x: None if x is None else x.ctypes.data

    def call(lat_=bs, sc_=C.byref(sc), M=M, N=N, marker=-1, wsb=ws_bytes, **kw):
        o = {**a, **kw}
        return lib.nfst_string_logprob(lat_, sc_, p(o["y"]), p(o["n"]), M, N, p(o["keep"]), marker, p(o["ws"]), wsb, p(o["num"]), p(o["z"]),
                                       p(o["status"]), None)

    for name in ("y", "n", "ws", "num", "z", "status"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(lat_=None) == ERR_ARG and call(sc_=None) == ERR_ARG
    assert call(sc_=C.byref(_lib.Scores(None, 0, None, None, 0))) == ERR_ARG
    assert call(marker=4) == ERR_ARG and call(keep=None) == ERR_ARG  # both tapes, neither
    assert call(keep=None, marker=16) == ERR_ARG and call(keep=None, marker=-3) == ERR_ARG
    assert call(N=0) == ERR_ARG and call(M=-1) == ERR_ARG and call(N=ops.EDIT_MAX_LEN + 1) == ERR_LIMIT
    assert call(wsb=ws_bytes - 1) == ERR_ARG and call(ws=ws[1:]) == ERR_ARG
    assert call(keep=None, marker=4, wsb=ws_bytes) == ERR_ARG  # (marker mode needs the larger workspace)
    empty = lat.c_struct().__class__.from_buffer_copy(lat.c_struct())
    empty.n_lattices = 0
    assert call(lat_=C.byref(empty)) == 0 and call(lat_=C.byref(empty), y=None, ws=None, num=None) == 0
    assert Q(C.byref(empty), M, N, 0) == 0 and call(lat_=C.byref(empty), status=None) == ERR_ARG
    assert a["status"][0] == 0 and np.all(a["num"] == 77.0) and np.all(a["z"] == 77.0)  # nothing ran


def test_wrappers_validate_before_any_launch():
    import torch

    from nfst_amd import decoders, ops
    from nfst_amd.lattice import LatticeBatch

    lat = LatticeBatch.from_synth(small_lattices()[:2])
    y, n = torch.zeros((2, 1, 5), dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.string_log_prob(lat, torch.zeros(lat.vocab), y, n, marker=4)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.merge_paths(y, n, torch.zeros((2, 1)), marker=4)
    with pytest.raises(ValueError):
        decoders.decode_strings(lat, torch.zeros(lat.vocab), 4)
    with pytest.raises(ValueError):
        decoders.decode_strings(lat, torch.zeros(lat.vocab), 4, keep={3}, marker=4)

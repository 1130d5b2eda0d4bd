"""The yardstick of ``nfst_string_prefix``, ``nfst_string_next`` and ``decoders.prefix_search``
(tests/strings_prefix_ref.py) against brute force over every path of the seven enumerable lattices of
tests/test_strings_cpu.py in both tape modes, the identities that tie its outputs together, the restated search on the
78-row grid, and the C entry points' host-side checks on host pointers.  Runs without a GPU;
tests/test_gpu_strings_prefix.py holds the kernels to the same restatement.

Tolerance, from float64 arithmetic only.  Measured here, the largest absolute difference between the restatement and
brute force over all cases: 3.6e-15 (log_prefix by both routes, eos, next, the identity and next against log_prefix
alike; the empty prefix against log Z 8.9e-16): both sides are log-sums of exp over up to 1948 paths; x 16 = 5.7e-14,
rounded up to a power of ten: BRUTE = 1e-13.
"""
import ctypes as C

import numpy as np
import pytest

from nfst_amd import synth
from tests import edge_cases as E
from tests import strings_prefix_ref as PR
from tests import strings_ref as SR
from tests.test_strings_cpu import enumerable, tapes

ERR_ARG, ERR_LIMIT = -1, -6
BRUTE = 1e-13
NEG = -np.inf
MEASURED = {}


def rec(tag, err):
    MEASURED[tag] = max(MEASURED.get(tag, 0.0), float(err))
    print(f"{tag}: {float(err):.3g}")
    return float(err)


def _case(i):
    name, l, seed = enumerable()[i]
    theta = synth.label_scores(seed, l.vocab, mean=-1.0, std=0.5)
    return name, l, E.score64(l, theta)


def _close(tag, got, want, where):
    """-inf exactly where brute force has it, BRUTE elsewhere"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert not np.isnan(got).any() and np.array_equal(np.isneginf(got), np.isneginf(want)), (tag, where)
    live = ~np.isneginf(want)
    if live.any():
        assert rec(tag, np.abs(got[live] - want[live]).max()) <= BRUTE, (tag, where)


def _brute_prefix(by, y):
    return PR._lse(w for s, w in by.items() if s[:len(y)] == tuple(y))


@pytest.mark.parametrize("case", range(7))
def test_restatement_equals_brute_force(case):
    """log_prefix, eos and next for every prefix of every string and for one symbol more than any path spells; the
    identity exp(log_prefix) = exp(eos) + sum_v exp(next[v]); next[v] = log_prefix of y.v; eos = string_log_prob."""
    name, l, s64 = _case(case)
    for tape in tapes(l):
        by, logz, paths = SR.brute_force(l, s64, **tape)
        prefixes = sorted({y[:i] for y in by for i in range(len(y) + 1)})
        if len(prefixes) > 60:
            prefixes = prefixes[:30] + prefixes[30::max(1, len(prefixes) // 30)]
        longest = max(by, key=len)
        prefixes += [longest + (longest[-1] if longest else int(l.label[0]),), (int(max(l.label)),) * 5]
        for y in prefixes:
            where = (name, sorted(tape), y)
            nxt, eos, log_prefix, z = PR.next_log_probs(l, s64, list(y), **tape)
            want = _brute_prefix(by, y)
            _close("brute log_prefix (F route)", log_prefix, want, where)
            h, hz = PR.prefix_log_prob(l, s64, list(y), **tape)
            _close("brute log_prefix (H route)", h, want, where)
            _close("brute eos", eos, by.get(tuple(y), NEG), where)
            _close("brute next", nxt, [_brute_prefix(by, tuple(y) + (v,)) for v in range(l.vocab)], where)
            assert abs(z - logz) <= BRUTE and abs(hz - logz) <= BRUTE
            if log_prefix > NEG:
                assert rec("identity", abs(PR._lse([eos] + list(nxt)) - h)) <= BRUTE, where
            num, _ = SR.string_log_prob(l, s64, list(y), **tape)
            _close("eos against string_log_prob", eos, num, where)
            for v in np.nonzero(nxt > NEG)[0][:3]:
                _close("next against log_prefix", nxt[v], PR.prefix_log_prob(l, s64, list(y) + [int(v)], **tape)[0], where)
            if "keep" in tape:  # a label off the tape is never a next symbol
                assert all(nxt[v] == NEG for v in range(l.vocab) if v not in tape["keep"])
        # the empty prefix: log Z, in marker mode less the share of the paths that end on a marker
        lost = [sc for sc, p in paths if "marker" in tape and SR.dangling(l.label[p], tape["marker"])]
        empty = PR.prefix_log_prob(l, s64, [], **tape)[0]
        assert rec("empty prefix", abs(np.logaddexp(empty, PR._lse(lost)) - logz)) <= BRUTE, (name, tape)
        assert "marker" in tape or abs(empty - logz) <= BRUTE
    assert name != "tape" or (len(lost) > 0 and (SR.MARK,) in by)  # a dangling marker, and a symbol equal to the marker


def test_the_search_finds_the_best_string_of_the_grid():
    l = SR.denominator(SR.SEED1)
    s64 = E.score64(l, synth.label_scores(1, 12, mean=-1.0, std=0.5))
    by, logz, _ = SR.brute_force(l, s64, marker=SR.MARK)
    assert len(by) == 40
    r = PR.prefix_search(l, s64, k=2, marker=SR.MARK)
    best = max(by, key=by.get)
    assert r["strings"][0] == (8,) == best  # (the Viterbi path spells the empty string)
    assert abs(r["log_prob"][0] - (by[best] - logz)) <= BRUTE
    ranked = sorted(by, key=lambda y: -by[y])
    for k in (1, 8, 64):  # whatever is certified is the argmax; a list as long as the lattice has strings is the whole ranking
        r = PR.prefix_search(l, s64, k=k, marker=SR.MARK)
        assert not r["exact"] or r["strings"][0] == best
        assert all(abs(lp - (by[y] - logz)) <= BRUTE for y, lp in zip(r["strings"], r["log_prob"]))
    assert set(r["strings"]) == set(ranked) and len(r["strings"]) == 40 and r["exact"] and r["bound"] == NEG
    assert np.abs(r["log_prob"] - np.array([by[y] - logz for y in ranked])).max() <= BRUTE  # (permutations of a string tie)
    # max_len = 0: the empty string alone is complete, everything else is set aside
    r = PR.prefix_search(l, s64, k=1, max_len=0, marker=SR.MARK)
    rest = PR._lse(w for y, w in by.items() if y)
    assert r["strings"] == [()] and not r["exact"] and abs(r["bound"] - (rest - logz)) <= BRUTE and r["steps"] == 1


def test_the_search_certifies_the_best_string_of_the_grid_at_k_2():
    """At k = 2 the restated search returns (8,) first with ``exact`` true.  The length-synchronous phase alone cannot
    certify it (``reserve=0, refine_steps=0``): the three symbols 8, 9 and 10 weigh about the same, so step 0 keeps the
    prefixes (8,) and (9,) and prunes (10,), whose log share -1.2397 is far above log p((8,)) = -2.9654, and the heaviest
    mass ever pruned is the bound.  With the pruned extensions set aside and taken up again, seven steps in all leave
    nothing unexplored that outweighs (8,).  A reserve too small for what must be set aside drops entries and says so."""
    l = SR.denominator(SR.SEED1)
    s64 = E.score64(l, synth.label_scores(1, 12, mean=-1.0, std=0.5))
    by, logz, _ = SR.brute_force(l, s64, marker=SR.MARK)
    best = max(by, key=by.get)
    r = PR.prefix_search(l, s64, k=2, marker=SR.MARK)
    print("bound", r["bound"], "first", r["log_prob"][0], "steps", r["steps"])
    assert r["strings"][0] == (8,) == best and r["exact"]
    assert r["bound"] <= r["log_prob"][0] and r["steps"] == 7
    plain = PR.prefix_search(l, s64, k=2, marker=SR.MARK, reserve=0, refine_steps=0)
    pruned = PR._lse(w for s, w in by.items() if s[:1] == (10,))
    assert plain["strings"][0] == (8,) and not plain["exact"] and plain["steps"] == 3 and abs(plain["bound"] - (pruned - logz)) <= BRUTE
    for kw in (dict(k=1), dict(k=8), dict(k=2, reserve=3), dict(k=2, refine_steps=2), dict(k=2, keep_mode=True)):
        tape = dict(keep={8, 9, 10}) if kw.pop("keep_mode", False) else dict(marker=SR.MARK)
        r = PR.prefix_search(l, s64, **tape, **kw)
        assert r["strings"][0] == best and (not r["exact"] or r["bound"] <= r["log_prob"][0]), kw
        assert all(abs(lp - (by[y] - logz)) <= BRUTE for y, lp in zip(r["strings"], r["log_prob"]))
    small = PR.prefix_search(l, s64, k=2, marker=SR.MARK, reserve=3)
    cut = PR.prefix_search(l, s64, k=2, marker=SR.MARK, refine_steps=2)
    assert not small["exact"] and not cut["exact"] and cut["steps"] == 5 and cut["bound"] > cut["log_prob"][0]


# ----------------------------------------------------------------------------- the C entry points
def test_exports_are_declared():
    from nfst_amd import _lib, decoders, ops
    from nfst_amd.scorers import LatticeScorer

    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "nfst_hip.h")).read()
    for name in ("nfst_string_prefix_ws_bytes", "nfst_string_prefix", "nfst_string_next_ws_bytes", "nfst_string_next"):
        assert name in _lib.EXPORTS and f" {name}(" in header
    assert _lib.ABI_VERSION == 7 and _lib.lib.nfst_abi_version() == 7  # functions were added, no struct changed
    assert ops.PrefixScores._fields == ("log_prefix", "logz", "log_prob")
    assert ops.NextSymbols._fields == ("next", "eos", "log_prefix", "logz")
    assert decoders.PrefixSearchResult._fields == ("strings", "lengths", "log_prob", "n_strings", "bound", "exact")
    assert callable(LatticeScorer.prefix_search) and callable(LatticeScorer.string_next_log_probs)
    for f in (ops.string_prefix_log_prob, ops.string_next_log_probs):
        assert "no gradient" in f.__doc__


def test_build_guard_covers_the_new_kernels():
    from nfst_amd.build import check_resources

    for k in ("k_string_prefix<true>", "k_string_prefix<false>", "k_string_label_index", "k_string_next<true>", "k_string_next<false>"):
        assert check_resources({k: {"vgpr_spill": 1, "scratch": 0}}) and check_resources({k: {"vgpr_spill": 0, "scratch": 16}})
        assert not check_resources({k: {"vgpr_spill": 0, "scratch": 0, "sgpr_spill": 3}})


def _host_batch():
    from nfst_amd.lattice import LatticeBatch

    lat = LatticeBatch.from_synth([synth.layered_lattice(s, n_states=12, avg_degree=2.5, vocab=16, width=3, span=2) for s in range(3)])
    assert lat.device.type == "cpu"
    return lat


@pytest.mark.parametrize("entry", ["nfst_string_prefix", "nfst_string_next"])
def test_argument_checks_return_before_any_launch(entry):
    from nfst_amd import _lib, ops

    lat = _host_batch()
    lib, bs = _lib.lib, C.byref(lat.c_struct())
    theta = np.zeros(16, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    B, M, N, V = lat.n_lattices, 4, 9, 16
    Q, QF = getattr(lib, entry + "_ws_bytes"), lib.nfst_string_logprob_ws_bytes
    assert Q(bs, M, 0, 0) == ERR_ARG and Q(bs, -1, N, 0) == ERR_ARG and Q(None, M, N, 0) == ERR_ARG
    assert Q(bs, M, ops.EDIT_MAX_LEN + 1, 0) == ERR_LIMIT
    ws_bytes = Q(bs, M, N, 0)
    cells = lat.total_rows * (N + 1) * M * 8
    assert ws_bytes >= cells and Q(bs, M, N, 1) >= ws_bytes + cells and Q(bs, 2 * M, N, 0) > ws_bytes > Q(bs, 0, N, 0) > 0
    if entry == "nfst_string_prefix":
        assert ws_bytes == QF(bs, M, N, 0)
    else:  # F, zn, z and az of every row, the in-arc and label lists
        assert ws_bytes >= cells + 24 * lat.total_rows + 12 * lat.total_arcs + 4 * B * (V + 1)
    ws = np.zeros(Q(bs, M, N, 1) // 8 + 2, np.float64)  # (16-byte aligned by numpy)
    a = dict(y=np.zeros((B, M, N), np.int32), n=np.zeros((B, M), np.int32), keep=np.ones(V, np.uint8), ws=ws,
             next=np.full((B, M, V), 77.0), eos=np.full((B, M), 77.0), pre=np.full((B, M), 77.0), z=np.full(B, 77.0),
             status=np.zeros(1, np.int32))
    outs = ("pre",) if entry == "nfst_string_prefix" else ("next", "eos", "pre")
    p = lambda x: None if x is None else x.ctypes.data

    def call(lat_=bs, sc_=C.byref(sc), M=M, N=N, marker=-1, wsb=ws_bytes, **kw):
        o = {**a, **kw}
        return getattr(lib, entry)(lat_, sc_, p(o["y"]), p(o["n"]), M, N, p(o["keep"]), marker, p(o["ws"]), wsb, *(p(o[k]) for k in outs),
                                   p(o["z"]), p(o["status"]), None)

    for name in ("y", "n", "ws", "z", "status") + outs:
        assert call(**{name: None}) == ERR_ARG, name
    assert call(lat_=None) == ERR_ARG and call(sc_=None) == ERR_ARG
    assert call(sc_=C.byref(_lib.Scores(None, 0, None, None, 0))) == ERR_ARG
    assert call(marker=4) == ERR_ARG and call(keep=None) == ERR_ARG  # both tapes, neither
    assert call(keep=None, marker=V) == ERR_ARG and call(keep=None, marker=-3) == ERR_ARG
    assert call(N=0) == ERR_ARG and call(M=-1) == ERR_ARG and call(N=ops.EDIT_MAX_LEN + 1) == ERR_LIMIT
    assert call(wsb=ws_bytes - 1) == ERR_ARG and call(ws=ws[1:]) == ERR_ARG
    assert call(keep=None, marker=4, wsb=ws_bytes) == ERR_ARG  # (marker mode needs the larger workspace)
    assert call(M=0) == 0 and call(M=0, y=None, n=None, **{k: None for k in outs}) == 0  # no prefix: a no-op
    assert call(M=0, ws=None) == ERR_ARG and call(M=0, z=None) == ERR_ARG
    empty = lat.c_struct().__class__.from_buffer_copy(lat.c_struct())
    empty.n_lattices = 0
    assert call(lat_=C.byref(empty)) == 0 and call(lat_=C.byref(empty), y=None, ws=None, z=None, **{k: None for k in outs}) == 0
    assert Q(C.byref(empty), M, N, 0) == 0 and call(lat_=C.byref(empty), status=None) == ERR_ARG
    assert a["status"][0] == 0 and all(np.all(a[k] == 77.0) for k in ("next", "eos", "pre", "z"))  # nothing ran


def test_the_lds_limit_is_checked_on_the_host():
    """A vocabulary whose label counts do not fit 160 KiB beside the reach flags: NFST_ERR_LIMIT from nfst_string_next
    (4 (max_rows + vocab) + 4100 bytes), while nfst_string_prefix, which builds no label lists, has no such limit."""
    from nfst_amd import _lib

    lat = _host_batch()
    lib = _lib.lib
    big = lat.c_struct().__class__.from_buffer_copy(lat.c_struct())
    big.vocab = 40 * 1024
    theta = np.zeros(big.vocab, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    B, M, N = lat.n_lattices, 1, 2
    ws = np.zeros(lib.nfst_string_next_ws_bytes(C.byref(big), M, N, 0) // 8 + 2, np.float64)
    y, n, st = np.zeros((B, M, N), np.int32), np.zeros((B, M), np.int32), np.zeros(1, np.int32)
    nx, e, pre, z = np.full((B, M, big.vocab), 77.0), np.full((B, M), 77.0), np.full((B, M), 77.0), np.full(B, 77.0)
    rc = lib.nfst_string_next(C.byref(big), C.byref(sc), y.ctypes.data, n.ctypes.data, M, N, None, 4, ws.ctypes.data, ws.nbytes,
                              nx.ctypes.data, e.ctypes.data, pre.ctypes.data, z.ctypes.data, st.ctypes.data, None)
    assert rc == ERR_LIMIT and np.all(nx == 77.0) and np.all(z == 77.0) and st[0] == 0


def test_wrappers_validate_before_any_launch():
    import torch

    from nfst_amd import decoders, ops
    from nfst_amd.lattice import LatticeBatch
    from tests.test_lattice_edit_cpu import small_lattices

    lat = LatticeBatch.from_synth(small_lattices()[:2])
    y, n = torch.zeros((2, 1, 5), dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int32)
    for f in (ops.string_prefix_log_prob, ops.string_next_log_probs):
        with pytest.raises(RuntimeError, match="MI355X only"):
            f(lat, torch.zeros(lat.vocab), y, n, marker=4)
    with pytest.raises(ValueError):
        decoders.prefix_search(lat, torch.zeros(lat.vocab), 4)
    with pytest.raises(ValueError):
        decoders.prefix_search(lat, torch.zeros(lat.vocab), 0, marker=4)
    with pytest.raises(RuntimeError, match="MI355X only"):
        decoders.prefix_search(lat, torch.zeros(lat.vocab), 4, marker=4)

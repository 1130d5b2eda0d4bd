"""The yardstick of the prefix states (tests/strings_extend_ref.py) against the references that brute force already holds
(tests/strings_prefix_ref.py): column by column against ``prefix_tables``, ``next``, ``eos`` and ``log_prefix`` against
``next_log_probs``, for every prefix of every string of the seven enumerable lattices of tests/test_strings_cpu.py in
both tape modes, prefixes that no path spells and dead slots included; the restated incremental search against the
restated search on the 78-row grid; and the C entry points' host-side checks on host pointers.  Runs without a GPU;
tests/test_gpu_strings_extend.py holds the kernels to the same restatement.

Every prefix of every string has its column checked, against the table of the first string that starts with it; where a
tape has more than 60 prefixes, ``next_log_probs`` (a whole table per call) is asked for the selection that
tests/test_strings_prefix_cpu.py makes and the two prefixes that no path spells.

Tolerance: both sides are float64 log-sums of the same terms in different groupings, over at most 1948 paths; the bound
is that of tests/test_strings_prefix_cpu.py, BRUTE = 1e-13.  Measured here: at most 1.8e-15.
"""
import ctypes as C

import numpy as np
import pytest

from nfst_amd import synth
from tests import edge_cases as E
from tests import strings_extend_ref as XR
from tests import strings_prefix_ref as PR
from tests import strings_ref as SR
from tests.test_strings_cpu import enumerable, tapes

ERR_ARG, ERR_LIMIT = -1, -6
BRUTE = 1e-13
NEG = -np.inf
MEASURED = {}


def _close(tag, got, want, where):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert not np.isnan(got).any() and np.array_equal(np.isneginf(got), np.isneginf(want)), (tag, where)
    live = ~np.isneginf(want)
    if live.any():
        err = float(np.abs(got[live] - want[live]).max())
        MEASURED[tag] = max(MEASURED.get(tag, 0.0), err)
        assert err <= BRUTE, (tag, where)


@pytest.mark.parametrize("case", range(7))
def test_columns_and_next_equal_the_table_references(case):
    name, l, seed = enumerable()[case]
    s64 = E.score64(l, synth.label_scores(seed, l.vocab, mean=-1.0, std=0.5))
    for tape in tapes(l):
        by, _, _ = SR.brute_force(l, s64, **tape)
        ctx = XR.Context(l, s64, **tape)
        strings = sorted(by)
        longest = max(by, key=len)
        strings += [longest + (longest[-1] if longest else int(l.label[0]),), (int(max(l.label)),) * 5]  # no path spells these
        cols, away = {}, None
        for y in strings:  # every prefix of every string, against the table of the first string that has it
            if all(y[:n] in cols for n in range(len(y) + 1)):
                continue
            F0, F1 = PR.prefix_tables(l, s64, list(y), **tape)
            reached = sorted(F0)
            away = [s for s in range(l.n_rows) if s not in F0]
            for n in range(len(y) + 1):
                p = y[:n]
                if p in cols:
                    continue
                c0, c1 = cols[p] = ctx.extend(cols[p[:-1]], p[-1]) if n else ctx.root()
                where = (name, sorted(tape), p)
                _close("column F0", c0[reached], [F0[s][n] for s in reached], where)
                _close("column F1", c1[reached], [F1[s][n] for s in reached], where)
                assert np.isneginf(c0[away]).all() and np.isneginf(c1[away]).all()
        prefixes = sorted(cols)
        if len(prefixes) > 60:  # (the selection of tests/test_strings_prefix_cpu.py, and the two that no path spells)
            prefixes = prefixes[:30] + prefixes[30::max(1, len(prefixes) // 30)] + [tuple(y) for y in strings[-2:]]
        for p in prefixes:
            nxt, eos, pre = ctx.next(cols[p])
            want = PR.next_log_probs(l, s64, list(p), **tape)
            where = (name, sorted(tape), p)
            _close("next", nxt, want[0], where)
            _close("eos", [eos], [want[1]], where)
            _close("log_prefix", [pre], [want[2]], where)
            assert abs(ctx.logz - want[3]) <= BRUTE
        assert any(np.isneginf(ctx.next(col)[2]) for col in cols.values())  # a prefix that no path spells is among them
        nxt, eos, pre = ctx.next(ctx.dead())
        assert np.isneginf(nxt).all() and eos == NEG and pre == NEG
        child = ctx.extend(ctx.dead(), int(l.label[0]))  # a dead parent has dead children
        assert np.isneginf(child[0]).all() and np.isneginf(child[1]).all()
        print(name, sorted(tape), len(cols), "prefixes", MEASURED)
        c = ctx.state_of(strings[0])
        assert np.array_equal(c[0], cols[tuple(strings[0])][0]) and np.array_equal(c[1], cols[tuple(strings[0])][1])


def test_the_incremental_search_equals_the_search():
    l = SR.denominator(SR.SEED1)
    assert l.n_rows == 78
    s64 = E.score64(l, synth.label_scores(1, 12, mean=-1.0, std=0.5))
    for kw in (dict(k=1), dict(k=2), dict(k=8), dict(k=64), dict(k=2, reserve=0, refine_steps=0), dict(k=2, reserve=3), dict(k=2, max_len=1),
               dict(k=1, max_len=0), dict(k=4, keep_mode=True)):
        tape = dict(keep={8, 9, 10}) if kw.pop("keep_mode", False) else dict(marker=SR.MARK)
        want, got = PR.prefix_search(l, s64, **tape, **kw), XR.prefix_search(l, s64, **tape, **kw)
        assert got["exact"] == want["exact"] and got["steps"] == want["steps"], kw
        if kw["k"] == 64:  # (permutations of a string tie to round-off)
            assert set(got["strings"]) == set(want["strings"])
        else:
            assert got["strings"] == want["strings"], kw
        _close("search log_prob", got["log_prob"], want["log_prob"], kw)
        _close("search bound", [got["bound"]], [want["bound"]], kw)


# ----------------------------------------------------------------------------- the C entry points
NAMES = ("nfst_string_prefix_open_ws_bytes", "nfst_string_prefix_open", "nfst_string_prefix_state_bytes", "nfst_string_prefix_extend",
         "nfst_string_prefix_state_next")


def test_exports_are_declared():
    from nfst_amd import _lib, decoders, ops
    from nfst_amd.scorers import LatticeScorer
    import inspect

    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "nfst_hip.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and f" {name}(" in header
    assert _lib.ABI_VERSION == 7 and _lib.lib.nfst_abi_version() == 7  # functions were added, no struct changed
    assert ops.PrefixState._fields == ("cells", "lengths")
    assert all(callable(getattr(ops.PrefixContext, f)) for f in ("root", "extend", "next", "state_of"))
    assert callable(LatticeScorer.prefix_context)
    assert inspect.signature(decoders.prefix_search).parameters["incremental"].default is False
    for f in (ops.string_prefix_open, ops.PrefixContext, decoders.prefix_search):
        assert "no gradient" in f.__doc__.lower()
    assert decoders.PrefixSearchResult._fields == ("strings", "lengths", "log_prob", "n_strings", "bound", "exact")


def test_build_guard_covers_the_new_kernels():
    from nfst_amd.build import check_resources

    for k in ("k_string_extend<true>", "k_string_extend<false>", "k_string_state_next<true>", "k_string_state_next<false>"):
        assert check_resources({k: {"vgpr_spill": 1, "scratch": 0}}) and check_resources({k: {"vgpr_spill": 0, "scratch": 16}})
        assert not check_resources({k: {"vgpr_spill": 0, "scratch": 0, "sgpr_spill": 3}})
    for k in ("k_string_next<true>", "k_string_prefix<false>", "k_string_label_index", "k_string_logprob_fwd<true>", "k_merge_paths"):
        assert check_resources({k: {"vgpr_spill": 1, "scratch": 0}})  # (the names it matched before)
    assert not check_resources({"k_string_extender": {"vgpr_spill": 1, "scratch": 8}})


def test_the_built_kernels_use_no_scratch():
    import json

    from nfst_amd import _lib

    res = json.load(open(_lib.LIB_PATH[:-3] + ".resources.json"))
    rows = {k: v for k, v in res.items() if k.startswith(("k_string_extend<", "k_string_state_next<"))}
    assert len(rows) == 4
    for k, v in rows.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["vgprs"] <= 128, (k, v)  # (1024 threads: 128 VGPRs a lane)


def _host_batch():
    from nfst_amd.lattice import LatticeBatch

    lat = LatticeBatch.from_synth([synth.layered_lattice(s, n_states=12, avg_degree=2.5, vocab=16, width=3, span=2) for s in range(3)])
    assert lat.device.type == "cpu"
    return lat


def test_argument_checks_return_before_any_launch():
    from nfst_amd import _lib

    lat = _host_batch()
    lib, bs = _lib.lib, C.byref(lat.c_struct())
    theta = np.zeros(16, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    B, V, TR = lat.n_lattices, 16, lat.total_rows
    Qc, Qs = lib.nfst_string_prefix_open_ws_bytes, lib.nfst_string_prefix_state_bytes
    empty = lat.c_struct().__class__.from_buffer_copy(lat.c_struct())
    empty.n_lattices = 0
    # the sizes
    assert Qc(None, 0) == ERR_ARG and Qc(C.byref(empty), 0) == 0
    ctx_bytes = Qc(bs, 0)
    assert ctx_bytes >= 36 * TR + 12 * lat.total_arcs + 4 * B * (V + 1) and Qc(bs, 1) > ctx_bytes  # (zn has two planes)
    assert ctx_bytes == lib.nfst_string_next_ws_bytes(bs, 0, 1, 0)  # nfst_string_next's workspace without a table
    assert Qs(None, 1, 0) == ERR_ARG and Qs(bs, -1, 0) == ERR_ARG and Qs(bs, 1025, 0) == ERR_LIMIT and Qs(C.byref(empty), 4, 0) == 0
    for M in (1, 3, 64, 1024):
        for mk in (0, 1):
            want = 8 * (1 + mk) * M * TR
            assert Qs(bs, M, mk) == (want + 255) // 256 * 256
    assert Qs(bs, 0, 0) == 0
    M_in, M_out = 3, 5
    f = lambda n: np.full(n // 8 + 2, 77.0)  # (16-byte aligned by numpy)
    a = dict(keep=np.ones(V, np.uint8), ctx=f(Qc(bs, 1)), pst=f(Qs(bs, M_in, 1)), ost=f(Qs(bs, M_out, 1)),
             par=np.zeros((B, M_out), np.int32), sym=np.zeros((B, M_out), np.int32), next=np.full((B, M_in, V), 77.0),
             eos=np.full((B, M_in), 77.0), pre=np.full((B, M_in), 77.0), z=np.full(B, 77.0), status=np.zeros(1, np.int32))
    p = lambda x: None if x is None else x.ctypes.data

    def opn(lat_=bs, sc_=C.byref(sc), marker=-1, wsb=ctx_bytes, **kw):
        o = {**a, **kw}
        return lib.nfst_string_prefix_open(lat_, sc_, p(o["keep"]), marker, p(o["ctx"]), wsb, p(o["z"]), p(o["status"]), None)

    def ext(lat_=bs, sc_=C.byref(sc), marker=-1, wsb=ctx_bytes, M_in=M_in, M_out=M_out, pb=None, ob=None, **kw):
        o = {**a, **kw}
        pb = Qs(bs, M_in, int(marker >= 0)) if pb is None else pb
        ob = Qs(bs, M_out, int(marker >= 0)) if ob is None else ob
        return lib.nfst_string_prefix_extend(lat_, sc_, p(o["keep"]), marker, p(o["ctx"]), wsb, p(o["pst"]), pb, M_in, p(o["par"]), p(o["sym"]),
                                             p(o["ost"]), ob, M_out, p(o["status"]), None)

    def nxt(lat_=bs, sc_=C.byref(sc), marker=-1, wsb=ctx_bytes, M=M_in, sb=None, **kw):
        o = {**a, **kw}
        sb = Qs(bs, M, int(marker >= 0)) if sb is None else sb
        return lib.nfst_string_prefix_state_next(lat_, sc_, p(o["keep"]), marker, p(o["ctx"]), wsb, p(o["pst"]), sb, M, p(o["next"]),
                                                 p(o["eos"]), p(o["pre"]), p(o["status"]), None)

    for call, names in ((opn, ("ctx", "z", "status")), (ext, ("ctx", "pst", "par", "sym", "ost", "status")),
                        (nxt, ("ctx", "pst", "next", "eos", "pre", "status"))):
        for name in names:
            assert call(**{name: None}) == ERR_ARG, (call.__name__, name)
        assert call(lat_=None) == ERR_ARG and call(sc_=None) == ERR_ARG
        assert call(sc_=C.byref(_lib.Scores(None, 0, None, None, 0))) == ERR_ARG
        assert call(marker=4) == ERR_ARG and call(keep=None) == ERR_ARG  # both tapes, neither
        assert call(keep=None, marker=V) == ERR_ARG and call(keep=None, marker=-3) == ERR_ARG
        assert call(wsb=ctx_bytes - 1) == ERR_ARG and call(ctx=a["ctx"][1:]) == ERR_ARG  # a short context, a misaligned one
        assert call(keep=None, marker=4, wsb=ctx_bytes) == ERR_ARG  # (marker mode needs the larger context)
        assert call(lat_=C.byref(empty)) == 0 and call(lat_=C.byref(empty), status=None) == ERR_ARG  # no lattice: a no-op
    # the states
    assert ext(pb=Qs(bs, M_in, 0) - 1) == ERR_ARG and ext(ob=Qs(bs, M_out, 0) - 1) == ERR_ARG and nxt(sb=Qs(bs, M_in, 0) - 1) == ERR_ARG
    assert ext(keep=None, marker=4, wsb=Qc(bs, 1), pb=Qs(bs, M_in, 0)) == ERR_ARG  # (marker mode: two planes)
    assert ext(pst=a["pst"][1:]) == ERR_ARG and ext(ost=a["ost"][1:]) == ERR_ARG and nxt(pst=a["pst"][1:]) == ERR_ARG
    assert ext(ost=a["pst"]) == ERR_ARG  # in place
    both = f(Qs(bs, M_in, 0) + Qs(bs, M_out, 0))
    assert ext(pst=both, ost=both[Qs(bs, M_in, 0) // 8 - 2:]) == ERR_ARG and ext(ost=both, pst=both[Qs(bs, M_out, 0) // 8 - 2:]) == ERR_ARG
    assert ext(M_in=-1) == ERR_ARG and ext(M_out=-1) == ERR_ARG and nxt(M=-1) == ERR_ARG
    assert ext(M_in=1025) == ERR_LIMIT and ext(M_out=1025) == ERR_LIMIT and nxt(M=1025) == ERR_LIMIT
    # the no-ops: no child, no hypothesis; every pointer of theirs may be null
    assert ext(M_out=0) == 0 and ext(M_out=0, pst=None, par=None, sym=None, ost=None) == 0
    assert nxt(M=0) == 0 and nxt(M=0, pst=None, next=None, eos=None, pre=None) == 0
    assert ext(M_out=0, ctx=None) == ERR_ARG and nxt(M=0, status=None) == ERR_ARG
    assert a["status"][0] == 0 and all(np.all(a[k] == 77.0) for k in ("ctx", "pst", "ost", "next", "eos", "pre", "z"))  # nothing ran


def test_the_lds_limit_is_checked_on_the_host():
    """The label lists of the largest vocabulary beside the reach flags of the largest lattice do not fit 160 KiB
    (4 (max_rows + vocab) + 4100 bytes): NFST_ERR_LIMIT from nfst_string_prefix_open, as from nfst_string_next."""
    from nfst_amd import _lib

    lat = _host_batch()
    lib = _lib.lib
    big = lat.c_struct().__class__.from_buffer_copy(lat.c_struct())
    big.vocab, big.max_rows = 32767, 8192
    theta = np.zeros(big.vocab, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    n = lib.nfst_string_prefix_open_ws_bytes(C.byref(big), 1)
    assert n > 0
    ws, z, st = np.full(n // 8 + 2, 77.0), np.full(lat.n_lattices, 77.0), np.zeros(1, np.int32)
    rc = lib.nfst_string_prefix_open(C.byref(big), C.byref(sc), None, 4, ws.ctypes.data, ws.nbytes, z.ctypes.data, st.ctypes.data, None)
    assert rc == ERR_LIMIT and np.all(ws == 77.0) and np.all(z == 77.0) and st[0] == 0
    big.vocab = 16  # (the sweep's own 8 max_rows + 4 bytes fit whenever the batch is within NFST_MAX_ROWS)
    assert 8 * big.max_rows + 4 <= 160 * 1024


def test_wrappers_validate_before_any_launch():
    import torch

    from nfst_amd import decoders, ops
    from nfst_amd.lattice import LatticeBatch
    from tests.test_lattice_edit_cpu import small_lattices

    lat = LatticeBatch.from_synth(small_lattices()[:2])
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.string_prefix_open(lat, torch.zeros(lat.vocab), marker=4)
    with pytest.raises(RuntimeError, match="MI355X only"):
        decoders.prefix_search(lat, torch.zeros(lat.vocab), 4, marker=4, incremental=True)
    with pytest.raises(ValueError):
        decoders.prefix_search(lat, torch.zeros(lat.vocab), 4, incremental=True)
    lens = torch.tensor([[2, 0, -1], [1, -1, 3]], dtype=torch.int32)
    par = torch.tensor([[0, 1, 2, -2, -1, 0], [1, 1, 0, 2, -2, -1]], dtype=torch.int32)
    assert ops.PrefixContext._lengths(lens, par).tolist() == [[3, 1, -1, 0, -1, 3], [-1, -1, 2, 4, 0, -1]]

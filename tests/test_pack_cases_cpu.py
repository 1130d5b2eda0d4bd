"""The branch corpus of tests/pack_cases.py -- CPU only.

Reach: every entry reaches the launch branches of ``k_pack_lattice`` it is named for, by the kernel's own predicates with
the kernel's constants (``nfst_pack_device_limits``), and the corpus covers every name of ``pack_cases.BRANCHES``.
The host packer, which is the device packer's reference (tests/test_gpu_pack.py), on the same shapes: its tile programs
replay to the float64 oracle's alpha and beta on the arcs that state 0 reaches (a breadth-first search of the test's own,
``pack_cases.analyse``), its meta records are what plain Python finds, and it refuses what ``pack_cases.error_rows`` says
it refuses."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from nfst_amd import _lib
from nfst_amd.lattice import LatticeBatch
from tests import pack_cases as PC
from tests.stream_check import replay

CASES = PC.cases()


def limits():
    lds, keys, threads = C.c_int64(), C.c_int32(), C.c_int32()
    assert _lib.lib.nfst_pack_device_limits(C.byref(lds), C.byref(keys), C.byref(threads)) == 0
    return int(lds.value), int(keys.value), int(threads.value)


def host_pack(lats, group_mode):
    n_rows, arc_off, src, label, dst, w = PC.batch_arcs(lats)
    return LatticeBatch.from_arcs(n_rows, arc_off, src, label, dst, lats[0].vocab, arc_w=w, group_mode=group_mode)


def assert_meta(lat: LatticeBatch, lats, analyses):
    for b, (l, a) in enumerate(zip(lats, analyses)):
        m = lat.meta_host[b]
        assert len(a["sinks"]) == 1 and a["acyclic"]
        got = {k: int(m[getattr(_lib, "META_" + k)]) for k in ("N_ROWS", "N_REACH", "N_ARCS", "N_DP", "SINK", "DEPTH")}
        want = dict(N_ROWS=l.n_rows, N_REACH=a["n_reach"], N_ARCS=a["n_arcs"], N_DP=a["n_dp"], SINK=a["sinks"][0], DEPTH=a["D"])
        assert got == want, (b, got, want)
        a0 = int(m[_lib.META_ARC_OFF])
        keep = a["canon"]
        assert np.array_equal(lat.arc_src.numpy()[a0:a0 + len(keep)], l.src[keep])
        assert np.array_equal(lat.arc_label.numpy()[a0:a0 + len(keep)], l.label[keep])
        assert np.array_equal(lat.arc_dst.numpy()[a0:a0 + len(keep)], l.dst[keep])
        if l.weight is not None:
            assert np.array_equal(lat.arc_w.numpy()[a0:a0 + len(keep)], l.weight[keep])


def test_limits_are_exported():
    lds, keys, threads = limits()
    assert lds % 1024 == 0 and 64 * 1024 < lds <= 160 * 1024  # (a workgroup of gfx950 has 160 KiB of LDS)
    assert keys * 8 <= lds and keys >= PC.MAX_ROWS             # (the level orders sort one key per state)
    assert threads == 1024
    assert _lib.lib.nfst_pack_device_limits(None, None, None) == -1


def test_every_entry_reaches_its_branches():
    lds, keys, _ = limits()
    launch = {"arcs_beyond_lds", "ranks_in_global", "counters_in_global", "count_falls_back", "count_falls_back_wide"}
    covered = set()
    for name, c in CASES.items():
        analyses = [PC.analyse(l) for l in c.lats]
        reached = set()
        for gm in c.group_modes:
            # (the predicates stand on figures that the host packer's meta confirms; it takes the two limit shapes as well)
            assert_meta(host_pack(c.lats, gm), c.lats, analyses)
            got = PC.batch_branches(c.lats, gm, lds, keys, analyses)
            if c.only:
                assert got & launch == c.only, (name, gm, got)
            # (the table of the counting pass only outgrows LDS under 8-lane groups: with wide groups alone P = 1)
            must = set(c.branches) - ({"count_falls_back"} if gm == 2 else set())
            assert must <= got, (name, gm, must - got)
            reached |= got
        assert set(c.branches) <= reached, (name, set(c.branches) - reached)
        covered |= reached & set(c.branches)
    assert covered == set(PC.BRANCHES), set(PC.BRANCHES) - covered
    # the shapes of the isolated entries, in figures
    a = PC.analyse(CASES["count_falls_back"].lats[0])
    assert int(a["indeg"].max()) == 64 and int(a["outdeg"].max()) == 64 and a["D"] + 1 >= 5560 and a["n"] <= 7782
    for direction in ("fwd", "bwd"):
        assert PC.layout_figures(a, direction, 0)[0] == 3 and PC.layout_figures(a, direction, 1)[0] == 1
    a = PC.analyse(CASES["limit_rows"].lats[0])
    assert a["n"] == 8190 and PC.layout_figures(a, "fwd", 0)[2] == 3
    a = PC.analyse(CASES["limit_pieces"].lats[0])
    assert PC.layout_figures(a, "fwd", 0)[1] > keys >= PC.layout_figures(a, "fwd", 1)[1]
    assert len(CASES["many"].lats) > PC.N_CUS


SMALL = [n for n, c in CASES.items() if c.small]
BIG = [n for n, c in CASES.items() if not c.small]


@pytest.mark.parametrize("name", SMALL)
def test_host_packer_replays_to_the_oracle_on_small_entries(name):
    c = CASES[name]
    theta = np.random.default_rng(3).normal(-2.3, 0.5, size=c.lats[0].vocab).astype(np.float32)
    for gm in (0, 1, 2):
        lat = host_pack(c.lats, gm)
        lat.validate()
        assert_meta(lat, c.lats, [PC.analyse(l) for l in c.lats])
        for b, l in enumerate(c.lats):
            src, label, dst, w = PC.reachable_arcs(l)
            sc = theta[label].astype(np.float64) + (w.astype(np.float64) if w is not None else 0.0)
            r = O.forward_backward(l.n_rows, src, dst, sc)
            extra = lat.arc_w.numpy() if w is not None else None
            assert np.allclose(replay(lat, b, "bwd", theta, extra), r["logbeta"], atol=1e-9, equal_nan=True), (name, gm, b)
            assert np.allclose(replay(lat, b, "fwd", theta, extra), r["logalpha"], atol=1e-9, equal_nan=True), (name, gm, b)


@pytest.mark.parametrize("name", BIG)
def test_host_packer_meta_on_big_entries(name):
    c = CASES[name]
    analyses = [PC.analyse(l) for l in c.lats]
    for gm in c.group_modes:
        lat = host_pack(c.lats, gm)
        lat.validate()
        assert_meta(lat, c.lats, analyses)


def test_host_packer_error_matrix():
    for name, lats, code, bad in PC.error_rows():
        n_rows, arc_off, src, label, dst = PC.raw_batch(lats)
        if code is None:
            LatticeBatch.from_arcs(n_rows, arc_off, src, label, dst, PC.ERROR_VOCAB).validate()
            continue
        with pytest.raises(_lib.NfstError) as e:
            LatticeBatch.from_arcs(n_rows, arc_off, src, label, dst, PC.ERROR_VOCAB)
        assert (e.value.code, e.value.lattice) == (code, bad), (name, e.value.code, e.value.lattice)

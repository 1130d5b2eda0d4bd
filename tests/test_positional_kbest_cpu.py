"""The NumPy restatement of nfst_positional_kbest (tests/positional_kbest_ref.py), which the GPU tests of
ops.positional_k_best rely on: against path enumeration on the six small lattices at every truncation, the three
consequences of the semantics (entry 0 is the max-plus path; without positions and with T >= depth it is nfst_kbest;
with T below the depth it is nfst_kbest's list without the longer paths) against tests/positional_ref.py and
tests/kbest_ref.py bit for bit, and the proofs that the inputs of the GPU cases are what they need (scores that really
tie inside the top 64, lattices with no, fewer than k and all paths listed).  Then the C entry points: exports, header,
ABI, the workspace formula and every argument check, on a host-packed batch (nothing touches a device).

The op has ONE launch flavour (the lists live in the workspace, the arcs are read from the canonical arrays, the LDS
holds 16 KiB of merge buffers, one int per row and one float per label), so there is no plan query: every shape takes
the same branch, and the LDS limit is max_rows + vocab <= 36862."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import edge_cases as E
from tests import kbest_ref as K
from tests import positional_kbest_ref as PK
from tests import positional_ref as R
from tests.test_positional_cpu import N_PATHS, small_lattices, truncations

NEG = -np.inf
F32 = np.float32
ERR_ARG, ERR_LIMIT = -1, -6  # (include/nfst_hip.h)
TIE_CASES = ("star", "funnel", "grid", "grid extras")

_PATHS = {}


def _paths(i):
    if i not in _PATHS:
        _PATHS[i] = R.enumerate_paths(small_lattices()[i])
    return _PATHS[i]


def _inputs(l, seed, T):
    rng = np.random.default_rng(seed)
    return rng.normal(-1.0, 0.8, size=l.vocab).astype(F32), rng.normal(0.0, 1.0, size=(T, l.vocab)).astype(F32)


def bits(x):
    return np.asarray(x, F32).view(np.int32)


# ----------------------------------------------------------------------------- against path enumeration
@pytest.mark.parametrize("i", range(6))
@pytest.mark.parametrize("with_pos", [True, False])
def test_restatement_equals_path_enumeration(i, with_pos):
    l = small_lattices()[i]
    assert len(_paths(i)) == N_PATHS[i]
    for name, T in truncations(l):
        theta, pos = _inputs(l, 700 + i, T)
        if not with_pos:
            pos = None
        fit = [p for p in _paths(i) if len(p) <= T]
        own = np.array([PK.path_score32(l, theta, pos, p) for p in fit], F32)
        order = np.argsort(-own, kind="stable")
        for k in (1, 7, 64):
            r = PK.k_best(l, theta, pos, T, k)
            n = r["n_paths"]
            assert n == min(k, len(fit)), (name, k)
            if name == "below":
                assert n == 0 and np.all(r["best"] == NEG)
                continue
            # the multiset of the top-k scores is the k largest right-nested float32 path scores
            assert np.array_equal(np.sort(bits(r["best"][:n])), np.sort(bits(own[order[:n]]))), (name, k)
            assert np.all(r["best"][n:] == NEG) and np.all(np.diff(r["best"][:n]) <= 0)
            for j, p in enumerate(r["arcs"]):
                assert bits(PK.path_score32(l, theta, pos, p)) == bits(r["best"][j]), (name, k, j)
                assert len(p) <= T and l.src[p[0]] == 0 and l.dst[p[-1]] == l.n_rows - 1
                assert all(l.dst[a] == l.src[b] for a, b in zip(p, p[1:]))
            assert len({tuple(p) for p in r["arcs"]}) == n  # pairwise distinct
            assert r["lengths"] == [len(p) for p in r["arcs"]] and r["labels"] == [[int(l.label[a]) for a in p] for p in r["arcs"]]
            # untied inputs: the order is the enumeration's.  Normal position scores never tie here; without them
            # paths over the same marks do (their order is the rule's, which the consequences below hold to nfst_kbest)
            untied = bool(np.all(np.diff(own[order[:n + 1]]) < 0))
            assert untied or not with_pos, (name, k)
            if untied:
                assert r["arcs"] == [fit[j] for j in order[:n]], (name, k)


@pytest.mark.parametrize("i", range(6))
def test_unreached_lists_change_nothing_and_smaller_k_is_a_prefix(i):
    """The restatement computes only the lists state 0 reaches; computing every list gives the same result.  And the
    top k' of a state is the first k' of its top k (float32 addition is monotone), which lets the GPU tests hold
    several k to one reference run of the expensive cases."""
    l = small_lattices()[i]
    for name, T in truncations(l):
        theta, pos = _inputs(l, 710 + i, T)
        full = PK.k_best(l, theta, pos, T, 64)
        every = PK.k_best(l, theta, pos, T, 64, every_list=True)
        assert np.array_equal(bits(full["best"]), bits(every["best"])) and full["arcs"] == every["arcs"], name
        for k in (1, 2, 7, 20):
            r = PK.k_best(l, theta, pos, T, k)
            n = min(k, full["n_paths"])
            assert r["n_paths"] == n and np.array_equal(bits(r["best"][:n]), bits(full["best"][:n])) and r["arcs"] == full["arcs"][:n]


# ----------------------------------------------------------------------------- the three consequences
@pytest.mark.parametrize("i", range(6))
def test_entry_zero_is_the_max_plus_path(i):
    l = small_lattices()[i]
    asc = np.random.default_rng(720 + i).normal(0.0, 0.3, size=l.n_arcs).astype(F32)
    for name, T in truncations(l):
        theta, pos = _inputs(l, 720 + i, T)
        for p, a in ((pos, None), (None, None), (pos, asc)):
            mp = R.max_plus(l, theta, p, T, a)
            r = PK.k_best(l, theta, p, T, 7, a)
            assert bits(r["best"][0]) == bits(mp["best"]), name
            if name == "below":
                assert r["n_paths"] == 0 and mp["arcs"] == []
            else:
                assert r["arcs"][0] == mp["arcs"] and r["labels"][0] == mp["labels"], name


def _kbest(l, theta, k, asc=None):
    th, e = K.arc_terms(l, theta, asc)
    return K.k_best(l.n_rows, l.src, l.dst, th, e, k, l.n_rows - 1)


@pytest.mark.parametrize("i", range(6))
def test_without_positions_it_is_k_best(i):
    """(ii) T >= depth: every output of nfst_kbest; (iii) T below the depth: its list without the paths longer than T,
    as long as neither list is truncated (the four lattices with fewer than 64 paths)."""
    l = small_lattices()[i]
    theta, _ = _inputs(l, 730 + i, 1)
    asc = np.random.default_rng(730 + i).normal(0.0, 0.3, size=l.n_arcs).astype(F32)
    for a in (None, asc):
        for k in (1, 7, 64):
            ref = _kbest(l, theta, k, a)
            for name, T in truncations(l):
                r = PK.k_best(l, theta, None, T, k, a)
                if name in ("depth", "beyond"):
                    assert r["n_paths"] == ref["n_paths"] and np.array_equal(bits(r["best"]), bits(ref["best"])) and r["arcs"] == ref["arcs"]
                elif k == 64 and N_PATHS[i] < 64:
                    keep = [j for j, p in enumerate(ref["arcs"]) if len(p) <= T]
                    assert r["n_paths"] == len(keep) < ref["n_paths"] == N_PATHS[i], name
                    assert np.array_equal(bits(r["best"][:len(keep)]), bits(ref["best"][keep])) and r["arcs"] == [ref["arcs"][j] for j in keep]
    assert sum(n < 64 for n in N_PATHS) == 4


# ----------------------------------------------------------------------------- the inputs of the GPU cases
def tie_truncations(lats):
    """(the longest path of the batch, halfway between its shortest and its longest)."""
    lens = [R.min_max_len(l) for l in lats]
    lo, hi = min(x[0] for x in lens), max(x[1] for x in lens)
    return hi, (lo + hi) // 2


def tie_reference(name, T, k=64):
    """The restatement of every lattice of a tie case at budget T (position scores: the first T rows of the case's)."""
    lats, theta, asc, pos, T_full = E.pos_tie_inputs(name)
    assert T <= T_full
    return [PK.k_best(l, theta, pos[b, :T], T, k, None if asc is None else asc[sl]) for b, (l, sl) in enumerate(zip(lats, E.arc_slices(lats)))]


@pytest.mark.parametrize("name", TIE_CASES)
def test_tie_inputs_tie_inside_the_top_64(name):
    lats = E.pos_tie_inputs(name)[0]
    Ts = tie_truncations(lats)
    assert Ts == {"star": (4, 4), "funnel": (6, 6)}.get(name, (102, 56))
    for T in sorted(set(Ts)):
        for b, r in enumerate(tie_reference(name, T)):
            best = r["best"][:r["n_paths"]]
            pairs = int(np.sum(best[1:] == best[:-1]))
            assert r["n_paths"] == 64 and 41 <= pairs <= 61, (name, T, b, pairs)


def test_neighbour_has_none_fewer_and_all_paths():
    l = E.pos_neighbour()
    theta, _ = _inputs(l, 740, 1)
    assert [PK.k_best(l, theta, None, T, 64)["n_paths"] for T in (3, 4, 6)] == [0, 3, 23]
    assert len(R.enumerate_paths(l)) == 23 and R.min_max_len(l) == (4, 6)


# ----------------------------------------------------------------------------- the C entry points
def test_exports_and_header():
    from nfst_amd import _lib

    assert {"nfst_positional_kbest", "nfst_positional_kbest_ws_bytes"} <= set(_lib.EXPORTS)
    with open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "nfst_hip.h")) as f:
        h = f.read()
    assert int(re.search(r"#define\s+NFST_ABI_VERSION\s+(\d+)", h).group(1)) == 7 == _lib.ABI_VERSION
    assert re.search(r"\bint\s+nfst_positional_kbest\s*\(", h) and re.search(r"\bint64_t\s+nfst_positional_kbest_ws_bytes\s*\(", h)


def test_workspace_formula():
    """8 (T + 1) total_rows k bytes of lists and (T + 1) total_rows bytes of marks, each part rounded up to 256."""
    from nfst_amd import _lib
    from nfst_amd.lattice import LatticeBatch

    lat = LatticeBatch.from_synth(small_lattices()[:3])
    bs = C.byref(lat.c_struct())
    f = _lib.lib.nfst_positional_kbest_ws_bytes
    up = lambda x: (x + 255) & ~255
    for T in (1, 6, 17):
        for k in (1, 7, 64):
            assert f(bs, T, k) == up(8 * (T + 1) * lat.total_rows * k) + up((T + 1) * lat.total_rows)
    assert f(bs, 0, 5) == ERR_ARG and f(bs, 6, 0) == ERR_ARG and f(bs, 6, 65) == ERR_LIMIT
    # 64-bit: the benchmark batch's rows at T = 140 and k = 64 pass 2^31 bytes by far
    big = _lib.Batch.from_buffer_copy(lat.c_struct())
    big.total_rows = 516236
    assert f(C.byref(big), 140, 64) == up(8 * 141 * 516236 * 64) + up(141 * 516236) > 2 ** 35
    assert _lib.lib.nfst_positional_ws_bytes(bs, 6, 4) == ERR_ARG and _lib.lib.nfst_positional_ws_bytes(bs, 6, 16) == ERR_ARG


def test_argument_checks_return_before_any_launch():
    from nfst_amd import _lib
    from nfst_amd.lattice import LatticeBatch

    lat = LatticeBatch.from_synth(small_lattices()[:3])  # host-packed: the checks run before anything touches a device
    assert lat.device.type == "cpu"
    V, B, T, k = lat.vocab, lat.n_lattices, 6, 5
    theta = np.zeros(V, F32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    lib = _lib.lib
    bs = C.byref(lat.c_struct())
    full = lib.nfst_positional_kbest_ws_bytes(bs, T, k)
    ws = np.zeros(full // 8 + 2, np.float64)  # (16-byte aligned by numpy)
    pos = np.zeros((B, T, V), F32)
    best, lens, n_paths = np.zeros((B, k), F32), np.zeros((B, k), np.int32), np.zeros(B, np.int32)
    paths = np.zeros((B, k, T), np.int32)
    p = lambda a: None if a is None else a.ctypes.data

    def call(T=T, k=k, stride=T * V, ws=ws, wsb=full, best=best, paths=paths, lens=lens, n_paths=n_paths, scores=C.byref(sc), bs=bs):
        return lib.nfst_positional_kbest(bs, scores, p(pos), stride, T, k, p(ws), wsb, p(best), p(paths), None, p(lens), p(n_paths), 0, None)

    assert call(k=0) == ERR_ARG
    assert call(k=-3) == ERR_ARG
    assert call(k=65, wsb=lib.nfst_positional_kbest_ws_bytes(bs, T, 64) * 2) == ERR_LIMIT
    assert call(T=0, stride=0) == ERR_ARG
    assert call(stride=V) == ERR_ARG
    assert call(stride=T * V + 1) == ERR_ARG
    assert call(ws=None) == ERR_ARG
    assert call(wsb=full - 1) == ERR_ARG
    assert call(wsb=lib.nfst_positional_kbest_ws_bytes(bs, T, k - 1)) == ERR_ARG
    assert call(ws=ws.view(np.uint8)[4:]) == ERR_ARG  # not 16-byte aligned
    for name in ("best", "paths", "lens", "n_paths"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(scores=None) == ERR_ARG
    assert call(bs=None) == ERR_ARG
    # nfst_kbest's payload limit: a lattice of 2^24 arcs or more (the batch records its largest lattice up to a cap)
    huge = _lib.Batch.from_buffer_copy(lat.c_struct())
    huge.reserved0 |= 0x7fffff << 8
    huge.total_arcs = 1 << 24
    assert call(bs=C.byref(huge)) == ERR_LIMIT
    huge.total_arcs = (1 << 24) - 1
    assert call(bs=C.byref(huge), k=0) == ERR_ARG
    # the LDS limit: 16392 + 4 (max_rows + vocab) bytes against 160 KiB (the scores and the workspace do not depend on either)
    wide = _lib.Batch.from_buffer_copy(lat.c_struct())
    wide.max_rows, wide.vocab = 8192, 36862 - 8192 + 1
    assert call(bs=C.byref(wide), stride=0) == ERR_LIMIT and 16392 + 4 * (8192 + 36862 - 8192) == 160 * 1024


def test_wrappers_validate_before_any_launch():
    import torch

    from nfst_amd import ops
    from nfst_amd.lattice import LatticeBatch
    from nfst_amd.scorers import LatticeScorer

    lat = LatticeBatch.from_synth(small_lattices()[:3])
    theta = torch.zeros(lat.vocab)
    for fn in (ops.positional_k_best, ops.positional_k_best_terms):
        with pytest.raises(RuntimeError):  # a host batch: no CPU fallback
            fn(lat, theta, 4, torch.zeros(4, lat.vocab))
    assert ops.PositionalKBestResult._fields == ("best", "paths", "arcs", "lengths", "n_paths")
    assert callable(LatticeScorer.positional_k_best) and callable(LatticeScorer.positional_nbest)


def test_build_guard_covers_the_new_kernels():
    from nfst_amd.build import check_resources

    for name in ("k_positional_kbest_sweep", "k_positional_kbest_walk"):
        assert check_resources({name: {"vgpr_spill": 4, "agprs": 0}})
        assert not check_resources({name: {"vgpr_spill": 0, "agprs": 0}})

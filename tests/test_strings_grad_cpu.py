"""The yardstick of ``nfst_string_logprob_grad`` (tests/strings_grad_ref.py) against brute force over every path and
against central differences of ``strings_ref.string_log_prob``, the two identities that tie the gradients of all strings
of a lattice together, and the C entry point's host-side checks on host pointers.  Runs without a GPU;
tests/test_gpu_strings_grad.py holds the kernels to the same restatement.

Tolerances, from float64 arithmetic only.  Measured here, the largest absolute difference over all cases:
  restatement against brute force   1.8e-14 (post_z; post_y 1.6e-14, grad_arc 2.0e-14): both sides are log-sums and sums
                                    of exp over up to 1948 paths; x 16, rounded up to a power of ten: BRUTE = 1e-12
  restatement against differences   1.6e-10 with the step H = 1e-4: the rounding of two log-sums over the step (2^-52
                                    |log_num| / H ~ 1e-11) plus H^2 / 6 times a third derivative of a log-sum-exp, whose
                                    arguments are probabilities (below 1.7e-9); x 16, rounded up: DIFF = 1e-8
  the identities over all strings   8.3e-16: sums of brute-force-bounded terms weighed by probabilities that add up to
                                    at most 1, so BRUTE holds them as well
"""
import ctypes as C

import numpy as np
import pytest

from nfst_amd import synth
from tests import edge_cases as E
from tests import strings_grad_ref as GR
from tests import strings_ref as SR
from tests.test_strings_cpu import enumerable, tapes

ERR_ARG, ERR_LIMIT = -1, -6
BRUTE = 1e-12
DIFF = 1e-8
H = 1e-4
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


@pytest.mark.parametrize("case", range(7))
def test_restatement_equals_brute_force(case):
    """Every string of the lattice, both tape modes: the posterior of every arc among the string's paths and among all
    paths, and log_num and logz; a string that no path spells gets zeros."""
    name, l, s64 = _case(case)
    for tape in tapes(l):
        by, logz, _ = SR.brute_force(l, s64, **tape)
        num, pz, _, _ = GR.brute_posteriors(l, s64, **tape)
        for y in by:
            py, rz, log_num, rlogz = GR.posteriors(l, s64, list(y), **tape)
            assert rec("brute post_y", np.abs(py - num[y]).max()) <= BRUTE, (name, tape, y)
            assert rec("brute post_z", np.abs(rz - pz).max()) <= BRUTE, (name, tape, y)
            assert abs(log_num - by[y]) <= BRUTE and abs(rlogz - logz) <= BRUTE
        best = max(by, key=lambda y: by[y])
        py, _, log_num, _ = GR.posteriors(l, s64, list(best) + [int(l.label.max())] * 3, **tape)
        assert log_num == NEG and not py.any() and not np.isnan(py).any()
        # grad_arc puts them together in ascending m; a zero upstream gradient leaves its candidate out
        ys = sorted(by, key=lambda y: -by[y])[:3]
        g_num = np.array([0.75, 0.0, -1.5][:len(ys)])
        want = 0.5 * pz + sum(g * num[y] for g, y in zip(g_num, ys))
        got = GR.grad_arc(l, s64, [list(y) for y in ys], g_num, 0.5, **tape)
        assert rec("brute grad_arc", np.abs(got - want).max()) <= BRUTE, (name, tape)


@pytest.mark.parametrize("case", [0, 3, 5, 6])
def test_restatement_equals_central_differences(case):
    """d log_num / d score and d logz / d score of ``strings_ref.string_log_prob`` by central differences in every arc's
    score (of at most 48 arcs, evenly spread), for the two heaviest strings, both tape modes."""
    name, l, s64 = _case(case)
    arcs = np.unique(np.linspace(0, l.n_arcs - 1, min(l.n_arcs, 48)).astype(np.int64))
    for tape in tapes(l):
        by, _, _ = SR.brute_force(l, s64, **tape)
        for y in sorted(by, key=lambda y: -by[y])[:2]:
            py, pz, _, _ = GR.posteriors(l, s64, list(y), **tape)
            for a in arcs:
                up, dn = s64.copy(), s64.copy()
                up[a] += H
                dn[a] -= H
                (n1, z1), (n0, z0) = SR.string_log_prob(l, up, list(y), **tape), SR.string_log_prob(l, dn, list(y), **tape)
                assert rec("diff post_y", abs((n1 - n0) / (2 * H) - py[a])) <= DIFF, (name, tape, y, a)
                assert rec("diff post_z", abs((z1 - z0) / (2 * H) - pz[a])) <= DIFF, (name, tape, y, a)


@pytest.mark.parametrize("case", range(7))
def test_gradients_of_all_strings_add_up(case):
    """Keep mode: the strings' probabilities add up to 1, so sum_y p(y) grad log p(y) = 0 for every arc.  Marker mode:
    they add up to 1 less the share D of the paths that end on an active marker, so the sum is minus the gradient of D
    (brute force: the dangling paths through the arc over Z, less D times the arc's posterior)."""
    name, l, s64 = _case(case)
    for tape in tapes(l):
        by, logz, _ = SR.brute_force(l, s64, **tape)
        _, _, d_dang, D = GR.brute_posteriors(l, s64, **tape)
        total = np.zeros(l.n_arcs)
        for y in by:
            py, pz, log_num, rlogz = GR.posteriors(l, s64, list(y), **tape)
            total += np.exp(log_num - rlogz) * (py - pz)
        assert rec("sum over strings", np.abs(total + d_dang).max()) <= BRUTE, (name, tape)
        assert "marker" in tape or (D == 0.0 and not d_dang.any())
    assert name != "tape" or D > 0.0  # (the tape lattice has paths that end on a marker)


# ----------------------------------------------------------------------------- the C entry point
def test_exports_are_declared():
    from nfst_amd import _lib, ops
    from nfst_amd.scorers import LatticeScorer

    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "nfst_hip.h")).read()
    for name in ("nfst_string_logprob_grad_ws_bytes", "nfst_string_logprob_grad"):
        assert name in _lib.EXPORTS and f" {name}(" in header
    assert _lib.ABI_VERSION == 7 and _lib.lib.nfst_abi_version() == 7  # functions were added, no struct changed
    assert ops.StringScores._fields == ("log_num", "logz", "log_prob")
    assert callable(ops.string_arc_posteriors) and callable(LatticeScorer.string_nll)
    assert "Forward only" not in ops.string_log_prob.__doc__
    import inspect

    assert inspect.signature(ops.string_log_prob).parameters["want_arc_grad"].default is False


def test_build_guard_covers_the_new_kernels():
    from nfst_amd.build import check_resources

    for k in ("k_string_logprob_index", "k_string_logprob_fwd<true>", "k_string_logprob_fwd<false>", "k_string_logprob_arcs<true>",
              "k_string_logprob_arcs<false>"):
        assert check_resources({k: {"vgpr_spill": 1, "scratch": 0}}) and check_resources({k: {"vgpr_spill": 0, "scratch": 16}})
        assert not check_resources({k: {"vgpr_spill": 0, "scratch": 0, "sgpr_spill": 3}})
    assert check_resources({"k_string_logprob<true>": {"vgpr_spill": 2, "scratch": 0}})


def test_grad_argument_checks_return_before_any_launch():
    from nfst_amd import _lib, ops
    from nfst_amd.lattice import LatticeBatch

    lat = LatticeBatch.from_synth([synth.layered_lattice(s, n_states=12, avg_degree=2.5, vocab=16, width=3, span=2) for s in range(3)])
    assert lat.device.type == "cpu"
    lib, bs = _lib.lib, C.byref(lat.c_struct())
    theta = np.zeros(16, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    B, M, N = lat.n_lattices, 4, 9
    Q, QF = lib.nfst_string_logprob_grad_ws_bytes, lib.nfst_string_logprob_ws_bytes
    assert Q(bs, M, 0, 0) == ERR_ARG and Q(bs, -1, N, 0) == ERR_ARG and Q(None, M, N, 0) == ERR_ARG
    assert Q(bs, M, ops.EDIT_MAX_LEN + 1, 0) == ERR_LIMIT
    ws_bytes = Q(bs, M, N, 0)
    cells = lat.total_rows * (N + 1) * M * 8
    assert ws_bytes >= QF(bs, M, N, 0) + cells + 8 * lat.total_rows + 8 * lat.total_arcs  # the forward's, F, az, the in-arc lists
    assert Q(bs, M, N, 1) >= ws_bytes + 2 * cells  # two rows per state and table in marker mode
    assert Q(bs, 2 * M, N, 0) > ws_bytes > Q(bs, 0, N, 0) > QF(bs, 0, N, 0)
    ws = np.zeros(Q(bs, M, N, 1) // 8 + 2, np.float64)  # (16-byte aligned by numpy)
    a = dict(y=np.zeros((B, M, N), np.int32), n=np.zeros((B, M), np.int32), keep=np.ones(16, np.uint8), ws=ws,
             gnum=np.ones((B, M)), gz=np.ones(B), grad=np.full(lat.total_arcs, 77.0), status=np.zeros(1, np.int32))
    p = lambda x: None if x is None else x.ctypes.data

    def call(lat_=bs, sc_=C.byref(sc), M=M, N=N, marker=-1, acc=0, wsb=ws_bytes, **kw):
        o = {**a, **kw}
        return lib.nfst_string_logprob_grad(lat_, sc_, p(o["y"]), p(o["n"]), M, N, p(o["keep"]), marker, p(o["gnum"]), p(o["gz"]), acc,
                                            p(o["ws"]), wsb, p(o["grad"]), p(o["status"]), None)

    for name in ("y", "n", "ws", "gnum", "gz", "grad", "status"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(lat_=None) == ERR_ARG and call(sc_=None) == ERR_ARG
    assert call(sc_=C.byref(_lib.Scores(None, 0, None, None, 0))) == ERR_ARG
    assert call(marker=4) == ERR_ARG and call(keep=None) == ERR_ARG  # both tapes, neither
    assert call(keep=None, marker=16) == ERR_ARG and call(keep=None, marker=-3) == ERR_ARG
    assert call(N=0) == ERR_ARG and call(M=-1) == ERR_ARG and call(N=ops.EDIT_MAX_LEN + 1) == ERR_LIMIT
    assert call(wsb=ws_bytes - 1) == ERR_ARG and call(ws=ws[1:]) == ERR_ARG
    assert call(wsb=QF(bs, M, N, 0)) == ERR_ARG  # (the forward's workspace is too small)
    assert call(keep=None, marker=4, wsb=ws_bytes) == ERR_ARG  # (marker mode needs the larger workspace)
    empty = lat.c_struct().__class__.from_buffer_copy(lat.c_struct())
    empty.n_lattices = 0
    assert call(lat_=C.byref(empty)) == 0 and call(lat_=C.byref(empty), y=None, ws=None, gnum=None, gz=None, grad=None) == 0
    assert Q(C.byref(empty), M, N, 0) == 0 and call(lat_=C.byref(empty), status=None) == ERR_ARG
    assert a["status"][0] == 0 and np.all(a["grad"] == 77.0)  # nothing ran


def test_wrappers_validate_before_any_launch():
    import torch

    from nfst_amd import ops
    from nfst_amd.lattice import LatticeBatch
    from tests.test_lattice_edit_cpu import small_lattices

    lat = LatticeBatch.from_synth(small_lattices()[:2])
    y, n = torch.zeros((2, 1, 5), dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.string_arc_posteriors(lat, torch.zeros(lat.vocab), y, n, marker=4)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.string_log_prob(lat, torch.zeros(lat.vocab, requires_grad=True), y, n, marker=4)

"""The NumPy restatement of the positional draws and forced scores (tests/positional_sample_ref.py), which the GPU tests
of ops.positional_sample_paths / ops.positional_score_paths rely on: against path enumeration at every truncation, the
cap on undecided walks for every case of tests/test_gpu_positional_sample.py (a condition on the inputs, held on the
reference alone), and the C entry points' host-side checks, exports, workspace formula and register guard."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import positional_ref as R
from tests import positional_sample_ref as S
from tests.test_positional_cpu import small_lattices, truncations

NEG = -np.inf
ERR_ARG, ERR_LIMIT = -1, -6  # (include/nfst_hip.h)

_PATHS = {}


def _paths(i):
    if i not in _PATHS:
        _PATHS[i] = R.enumerate_paths(small_lattices()[i])
    return _PATHS[i]


def _inputs(l, seed, T):
    rng = np.random.default_rng(seed)
    return rng.normal(-1.0, 0.8, size=l.vocab).astype(np.float32), rng.normal(0.0, 1.0, size=(T, l.vocab)).astype(np.float32)


@pytest.mark.parametrize("i", range(6))
@pytest.mark.parametrize("with_pos", [True, False])
def test_step_probabilities_multiply_to_the_path_probability_and_sum_to_one(i, with_pos):
    l = small_lattices()[i]
    for name, T in truncations(l):
        theta, pos = _inputs(l, 500 + i, T)
        if not with_pos:
            pos = None
        score = R.arc_score64(l, theta)
        smp = S.Sampler(l, score, pos, T)
        bf = R.brute_force(l, score, pos, T, _paths(i))
        if name == "below":
            assert smp.logz == NEG and bf["logz"] == NEG
            assert smp.walk(np.zeros(T, np.float32)) == {"arcs": [], "labels": [], "length": 0, "logq": 0.0, "margin": np.inf}
            continue
        assert abs(smp.logz - bf["logz"]) <= 1e-12 * max(1.0, abs(bf["logz"]))
        total = 0.0
        for p in _paths(i):
            lp = smp.path_logprob(p)
            if len(p) > T:
                assert lp == NEG
                continue
            want = smp.path_score(p) - bf["logz"]  # S_T - log Z_T of the enumeration
            assert abs(np.exp(lp) - np.exp(want)) <= 1e-12, (name, p)
            total += np.exp(lp)
            # the forced score of the path's labels is its S_T, it ends at the sink and counts every mark
            marks = [int(l.label[a]) for a in p] + [0] * (T - len(p))
            fs, end, n = S.forced_score(l, score, pos, marks)
            assert abs(fs - smp.path_score(p)) <= 1e-12 * max(1.0, abs(fs)) and end == l.n_rows - 1 and n == len(p)
        assert abs(total - 1.0) <= 1e-12, name


def test_forced_score_off_the_lattice_and_forbidden_entries():
    l = small_lattices()[0]
    T = R.min_max_len(l)[1]
    theta, pos = _inputs(l, 7, T)
    score = R.arc_score64(l, theta)
    p = _paths(0)[5]
    marks = [int(l.label[a]) for a in p] + [0] * (T - len(p))
    bad = list(marks)
    bad[1] = int(max(set(range(l.vocab)) - {int(l.label[a]) for a in np.nonzero(l.src == l.dst[p[0]])[0]}))
    assert S.forced_score(l, score, pos, bad) == (NEG, 0, 1)
    dead = pos.copy()
    dead[2, marks[2]] = NEG
    fs, end, n = S.forced_score(l, score, dead, marks)
    assert fs == NEG and end == l.n_rows - 1 and n == len(p)


def test_walks_follow_the_uniforms():
    """u = 0 takes the first arc of positive weight at every step, u just below 1 the last; forbidding that first arc
    moves the walk to the next one (an arc of weight zero is never taken)."""
    l = small_lattices()[0]
    T = R.min_max_len(l)[1]
    theta, pos = _inputs(l, 8, T)
    score = R.arc_score64(l, theta)
    smp = S.Sampler(l, score, pos, T)
    lo = smp.walk(np.zeros(T, np.float32))
    hi = smp.walk(np.full(T, np.nextafter(np.float32(1), np.float32(0))))
    s = 0
    for t, a in enumerate(lo["arcs"]):
        out, p = smp.step_probs(t, s)
        assert a == out[np.nonzero(p > 0)[0][0]]
        s = int(l.dst[a])
    s = 0
    for t, a in enumerate(hi["arcs"]):
        out, p = smp.step_probs(t, s)
        assert a == out[np.nonzero(p > 0)[0][-1]]
        s = int(l.dst[a])
    first = lo["arcs"][1]
    out, p = smp.step_probs(1, int(l.src[first]))
    if (p > 0).sum() > 1:
        pos2 = pos.copy()
        pos2[1, l.label[first]] = NEG
        other = S.Sampler(l, score, pos2, T).walk(np.zeros(T, np.float32))
        assert other["arcs"][0] == lo["arcs"][0] and other["arcs"][1] != first


# ----------------------------------------------------------------------------- the cap on undecided walks
def test_prototype_small_lattices_are_decided():
    """The six lattices x five truncations, 64 walks each: nothing is undecided at 1e-6."""
    n = bad = 0
    smallest = np.inf
    for i, l in enumerate(small_lattices()):
        for name, T in truncations(l):
            theta, pos = _inputs(l, 600 + i, T)
            walks = S.Sampler(l, R.arc_score64(l, theta), pos, T).walks(S.small_uniforms(i, T))
            n += len(walks)
            bad += S.undecided(walks)
            if name != "below":
                smallest = min(smallest, min(w["margin"] for w in walks))
    assert n == 6 * 5 * 64 and bad == 0 and smallest > S.DECIDED


def test_every_gpu_comparison_stays_within_the_cap():
    """Every comparison of tests/test_gpu_positional_sample.py against the restatement, rebuilt here from the same case
    table: at most 1 % of its walks may be undecided (a condition on the inputs; a seed that breaks it is replaced)."""
    from tests import test_gpu_positional_sample as G

    seen = 0
    for name, make in G.COMPARED.items():
        for case in make():
            refs = G.reference_walks(case)
            for threshold in case.thresholds:
                walks = [w for per in refs for w in per]
                assert S.undecided(walks, threshold) <= S.CAP * len(walks), (name, case.tag, threshold)
            seen += 1
    assert seen >= len(G.COMPARED)


# ----------------------------------------------------------------------------- the C entry points
def test_exports_are_declared():
    from nfst_amd import _lib

    assert {"nfst_positional_sample", "nfst_positional_score_paths"} <= set(_lib.EXPORTS)
    with open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "nfst_hip.h")) as f:
        h = f.read()
    assert int(re.search(r"#define\s+NFST_POS_WS_SAMPLE\s+(\d+)", h).group(1)) == _lib.POS_WS_SAMPLE
    assert int(re.search(r"#define\s+NFST_ABI_VERSION\s+(\d+)", h).group(1)) == 7
    for name in ("nfst_positional_sample", "nfst_positional_score_paths"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", h)


def test_workspace_formula():
    """12 bytes per arc + 12 (T + 1) total_rows, every part rounded up to 256 bytes; no by-destination order."""
    from nfst_amd import _lib
    from nfst_amd.lattice import LatticeBatch

    lat = LatticeBatch.from_synth(small_lattices()[:3])
    bs = C.byref(lat.c_struct())
    up = lambda x: (x + 255) & ~255
    for T in (1, 6, 17):
        rows, A = (T + 1) * lat.total_rows, lat.total_arcs
        want = up(8 * A) + up(4 * A) + up(8 * rows) + up(4 * rows)
        got = _lib.lib.nfst_positional_ws_bytes(bs, T, _lib.POS_WS_SAMPLE)
        assert got == want and 12 * A + 12 * rows <= got < 12 * A + 12 * rows + 4 * 256
        assert got < _lib.lib.nfst_positional_ws_bytes(bs, T, _lib.POS_WS_POSTERIOR)
    assert _lib.lib.nfst_positional_ws_bytes(bs, 0, _lib.POS_WS_SAMPLE) == ERR_ARG
    assert _lib.lib.nfst_positional_ws_bytes(bs, 6, 16) == ERR_ARG


def test_argument_checks_return_before_any_launch():
    from nfst_amd import _lib
    from nfst_amd.lattice import LatticeBatch

    lat = LatticeBatch.from_synth(small_lattices()[:3])  # host-packed: the checks run before anything touches a device
    assert lat.device.type == "cpu"
    V, B, T, K = lat.vocab, lat.n_lattices, 6, 4
    theta = np.zeros(V, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    lib = _lib.lib
    bs = C.byref(lat.c_struct())
    full = lib.nfst_positional_ws_bytes(bs, T, _lib.POS_WS_SAMPLE)
    ws = np.zeros(full // 8 + 2, np.float64)
    pos = np.zeros((B, T, V), np.float32)
    z64, z32 = np.zeros(B, np.float64), np.zeros(B, np.float32)
    paths, arcs = np.zeros((B, K, T), np.int32), np.zeros((B, K, T), np.int32)
    lens, logq = np.zeros((B, K), np.int32), np.zeros((B, K), np.float32)
    p = lambda a: None if a is None else a.ctypes.data

    def call(T=T, k=K, stride=T * V, ws=ws, wsb=full, z64=z64, paths=paths, lens=lens, logq=logq, scores=C.byref(sc)):
        return lib.nfst_positional_sample(bs, scores, p(pos), stride, T, k, None, 0, 0, p(ws), wsb, p(z64), p(z32), p(paths), p(arcs),
                                          p(lens), p(logq), None)

    assert call(k=0) == ERR_ARG
    assert call(k=-3) == ERR_ARG
    assert call(T=0, stride=0) == ERR_ARG
    assert call(stride=V) == ERR_ARG
    assert call(stride=T * V + 1) == ERR_ARG
    assert call(ws=None) == ERR_ARG
    assert call(wsb=full - 1) == ERR_ARG
    assert call(wsb=lib.nfst_positional_ws_bytes(bs, T, 0)) == ERR_ARG  # the draws need the stored rows
    for name in ("z64", "paths", "lens", "logq"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(scores=None) == ERR_ARG
    assert call(k=2 ** 31 // B + 1) == ERR_LIMIT  # more walks than the 32-bit walk word of the Philox counter
    marks =np.zeros((B, K, T), np.int32)
    tot, end = np.zeros((B, K), np.float32), np.zeros((B, K), np.int32)

    def scall(T=T, k=K, stride=T * V, marks=marks, tot=tot, end=end, lens=lens):
        return lib.nfst_positional_score_paths(bs, C.byref(sc), p(pos), stride, T, p(marks), k, p(tot), p(end), p(lens), None)

    assert scall(k=0) == ERR_ARG
    assert scall(T=0) == ERR_ARG
    assert scall(stride=3) == ERR_ARG
    for name in ("marks", "tot", "end", "lens"):
        assert scall(**{name: None}) == ERR_ARG, name
    assert scall(k=64 * 65535 + 1) == ERR_LIMIT  # the grid's y dimension


def test_lds_limit_is_the_plan_querys():
    """A batch beyond nfst_positional's LDS limit is refused with the code of nfst_positional_plan, on the host."""
    from nfst_amd import _lib, synth
    from nfst_amd.lattice import LatticeBatch

    l = synth.layered_lattice(5, n_states=7000, avg_degree=2.0, vocab=16, width=8, span=2, max_degree=4)
    lat = LatticeBatch.from_synth([l])
    bs = C.byref(lat.c_struct())
    assert _lib.lib.nfst_positional_plan(bs, 0, None, None) == ERR_LIMIT
    theta = np.zeros(lat.vocab, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    T, K = 4, 2
    n = _lib.lib.nfst_positional_ws_bytes(bs, T, _lib.POS_WS_SAMPLE)
    ws = np.zeros(n // 8 + 2, np.float64)
    z = np.zeros(1, np.float64)
    paths, lens, logq = np.zeros((1, K, T), np.int32), np.zeros((1, K), np.int32), np.zeros((1, K), np.float32)
    assert _lib.lib.nfst_positional_sample(bs, C.byref(sc), None, 0, T, K, None, 0, 0, ws.ctypes.data, n, z.ctypes.data, None,
                                           paths.ctypes.data, None, lens.ctypes.data, logq.ctypes.data, None) == ERR_LIMIT


def test_wrappers_validate_before_any_launch():
    import torch

    from nfst_amd import ops
    from nfst_amd.lattice import LatticeBatch

    lat = LatticeBatch.from_synth(small_lattices()[:3])
    theta = torch.zeros(lat.vocab)
    with pytest.raises(RuntimeError):  # a host batch: no CPU fallback
        ops.positional_sample_paths(lat, theta, 4, torch.zeros(4, lat.vocab))
    with pytest.raises(RuntimeError):
        ops.positional_score_paths(lat, theta, torch.zeros(3, 2, 4, dtype=torch.int32), torch.zeros(4, lat.vocab))


def test_build_guard_covers_the_new_kernels():
    from nfst_amd.build import check_resources

    for name in ("k_positional_walk<true>", "k_positional_walk<false>", "k_positional_score"):
        assert check_resources({name: {"vgpr_spill": 4, "agprs": 0}})
        assert not check_resources({name: {"vgpr_spill": 0, "agprs": 0}})

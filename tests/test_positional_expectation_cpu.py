"""The NumPy restatement of nfst_positional_expectation (tests/positional_expectation_ref.py), which the GPU tests of
ops.positional_expectation* rely on: against path enumeration for every kind of value at every truncation, against
central finite differences of its own E[V], the identities of the semantics, entropy and KL against
enumeration, and -- without positions -- against tests/expectation_ref.py.  Then the C entry points: the exports, every
host-side argument check, the workspace formula, the plan query at the last row count it takes, and the register guard
of the new kernel."""
import ctypes as C
import re

import numpy as np
import pytest

from nfst_amd import synth
from tests import edge_cases as E
from tests import expectation_ref as X
from tests import positional_expectation_ref as PX
from tests import positional_ref as R
from tests.test_positional_cpu import _paths, small_lattices, truncations

NEG = -np.inf
ERR_ARG, ERR_LIMIT = -1, -6  # (include/nfst_hip.h)
LDS_LIMIT = 160 * 1024
KINDS = ("pos_values", "label_values", "arc_values", "coef", "all")


def inputs(l, seed, T, kind, forbid=True):
    """(theta, pos, values dict) of one lattice: scores as tests/test_positional_cpu.py draws them; with ``forbid`` a few
    entries of pos are -inf and the pos_values behind them NaN."""
    rng = np.random.default_rng(seed)
    theta = rng.normal(-1.0, 0.8, size=l.vocab).astype(np.float32)
    pos = rng.normal(0.0, 1.0, size=(T, l.vocab)).astype(np.float32)
    v = {}
    if kind in ("pos_values", "all"):
        v["pos_values"] = rng.normal(0.0, 2.0, size=(T, l.vocab)).astype(np.float32)
    if kind in ("label_values", "all"):
        v["label_values"] = rng.normal(0.5, 1.0, size=l.vocab).astype(np.float32)
    if kind in ("arc_values", "all"):
        v["arc_values"] = rng.normal(0.0, 1.5, size=l.n_arcs).astype(np.float32)
    if kind in ("coef", "all"):
        v["coef"] = 1.0 if kind == "coef" else -0.75
    if forbid:
        hit = rng.random(size=pos.shape) < 0.08
        hit[:, synth.BOS] = False  # (position 0 stays open)
        pos[hit] = NEG
        if "pos_values" in v:
            v["pos_values"][hit] = np.nan
    return theta, pos, v


def close(tag, got, want, tol):
    for k in PX.KEYS:
        g, w = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        assert not np.isnan(g).any(), (tag, k)
        if k == "logz":
            assert (g == w) if not np.isfinite(w) else abs(g - w) <= 1e-12 * max(1.0, abs(w)), (tag, k, g, w)
        else:
            assert np.abs(g - w).max() <= tol, (tag, k, np.abs(g - w).max(), tol)


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("i", range(6))
@pytest.mark.parametrize("kind", KINDS)
def test_reference_equals_path_enumeration(i, kind):
    l = small_lattices()[i]
    alive = 0
    for name, T in truncations(l):
        theta, pos, v = inputs(l, 500 + i, T, kind)
        score = R.arc_score64(l, theta)
        ref = PX.expectation(l, score, pos, T, **v)
        bf = PX.brute_force(l, score, pos, T, paths=_paths(i), **v)
        close((i, kind, name), ref, bf, 1e-12 * max(1.0, bf["M"]))
        if name == "below":
            assert ref["logz"] == NEG and ref["ev"] == 0.0 and not ref["pos_cov"].any() and not ref["arc_cov"].any()
        alive += np.isfinite(ref["logz"])
        sp = R.sum_product(l, score, pos, T)  # the masses are those of the sum-product restatement
        assert ref["logz"] == sp["logz"] or abs(ref["logz"] - sp["logz"]) <= 1e-12 * max(1.0, abs(sp["logz"]))
        assert np.abs(ref["pos_post"] - sp["pos_post"]).max() <= 1e-12 and np.abs(ref["arc_post"] - sp["arc_post"]).max() <= 1e-12
    assert alive >= 2  # (the -inf entries have not emptied every case)


@pytest.mark.parametrize("i", [0, 4])
def test_reference_cov_is_the_gradient_of_its_expectation(i):
    """For values that do not depend on the scores, pos_cov = dE[V]/dpos and arc_cov = dE[V]/d(arc score)."""
    l = small_lattices()[i]
    T = R.min_max_len(l)[1]
    theta, pos, v = inputs(l, 600 + i, T, "all", forbid=False)
    del v["coef"]
    pos = pos.astype(np.float64)
    score = R.arc_score64(l, theta)
    ref = PX.expectation(l, score, pos, T, **v)
    h, tol = 1e-4, 1e-6 * max(1.0, ref["M"])
    ev = lambda sc, ps: PX.expectation(l, sc, ps, T, **v)["ev"]
    for t in range(T):
        for lab in range(l.vocab):
            up, dn = pos.copy(), pos.copy()
            up[t, lab] += h
            dn[t, lab] -= h
            assert abs((ev(score, up) - ev(score, dn)) / (2 * h) - ref["pos_cov"][t, lab]) <= tol, (t, lab)
    for a in range(l.n_arcs):
        up, dn = score.copy(), score.copy()
        up[a] += h
        dn[a] -= h
        assert abs((ev(up, pos) - ev(dn, pos)) / (2 * h) - ref["arc_cov"][a]) <= tol, a


def check_identities(l, ref, len_logz):
    """sum pos_cov = sum arc_cov = Cov(L, V), per-label sums agree; returns (largest violation, Cov(L, V))."""
    cov_lv = ref["arc_cov"].sum()
    worst = abs(ref["pos_cov"].sum() - cov_lv)
    per_label = np.bincount(l.label, weights=ref["arc_cov"], minlength=l.vocab)
    worst = max(worst, np.abs(ref["pos_cov"].sum(axis=0) - per_label).max())
    return worst, cov_lv


@pytest.mark.parametrize("i", range(6))
def test_identities_at_every_truncation(i):
    l = small_lattices()[i]
    for name, T in truncations(l):
        theta, pos, v = inputs(l, 700 + i, T, "all")
        score = R.arc_score64(l, theta)
        ref = PX.expectation(l, score, pos, T, **v)
        sp = R.sum_product(l, score, pos, T)
        if name == "below":
            assert ref["logz"] == NEG
            continue
        if not np.isfinite(ref["logz"]):
            continue
        tol = 1e-12 * max(1.0, ref["M"])
        p_len = np.exp(sp["len_logz"] - sp["logz"])
        L = np.arange(T + 1)
        e_len, var_len = (L * p_len).sum(), (L * L * p_len).sum() - (L * p_len).sum() ** 2
        # Cov(L, V) from the path side of the same restatement: E[L V] - E[L] E[V] by a second expectation with values
        # that count the arcs
        worst, cov_lv = check_identities(l, ref, sp["len_logz"])
        assert worst <= tol * T, name
        # label_values = 1 alone: E[V] = E[L], Cov(L, V) = Var(L) from len_logz
        ones = PX.expectation(l, score, pos, T, label_values=np.ones(l.vocab, np.float32))
        assert abs(ones["ev"] - e_len) <= 1e-12 * T and abs(ones["arc_cov"].sum() - var_len) <= 1e-11 * T * T, name
        assert abs(ones["pos_cov"].sum() - var_len) <= 1e-11 * T * T, name
        # Cov(L, V) of the general values is the covariance of V with the arc count: by enumeration
        bf = PX.brute_force(l, score, pos, T, paths=_paths(i), **v)
        lens = np.array([len(p) for p in _paths(i) if len(p) <= T], np.float64)
        cov_bf = (bf["p"] * lens * bf["V"]).sum() - (bf["p"] * lens).sum() * bf["ev"]
        assert abs(cov_lv - cov_bf) <= 1e-11 * T * max(1.0, ref["M"]), name
        # score_coef = 1 alone: H = log Z - E[V] is -sum p log p
        ent = PX.expectation(l, score, pos, T, coef=1.0)
        assert abs((ent["logz"] - ent["ev"]) - bf["H"]) <= 1e-12 * max(1.0, ent["M"]), name


@pytest.mark.parametrize("i", [0, 5])
def test_entropy_gradient_is_minus_c(i):
    l = small_lattices()[i]
    T = R.min_max_len(l)[1]
    theta, pos, _ = inputs(l, 800 + i, T, "coef", forbid=False)
    pos = pos.astype(np.float64)
    score = R.arc_score64(l, theta)
    ref = PX.expectation(l, score, pos, T, coef=1.0)
    H = lambda ps: (lambda r: r["logz"] - r["ev"])(PX.expectation(l, score, ps, T, coef=1.0))
    h = 1e-4
    for t in range(T):
        for lab in range(0, l.vocab, 3):
            up, dn = pos.copy(), pos.copy()
            up[t, lab] += h
            dn[t, lab] -= h
            assert abs((H(up) - H(dn)) / (2 * h) + ref["pos_cov"][t, lab]) <= 1e-6 * max(1.0, ref["M"]), (t, lab)


def kl_ref(l, theta_p, pos_p, theta_q, pos_q, T):
    """KL(p_T || q_T) by the restatement: one expectation under p with the score differences as values."""
    sp, sq = R.arc_score64(l, theta_p), R.arc_score64(l, theta_q)
    with np.errstate(invalid="ignore"):
        dv = pos_p.astype(np.float64) - pos_q.astype(np.float64)
    rp = PX.expectation(l, sp, pos_p, T, pos_values=dv, arc_values=sp - sq)
    rq = PX.expectation(l, sq, pos_q, T)
    return rq["logz"] - rp["logz"] + rp["ev"], rp, rq


@pytest.mark.parametrize("i", range(6))
def test_kl_against_enumeration_and_zero_with_itself(i):
    l = small_lattices()[i]
    T = R.min_max_len(l)[1] - 1
    theta_p, pos_p, _ = inputs(l, 900 + i, T, "coef")
    theta_q, pos_q, _ = inputs(l, 950 + i, T, "coef", forbid=False)
    kl, rp, rq = kl_ref(l, theta_p, pos_p, theta_q, pos_q, T)
    bp = PX.brute_force(l, R.arc_score64(l, theta_p), pos_p, T, paths=_paths(i))
    bq = PX.brute_force(l, R.arc_score64(l, theta_q), pos_q, T, paths=_paths(i))
    ok = bp["p"] > 0
    want = float((bp["p"][ok] * ((bp["S"][ok] - bp["logz"]) - (bq["S"][ok] - bq["logz"]))).sum())
    assert np.isfinite(want) and want > 0.0
    assert abs(kl - want) <= 1e-12 * max(1.0, rp["M"])
    same, rs, _ = kl_ref(l, theta_p, pos_p, theta_p, pos_p, T)
    assert same == 0.0 and not rs["pos_cov"].any() and not rs["arc_cov"].any()


@pytest.mark.parametrize("i", range(6))
@pytest.mark.parametrize("extra", [0, 3])
def test_without_positions_and_full_length_it_is_the_expectation_reference(i, extra):
    l = small_lattices()[i]
    T = R.min_max_len(l)[1] + extra
    theta, _, v = inputs(l, 1000 + i, T, "all")
    del v["pos_values"]
    score = R.arc_score64(l, theta)
    ref = PX.expectation(l, score, None, T, **v)
    value = v["label_values"].astype(np.float64)[l.label] + v["arc_values"].astype(np.float64) + v["coef"] * score
    x = X.expectation(l.n_rows, l.src, l.dst, score, value)
    tol = 1e-12 * max(1.0, ref["M"])
    assert abs(ref["logz"] - x["logZ"]) <= 1e-12 * max(1.0, abs(x["logZ"])) and abs(ref["ev"] - x["ev"]) <= tol
    assert np.abs(ref["arc_post"] - x["posterior"]).max() <= 1e-12 and np.abs(ref["arc_cov"] - x["cov"]).max() <= tol


# ----------------------------------------------------------------------------- the C entry points
NAMES = ("nfst_positional_expectation_ws_bytes", "nfst_positional_expectation_plan", "nfst_positional_expectation")


def test_exports_are_declared_and_bound():
    import os

    from nfst_amd import _lib

    assert set(NAMES) <= set(_lib.EXPORTS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "nfst_hip.h")) as f:
        text = f.read()
    for name in NAMES:
        assert re.search(r"^(int|int64_t) " + name + r"\(", text, re.M), name
    assert _lib.ABI_VERSION == 7  # functions only: no struct changed


def _host_batch(lats):
    from nfst_amd.lattice import LatticeBatch

    lat = LatticeBatch.from_synth(lats)  # host-packed: the checks run before anything touches a device
    assert lat.device.type == "cpu"
    return lat


def _round(x):
    return (int(x) + 255) & ~255


def test_workspace_formula():
    from nfst_amd import _lib

    lat = _host_batch(small_lattices()[:3])
    bs = C.byref(lat.c_struct())
    lib = _lib.lib
    assert lib.nfst_positional_expectation_ws_bytes(bs, 0) == ERR_ARG
    assert lib.nfst_positional_expectation_ws_bytes(None, 4) == ERR_ARG
    A, TR, B = lat.total_arcs, lat.total_rows, lat.n_lattices
    for T in (1, 6, 37):
        rows = (T + 1) * TR
        want = (sum(_round(k * A) for k in (8, 4, 4, 8, 8, 8, 8)) + sum(_round(k * rows) for k in (8, 4, 8)) + _round(4 * (TR + B)))
        got = lib.nfst_positional_expectation_ws_bytes(bs, T)
        assert got == want and got >= 20 * rows + 48 * A + 4 * TR
        assert got == lib.nfst_positional_ws_bytes(bs, T, 1) + _round(8 * rows) + 2 * _round(8 * A)


def test_argument_checks_return_before_any_launch():
    from nfst_amd import _lib

    lat = _host_batch(small_lattices()[:3])
    V, B, T, A = lat.vocab, lat.n_lattices, 6, lat.total_arcs
    theta = np.zeros(V, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    lib = _lib.lib
    bs = C.byref(lat.c_struct())
    full = lib.nfst_positional_expectation_ws_bytes(bs, T)
    ws = np.zeros(full // 8 + 2, np.float64)  # (16-byte aligned by numpy)
    pos, pv = np.zeros((B, T, V), np.float32), np.zeros((B, T, V), np.float32)
    lv, av = np.zeros((B, V), np.float32), np.zeros(A, np.float32)
    z64, ev64 = np.zeros(B, np.float64), np.zeros(B, np.float64)
    p = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)

    def call(T=T, stride=T * V, pv_stride=T * V, lv_stride=V, coef=0.5, ws=ws, wsb=full, z64=z64, ev64=ev64, scores=C.byref(sc),
             lat_=bs):
        return lib.nfst_positional_expectation(lat_, scores, p(pos), stride, T, p(pv), pv_stride, p(lv), lv_stride, p(av), coef,
                                               p(ws), wsb, p(z64), None, p(ev64), None, None, None, None, None, None)

    assert call(lat_=None) == ERR_ARG and call(scores=None) == ERR_ARG
    assert call(T=0, stride=0, pv_stride=0) == ERR_ARG and call(T=-3, stride=0, pv_stride=0) == ERR_ARG
    for bad in (V, T * V + 1, -1):
        assert call(stride=bad) == ERR_ARG and call(pv_stride=bad) == ERR_ARG
    for bad in (1, V + 1, T * V, -V):
        assert call(lv_stride=bad) == ERR_ARG
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert call(coef=bad) == ERR_ARG
    assert call(z64=None) == ERR_ARG and call(ev64=None) == ERR_ARG
    assert call(ws=None) == ERR_ARG and call(ws=ws.ctypes.data + 8) == ERR_ARG
    assert call(wsb=full - 1) == ERR_ARG
    assert call(wsb=lib.nfst_positional_ws_bytes(bs, T, 1)) == ERR_ARG  # nfst_positional's workspace is too short


def _plan(lat):
    from nfst_amd import _lib, ops

    try:
        return ops.positional_expectation_plan(lat)
    except _lib.NfstError as e:
        return e.code


def exp_lds(max_rows, vocab):
    """Dynamic LDS of nfst_positional_expectation without staged arcs (include/nfst_hip.h)."""
    return 40 * int(max_rows) + 36 * int(vocab) + 4112


def rowmax_states(vocab=256):
    """n_states of ``E.pos_rowmax`` whose batch packs to the most rows the op takes beside ``vocab`` labels: the limit
    from the formula, the lattice's own scratch rows from the packer (the packed batch has ``n_states + 5`` rows at
    ``E.POS_ROWMAX_STATES``)."""
    spare = int(_host_batch(E.pos_rowmax_batch()).max_rows) - E.POS_ROWMAX_STATES
    return (LDS_LIMIT - 4112 - 36 * vocab) // 40 - spare


def rowmax_batch(over=0):
    return [E.pos_rowmax(rowmax_states() + over), E.pos_neighbour(256)]


def test_plan_query_is_the_rule_of_the_header():
    from nfst_amd import _lib

    batches = {"small": small_lattices()[:3], "big": [E.pos_large("big"), E.pos_neighbour()], "degrees": E.pos_degree_classes(),
               "rowmax": rowmax_batch(), "rowmax + 1": rowmax_batch(1)}
    seen = set()
    for name, lats in batches.items():
        lat = _host_batch(lats)
        lds = exp_lds(lat.max_rows, lat.vocab)
        more = 4 * (int(lat.max_rows) + 1 + max(l.n_arcs for l in lats)) + 16
        want = ERR_LIMIT if lds > LDS_LIMIT else ((lds + more, True) if lds + more <= LDS_LIMIT else (lds, False))
        assert _plan(lat) == want, (name, _plan(lat), want)
        seen.add(want if want == ERR_LIMIT else want[1])
    assert seen == {True, False, ERR_LIMIT}
    lat = _host_batch(batches["small"])
    bs = C.byref(lat.c_struct())
    lds, staged = C.c_int64(-1), C.c_int32(-1)
    assert _lib.lib.nfst_positional_expectation_plan(bs, None, None) == 0
    assert _lib.lib.nfst_positional_expectation_plan(bs, C.byref(lds), None) == 0 and lds.value == _plan(lat)[0]
    assert _lib.lib.nfst_positional_expectation_plan(bs, None, C.byref(staged)) == 0 and staged.value == 1
    assert _lib.lib.nfst_positional_expectation_plan(None, C.byref(lds), C.byref(staged)) == ERR_ARG


def test_last_row_count_the_plan_takes():
    lat = _host_batch(rowmax_batch())
    limit_rows = (LDS_LIMIT - 4112 - 36 * lat.vocab) // 40  # from the formula
    assert lat.vocab == 256 and lat.max_rows == limit_rows
    assert exp_lds(lat.max_rows, lat.vocab) <= LDS_LIMIT < exp_lds(lat.max_rows + 1, lat.vocab)
    assert _plan(lat) == (exp_lds(lat.max_rows, lat.vocab), False)
    over = _host_batch(rowmax_batch(1))
    assert over.max_rows == lat.max_rows + 1 and _plan(over) == ERR_LIMIT
    # the launcher refuses it too, on the host
    from nfst_amd import _lib

    theta = np.zeros(over.vocab, np.float32)
    sc = _lib.Scores(theta.ctypes.data, 0, None, None, 0)
    bs = C.byref(over.c_struct())
    T = 2
    n = _lib.lib.nfst_positional_expectation_ws_bytes(bs, T)
    ws = np.zeros(n // 8 + 2, np.float64)
    z, ev = np.zeros(2, np.float64), np.zeros(2, np.float64)
    assert _lib.lib.nfst_positional_expectation(bs, C.byref(sc), None, 0, T, None, 0, None, 0, None, 0.0, ws.ctypes.data, n, z.ctypes.data,
                                                None, ev.ctypes.data, None, None, None, None, None, None) == ERR_LIMIT


def test_baseline_sized_arc_records_do_not_fit_beside_the_row_pairs():
    """The unstaged flavour on a lattice whose arcs nfst_positional stages: 40-byte row pairs leave less room."""
    from nfst_amd import ops

    l = synth.layered_lattice(7, n_states=2000, avg_degree=10.0, vocab=64, width=16, span=3, max_degree=24)
    lat = _host_batch([l])
    assert ops.positional_plan(lat)[1] is True and _plan(lat)[1] is False


def test_build_guard_covers_the_expectation_kernel():
    from nfst_amd.build import check_resources

    for name in ("k_positional_expect<true, false>", "k_positional_expect<false, true>"):
        assert check_resources({name: {"vgpr_spill": 4, "agprs": 0}})
        assert not check_resources({name: {"vgpr_spill": 0, "agprs": 0}})


def test_wrappers_validate_before_any_launch():
    import torch

    from nfst_amd import ops

    lat = _host_batch(small_lattices()[:3])
    V, B, A = lat.vocab, lat.n_lattices, lat.total_arcs
    theta, pos = torch.zeros(V), torch.zeros(4, V)
    with pytest.raises(RuntimeError):  # a host batch: no CPU fallback
        ops.positional_expectation_terms(lat, theta, pos)
    for fn in (ops.positional_expectation, ops.positional_entropy):
        with pytest.raises(RuntimeError):
            fn(lat, theta, pos)
    with pytest.raises(RuntimeError):
        ops.positional_kl_divergence(lat, theta, pos, theta, pos)
    for bad in (torch.zeros(5, V), torch.zeros(4, V + 1), torch.zeros(2, 4, V), torch.zeros(V), torch.zeros(4, V, dtype=torch.int32),
                np.zeros((4, V), np.float32)):
        with pytest.raises(ValueError):
            ops._position_values(lat, bad, 4, "pos_values")
    assert ops._position_values(lat, None, 4, "pos_values") == (None, 0)
    pv, stride = ops._position_values(lat, torch.zeros(B, 4, V, dtype=torch.float64), 4, "pos_values")
    assert pv.dtype == torch.float32 and stride == 4 * V
    assert ops._position_values(lat, torch.zeros(4, V), 4, "pos_values")[1] == 0
    assert isinstance(ops.positional_expectation_plan(lat), tuple)
    assert ops.PositionalExpectationResult._fields == ("logz64", "logz", "ev64", "ev", "pos_posterior", "arc_posterior", "pos_cov",
                                                       "arc_cov")

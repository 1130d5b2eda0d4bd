"""ops.positional_expectation* (nfst_positional_expectation: the first-order expectation semiring on the
time-synchronous sweeps) against the NumPy restatement of tests/positional_expectation_ref.py, which
tests/test_positional_expectation_cpu.py proves against path enumeration.

Bounds, all from the project.  float64 outputs (logz64, ev64) within 1e-9 * max(1, |ref|) resp. 1e-9 * max(1, M) with
M = sum_{t,a} P(a at t) |v_t(a)| (tests/test_gpu_expectation.py's TOL64); float32 E[V], pos_cov and arc_cov within
1e-5 * max(1, M); posteriors within 2e-6.  On every case logz64 / logz / pos_posterior / arc_posterior are also held
bit for bit to ops.positional_forward_backward.  The largest error of every kind goes to
positional_expectation_errors.json in the directory of run outputs (profiles/README.md)."""
import dataclasses
import glob
import itertools
import json
import os

import numpy as np
import pytest
import torch

from nfst_amd import _lib, ops, synth
from nfst_amd.lattice import LatticeBatch
from nfst_amd.scorers import LatticeScorer
from tests import edge_cases as E
from tests import positional_expectation_ref as PX
from tests import positional_ref as R
from tests.test_gpu_positional import _same_vocab, big_pair, cached, degree_classes, large, shared_lattices, small6
from tests.test_positional_cpu import truncations
from tests.test_positional_expectation_cpu import LDS_LIMIT, exp_lds, rowmax_batch

pytestmark = pytest.mark.gpu
PAD, BOS = synth.PAD, synth.BOS
NEG = -np.inf
TOL64, TOL32, TOLP = 1e-9, 1e-5, 2e-6
KINDS = ("pos_values", "label_values", "arc_values", "coef", "all")
ALL = dict(want_pos_posterior=True, want_arc_posterior=True, want_pos_cov=True, want_arc_cov=True)

_ERR = {}


def rec(tag, err):
    _ERR[tag] = max(_ERR.get(tag, 0.0), float(err))
    return float(err)


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for out in sorted(glob.glob(os.path.join(root, "*_out"))):
        if _ERR and os.path.isdir(out):
            with open(os.path.join(out, "positional_expectation_errors.json"), "w") as f:
                json.dump(dict(sorted(_ERR.items())), f, indent=1)


@dataclasses.dataclass
class Case:
    lats: list
    T: int
    theta: np.ndarray  # [V] or [B, V]
    pos: np.ndarray = None  # [T, V], [B, T, V] or None
    asc: np.ndarray = None  # [total_arcs] or None
    pv: np.ndarray = None  # [T, V], [B, T, V] or None
    lv: np.ndarray = None  # [V], [B, V] or None
    av: np.ndarray = None  # [total_arcs] or None
    coef: float = 0.0


def make_case(lats, seed, T, kind="all", shared=False, extras=False, no_pos=False):
    """Inputs of one launch: scores as tests/test_gpu_positional.py draws them (NaN in the pad column of pos: it enters no
    output), values of the ``kind`` asked for; ``shared``: one table for the batch wherever the op takes one; ``extras``:
    per-arc scores (with table weights when the lattices have them)."""
    rng = np.random.default_rng(seed)
    B, V, A = len(lats), lats[0].vocab, sum(l.n_arcs for l in lats)
    c = Case(lats, T, rng.normal(-1.0, 0.8, size=(V,) if shared else (B, V)).astype(np.float32))
    if not no_pos:
        c.pos = rng.normal(0.0, 1.0, size=(T, V) if shared else (B, T, V)).astype(np.float32)
        c.pos[..., PAD] = np.nan
    if extras:
        c.asc = rng.normal(0.0, 0.3, size=A).astype(np.float32)
    if kind in ("pos_values", "all") and not no_pos:
        c.pv = rng.normal(0.0, 2.0, size=(T, V) if shared else (B, T, V)).astype(np.float32)
    if kind in ("label_values", "all"):
        c.lv = rng.normal(0.5, 1.0, size=(V,) if shared else (B, V)).astype(np.float32)
    if kind in ("arc_values", "all"):
        c.av = rng.normal(0.0, 1.5, size=A).astype(np.float32)
    if kind in ("coef", "all"):
        c.coef = 1.0
    return c


def weighted(lats, seed=5):
    rng = np.random.default_rng(seed)
    return [dataclasses.replace(l, weight=rng.normal(0.0, 0.4, size=l.n_arcs).astype(np.float32)) for l in lats]


def _per(x, b, shared_ndim):
    return None if x is None else (x if x.ndim == shared_ndim else x[b])


def reference(c: Case):
    out, a0 = [], 0
    for b, l in enumerate(c.lats):
        sl = slice(a0, a0 + l.n_arcs)
        a0 += l.n_arcs
        score = R.arc_score64(l, _per(c.theta, b, 1), None if c.asc is None else c.asc[sl])
        out.append(PX.expectation(l, score, _per(c.pos, b, 2), c.T, _per(c.pv, b, 2), _per(c.lv, b, 1),
                                  None if c.av is None else c.av[sl], c.coef))
    return out


def launch(lat, c: Case, dev, **want):
    t = lambda x: None if x is None else torch.from_numpy(x).to(dev)
    return ops.positional_expectation_terms(lat, t(c.theta), t(c.pos), c.T, t(c.asc), t(c.pv), t(c.lv), t(c.av), c.coef,
                                            **(want or ALL))


def eq(x, y):
    return torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def check(tag, lat, c: Case, r, refs, dev, fb=True):
    """Every output against the restatement; and the masses bit for bit against ops.positional_forward_backward."""
    B, T = len(c.lats), c.T
    for x in r:
        assert x is None or not torch.isnan(x).any(), tag
    z64, z32, e64, e32 = (x.cpu().numpy() for x in (r.logz64, r.logz, r.ev64, r.ev))
    pp, ap, pc, ac = (None if x is None else x.cpu().numpy() for x in (r.pos_posterior, r.arc_posterior, r.pos_cov, r.arc_cov))
    a0 = 0
    for b, (l, ref) in enumerate(zip(c.lats, refs)):
        sl = slice(a0, a0 + l.n_arcs)
        a0 += l.n_arcs
        M = max(1.0, ref["M"])
        if np.isfinite(ref["logz"]):
            assert rec(tag + ".logz64", abs(z64[b] - ref["logz"]) / max(1.0, abs(ref["logz"]))) <= TOL64, (tag, b, z64[b], ref["logz"])
        else:
            assert z64[b] == NEG and z32[b] == NEG and e64[b] == 0.0 and e32[b] == 0.0, (tag, b)
        print(f"{tag} b={b} M={ref['M']:.3e} ev64 err {abs(e64[b] - ref['ev']):.3e} ev32 err {abs(float(e32[b]) - ref['ev']):.3e}")
        assert rec(tag + ".ev64", abs(e64[b] - ref["ev"]) / M) <= TOL64, (tag, b, e64[b], ref["ev"])
        assert rec(tag + ".ev32", abs(float(e32[b]) - ref["ev"]) / M) <= TOL32, (tag, b)
        if pp is not None:
            assert rec(tag + ".pos_post", np.abs(pp[b] - ref["pos_post"]).max()) <= TOLP, (tag, b)
        if ap is not None:
            assert rec(tag + ".arc_post", np.abs(ap[sl] - ref["arc_post"]).max()) <= TOLP, (tag, b)
        if pc is not None:
            assert rec(tag + ".pos_cov", np.abs(pc[b] - ref["pos_cov"]).max() / M) <= TOL32, (tag, b)
        if ac is not None:
            assert rec(tag + ".arc_cov", np.abs(ac[sl] - ref["arc_cov"]).max() / M) <= TOL32, (tag, b)
    if fb:
        t = lambda x: None if x is None else torch.from_numpy(x).to(dev)
        f = ops.positional_forward_backward(lat, t(c.theta), t(c.pos), T, t(c.asc), want_pos_posterior=True, want_arc_posterior=True)
        assert eq(r.logz64, f.logz64) and eq(r.logz, f.logz), tag
        assert r.pos_posterior is None or eq(r.pos_posterior, f.pos_posterior), tag
        assert r.arc_posterior is None or eq(r.arc_posterior, f.arc_posterior), tag


def run_and_check(tag, c: Case, dev, lat=None, **pack):
    lat = LatticeBatch.from_synth(c.lats, device=dev, **pack) if lat is None else lat
    refs = reference(c)
    r = launch(lat, c, dev)
    check(tag, lat, c, r, refs, dev)
    return lat, r, refs


def per_lattice_bits(lat, lats, r, skip=()):
    out = []
    for b, l in enumerate(lats):
        a0 = int(lat.arc_off[b])
        per = {}
        for k, x in r._asdict().items():
            if x is None or k in skip:
                continue
            x = x.cpu().numpy()
            per[k] = np.ascontiguousarray(x[a0:a0 + l.n_arcs] if k.startswith("arc_") else x[b:b + 1]).view(np.uint8).copy()
        out.append(per)
    return out


def same(x, y, where):
    assert x.keys() == y.keys(), where
    for k in x:
        assert np.array_equal(x[k], y[k]), (where, k)


def cov_close(lat, lats, r1, r2, refs1, tag):
    """pos_cov of two launches of the same lattices: float64 LDS atomics in any order, each within the bound of the
    reference, so within twice the bound of each other."""
    for b, ref in enumerate(refs1):
        d = (r1.pos_cov[b] - r2.pos_cov[b]).abs().max().item()
        assert rec(tag, d / max(1.0, ref["M"])) <= 2 * TOL32, (tag, b)


# ----------------------------------------------------------------------------- (a) six small lattices, every truncation
@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("shared", [False, True])
def test_small_batch_at_every_truncation(dev, shared, extras):
    """Both EXTRA flavours (table weights + arc_scores + arc_values, and none), shared and per-lattice tables, every
    value kind alone (in turn) and all together with score_coef = 1."""
    lats = weighted(small6()) if extras else small6()
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert (lat.weighted != 0) == extras and ops.positional_expectation_plan(lat)[1] is True
    seen, alone = set(), set()
    for i, T in enumerate(sorted({T for l in lats for _, T in truncations(l)})):
        for kind in ("all", KINDS[i % 4]):
            c = make_case(lats, 2000 + T, T, kind, shared=shared, extras=extras)
            if extras and kind != "all":
                c.av = np.random.default_rng(T).normal(0.0, 1.0, size=lat.total_arcs).astype(np.float32)
            _, r, refs = run_and_check(f"a.{int(shared)}{int(extras)}.{kind}", c, dev, lat)
            dead = [not np.isfinite(x["logz"]) for x in refs]
            seen.add((any(dead), not all(dead)))
            alone.add(kind)
            for b in np.nonzero(dead)[0]:
                assert not r.pos_cov[b].any() and not r.pos_posterior[b].any() and float(r.ev64[b]) == 0.0
    assert (True, True) in seen and (False, True) in seen and alone == set(KINDS)


# ----------------------------------------------------------------------------- (b) staged and unstaged launches
@pytest.mark.parametrize("extras", [False, True])
def test_unstaged_beside_a_small_neighbour(dev, extras):
    """k_positional_expect<EXTRA, false>: `big` (481 rows, 42 718 arcs, G = 64) beside a 13-row lattice."""
    l, T = large("big", extras)
    lats = [l, cached(("neighbour", extras), lambda: E.pos_neighbour(weighted=extras))]
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert ops.positional_expectation_plan(lat)[1] is False and R.batch_groups(lat) == [64, 2] and T == 62
    run_and_check(f"unstaged.{int(extras)}", make_case(lats, 2100, T, "all", extras=extras), dev, lat)


@pytest.mark.parametrize("extras", [False, True])
def test_staged_and_unstaged_give_the_same_bits(dev, extras):
    """The thirteen lattices (six small, seven degree classes: G = 8, 16 and 32) in a batch whose arcs are staged in LDS
    and, beside `big`, in one that reads the canonical arrays: the same bits in everything but pos_cov."""
    lats = shared_lattices()
    big = large("big")[0]
    T = cached("shared T", lambda: max(R.min_max_len(l)[1] for l in lats))
    cu = make_case(lats + [big], 2200, T, "all", extras=extras)
    n = sum(l.n_arcs for l in lats)
    cs = Case(lats, T, cu.theta[:-1], cu.pos[:-1], None if cu.asc is None else cu.asc[:n], cu.pv[:-1], cu.lv[:-1], cu.av[:n], cu.coef)
    lat_s, lat_u = LatticeBatch.from_synth(lats, device=dev), LatticeBatch.from_synth(lats + [big], device=dev)
    assert ops.positional_expectation_plan(lat_s)[1] is True and ops.positional_expectation_plan(lat_u)[1] is False
    assert set(R.batch_groups(lat_s)) >= {8, 16, 32}
    _, rs, refs = run_and_check(f"bits.{int(extras)}", cs, dev, lat_s)
    ru = launch(lat_u, cu, dev)
    for b, (x, y) in enumerate(zip(per_lattice_bits(lat_s, lats, rs, ("pos_cov",)), per_lattice_bits(lat_u, lats, ru, ("pos_cov",)))):
        assert set(x) == {"logz64", "logz", "ev64", "ev", "pos_posterior", "arc_posterior", "arc_cov"}
        same(x, y, b)
    cov_close(lat_s, lats, rs, ru, refs, "bits.pos_cov")
    assert all(np.isfinite(x["logz"]) for x in refs)


def test_star_and_funnel_at_one_lane_per_state(dev):
    """G = 1 with out-degree 200 and in-degree 200 (above 64: more than a wave's worth of arcs per state)."""
    lats = E.packing_lattices()
    T = max(R.min_max_len(l)[1] for l in lats)
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert R.batch_groups(lat)[:2] == [1, 1] and np.bincount(lats[0].src).max() == 200
    run_and_check("star", make_case(lats, 2300, T, "all"), dev, lat)
    lat2 = LatticeBatch.from_synth(lats, device=dev, **E.STAR_PACKINGS[3])  # another packing: other scratch rows, the same bits
    assert lat2.max_rows != lat.max_rows
    c = make_case(lats, 2300, T, "all")
    r1, r2 = launch(lat, c, dev), launch(lat2, c, dev)
    for x, y in zip(per_lattice_bits(lat, lats, r1, ("pos_cov",)), per_lattice_bits(lat2, lats, r2, ("pos_cov",))):
        same(x, y, "packing")


@pytest.mark.parametrize("shared", [False, True])
def test_more_rows_than_threads(dev, shared):
    lats, T = big_pair()  # 1 101 rows beside 13
    assert lats[0].n_rows == 1101 and lats[1].n_rows == 13
    run_and_check(f"rows1101.{int(shared)}", make_case(lats, 2400, T, "all", shared=shared), dev)


def test_three_hundred_lattices_equal_three(dev):
    base = small6()[:3]
    T = 6
    c3 = make_case(base, 2500, T, "all")
    lat3, r3, refs = run_and_check("many", c3, dev)
    tile = lambda x: None if x is None else np.tile(x, (100,) + (1,) * (x.ndim - 1))
    c = Case(base * 100, T, tile(c3.theta), tile(c3.pos), None, tile(c3.pv), tile(c3.lv), tile(c3.av), c3.coef)
    lat = LatticeBatch.from_synth(base * 100, device=dev)
    r = launch(lat, c, dev)
    n = lat3.total_arcs
    for k in range(100):
        for key, x3 in r3._asdict().items():
            x = getattr(r, key)
            part = x[n * k:n * (k + 1)] if key.startswith("arc_") else x[3 * k:3 * k + 3]
            if key == "pos_cov":
                assert (part - x3).abs().max().item() <= 2 * TOL32 * max(1.0, max(y["M"] for y in refs)), k
            else:
                assert eq(part, x3), (k, key)


# ----------------------------------------------------------------------------- (c) output subsets
def test_every_subset_of_the_optional_outputs(dev):
    lats = small6()
    T = 9
    c = make_case(lats, 2600, T, "all", extras=True)
    lat, full, refs = run_and_check("subsets", c, dev)
    names = ("pos_posterior", "arc_posterior", "pos_cov", "arc_cov")
    for on in itertools.product([False, True], repeat=4):
        r = launch(lat, c, dev, **{"want_" + k: v for k, v in zip(names, on)})
        for k in ("logz64", "logz", "ev64", "ev"):
            assert eq(getattr(r, k), getattr(full, k)), (on, k)
        for k, want in zip(names, on):
            got = getattr(r, k)
            assert (got is not None) == want, (on, k)
            if want and k == "pos_cov":
                cov_close(lat, lats, r, full, refs, "subsets.pos_cov")
            elif want:
                assert eq(got, getattr(full, k)), (on, k)


# ----------------------------------------------------------------------------- (d) the identities on the GPU outputs
def test_identities(dev):
    lats = small6()
    T = 11
    lat = LatticeBatch.from_synth(lats, device=dev)
    c = make_case(lats, 2700, T, "all")
    _, r, refs = run_and_check("id.all", c, dev, lat)
    al = lat.arc_lattice()
    for b, ref in enumerate(refs):
        if np.isfinite(ref["logz"]):
            pc, ac = r.pos_cov[b].double().sum().item(), r.arc_cov[al == b].double().sum().item()
            tol = TOL32 * max(1.0, ref["M"])
            assert abs(pc - ac) <= 2 * tol and abs(ac - ref["arc_cov"].sum()) <= tol, b
    # label_values = 1 alone: E[V] = E[L] and Cov(L, V) = Var(L), both from len_logz of the posterior op
    ones = Case(lats, T, c.theta, c.pos, lv=np.ones(lat.vocab, np.float32))
    _, r1, refs1 = run_and_check("id.len", ones, dev, lat)
    t = lambda x: torch.from_numpy(x).to(dev)
    f = ops.positional_forward_backward(lat, t(c.theta), t(c.pos), T, want_pos_posterior=False, want_len=True)
    ll, z = f.len_logz.cpu().numpy(), f.logz64.cpu().numpy()
    L = np.arange(T + 1)
    live = 0
    for b in range(len(lats)):
        if np.isfinite(z[b]):
            live += 1
            p = np.exp(ll[b] - z[b])
            e_len, var = (L * p).sum(), (L * L * p).sum() - (L * p).sum() ** 2
            assert rec("id.E[L]", abs(r1.ev64[b].item() - e_len) / max(1.0, refs1[b]["M"])) <= TOL64
            assert abs(r1.arc_cov[al == b].double().sum().item() - var) <= TOL32 * max(1.0, refs1[b]["M"])
            assert abs(r1.pos_cov[b].double().sum().item() - var) <= TOL32 * max(1.0, refs1[b]["M"])
    assert live >= 4
    # score_coef = 1 alone: H = log Z - E[V]; ops.positional_entropy is that difference taken in float64
    ent = Case(lats, T, c.theta, c.pos, coef=1.0)
    _, r2, refs2 = run_and_check("id.H", ent, dev, lat)
    H = ops.positional_entropy(lat, t(c.theta), t(np.nan_to_num(c.pos)), T)
    for b, ref in enumerate(refs2):
        if np.isfinite(ref["logz"]):
            assert abs(H[b].item() - (ref["logz"] - ref["ev"])) <= TOL32 * max(1.0, ref["M"]) and H[b].item() > 0.0


# ----------------------------------------------------------------------------- (e) -inf entries
def test_minus_infinity_entries_with_nan_values_behind_them(dev):
    lats = small6()[:3]
    T = 6
    c = make_case(lats, 2800, T, "all")
    V = lats[0].vocab
    # lattice 0: exactly one path left alive; lattice 1: emptied by a position at which every label is -inf; lattice 2:
    # a few entries forbidden.  Behind every -inf the values are NaN.
    keep = R.enumerate_paths(lats[0])[5]
    one = np.full((T, V), NEG, np.float32)
    for t_, a in enumerate(keep):
        one[t_, lats[0].label[a]] = c.pos[0, t_, lats[0].label[a]]
    c.pos[0] = one
    c.pos[1, 1, :] = NEG
    hit = np.random.default_rng(1).random(size=(T, V)) < 0.1
    hit[:, BOS] = False
    c.pos[2][hit] = NEG
    c.pv[np.isneginf(c.pos)] = np.nan
    dead_label = int(lats[2].label[np.nonzero(lats[2].src == lats[2].dst[0])[0][0]])
    c.theta[2, dead_label] = NEG  # a label at -inf: its label value is NaN too
    c.lv[2, dead_label] = np.nan
    lat, r, refs = run_and_check("inf", c, dev)
    assert float(r.logz64[1]) == NEG and float(r.ev64[1]) == 0.0 and not r.pos_cov[1].any() and not r.pos_posterior[1].any()
    assert np.isfinite(refs[0]["logz"]) and np.isfinite(refs[2]["logz"])
    # one path: no variance, so no covariance, and E[V] is the path's value
    assert r.pos_cov[0].abs().max().item() <= TOL32 * max(1.0, refs[0]["M"]) and abs(refs[0]["ev"]) > 0.1
    pp = r.pos_posterior[0].cpu().numpy()
    assert set(np.unique(pp)) <= {0.0, 1.0} and pp.sum() == len(keep)


# ----------------------------------------------------------------------------- (f) against nfst_expectation
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("extra", [0, 3])
def test_without_positions_it_is_the_expectation_op(dev, extra, exact):
    """nfst_expectation keeps an arc's value as ONE float32 (csrc/expect_kernels.h; tests/test_gpu_expectation.py rounds
    its reference's values the same way), this op as float64.  ``exact``: label and arc values on the 0.25 grid and
    score_coef = 0, so that every arc's value is a float32 and the two E[V] agree as float64 outputs do; otherwise
    (score_coef = 1) the other op's E[V] carries one float32 rounding per arc value, 2^-24 M at most, on top."""
    lats = weighted(small6())
    lat = LatticeBatch.from_synth(lats, device=dev)
    T = int(lat.depth.max()) + extra
    c = make_case(lats, 2900, T, "all", extras=True, no_pos=True)
    assert c.pos is None and c.pv is None
    if exact:
        c.lv, c.av, c.coef = E.quarter(c.lv), E.quarter(c.av), 0.0
    _, r, refs = run_and_check(f"nopos.{extra}{int(exact)}", c, dev, lat)
    t = lambda x: torch.from_numpy(x).to(dev)
    x = ops.expectation_terms(lat, t(c.theta), t(c.asc), t(c.lv), t(c.av), c.coef, want_posterior=True, want_cov=True)
    M = max(1.0, max(ref["M"] for ref in refs))
    assert rec("nopos.logz", ((r.logz64 - x.logz64).abs() / x.logz64.abs().clamp(min=1.0)).max().item()) <= TOL64
    assert rec(f"nopos.ev64.{int(exact)}", (r.ev64 - x.ev64).abs().max().item() / M) <= TOL64 + (0.0 if exact else 2.0 ** -24)
    assert rec("nopos.arc_post", (r.arc_posterior - x.posterior).abs().max().item()) <= TOLP
    assert rec("nopos.arc_cov", (r.arc_cov - x.cov).abs().max().item() / M) <= TOL32


# ----------------------------------------------------------------------------- (g) exponent range, T = 1, the row limit
@pytest.mark.parametrize("name", E.RANGE_CASES)
def test_exponent_range(dev, name):
    """|log Z| up to 2.6e5 with score_coef = 1: E[V] is of the size of log Z."""
    lats, theta, asc, pos, T = E.pos_range_inputs(name)
    c = make_case(lats, 3000, T, "all", extras=True)
    c.theta, c.asc, c.pos = theta, asc, pos
    _, r, refs = run_and_check(f"range.{name}", c, dev)
    assert max(abs(x["logz"]) for x in refs) > E.RANGE_LOGZ[name] and max(x["M"] for x in refs) > E.RANGE_LOGZ[name]
    assert all(torch.isfinite(x).all() for x in r)


@pytest.mark.parametrize("T", [1, 9])
def test_truncation_extremes(dev, T):
    lats = E.mixed_batch()
    c = make_case(lats, 3100 + T, T, "all")
    _, r, refs = run_and_check(f"trunc.{T}", c, dev)
    live = [bool(np.isfinite(x["logz"])) for x in refs]
    assert live == {1: [False] * 5 + [True], 9: [True, True, False, False, True, True]}[T]


def test_last_row_count_the_plan_takes(dev):
    lats = rowmax_batch()
    lat = LatticeBatch.from_synth(lats, device=dev)
    assert exp_lds(lat.max_rows, lat.vocab) <= LDS_LIMIT < exp_lds(lat.max_rows + 1, lat.vocab)
    assert ops.positional_expectation_plan(lat) == (exp_lds(lat.max_rows, lat.vocab), False)
    T = 20
    assert R.min_max_len(lats[0])[0] < T
    run_and_check("rowmax", make_case(lats, 3200, T, "all"), dev, lat)
    over = LatticeBatch.from_synth(rowmax_batch(1), device=dev)
    c = make_case(rowmax_batch(1), 3200, 2, "coef")
    with pytest.raises(_lib.NfstError) as e:
        launch(over, c, dev)
    assert e.value.code == -6
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- (h) autograd
def _grads(c: Case, refs, g, lat):
    """The analytic gradients of sum_b g_b E_b[V] from the restatement: per lattice, unsummed."""
    k = c.coef
    d_pos = np.stack([(x["pos_cov"] + k * x["pos_post"]) * gb for x, gb in zip(refs, g)])
    d_pv = np.stack([x["pos_post"] * gb for x, gb in zip(refs, g)])
    d_arc = np.concatenate([(x["arc_cov"] + k * x["arc_post"]) * gb for x, gb in zip(refs, g)])
    d_av = np.concatenate([x["arc_post"] * gb for x, gb in zip(refs, g)])
    return dict(pos=d_pos, theta=d_pos.sum(axis=1), asc=d_arc, pv=d_pv, lv=d_pv.sum(axis=1), av=d_av)


def _leaves(c: Case, dev):
    out = {}
    for k, x in (("theta", c.theta), ("pos", c.pos), ("asc", c.asc), ("pv", c.pv), ("lv", c.lv), ("av", c.av)):
        out[k] = None if x is None else torch.from_numpy(np.nan_to_num(x)).to(dev).requires_grad_(True)
    return out


def _clean(c: Case):
    c.pos = np.nan_to_num(c.pos)  # (a NaN input would give a NaN * 0 gradient in torch's own arithmetic)
    return c


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("coef", [0.0, 1.0])
def test_autograd_of_the_expectation(dev, shared, coef):
    lats = weighted(small6())
    T = 13
    c = _clean(make_case(lats, 3300, T, "all", shared=shared, extras=True))
    c.coef = coef
    lat = LatticeBatch.from_synth(lats, device=dev)
    refs = reference(c)
    g = np.linspace(0.5, 2.0, len(lats)).astype(np.float32)
    x = _leaves(c, dev)
    ev = ops.positional_expectation(lat, x["theta"], x["pos"], T, x["asc"], x["pv"], x["lv"], x["av"], coef)
    ev.backward(torch.from_numpy(g).to(dev))
    want = _grads(c, refs, g, lat)
    M = max(1.0, max(r["M"] for r in refs)) * float(g.max())
    for k, leaf in x.items():
        w = want[k]
        if shared and k in ("pos", "theta", "pv", "lv"):
            w = w.sum(axis=0)
        assert leaf.grad.shape == leaf.shape, k
        assert rec(f"grad.ev.{k}", np.abs(leaf.grad.cpu().numpy() - w).max() / M) <= TOL32 * (len(lats) if shared else 1), k
    for b, ref in enumerate(refs):
        assert abs(ev[b].item() - ref["ev"]) <= TOL32 * max(1.0, ref["M"])


@pytest.mark.parametrize("shared", [False, True])
def test_autograd_of_the_entropy(dev, shared):
    lats = small6()
    T = 13
    c = _clean(make_case(lats, 3400, T, "coef", shared=shared, extras=True))
    lat = LatticeBatch.from_synth(lats, device=dev)
    refs = reference(c)
    g = np.linspace(0.5, 2.0, len(lats)).astype(np.float32)
    x = _leaves(c, dev)
    H = ops.positional_entropy(lat, x["theta"], x["pos"], T, x["asc"])
    H.backward(torch.from_numpy(g).to(dev))
    c0 = dataclasses.replace(c, coef=0.0)  # -c alone: no coef * posterior term
    want = _grads(c0, refs, -g, lat)
    M = max(1.0, max(r["M"] for r in refs)) * float(g.max())
    for k in ("theta", "pos", "asc"):
        w = want[k].sum(axis=0) if shared and k != "asc" else want[k]
        assert rec(f"grad.H.{k}", np.abs(x[k].grad.cpu().numpy() - w).max() / M) <= TOL32 * (len(lats) if shared else 1), k
    live = [bool(np.isfinite(ref["logz"])) for ref in refs]
    assert live == [True] * 5 + [False]  # (the last lattice has no path of 13 arcs: -inf, never a NaN, and no gradient)
    for b, ref in enumerate(refs):
        if live[b]:
            assert abs(H[b].item() - (ref["logz"] - ref["ev"])) <= TOL32 * max(1.0, ref["M"])
        else:
            assert H[b].item() == NEG and (shared or not x["pos"].grad[b].any())


def test_autograd_of_the_kl_divergence_and_zero_gradient_at_q_equal_p(dev):
    lats = small6()
    T = 24  # (every lattice has a path: KL of two empty distributions is -inf - -inf, as ops.kl_divergence gives it)
    cp = _clean(make_case(lats, 3500, T, "coef", extras=True))
    cq = _clean(make_case(lats, 3501, T, "coef", shared=True, extras=True))
    lat = LatticeBatch.from_synth(lats, device=dev)
    # the restatement: an expectation under p with the score differences as values
    cv = dataclasses.replace(cp, pv=cp.pos - cq.pos[None], lv=cp.theta - cq.theta[None], av=cp.asc - cq.asc, coef=0.0)
    rp, rq = reference(cv), reference(dataclasses.replace(cq, coef=0.0))
    p, q = _leaves(cp, dev), _leaves(cq, dev)
    kl = ops.positional_kl_divergence(lat, p["theta"], p["pos"], q["theta"], q["pos"], T, p["asc"], q["asc"])
    kl.sum().backward()
    M = max(1.0, max(r["M"] for r in rp))
    for b in range(len(lats)):
        want = rq[b]["logz"] - rp[b]["logz"] + rp[b]["ev"]
        assert want > 0.0 and rec("kl", abs(kl[b].item() - want) / M) <= TOL32, b
    one = np.ones(len(lats), np.float32)
    gp = _grads(cv, rp, one, lat)
    assert rec("grad.kl.pos_p", np.abs(p["pos"].grad.cpu().numpy() - gp["pos"]).max() / M) <= TOL32
    assert rec("grad.kl.theta_p", np.abs(p["theta"].grad.cpu().numpy() - gp["theta"]).max() / M) <= TOL32
    assert rec("grad.kl.arc_p", np.abs(p["asc"].grad.cpu().numpy() - gp["asc"]).max() / M) <= TOL32
    dq_pos = np.stack([y["pos_post"] - x["pos_post"] for x, y in zip(rp, rq)])
    dq_arc = np.concatenate([y["arc_post"] - x["arc_post"] for x, y in zip(rp, rq)])
    assert rec("grad.kl.pos_q", np.abs(q["pos"].grad.cpu().numpy() - dq_pos.sum(axis=0)).max()) <= TOLP * len(lats)
    assert rec("grad.kl.theta_q", np.abs(q["theta"].grad.cpu().numpy() - dq_pos.sum(axis=(0, 1))).max()) <= TOLP * len(lats) * T
    assert rec("grad.kl.arc_q", np.abs(q["asc"].grad.cpu().numpy() - dq_arc).max()) <= 2 * TOLP
    # q = p (separate tensors with the same values): KL = 0 and the gradient in q is exactly 0 -- the two launches
    # write the same posterior bits
    p, q = _leaves(cp, dev), _leaves(cp, dev)
    kl = ops.positional_kl_divergence(lat, p["theta"], p["pos"], q["theta"], q["pos"], T, p["asc"], q["asc"])
    kl.sum().backward()
    assert kl.abs().max().item() <= TOL32
    for k in ("theta", "pos", "asc"):
        assert not q[k].grad.any(), k
        assert p[k].grad.abs().max().item() <= TOL32, k


def test_scorer_methods_and_the_risk(dev):
    """LatticeScorer.positional_risk: the expected Hamming loss against a gold sequence, and its gradients."""
    lats = small6()
    T = 13
    c = _clean(make_case(lats, 3600, T, "pos_values", shared=False))
    c.theta = c.theta[0].copy()
    gold = np.random.default_rng(3).integers(3, lats[0].vocab, size=(len(lats), T))
    c.pv = np.ones_like(c.pv)
    np.put_along_axis(c.pv, gold[..., None], 0.0, axis=2)  # cost 0 at the gold label, 1 elsewhere
    lat = LatticeBatch.from_synth(lats, device=dev)
    refs = reference(c)
    sc = LatticeScorer(lat.vocab, theta=c.theta).to(dev).set_lattice(lat)
    pos = torch.from_numpy(c.pos).to(dev).requires_grad_(True)
    cost = torch.from_numpy(c.pv).to(dev).requires_grad_(True)
    risk = sc.positional_risk(pos, cost)
    risk.sum().backward()
    want = _grads(c, refs, np.ones(len(lats), np.float32), lat)
    M = max(1.0, max(r["M"] for r in refs))
    for b, ref in enumerate(refs):
        assert 0.0 <= ref["ev"] <= T and abs(risk[b].item() - ref["ev"]) <= TOL32 * max(1.0, ref["M"])
    assert rec("grad.risk.pos", np.abs(pos.grad.cpu().numpy() - want["pos"]).max() / M) <= TOL32
    assert rec("grad.risk.theta", np.abs(sc.theta.grad.cpu().numpy() - want["theta"].sum(axis=0)).max() / M) <= TOL32 * len(lats)
    assert rec("grad.risk.cost", np.abs(cost.grad.cpu().numpy() - want["pv"]).max()) <= TOLP
    assert torch.equal(sc.positional_expectation(pos.detach(), pos_values=cost.detach()), risk.detach())
    H = sc.positional_entropy(pos.detach())
    assert torch.equal(H, ops.positional_entropy(lat, sc.theta.detach(), pos.detach()))


def test_hessian_vector_product_against_finite_differences(dev):
    """pos_cov / arc_cov for values (u_pos, u_arc) = (Hessian of log Z_T) u: central differences of the restatement's
    posteriors along u (h = 1e-4, bound 1e-6 scaled by max(1, M), as tests/test_positional_expectation_cpu.py)."""
    lats = small6()[:3]
    T = 7
    c = _clean(make_case(lats, 3700, T, "pos_values"))
    c.av = np.random.default_rng(4).normal(0.0, 1.0, size=sum(l.n_arcs for l in lats)).astype(np.float32)
    c.asc = np.zeros_like(c.av)
    _, r, refs = run_and_check("hvp", c, dev)
    h, a0 = 1e-4, 0
    for b, l in enumerate(lats):
        sl = slice(a0, a0 + l.n_arcs)
        a0 += l.n_arcs
        score = R.arc_score64(l, c.theta[b])
        u_pos, u_arc = c.pv[b].astype(np.float64), c.av[sl].astype(np.float64)
        up = R.sum_product(l, score + h * u_arc, c.pos[b].astype(np.float64) + h * u_pos, T)
        dn = R.sum_product(l, score - h * u_arc, c.pos[b].astype(np.float64) - h * u_pos, T)
        tol = 1e-6 * max(1.0, refs[b]["M"]) + TOL32 * max(1.0, refs[b]["M"])
        assert rec("hvp.pos", np.abs(r.pos_cov[b].cpu().numpy() - (up["pos_post"] - dn["pos_post"]) / (2 * h)).max()) <= tol
        assert rec("hvp.arc", np.abs(r.arc_cov[sl].cpu().numpy() - (up["arc_post"] - dn["arc_post"]) / (2 * h)).max()) <= tol


def test_second_backward_raises(dev):
    lats = small6()[:3]
    c = _clean(make_case(lats, 3800, 6, "pos_values"))
    lat = LatticeBatch.from_synth(lats, device=dev)
    x = _leaves(c, dev)
    for fn in (lambda: ops.positional_expectation(lat, x["theta"], x["pos"], pos_values=x["pv"]),
               lambda: ops.positional_entropy(lat, x["theta"], x["pos"]),
               lambda: ops.positional_kl_divergence(lat, x["theta"], x["pos"], x["theta"].detach() * 0.5, x["pos"].detach())):
        (g,) = torch.autograd.grad(fn().sum(), x["pos"], create_graph=True)
        with pytest.raises(RuntimeError):
            g.sum().backward()


# ----------------------------------------------------------------------------- (i) repeatability
def test_two_launches_and_another_batch_order_give_the_same_bits(dev):
    lats = _same_vocab(small6() + big_pair()[0])
    T = 30
    c = make_case(lats, 3900, T, "all", extras=True)
    lat, r1, refs = run_and_check("repeat", c, dev)
    r2 = launch(lat, c, dev)
    for x, y in zip(per_lattice_bits(lat, lats, r1, ("pos_cov",)), per_lattice_bits(lat, lats, r2, ("pos_cov",))):
        same(x, y, "again")
    cov_close(lat, lats, r1, r2, refs, "repeat.pos_cov")
    order = [7, 2, 5, 0, 6, 3, 1, 4]
    off = np.concatenate([[0], np.cumsum([l.n_arcs for l in lats])])
    arcs = lambda x: np.concatenate([x[off[i]:off[i + 1]] for i in order])
    cp = Case([lats[i] for i in order], T, c.theta[order], c.pos[order], arcs(c.asc), c.pv[order], c.lv[order], arcs(c.av), c.coef)
    lat_p = LatticeBatch.from_synth(cp.lats, device=dev)
    rp = launch(lat_p, cp, dev)
    a, p = per_lattice_bits(lat, lats, r1, ("pos_cov",)), per_lattice_bits(lat_p, cp.lats, rp, ("pos_cov",))
    for j, i in enumerate(order):
        same(a[i], p[j], (i, j))
        assert (r1.pos_cov[i] - rp.pos_cov[j]).abs().max().item() <= 2 * TOL32 * max(1.0, refs[i]["M"])


def test_snips_shaped_batch_with_and_without_chunked_programs(dev):
    lats = synth.snips_shaped_batch(4, vocab=250)
    T = max(R.min_max_len(l)[1] for l in lats)
    c = make_case(lats, 4000, T, "all")
    plain = LatticeBatch.from_synth(lats).to(dev, auto_chunks=False)
    host = LatticeBatch.from_synth(lats)
    assert host.build_chunks(force=True)
    chunked = host.to(dev)
    assert chunked.chunks is not None and plain.chunks is None
    _, r1, refs = run_and_check("snips", c, dev, plain)
    r2 = launch(chunked, c, dev)
    for x, y in zip(per_lattice_bits(plain, lats, r1, ("pos_cov",)), per_lattice_bits(chunked, lats, r2, ("pos_cov",))):
        same(x, y, "chunks")
    cov_close(plain, lats, r1, r2, refs, "snips.pos_cov")


# ----------------------------------------------------------------------------- (j) wrappers
def test_wrapper_errors_raise_before_any_launch(dev):
    lats = small6()[:3]
    lat = LatticeBatch.from_synth(lats, device=dev)
    V, A = lat.vocab, lat.total_arcs
    theta, good = torch.zeros(V, device=dev), torch.zeros(3, 6, V, device=dev)
    terms = ops.positional_expectation_terms
    for bad in (torch.zeros(3, 6, V + 1, device=dev), torch.zeros(2, 6, V, device=dev), torch.zeros(V, device=dev), good.cpu(),
                torch.zeros(3, 5, V, device=dev), good.long()):
        with pytest.raises(ValueError):
            terms(lat, theta, good, pos_values=bad)
        with pytest.raises(ValueError):
            ops.positional_expectation(lat, theta, good, pos_values=bad)
    for bad in (torch.zeros(V + 1, device=dev), torch.zeros(2, V, device=dev), torch.zeros(V)):
        with pytest.raises(ValueError):
            terms(lat, theta, good, label_values=bad)
    for bad in (torch.zeros(A + 1, device=dev), torch.zeros(A)):
        with pytest.raises(ValueError):
            terms(lat, theta, good, arc_values=bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            terms(lat, theta, good, score_coef=bad)
    with pytest.raises(ValueError):
        terms(lat, theta, good, T=5)
    with pytest.raises(ValueError):
        terms(lat, theta, None, T=0)
    with pytest.raises(ValueError):
        ops.positional_entropy(lat, theta.cpu(), good)
    with pytest.raises(ValueError):
        ops.positional_kl_divergence(lat, theta, good, theta, torch.zeros(3, 5, V, device=dev))
    r = terms(lat, theta, None)  # no positions, no values, nothing asked for: log Z and E[V] = 0
    assert r.pos_posterior is None and r.arc_cov is None and not r.ev64.any() and torch.isfinite(r.logz64).all()

"""The epilogue of the forward-backward step: the posterior pass with its preloaded arc groups and
its remainder loop, the 16-byte row outputs, and the output-store helper (csrc/out_store.h).

Single lattices straddle the capacity of the preload -- 7 groups of 4 arcs on each of 768 helper threads hold 21,504 arcs;
what is beyond goes through the remainder loop, 4 groups per thread and trip, i.e. 16,384 arcs per trip -- and the
capacities 8 and 9 groups would have (24,576 and 27,648: the sizes at which a preload fitted to the batch changes kernels),
and run alone and as the second lattice of a batch whose first lattice has 4k+1, 4k+2, 4k+3 arcs and rows, which leaves
``arc_off`` and ``row_off`` unaligned: the scalar heads and tails of the arc pass and of the row stores.  Every shape runs
with posteriors and rows, rows only, label sums only and caller ``arc_scores``, on the default flavour and on
``tuning(tw=0)``, twice.

Bounds: log Z 1e-5 and posteriors 2e-6 against the float64 oracle (the suite's bounds, tests/test_gpu_parity.py); everything
else is equality of bits: alone against inside a batch, flavour against flavour, launch against launch.  The label sums are
accumulated by float atomics in LDS, whose order is not fixed: they are held to the oracle (1e-4, as in the parity tests), not to bits.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from nfst_amd import ops, synth, _lib
from nfst_amd.lattice import LatticeBatch
from nfst_amd.synth import SynthLattice

pytestmark = pytest.mark.gpu

V = 256
GROUP_ARCS = 768 * 4  # arcs one preloaded group per helper thread covers
# the capacity of the 7 preloaded groups and the one 8 would have, straddled; 26,000: deep in the remainder loop; 28,001 / 32,002:
# beyond what 9 groups would hold, with odd tails
ARCS = [7 * GROUP_ARCS - 4, 7 * GROUP_ARCS, 7 * GROUP_ARCS + 4, 8 * GROUP_ARCS - 4, 8 * GROUP_ARCS, 8 * GROUP_ARCS + 4,
        26000, 28001, 32002]


def with_parallel_arcs(l: SynthLattice, n_arcs: int, seed: int) -> SynthLattice:
    """``l`` padded to ``n_arcs`` arcs: new arcs copy the source and destination of an existing one (never the sink's self
    loop) under a label their source does not use yet, spread evenly over the states, so levels and depth stay what they were."""
    rng = np.random.default_rng(seed)
    used = np.zeros((l.n_rows, l.vocab), bool)
    used[l.src, l.label] = True
    used[:, :synth.N_SPECIAL] = True
    cand = np.nonzero(l.src != l.dst)[0]
    src, label, dst = [l.src], [l.label], [l.dst]
    need = n_arcs - l.n_arcs
    assert need >= 0
    order = rng.permutation(cand)
    k = 0
    new_s, new_l, new_d = [], [], []
    while need > 0:
        a = int(order[k % order.shape[0]])
        k += 1
        s = int(l.src[a])
        free = np.nonzero(~used[s])[0]
        if free.shape[0] == 0:
            continue
        lab = int(free[rng.integers(0, free.shape[0])])
        used[s, lab] = True
        new_s.append(s); new_l.append(lab); new_d.append(int(l.dst[a]))
        need -= 1
    src = np.concatenate(src + [np.array(new_s, np.int32)])
    label = np.concatenate(label + [np.array(new_l, np.int32)])
    dst = np.concatenate(dst + [np.array(new_d, np.int32)])
    o = np.lexsort((label, src))
    out = SynthLattice(l.n_rows, l.vocab, src[o].astype(np.int32), label[o].astype(np.int32), dst[o].astype(np.int32))
    assert out.n_arcs == n_arcs
    return out


@functools.lru_cache(maxsize=None)
def base_lattice() -> SynthLattice:
    return synth.layered_lattice(4242, n_states=2001, avg_degree=9.0, vocab=V, width=128, span=4)


@functools.lru_cache(maxsize=None)
def big_lattice(n_arcs: int) -> SynthLattice:
    return with_parallel_arcs(base_lattice(), n_arcs, seed=n_arcs)


@functools.lru_cache(maxsize=None)
def lead_lattice(k: int) -> SynthLattice:
    """A small lattice with 4i + k rows and 4j + k arcs."""
    S = 40
    while (S + 1) % 4 != k:
        S += 1
    l = synth.layered_lattice(77 + k, n_states=S, avg_degree=4.0, vocab=V, width=4, span=2)
    n = l.n_arcs
    while n % 4 != k:
        n += 1
    return with_parallel_arcs(l, n, seed=k)


def tiny_lattices():
    """2 rows / 2 arcs, 3 rows / 3 arcs, and 3 rows / 2 + 1 arcs with a pair of parallel arcs."""
    return [synth._finish(2, V, [0], [synth.EOS], [1]),
            synth._finish(3, V, [0, 1], [synth.BOS, synth.EOS], [1, 2]),
            synth._finish(3, V, [0, 1, 1], [synth.BOS, synth.EOS, 7], [1, 2, 2])]


THETA = synth.label_scores(11, V)


def arc_scores_of(l: SynthLattice) -> np.ndarray:
    return np.random.default_rng(l.n_arcs).normal(0.0, 0.3, size=l.n_arcs).astype(np.float32)


_ORACLE = {}


def oracle_of(l: SynthLattice, key, scored: bool):
    """float64 forward-backward of one lattice, computed once per (lattice, with / without arc scores)."""
    if (key, scored) not in _ORACLE:
        sc = THETA[l.label].astype(np.float64)
        if scored:
            sc = sc + arc_scores_of(l).astype(np.float64)
        _ORACLE[(key, scored)] = O.forward_backward(l.n_rows, l.src, l.dst, sc)
    return _ORACLE[(key, scored)]


def same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


def run_all(lat, arc_scores):
    """The four output combinations, twice each (launch against launch), on the current flavour; tensors on the host."""
    th = torch.from_numpy(THETA)
    out = {}
    for name, kw in (("full", dict()), ("rows", dict(want_posterior=False)),
                     ("gth", dict(want_alpha_beta=False, want_posterior=False, want_grad_theta=True)),
                     ("scored", dict(arc_scores=arc_scores, want_me=True))):
        a = ops.forward_backward(lat, th, **kw)
        b = ops.forward_backward(lat, th, **kw)
        for f in ("logalpha", "logbeta", "posterior", "logz64", "logz"):
            assert same(getattr(a, f), getattr(b, f)), (name, f, "two consecutive launches")
        out[name] = a
    return out


def rows_of(t, lat, b):
    r0, n = int(lat.row_off[b]), int(lat.n_rows[b])
    return t[r0:r0 + n]


def arcs_of(t, lat, b):
    a0, a1 = int(lat.arc_off[b]), int(lat.arc_off[b + 1]) if b + 1 < lat.n_lattices else lat.total_arcs
    return t[a0:a1]


def check_against_oracle(res, lat, b, l, key):
    for name, scored in (("full", False), ("scored", True)):
        o = oracle_of(l, key, scored)
        r = res[name]
        assert abs(float(r.logz64[b]) - o["logZ"]) <= 1e-5 and abs(float(r.logz[b]) - o["logZ"]) <= 1e-5, name
        post = arcs_of(r.posterior, lat, b).cpu().numpy()
        assert post.shape[0] == l.n_arcs
        assert np.max(np.abs(post - o["posterior"])) <= 2e-6, name
        for got, ref in ((r.logalpha, o["logalpha"]), (r.logbeta, o["logbeta"])):
            got = rows_of(got, lat, b).cpu().numpy().astype(np.float64)
            inf = np.isneginf(ref)
            assert np.array_equal(np.isneginf(got), inf)
            half_ulp = 0.5 * np.spacing(np.abs(ref[~inf]).astype(np.float32)).astype(np.float64)  # (float32 outputs)
            assert np.all(np.abs(got[~inf] - ref[~inf]) <= 1e-5 + half_ulp), name
    # rows only: the bits of the full run; the (mantissa, exponent) pairs give log beta back
    assert torch.equal(res["rows"].logalpha, res["full"].logalpha) and torch.equal(res["rows"].logbeta, res["full"].logbeta)
    assert res["rows"].posterior is None
    me = rows_of(res["scored"].beta_me, lat, b).cpu().numpy()
    lb = rows_of(res["scored"].logbeta, lat, b).cpu().numpy().astype(np.float64)
    reach = me[:, 0] > 0
    assert np.array_equal(reach, np.isfinite(lb))
    from_me = np.log(me[reach, 0].astype(np.float64)) + np.ascontiguousarray(me[reach, 1]).view(np.int32).astype(np.float64) * np.log(2.0)
    assert np.max(np.abs(from_me - lb[reach]) / np.maximum(1.0, np.abs(lb[reach]))) <= 1e-6
    # label sums against the oracle's posteriors
    o = oracle_of(l, key, False)
    ref_g = np.bincount(l.label, weights=o["posterior"], minlength=V)
    assert np.max(np.abs(res["gth"].grad_theta[b].cpu().numpy() - ref_g)) <= 1e-4
    assert torch.equal(res["gth"].logz64, res["full"].logz64)


def check_same_bits(res_a, lat_a, b_a, res_b, lat_b, b_b, what):
    for name in ("full", "scored"):
        for f in ("logalpha", "logbeta"):
            assert torch.equal(rows_of(getattr(res_a[name], f), lat_a, b_a), rows_of(getattr(res_b[name], f), lat_b, b_b)), (what, name, f)
        assert torch.equal(arcs_of(res_a[name].posterior, lat_a, b_a), arcs_of(res_b[name].posterior, lat_b, b_b)), (what, name)
        assert torch.equal(res_a[name].logz64[b_a], res_b[name].logz64[b_b]), (what, name)
    # (compared as words: a negative exponent read as a float is a NaN)
    assert torch.equal(rows_of(res_a["scored"].beta_me, lat_a, b_a).view(torch.int32), rows_of(res_b["scored"].beta_me, lat_b, b_b).view(torch.int32)), what


def both_flavours(lat, arc_scores):
    default = run_all(lat, arc_scores)
    with _lib.tuning(tw=0):
        pipeline = run_all(lat, arc_scores)
    for b in range(lat.n_lattices):
        check_same_bits(default, lat, b, pipeline, lat, b, "tile waves against the pipeline")
    return default


@pytest.mark.parametrize("n_arcs", ARCS)
def test_capacity_boundaries_alone_and_unaligned(dev, n_arcs):
    big = big_lattice(n_arcs)
    xs = arc_scores_of(big)
    alone = LatticeBatch.from_synth([big], device=dev)
    # the float32 tile-wave kernel runs all-compact batches up to 192 tiles (deeper ones: the precise flavour)
    assert alone.c_struct().reserved0 & 1 and alone.c_struct().max_tiles <= 192
    assert (alone.c_struct().reserved0 >> 8) == n_arcs
    ref = both_flavours(alone, torch.from_numpy(xs))
    check_against_oracle(ref, alone, 0, big, n_arcs)
    for k in (1, 2, 3):
        lead = lead_lattice(k)
        assert lead.n_arcs % 4 == k and lead.n_rows % 4 == k
        lat = LatticeBatch.from_synth([lead, big], device=dev)
        assert int(lat.arc_off[1]) % 4 == k and int(lat.row_off[1]) % 4 == k
        got = both_flavours(lat, torch.from_numpy(np.concatenate([arc_scores_of(lead), xs])))
        check_same_bits(got, lat, 1, ref, alone, 0, f"second lattice behind 4i+{k} rows and arcs against alone")
        check_against_oracle(got, lat, 0, lead, ("lead", k))
        assert torch.equal(got["gth"].logz64[1], ref["gth"].logz64[0])
        assert np.max(np.abs((got["gth"].grad_theta[1] - ref["gth"].grad_theta[0]).cpu().numpy())) <= 1e-4


def test_lattices_of_fewer_than_four_arcs_and_rows(dev):
    """Lattices of 2 .. 4 arcs and 2 .. 3 rows, packed back to back: whole lattices inside one 16-byte group, in a head or in a tail."""
    tiny = tiny_lattices()
    group = [tiny[0], tiny[1], tiny[2], tiny[0], lead_lattice(3), tiny[2], tiny[1]]
    lat = LatticeBatch.from_synth(group, device=dev)
    xs = np.concatenate([arc_scores_of(l) for l in group])
    got = both_flavours(lat, torch.from_numpy(xs))
    for b, l in enumerate(group):
        key = ("tiny", l.n_rows, l.n_arcs) if l.n_rows < 4 else ("lead", 3)
        check_against_oracle(got, lat, b, l, key)
        one = LatticeBatch.from_synth([l], device=dev)
        check_same_bits(got, lat, b, both_flavours(one, torch.from_numpy(arc_scores_of(l))), one, 0, f"lattice {b} against alone")


def test_backward_rows_match_the_fused_step(dev):
    """k_backward's row outputs go through the same 16-byte row stores: bits of the forward-backward step, aligned and not."""
    th = torch.from_numpy(THETA)
    for k in (1, 2, 3):
        lat = LatticeBatch.from_synth([lead_lattice(k), big_lattice(ARCS[0]), tiny_lattices()[1], lead_lattice(k)], device=dev)
        for tw in (1, 0):
            with _lib.tuning(tw=tw):
                fb = ops.forward_backward(lat, th, want_me=True)
                bw = ops.backward(lat, th, want_me=True)
                assert torch.equal(bw.logbeta, fb.logbeta) and torch.equal(bw.logz64, fb.logz64)
                assert torch.equal(bw.beta_me.view(torch.int32), fb.beta_me.view(torch.int32))

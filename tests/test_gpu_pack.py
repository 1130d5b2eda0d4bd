"""The packer on the device against the host packer (``-m gpu``, through the C ABI): bit for bit.

``nfst_pack_device_plan`` / ``_emit`` and ``nfst_dense_to_arcs_count`` / ``_write`` (include/nfst_hip.h) must give
exactly the arrays of ``nfst_pack_arcs`` / ``nfst_pack_dense`` -- canonical arcs, row pointers, tile programs,
slot -> arc maps, meta records, header -- on the corpus of ``corpus()`` below (generated shapes, the shapes of the
BASELINE configs) and on the branch corpus of tests/pack_cases.py (one entry per launch branch of ``k_pack_lattice``:
what lives in LDS or in global memory, which counting method plans the tiles, unreachable states that own arcs, self
loops, batches without arcs), under every group mode, and refuse what the host packer refuses with the same error codes
and the same lattice index.  The host packer is the reference; what both packers could get wrong together is caught by
the float64 oracle on the arcs that state 0 reaches (tests/test_pack_cases_cpu.py holds the host packer to it as well)."""
import warnings

import numpy as np
import pytest
import torch

from nfst_amd import _lib, ops, synth
from nfst_amd.constraints import ConstraintDFA
from nfst_amd.lattice import LatticeBatch
from oracle import oracle as O
from tests import pack_cases as PC

pytestmark = pytest.mark.gpu

CASES = PC.cases()


def same(a: LatticeBatch, b: LatticeBatch, what=""):
    assert a._h == b._h, (what, a._h, b._h)
    assert np.array_equal(a.meta_host, b.meta_host), what
    for k in LatticeBatch._FIELDS:
        x, y = a._t[k], b._t[k]
        assert (x is None) == (y is None), (what, k)
        if x is not None:
            x, y = x.cpu(), y.cpu()
            if not torch.equal(x, y):
                bad = (x != y).nonzero().flatten()
                raise AssertionError(f"{what}: {k} differs at {bad.numel()} of {x.numel()} entries, first {int(bad[0])}: "
                                     f"{int(x[bad[0]])} vs {int(y[bad[0]])}")


def corpus():
    V = 256
    star_src = [0] + [1] * 200 + list(range(2, 202)) + [202]
    star_lab = [synth.BOS] + list(range(3, 203)) + [5] * 200 + [synth.EOS]
    star_dst = [1] + list(range(2, 202)) + [202] * 200 + [203]
    return {
        "small40": [synth.layered_lattice(3, n_states=30, avg_degree=3.0, vocab=40, width=4, span=2),
                    synth.edit_lattice([10, 11, 12, 13], [20, 21, 22], vocab=40, seed=2)],
        "mixed64": [synth.layered_lattice(4, n_states=200, avg_degree=8.0, vocab=64, width=9, span=5),
                    synth.layered_lattice(5, n_states=64, avg_degree=5.0, vocab=64, width=1, span=6),
                    synth.layered_lattice(7, n_states=120, avg_degree=6.0, vocab=64, width=6, span=4)],
        "weighted64": [synth.layered_lattice(6, n_states=150, avg_degree=6.0, vocab=64, width=7, span=3, weighted=True),
                       synth.layered_lattice(8, n_states=90, avg_degree=4.0, vocab=64, width=2, span=2, weighted=True)],
        "star200": [synth._finish(204, V, star_src, star_lab, star_dst)],  # fan-out and fan-in of 200: carry pieces, partial groups
        "trivial": [synth._finish(2, 8 + 3, [0], [synth.EOS], [1]), synth._finish(3, 8 + 3, [0, 1], [synth.BOS, synth.EOS], [1, 2])],
        "baseline": synth.bench_batch(6),
        "baseline_width4": synth.bench_batch(3, width=4),
        "snips": synth.snips_shaped_batch(5),
        "chains": [synth.layered_lattice(20 + i, n_states=n, avg_degree=2.0, vocab=24, width=1, span=1 + i % 2, max_degree=6, weighted=(i % 2 == 1)) for i, n in enumerate((4, 9, 17, 450))],
    }


@pytest.mark.parametrize("name", list(corpus()))
@pytest.mark.parametrize("group_mode", [0, 1, 2])
def test_device_packer_equals_host_packer(dev, name, group_mode):
    lats = corpus()[name]
    if name == "chains":  # (weighted and unweighted lattices do not share a batch)
        groups = [[l for l in lats if l.weight is None], [l for l in lats if l.weight is not None]]
    else:
        groups = [lats]
    for g in groups:
        n_rows, arc_off, src, label, dst, w = synth.batch_arcs(g)
        host = LatticeBatch.from_arcs(n_rows, arc_off, src, label, dst, g[0].vocab, arc_w=w, group_mode=group_mode)
        devb = LatticeBatch.from_arcs_device(n_rows, arc_off, src, label, dst, g[0].vocab, arc_w=w, device=dev, group_mode=group_mode)
        torch.cuda.synchronize()
        same(host, devb, f"{name} group_mode {group_mode}")
        devb.validate()
        # ... and the kernels run on it
        theta = torch.from_numpy(synth.label_scores(1, g[0].vocab))
        # (same kernels on both: a batch packed on the device has no chunked programs)
        a, b = ops.forward_backward(host.to(dev, auto_chunks=False), theta), ops.forward_backward(devb, theta)
        assert torch.equal(a.logz64, b.logz64) and torch.equal(a.posterior, b.posterior)


@pytest.mark.parametrize("pad", [0, 7])
@pytest.mark.parametrize("weighted", [False, True])
def test_dense_tables_on_the_device(dev, pad, weighted):
    """``set_masks`` with the collated tables already on the GPU (lightning.py:417): reachable rows -> arcs -> packed
    batch without a table leaving the device; pad-id padding rows (all-True rows, transition = pad) are ignored."""
    lats = [synth.layered_lattice(30 + i, n_states=40 + 50 * i, avg_degree=5.0, vocab=48, width=3 + i, span=3, weighted=weighted) for i in range(3)]
    lats.append(synth.edit_lattice([10, 11, 12], [20, 21, 22, 23], vocab=48, seed=3) if not weighted else
                synth.layered_lattice(39, n_states=25, avg_degree=3.0, vocab=48, width=2, span=2, weighted=True))
    em, tr = synth.collate_dense([l.dense(weighted=weighted) for l in lats], pad=pad)
    host = LatticeBatch.from_dense(em, tr)
    devb = LatticeBatch.from_dense(torch.from_numpy(em).to(dev), torch.from_numpy(tr).to(dev))
    torch.cuda.synchronize()
    assert devb.device.type == "cuda"
    same(host, devb, f"dense pad {pad} weighted {weighted}")


def test_device_packer_error_codes(dev):
    V = 8

    def arcs(src, lab, dst, n):
        return dict(n_rows=np.array([n], np.int32), arc_off=np.array([0, len(src)], np.int64), src=np.array(src, np.int32),
                    label=np.array(lab, np.int32), dst=np.array(dst, np.int32), vocab=V, device=dev)
    for bad, code in (((([0, 1, 2, 2], [1, 3, 3, 4], [1, 2, 1, 3], 4)), -3),   # 0 -> 1 -> 2 -> 1: cycle
                      ((([0, 0], [3, 4], [1, 2], 3)), -4),                      # two states without out arcs
                      ((([0, 0, 1], [3, 3, 2], [1, 1, 2], 3)), -5),             # same (state, label) twice
                      ((([0], [3], [5], 2)), -2),                               # state index out of range
                      ((([0], [3], [1], 9000)), -6)):                           # more rows than the engine takes
        with pytest.raises(_lib.NfstError) as e:
            LatticeBatch.from_arcs_device(**arcs(*bad))
        assert e.value.code == code, (bad, e.value.code)
        with pytest.raises(_lib.NfstError) as e2:
            LatticeBatch.from_arcs(**{k: v for k, v in arcs(*bad).items() if k != "device"})
        assert e2.value.code == code
    # a wide vocabulary is the host packer's: the device packer says so, from_dense falls back
    with pytest.raises(_lib.NfstError) as e:
        LatticeBatch.from_arcs_device(np.array([2], np.int32), np.array([0, 1], np.int64), np.array([0], np.int32), np.array([5], np.int32),
                                      np.array([1], np.int32), 3000, device=dev)
    assert e.value.code == -6


def test_baseline_batch_packed_on_the_device(dev):
    """BASELINE configs[1] (256 x ~2k states / ~20k arcs) from 12-byte arc lists: bit-identical to the host packer, and
    the step on it gives the same bits."""
    lats = synth.bench_batch(256)
    n_rows, arc_off, src, label, dst, w = synth.batch_arcs(lats)
    host = LatticeBatch.from_arcs(n_rows, arc_off, src, label, dst, 256)
    devb = LatticeBatch.from_arcs_device(n_rows, arc_off, src, label, dst, 256, device=dev)
    torch.cuda.synchronize()
    same(host, devb, "baseline 256")


# ---------------------------------------------------------------- the branch corpus of tests/pack_cases.py
def _oracle(l, theta):
    """the float64 oracle on the arcs that state 0 reaches (the breadth-first search of pack_cases.analyse)"""
    src, label, dst, w = PC.reachable_arcs(l)
    sc = theta[label].astype(np.float64) + (w.astype(np.float64) if w is not None else 0.0)
    return O.forward_backward(l.n_rows, src, dst, sc), w


def _pack_both(dev, lats, group_mode):
    n_rows, arc_off, src, label, dst, w = PC.batch_arcs(lats)
    host = LatticeBatch.from_arcs(n_rows, arc_off, src, label, dst, lats[0].vocab, arc_w=w, group_mode=group_mode)
    devb = LatticeBatch.from_arcs_device(n_rows, arc_off, src, label, dst, lats[0].vocab, arc_w=w, device=dev, group_mode=group_mode)
    torch.cuda.synchronize()
    return host, devb


BRANCH_PARAMS = [(name, gm) for name, c in CASES.items() if not c.branches & {"limit_pieces", "limit_rows"} for gm in c.group_modes]


@pytest.mark.parametrize("name,group_mode", BRANCH_PARAMS)
def test_device_packer_equals_host_packer_at_every_branch(dev, name, group_mode):
    """Bit for bit on every entry of the branch corpus; the same bits out of forward-backward on both batches; and log Z
    within 1e-8 of the float64 oracle on the arcs that state 0 reaches, which is what catches a mistake that both packers
    share.  The bound is the one of the float64-mantissa flavour of the sweeps (tests/test_gpu_chunks_device.py,
    tests/test_gpu_tile_wave_edges.py), so that comparison runs the beta sweep under ``precise=1``: its values fit LDS up
    to NFST_MAX_ROWS rows, and programs deeper than 192 tiles take that flavour anyway."""
    c = CASES[name]
    host, devb = _pack_both(dev, c.lats, group_mode)
    same(host, devb, f"{name} group_mode {group_mode}")
    devb.validate()
    theta_h = synth.label_scores(1, c.lats[0].vocab)
    theta = torch.from_numpy(theta_h)
    a, b = ops.forward_backward(host.to(dev, auto_chunks=False), theta), ops.forward_backward(devb, theta)
    assert torch.equal(a.logz64, b.logz64) and torch.equal(a.posterior, b.posterior)
    with _lib.tuning(precise=1):
        z = ops.backward(devb, theta).logz64.cpu().numpy()
        fb = ops.forward_backward(devb, theta) if "junk_weighted" in c.branches else None
    worst = 0.0
    for i, l in enumerate(c.lats):
        o, w = _oracle(l, theta_h)
        err = abs(float(z[i]) - o["logZ"])
        worst = max(worst, err)
        assert err <= 1e-8, (name, group_mode, i, float(z[i]), o["logZ"])
        if fb is not None:  # the weighted entry with junk: the weights follow the compaction, and the weighted sweeps agree
            a0, n = int(devb.arc_off[i]), int(devb.n_arcs[i])
            assert np.array_equal(devb.arc_w.cpu().numpy()[a0:a0 + n], w)
            assert abs(float(fb.logz64[i]) - o["logZ"]) <= 1e-8
            assert np.max(np.abs(fb.posterior.cpu().numpy()[a0:a0 + n] - o["posterior"])) <= 2e-6  # (the posteriors' bound of that flavour)
    print(f"{name} group_mode {group_mode}: worst |logz64 - oracle| = {worst:.3e}")


def _raw(lats):
    n_rows, arc_off, src, label, dst = PC.raw_batch(lats)
    return dict(n_rows=n_rows, arc_off=arc_off, src=src, label=label, dst=dst, vocab=PC.ERROR_VOCAB)


def test_device_packer_error_matrix(dev):
    """Every row of pack_cases.error_rows: the same code and the same lattice index from both packers (the first
    offending arc of the first bad lattice decides; SINK before CYCLE), and after every refusal a good batch packs on the
    same device as if nothing had happened."""
    good = CASES["no_arcs_mid_batch"].lats
    for name, lats, code, bad in PC.error_rows():
        kw = _raw(lats)
        if code is None:
            host, devb = LatticeBatch.from_arcs(**kw), LatticeBatch.from_arcs_device(device=dev, **kw)
            torch.cuda.synchronize()
            same(host, devb, name)
            devb.validate()
            continue
        with pytest.raises(_lib.NfstError) as e:
            LatticeBatch.from_arcs(**kw)
        assert (e.value.code, e.value.lattice) == (code, bad), (name, "host", e.value.code, e.value.lattice)
        with pytest.raises(_lib.NfstError) as e:
            LatticeBatch.from_arcs_device(device=dev, **kw)
        assert (e.value.code, e.value.lattice) == (code, bad), (name, "device", e.value.code, e.value.lattice)
        host, devb = _pack_both(dev, good, 0)
        same(host, devb, f"a good batch after: {name}")


@pytest.mark.parametrize("name", ["limit_pieces", "limit_rows"])
def test_beyond_the_device_packer_every_route_lands_on_the_host_packer(dev, name):
    """More pieces than sort keys fit LDS, and scratch rows beyond NFST_MAX_ROWS: the kernel itself refuses (-6).  The host
    packer takes both shapes (it has no key limit, and sums the state as a chain where a tree's scratch rows would not
    fit), so its batch is the reference, and the three routes that catch the refusal -- from_dense on GPU tables, restrict
    and intersect on a GPU batch -- must hand out exactly that batch."""
    c = CASES[name]
    l, gm = c.lats[0], c.group_modes[0]
    n_rows, arc_off, src, label, dst, w = PC.batch_arcs(c.lats)
    with pytest.raises(_lib.NfstError) as e:
        LatticeBatch.from_arcs_device(n_rows, arc_off, src, label, dst, l.vocab, device=dev, group_mode=gm)
    assert (e.value.code, e.value.lattice) == (PC.ERR_LIMIT, 0)
    host = LatticeBatch.from_arcs(n_rows, arc_off, src, label, dst, l.vocab, group_mode=gm)
    host.validate()
    em, tr = l.dense()
    em_d, tr_d = torch.from_numpy(em[None]).to(dev), torch.from_numpy(tr[None]).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the copy of the tables to the host is announced once per process)
        dense = LatticeBatch.from_dense(em_d, tr_d, group_mode=gm)
    assert dense.device.type == "cuda"
    same(host, dense, f"{name}: from_dense on GPU tables")
    on_gpu = host.to(dev, auto_chunks=False)
    with pytest.warns(UserWarning, match="restrict packs this batch on the host"):
        sub, arc_map = on_gpu.restrict(torch.ones(host.total_arcs, dtype=torch.bool, device=dev), group_mode=gm)
    assert sub.device.type == "cuda" and torch.equal(arc_map.cpu(), torch.arange(host.total_arcs))
    same(host, sub, f"{name}: restrict")
    with pytest.warns(UserWarning, match="intersect packs this batch on the host"):
        prod = on_gpu.intersect(ConstraintDFA.accept_all(l.vocab), group_mode=gm)
    assert torch.equal(prod.arc_map.cpu(), torch.arange(host.total_arcs))  # (every state with q = 0: the product is the lattice)
    same(host, prod.lattice, f"{name}: intersect")


# ---------------------------------------------------------------- the dense front end
def _dense_lattice(V, weighted):
    """0 -bos-> 1, 1 fans out to twenty states (a frontier wider than the sixteen waves of k_dense_reach), those join in
    22, 22 -> 23 over every label from 3 to V - 1 (the last, partial 64-lane step of k_dense_write), 23 -eos-> 24"""
    arcs = [(0, PC.BOS, 1)] + [(1, 3 + i, 2 + i) for i in range(20)] + [(2 + i, 3 + i % 5, 22) for i in range(20)]
    arcs += [(2 + i, V - 1 - i % 3, 22) for i in range(0, 20, 2)] + [(22, l, 23) for l in range(3, V)] + [(23, PC.EOS, 24), (24, PC.PAD, 24)]
    return PC.make(25, V, arcs, weight_seed=7 if weighted else None)


def _pad_tables(tables, R, pad):
    em0, tr0 = tables[0]
    em = np.full((len(tables), R) + em0.shape[1:], pad if em0.dtype != np.float32 else (0.0 if pad else -np.inf), dtype=em0.dtype)
    tr = np.full((len(tables), R) + tr0.shape[1:], pad, dtype=np.int64)
    for i, (e, t) in enumerate(tables):
        em[i, :e.shape[0]], tr[i, :t.shape[0]] = e, t
    return em, tr


def _dense_both(dev, em, tr, what):
    host = LatticeBatch.from_dense(em, tr)
    devb = LatticeBatch.from_dense(torch.from_numpy(em).to(dev), torch.from_numpy(tr).to(dev))
    torch.cuda.synchronize()
    assert devb.device.type == "cuda"
    same(host, devb, what)
    return host


@pytest.mark.parametrize("R", [40, 8192])
@pytest.mark.parametrize("V", [64, 65, 130, 250])
@pytest.mark.parametrize("weighted", [False, True])
def test_dense_tables_of_every_width_and_height(dev, V, R, weighted):
    """V across the 64-lane steps of the ballot loop; R = 8192 is the whole 96 KiB of LDS of k_dense_reach.  The padding
    rows claim arcs everywhere, to a pad id beyond R: no reachable row leads there, so they are ignored."""
    tables = [_dense_lattice(V, weighted).dense(weighted=weighted), CASES["junk_low_ids"].lats[0].dense(weighted=weighted)]
    tables[1] = tuple(np.pad(t, ((0, 0), (0, V - t.shape[1])), constant_values=(-np.inf if t.dtype == np.float32 else 0)) for t in tables[1])
    em, tr = _pad_tables(tables, R, R + 5)
    host = _dense_both(dev, em, tr, f"dense V {V} R {R} weighted {weighted}")
    assert host.n_rows[0] == R and int(host.n_arcs[0]) == _dense_lattice(V, weighted).n_arcs


def test_dense_tables_of_one_row(dev):
    """R = 1: state 0 is the sink, with or without its pad self loop"""
    for weighted in (False, True):
        em = np.zeros((3, 1, 70), dtype=np.bool_)
        em[1, 0, PC.PAD] = em[2, 0, 69] = True
        tr = np.zeros((3, 1, 70), dtype=np.int64)
        if weighted:
            em = np.where(em, np.float32(-0.25), np.float32(-np.inf)).astype(np.float32)
        host = _dense_both(dev, em, tr, f"one row weighted {weighted}")
        assert host.total_arcs == 2 and host.total_dp_arcs == 0


def test_dense_tables_given_as_bytes_and_with_special_floats(dev):
    V = 70
    l = _dense_lattice(V, True)
    # bool tables given as uint8 with values other than 1
    em, tr = _pad_tables([l.dense()], 40, 0)
    em8 = em.astype(np.uint8) * np.uint8(5)
    em8[em8 > 0] += (np.arange(int((em8 > 0).sum())) % 250).astype(np.uint8)
    assert em8.max() > 1 and np.array_equal(em8 != 0, em)
    ref = LatticeBatch.from_dense(em, tr)
    devb = LatticeBatch.from_dense(torch.from_numpy(em8).to(dev), torch.from_numpy(tr).to(dev))
    same(ref, devb, "uint8 tables")
    same(ref, LatticeBatch.from_dense(em8, tr), "uint8 tables on the host")
    # float tables with +inf and NaN in reachable rows: "has an arc" is `> -inf` on both sides, so +inf is an arc
    # and NaN is none (its transition, out of range here, is never read)
    em, tr = _pad_tables([l.dense(weighted=True)], 40, 0)
    assert not em[0, 22, 0] > -np.inf and not em[0, 1, 40] > -np.inf
    em[0, 22, 0], tr[0, 22, 0] = np.nan, 4000
    em[0, 1, 40], tr[0, 1, 40] = np.nan, -3
    em[0, 22, 5] = np.inf
    em[0, 23, 1], tr[0, 23, 1] = np.inf, 24
    with np.errstate(invalid="ignore"):
        n_cells = int((em[0, :25] > -np.inf).sum())
    host = _dense_both(dev, em, tr, "float tables with inf and nan")
    assert host.total_arcs == n_cells == l.n_arcs + 1
    assert int(torch.isinf(host.arc_w).sum()) == 2 and not bool(torch.isnan(host.arc_w).any())


def test_dense_destinations_out_of_range(dev):
    """in an unreachable row: ignored; in a reachable row of lattice 1 of 3: NFST_ERR_INDEX naming lattice 1, from both"""
    V = 65
    for weighted in (False, True):
        l = _dense_lattice(V, weighted)
        em, tr = _pad_tables([l.dense(weighted=weighted)] * 3, 40, 0)
        em[:, 30, 64] = 0.5 if weighted else True  # row 30 is a padding row: nothing reaches it
        tr[:, 30, 64] = 40
        tr[2, 31, 3] = -1                          # (no arc in that cell at all)
        _dense_both(dev, em, tr, "out of range in unreachable rows")
        for bad in (40, -1, 1 << 33):
            tr2 = tr.copy()
            tr2[1, 22, 64] = bad                   # row 22 is reachable, label 64 is an arc of it
            with pytest.raises(_lib.NfstError) as e:
                LatticeBatch.from_dense(em, tr2)
            assert (e.value.code, e.value.lattice) == (PC.ERR_INDEX, 1)
            with pytest.raises(_lib.NfstError) as e:
                LatticeBatch.from_dense(torch.from_numpy(em).to(dev), torch.from_numpy(tr2).to(dev))
            assert (e.value.code, e.value.lattice) == (PC.ERR_INDEX, 1), bad
        _dense_both(dev, em, tr, "a good batch after the refusals")


def test_dense_tables_of_the_junk_entries(dev):
    """rows that nothing reaches but that own arcs -- among themselves, in cycles, into reachable rows -- never become arcs"""
    names = [n for n, c in CASES.items() if "junk_arcs" in c.branches and c.small]
    plain = [CASES[n].lats[0] for n in names if CASES[n].lats[0].weight is None]
    em, tr = _pad_tables([l.dense() for l in plain], 9, 0)
    host = _dense_both(dev, em, tr, "junk entries")
    for b, l in enumerate(plain):
        assert int(host.n_arcs[b]) == PC.analyse(l)["n_arcs"] < l.n_arcs
    wl = CASES["junk_weighted"].lats[0]
    em, tr = _pad_tables([wl.dense(weighted=True)], 12, 0)
    host = _dense_both(dev, em, tr, "the weighted junk entry")
    assert np.array_equal(host.arc_w.numpy(), PC.reachable_arcs(wl)[3])

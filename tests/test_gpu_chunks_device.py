"""Chunked programs cut on the device for batches packed on the device (``from_arcs_device(..., chunks=...)``,
``nfst_pack_chunks_device_*``, chunk_pack_kernels.h): bit-identical to the host cutter (``nfst_pack_chunks``) on the same
batch, and the reference's call path -- ``set_masks`` on dense tables that live on the GPU -- through the chunked sweeps
(``-m gpu``)."""
import numpy as np
import pytest
import torch

from nfst_amd import _lib, ops, synth
from nfst_amd.lattice import ChunkProgram, LatticeBatch
from nfst_amd.scorers import LatticeScorer
from oracle import oracle as O
from tests import pack_cases as PC

pytestmark = pytest.mark.gpu


def _cut_both_ways(dev, lats, chunks, **opts):
    """(device batch cut on the device, programs the host cutter makes from a host copy of the same batch)"""
    n_rows, arc_off, src, label, dst, w = synth.batch_arcs(lats)
    lat = LatticeBatch.from_arcs_device(n_rows, arc_off, src, label, dst, lats[0].vocab, arc_w=w, device=dev, chunks=chunks,
                                        chunk_opts=opts or None)
    ref = ChunkProgram.build(lat.to("cpu", auto_chunks=False), force=chunks == "force", **opts)
    return lat, ref


def _assert_identical(lat, ref):
    assert lat._chunks_tried
    if ref is None:
        assert lat.chunks is None
        return
    ck = lat.chunks
    assert ck is not None
    assert np.array_equal(ck.meta_host, ref.meta_host), (ck.meta_host[:2], ref.meta_host[:2])
    assert ck._h == ref._h
    for k in ChunkProgram._FIELDS:
        got, want = ck._t[k].cpu().numpy(), ref._t[k].numpy()
        assert got.dtype == want.dtype and got.shape == want.shape, (k, got.shape, want.shape)
        diff = np.flatnonzero(got != want)
        assert diff.size == 0, (k, diff.size, int(diff[0]), got[diff[:4]], want[diff[:4]])
    assert ck.ws is not None and ck.ws.device == lat.device and not bool(ck.ws.any())


@pytest.mark.parametrize("chunks", [True, "force"])
@pytest.mark.parametrize("n", [1, 8, 16, 64])
def test_snips_shaped_batches_cut_as_the_host_cuts_them(dev, n, chunks):
    lat, ref = _cut_both_ways(dev, synth.snips_shaped_batch(n), chunks)
    assert (ref is not None) == (n > 1 or chunks == "force")  # (the cost model: one lattice alone is not worth the fixed costs)
    _assert_identical(lat, ref)


@pytest.mark.parametrize("chunks", [True, "force"])
def test_one_deep_narrow_machine(dev, chunks):
    """bench.py's decode_b1_deep_narrow: two states per position, 750 levels"""
    lats = [synth.layered_lattice(4242, n_states=1500, avg_degree=3.0, vocab=250, width=2, span=1, max_degree=40)]
    lat, ref = _cut_both_ways(dev, lats, chunks)
    assert ref is not None
    _assert_identical(lat, ref)


@pytest.mark.parametrize("chunks", [True, "force"])
def test_more_lattices_than_cus(dev, chunks):
    """2 B > 256 workgroups: 512 threads and 64 KiB of LDS per program"""
    rng = np.random.default_rng(77)
    lats = [synth.layered_lattice(7000 + i, n_states=int(rng.integers(30, 160)), avg_degree=3.0, vocab=48, width=int(rng.choice([1, 2, 3])),
                                  span=int(rng.choice([1, 2])), max_degree=8) for i in range(160)]
    lat, ref = _cut_both_ways(dev, lats, chunks)
    if chunks == "force":
        assert ref is not None and ref._h["threads"] == 512
    _assert_identical(lat, ref)


@pytest.mark.parametrize("seed", list(range(12)))
def test_random_cuts_as_the_host_makes_them(dev, seed):
    """the generators and options of test_chunks_cpu.test_random_cuts_replayed_on_the_host"""
    rng = np.random.default_rng(4000 + seed)
    V = int(rng.choice([24, 64]))
    lats = []
    while len(lats) < int(rng.integers(1, 6)):
        try:
            lats.append(synth.layered_lattice(int(rng.integers(1, 1 << 30)), n_states=int(rng.choice([4, 9, 30, 80, 200])),
                                              avg_degree=float(rng.choice([1.5, 3.0, 5.0])), vocab=V, width=int(rng.choice([1, 2, 3, 5, 8])),
                                              span=int(rng.choice([1, 2, 3])), max_degree=min(10, (V - 12) // 2)))
        except AssertionError:
            continue
    opts = dict(threads=int(rng.choice([64, 128, 512, 1024])), max_chunks=int(rng.choice([0, 0, 1, 2, 5])), lds_bytes=int(rng.choice([0, 8192, 32768])))
    for chunks in ("force", True):
        lat, ref = _cut_both_ways(dev, lats, chunks, **opts)
        _assert_identical(lat, ref)


def test_batches_that_are_not_cut(dev):
    """the BASELINE shape (no, not even forced: its arcs reach too far back) and levels of 48 states (reach > 63)"""
    for chunks in (True, "force"):
        lat, ref = _cut_both_ways(dev, synth.bench_batch(4), chunks)
        assert ref is None
        _assert_identical(lat, ref)
    wide = [synth.layered_lattice(5, n_states=300, avg_degree=6.0, vocab=64, width=48, span=1, max_degree=24)]
    lat, ref = _cut_both_ways(dev, wide, "force")
    assert ref is None
    _assert_identical(lat, ref)


_PC = PC.cases()


@pytest.mark.parametrize("name", [n for n, c in _PC.items() if c.small and c.branches & {"junk_arcs", "inner_self_loops"}] + ["count_falls_back"])
def test_branch_corpus_cut_as_the_host_cuts_it(dev, name):
    """The cutter reads the packer's workspace (depths, heights, arc lists by canonical id).  The entries of
    tests/pack_cases.py whose workspace differs from the input: unreachable states that own arcs (canonical ids shift,
    depths of -1 between depths that count), self loops (arcs that are in no list), and the deep, narrow chain whose
    planning pass counted its tiles by laying them out, which leaves other scans in the workspace than the counting
    tables do."""
    lat, ref = _cut_both_ways(dev, _PC[name].lats, "force")
    assert ref is not None
    _assert_identical(lat, ref)


def test_defaults_and_bad_options(dev):
    lats = synth.snips_shaped_batch(4, vocab=64, first_seed=5200)
    n_rows, arc_off, src, label, dst, _ = synth.batch_arcs(lats)
    assert LatticeBatch.from_arcs_device(n_rows, arc_off, src, label, dst, 64, device=dev).chunks is None
    em, tr = synth.collate_dense([l.dense() for l in lats])
    em_d, tr_d = torch.from_numpy(em).to(dev), torch.from_numpy(tr).to(dev)
    assert LatticeBatch.from_dense(em_d, tr_d).chunks is None
    assert LatticeScorer(64).to(dev).set_masks(em_d, tr_d).lattice.chunks is None
    with pytest.raises(_lib.NfstError):
        LatticeBatch.from_arcs_device(n_rows, arc_off, src, label, dst, 64, device=dev, chunks=True, chunk_opts=dict(threads=100))
    with pytest.raises(ValueError):
        LatticeBatch.from_arcs_device(n_rows, arc_off, src, label, dst, 64, device=dev, chunks="always")


@pytest.mark.parametrize("n", [8, 64])
def test_set_masks_on_gpu_tables_runs_the_chunked_sweeps(dev, n):
    """the reference's trainer: collated dense tables moved to the GPU, then set_masks (lightning.py:417)"""
    V = 250
    lats = synth.snips_shaped_batch(n, vocab=V)
    em, tr = synth.collate_dense([l.dense() for l in lats])
    em_d, tr_d = torch.from_numpy(em).to(dev), torch.from_numpy(tr).to(dev)
    theta0 = synth.label_scores(64, V, mean=-1.5, std=0.8)
    model = LatticeScorer(V, theta=theta0, chunks=True).to(dev)
    model.set_masks(em_d, tr_d)
    lat = model.lattice
    assert lat.chunks is not None
    r = ops.forward_backward(lat, model.theta.detach())
    assert not lat.chunks.flagged().any()
    for b, l in enumerate(lats):
        o = O.forward_backward(l.n_rows, l.src, l.dst, theta0[l.label].astype(np.float64))
        assert abs(float(r.logz64[b]) - o["logZ"]) <= 1e-8, b
    model.log_z().sum().backward()
    general = LatticeScorer(V, theta=theta0).to(dev)
    general.set_masks(em_d, tr_d)
    assert general.lattice.chunks is None
    general.log_z().sum().backward()
    g, want = model.theta.grad, general.theta.grad
    assert torch.max(torch.abs(g - want)).item() <= 2e-6 * max(1.0, float(want.abs().max()))

"""Host-side parts of cutting chunked programs for batches packed on the device: the layout step the device cutter shares
with nfst_pack_chunks (``nfst_pack_chunks_device_layout``) and the ``chunks`` keyword of the constructors and of
``LatticeScorer`` on host tables.  The device cutter itself: tests/test_gpu_chunks_device.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from nfst_amd import _lib, synth
from nfst_amd._lib import lib
from nfst_amd.lattice import ChunkProgram, LatticeBatch
from nfst_amd.scorers import LatticeScorer


def _summaries(ref: ChunkProgram, cycles: float) -> np.ndarray:
    """what the device's planning pass reads back for the programs of ``ref``"""
    m = ref.meta_host.reshape(-1, _lib.CHK_META_WORDS)
    tab = ref._t["tab"].numpy().reshape(-1, 4)
    out = np.zeros((m.shape[0], _lib.CHK_SUM_WORDS), dtype=np.int32)
    for i, cm in enumerate(m):
        last = tab[cm[_lib.CHK_TAB_OFF] + cm[_lib.CHK_C] - 1]
        out[i, :6] = (1, cm[_lib.CHK_C], cm[_lib.CHK_F], cm[_lib.CHK_R], cm[_lib.CHK_NPOS], last[1] + last[2])
        out[i, 6:8] = np.array([cycles], dtype=np.float64).view(np.int32)
    return out


def _layout(lat: LatticeBatch, summary: np.ndarray, force: bool, **opts):
    co = _lib.ChunkOpts(int(opts.get("threads", 0)), int(opts.get("lds_bytes", 0)), 1 if force else 0, int(opts.get("max_chunks", 0)), 0, 0)
    meta = np.zeros(lat.n_lattices * 2 * _lib.CHK_META_WORDS, dtype=np.int32)
    v, cut = _lib.Chunks(), C.c_int32(-1)
    summary = np.ascontiguousarray(summary)
    _lib.check(lib.nfst_pack_chunks_device_layout(summary.ctypes.data, lat.meta_host.ctypes.data, C.byref(lat.c_struct()), C.byref(co),
                                                  meta.ctypes.data, C.byref(v), C.byref(cut)), "nfst_pack_chunks_device_layout")
    return cut.value, meta, v


@pytest.mark.parametrize("opts", [dict(), dict(threads=256, max_chunks=3)])
def test_layout_step_is_the_host_cutters(opts):
    lat = LatticeBatch.from_synth(synth.snips_shaped_batch(12))
    ref = ChunkProgram.build(lat, force=True, **opts)
    assert ref is not None
    cut, meta, v = _layout(lat, _summaries(ref, 0.0), True, **opts)
    assert cut == 1
    assert np.array_equal(meta.reshape(ref.meta_host.shape), ref.meta_host)
    assert {k: int(getattr(v, k)) for k in ChunkProgram._HEADER} == ref._h
    # the choice of the flavour: modelled cycles far beyond the general kernels' -> no programs unless forced
    assert _layout(lat, _summaries(ref, 1e12), False, **opts)[0] == 0
    assert _layout(lat, _summaries(ref, 1e12), True, **opts)[0] == 1
    # one program that could not be cut: none for the batch
    s = _summaries(ref, 0.0)
    s[3, 0] = 0
    assert _layout(lat, s, True, **opts)[0] == 0
    with pytest.raises(_lib.NfstError):
        _layout(lat, _summaries(ref, 0.0), True, threads=100)


def test_layout_step_declines_what_the_host_cutter_declines_without_looking():
    lat = LatticeBatch.from_synth(synth.bench_batch(2))
    assert lat.max_tiles <= 160
    summary = np.zeros((4, _lib.CHK_SUM_WORDS), dtype=np.int32)
    assert _layout(lat, summary, False)[0] == 0


def test_chunks_keyword_on_host_tables():
    """tables on the host: the host cutter, before the batch moves; the same programs as build_chunks"""
    lats = synth.snips_shaped_batch(6, vocab=64, first_seed=5200)
    em, tr = synth.collate_dense([l.dense() for l in lats])
    plain = LatticeBatch.from_dense(em, tr)
    assert plain.chunks is None
    lat = LatticeBatch.from_dense(em, tr, chunks="force", chunk_opts=dict(threads=256))
    ref = ChunkProgram.build(plain, force=True, threads=256)
    assert lat.chunks is not None and lat.chunks._h == ref._h
    for k in ChunkProgram._FIELDS:
        assert torch.equal(lat.chunks._t[k], ref._t[k]), k
    model = LatticeScorer(64, chunks="force").set_masks(torch.from_numpy(em), torch.from_numpy(tr))
    assert model.lattice.chunks is not None and model.lattice.chunks._h == ChunkProgram.build(plain, force=True)._h
    assert LatticeScorer(64).set_masks(torch.from_numpy(em), torch.from_numpy(tr)).lattice.chunks is None
    with pytest.raises(ValueError):
        LatticeBatch.from_dense(em, tr, chunks="yes")

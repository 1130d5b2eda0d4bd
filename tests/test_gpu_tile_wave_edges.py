"""Both flavours of the tile-wave sweep loop (``tile_sweep2``, float32 and float64 mantissas) at the loop's edges (``-m gpu``).

The loop takes four tiles per trip and walks a ring of at most ``kMaxRing`` = 12 decoded tiles.  Its edges are programs
shorter than one trip (1, 2, 3 tiles), every length of the tail behind whole trips, and the ring's first wrap.  The
float64 flavour otherwise runs only on programs deeper than 192 tiles, so here it is forced (``precise=1``) on chains of
1 .. 20 levels, beside the float32 flavour (``precise=0, tw=1``), both against the float64 oracle.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from nfst_amd import ops, synth, _lib
from nfst_amd.lattice import LatticeBatch

pytestmark = pytest.mark.gpu
V = 24
K_MAX_RING = 12  # kMaxRing of csrc/tile_pipeline.h: longer programs wrap the ring
# the bounds the suite holds the two flavours to: test_deep_chain_case_of_round_2 (float64 mantissas) and the fuzz test (float32)
TOL = {"precise": dict(logz=1e-8, post=2e-6), "float32": dict(logz=1e-5, post=1e-5)}
FLAVOURS = {"precise": dict(precise=1), "float32": dict(precise=0, tw=1)}
# levels per chain: at most 8 lattices per batch; a chain of n states is a program of n tiles in either direction
BATCHES = [[1, 2, 3, 4, 5, 6, 7], [8, 9, 10, 11, 12, 13, 14, 15], [16, 17, 18, 19, 20, 3, 12, 13]]
EXTRAS = ["none", "weights", "weights+scores"]


def _tiny_chain(n_states, weighted, seed):
    """Chains below the four states ``synth.layered_lattice`` starts at: 0 --bos--> 1 ==(two parallel arcs)==> 2 --eos--> sink."""
    src, lab, dst = [], [], []
    for s in range(n_states - 1):
        for l in ([synth.BOS] if s == 0 else [synth.N_SPECIAL + s, synth.N_SPECIAL + 7 + s]):
            src.append(s), lab.append(l), dst.append(s + 1)
    src.append(n_states - 1), lab.append(synth.EOS), dst.append(n_states)
    w = np.random.default_rng(seed).normal(-0.5, 0.25, size=len(src)).astype(np.float32) if weighted else None
    return synth._finish(n_states + 1, V, src, lab, dst, w)


def _chain(n_states, weighted, seed):
    if n_states < 4:
        return _tiny_chain(n_states, weighted, seed)
    return synth.layered_lattice(seed, n_states=n_states, avg_degree=2.5, vocab=V, width=1, span=1 + seed % 2, max_degree=6,
                                 weighted=weighted)


@pytest.fixture(scope="module")
def cases(dev):
    """Per (batch, extras): the lattices, scores and oracle results, computed once; per group mode the packed batch."""
    out = {}
    for bi, levels in enumerate(BATCHES):
        for ex in EXTRAS:
            lats = [_chain(n, ex != "none", 100 * bi + i) for i, n in enumerate(levels)]
            theta = synth.label_scores(7 + bi, V, mean=-1.0, std=1.0)
            packed = {gm: LatticeBatch.from_synth(lats, device=dev, group_mode=gm) for gm in (0, 2)}
            lat = packed[0]
            asc = None
            if ex == "weights+scores":
                asc = np.random.default_rng(50 + bi).normal(0.0, 0.5, size=lat.total_arcs).astype(np.float32)
            ref = []
            for b, l in enumerate(lats):
                a0 = int(lat.arc_off[b])
                sc = theta[l.label].astype(np.float64)
                if l.weight is not None:
                    sc = sc + l.weight
                if asc is not None:
                    sc = sc + asc[a0:a0 + l.n_arcs]
                ref.append(O.forward_backward(l.n_rows, l.src, l.dst, sc))
            out[bi, ex] = dict(lats=lats, theta=theta, asc=asc, packed=packed, ref=ref)
    return out


def test_tile_counts_cover_the_loops_edges(cases):
    """Short programs (1, 2, 3 tiles), every tail length behind whole trips without and with a ring wrap."""
    counts = set()
    for c in cases.values():
        for lat in c["packed"].values():
            m = lat.meta_host
            counts |= set(int(x) for x in m[:, _lib.META_FWD_TILES]) | set(int(x) for x in m[:, _lib.META_BWD_TILES])
    assert {1, 2, 3} <= counts, sorted(counts)
    assert {n % 4 for n in counts if 4 <= n <= K_MAX_RING} == {0, 1, 2, 3}, sorted(counts)
    assert {n % 4 for n in counts if n > K_MAX_RING} == {0, 1, 2, 3}, sorted(counts)


@pytest.mark.parametrize("gm", [0, 2])  # (2: wide groups -- the exact path of tile_math3p; float32 takes tile_sweep)
@pytest.mark.parametrize("ex", EXTRAS)
@pytest.mark.parametrize("bi", range(len(BATCHES)))
def test_both_flavours_against_oracle(cases, bi, ex, gm):
    c = cases[bi, ex]
    lat, lats = c["packed"][gm], c["lats"]
    th = torch.from_numpy(c["theta"])
    t = None if c["asc"] is None else torch.from_numpy(c["asc"])
    z_full = {}
    for name, switches in FLAVOURS.items():
        with _lib.tuning(**switches):
            f, bw = ops.forward_backward(lat, th, arc_scores=t), ops.backward(lat, th, arc_scores=t)
            torch.cuda.synchronize()
        z, zb, post = f.logz64.cpu().numpy(), bw.logz64.cpu().numpy(), f.posterior.cpu().numpy()
        z_full[name] = z
        tol = TOL[name]
        for b, l in enumerate(lats):
            o, a0, where = c["ref"][b], int(lat.arc_off[b]), (name, BATCHES[bi][b])
            assert abs(z[b] - o["logZ"]) <= tol["logz"], where
            assert abs(zb[b] - o["logZ"]) <= tol["logz"], where
            assert abs(zb[b] - z[b]) <= tol["logz"], where
            assert np.max(np.abs(post[a0:a0 + l.n_arcs] - o["posterior"])) <= tol["post"], where
    assert np.max(np.abs(z_full["precise"] - z_full["float32"])) <= 1e-4

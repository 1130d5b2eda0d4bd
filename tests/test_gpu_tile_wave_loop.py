"""The tile waves' loop (``WeightWave<.., FULL>::run_tiles``, csrc/tile_pipeline.h) where cursors can go wrong (``-m gpu``).

A tile wave decodes every fourth tile of its sweep's program, three tiles per trip, into a ring of R slots; its tile number,
its ring slot and its place in the program are cursors, and without per-arc extras the last one to five tiles of a wave are
straight-line code behind the trip.  So the cases are programs of 1 .. 21 tiles (chains of 1 .. 21 states): R + 9 for the
deepest ring, kMaxRing = 12 -- tile waves without a tile (1 - 3 tiles), with 1 .. 6 tiles (every length of the tail, the
first whole trip), the first and the second wrap of the slot cursor for R = 4, 8 and 12 -- and one batch that mixes a
1-tile program with the longest.  Every ring depth the launcher can choose for such lattices is run: 12 by itself; 8 and 4
only when LDS is held back (``NFST_LDS_RESERVE_KB``, read once per process), so those run in a child process per value
(``python tests/test_gpu_tile_wave_loop.py``, which prints what the in-process test asserts on).  ``ops.backward`` and
``ops.viterbi`` keep 12 slots under every reserve.

Per program length: forward_backward float32 with and without ``grad_theta`` (label weights preloaded by the helper waves
or not), ``precise=1``, caller ``arc_scores`` (one array of extras) and table weights + ``arc_scores`` (two) -- staged in
LDS where at least eight slots fit beside them, gathered from memory otherwise and under ``precise=1`` --, ``ops.backward``
and ``ops.viterbi``.  References: the float64 oracle at the bounds of tests/test_gpu_tile_wave_edges.py (log Z 1e-5 /
posteriors 1e-5, precise 1e-8 / 2e-6), and for float32 forward_backward the loader + decoder + sweep pipeline
(``_lib.tuning(tw=0)``) bit for bit on logz64, logalpha, logbeta, beta_me and posterior, but for that pair's known exponent
word of exact zeros in ``beta_me`` (tests/test_gpu_sweep_slots.py).  Viterbi: the best score within the rounding of a
float32 sum of the path's terms (terms x 2^-23 x sum |term|) of the oracle's, and the path's own score equal to it.
The largest error of every check goes to tile_wave_loop_errors.json in the directory of run outputs (profiles/README.md).
"""
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import pytest
import torch

from oracle import oracle as O
from nfst_amd import ops, synth, _lib
from nfst_amd.lattice import LatticeBatch

pytestmark = pytest.mark.gpu
V = 24
K_MAX_RING = 12
LENGTHS = list(range(1, K_MAX_RING + 10))  # 1 .. R + 9 tiles
BATCHES = [LENGTHS[0:7], LENGTHS[7:14], LENGTHS[14:21], [1, LENGTHS[-1], 2, 5]]  # (the last: idle and busy tile waves in one launch)
EXTRAS = ["none", "scores", "weights+scores"]
TOL = {"precise": dict(logz=1e-8, post=2e-6), "float32": dict(logz=1e-5, post=1e-5)}
FIELDS = ("logz64", "logalpha", "logbeta", "beta_me", "posterior")
# NFST_LDS_RESERVE_KB -> ring slots per sweep of forward_backward (float32, precise) for lattices of a few dozen states
DEPTHS = {0: (12, 12), 48: (12, 8), 80: (8, 4), 96: (4, 4)}


def _constants():
    csrc = os.path.join(ROOT, "nfst_amd", "csrc")
    text = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "tile_pipeline.h")).read() + open(os.path.join(csrc, "kernels.hip")).read())
    env = {}
    for name in ("kSlotWords2", "kSlotWordsP", "kMaxRing", "kSweepFlags", "kMaxLds"):
        m = re.search(r"\b" + name + r"\s*=\s*([^,;]+)[,;]", text)
        assert m, name
        env[name] = int(eval(m.group(1), {"__builtins__": {}}, dict(env)))
    return env


def ring_depths(rows, vocab, reserve_kb, staged_arcs=0):
    """plan_forward_backward's ring slots per sweep (csrc/kernels.hip: ring_slots, LdsPlan): float32, precise, and float32
    beside `staged_arcs` staged extras (0: not staged -- fewer than eight slots would be left)."""
    c = _constants()
    rows2, v2, v4 = (rows + 1) & ~1, (vocab + 3) & ~1, (vocab + 3) & ~3
    slots = lambda fixed, slot: min((c["kMaxLds"] - reserve_kb * 1024 - fixed) // slot, c["kMaxRing"]) & ~3
    fixed = (2 * rows2 + v2) * 8 + v4 * 4 + 2 * c["kSweepFlags"] * 4 + 1024
    r32 = slots(fixed, c["kSlotWords2"] * 8)
    rp = slots((2 * rows2 + v2) * 16 + v4 * 4 + 2 * c["kSweepFlags"] * 4 + 2048, c["kSlotWordsP"] * 8)
    rs = slots(fixed + ((staged_arcs + 8 + 3) & ~3) * 4, c["kSlotWords2"] * 8) if staged_arcs else 0
    return r32, rp, (rs if rs >= 8 else 0)


def chain(n_states, weighted, seed):
    """A program of n_states tiles in either direction (tests/test_gpu_tile_wave_edges.py)."""
    if n_states >= 4:
        return synth.layered_lattice(seed, n_states=n_states, avg_degree=2.5, vocab=V, width=1, span=1 + seed % 2, max_degree=6,
                                     weighted=weighted)
    src, lab, dst = [], [], []
    for s in range(n_states - 1):
        for l in ([synth.BOS] if s == 0 else [synth.N_SPECIAL + s, synth.N_SPECIAL + 7 + s]):
            src.append(s), lab.append(l), dst.append(s + 1)
    src.append(n_states - 1), lab.append(synth.EOS), dst.append(n_states)
    w = np.random.default_rng(seed).normal(-0.5, 0.25, size=len(src)).astype(np.float32) if weighted else None
    return synth._finish(n_states + 1, V, src, lab, dst, w)


_CASES = {}


def case(bi, ex, dev):
    """lattices, scores and the oracle's results of one (batch, extras), computed once"""
    if (bi, ex) not in _CASES:
        lats = [chain(n, ex == "weights+scores", 100 * bi + i) for i, n in enumerate(BATCHES[bi])]
        theta = synth.label_scores(7 + bi, V, mean=-1.0, std=1.0)
        lat = LatticeBatch.from_synth(lats, device=dev)
        asc = None if ex == "none" else np.random.default_rng(50 + bi).normal(0.0, 0.5, size=lat.total_arcs).astype(np.float32)
        ref, vit = [], []
        for b, l in enumerate(lats):
            a0 = int(lat.arc_off[b])
            sc = theta[l.label].astype(np.float64)
            if l.weight is not None:
                sc = sc + l.weight
            if asc is not None:
                sc = sc + asc[a0:a0 + l.n_arcs]
            ref.append(O.forward_backward(l.n_rows, l.src, l.dst, sc))
            vit.append((sc, O.viterbi(l.n_rows, l.src, l.label, l.dst, sc.astype(np.float32), l.n_rows + 1)))
        _CASES[bi, ex] = dict(lats=lats, lat=lat, theta=theta, asc=asc, ref=ref, vit=vit)
    return _CASES[bi, ex]


def run_all(dev, reserve_kb):
    """Every batch through every instantiation: ({check: largest error}, [failures], {what ran})."""
    err, bad, ran = {}, [], {"lengths": set(), "staged": set(), "depths": set()}

    def rec(tag, e, bound):
        e = float(e)
        err[tag] = max(err.get(tag, 0.0), e)
        if not e <= bound:
            bad.append((tag, e, bound))

    for bi in range(len(BATCHES)):
        for ex in EXTRAS:
            c = case(bi, ex, dev)
            lat, lats = c["lat"], c["lats"]
            th = torch.from_numpy(c["theta"])
            t = None if c["asc"] is None else torch.from_numpy(c["asc"])
            m = lat.meta_host
            ran["lengths"] |= set(int(x) for x in m[:, _lib.META_BWD_TILES]) | set(int(x) for x in m[:, _lib.META_FWD_TILES])
            r32, rp, rs = ring_depths(int(max(l.n_rows for l in lats)), V, reserve_kb, 0 if ex == "none" else int(max(l.n_arcs for l in lats)))
            ran["depths"] |= {("float32", rs or r32), ("precise", rp)}
            if ex != "none":
                ran["staged"].add(bool(rs))
            runs = [("float32", dict(precise=0, tw=1), dict()), ("precise", dict(precise=1), dict())]
            if ex == "none":
                runs.append(("float32", dict(precise=0, tw=1), dict(want_grad_theta=True)))
            for name, switches, kw in runs:
                tag = f"{name}/{ex}" + ("/grad_theta" if kw else "")
                with _lib.tuning(**switches):
                    f = ops.forward_backward(lat, th, arc_scores=t, want_me=True, **kw)
                    bw = ops.backward(lat, th, arc_scores=t)
                    torch.cuda.synchronize()
                z, zb, post = f.logz64.cpu().numpy(), bw.logz64.cpu().numpy(), f.posterior.cpu().numpy()
                for b, l in enumerate(lats):
                    o, a0 = c["ref"][b], int(lat.arc_off[b])
                    rec(tag + "/logz", abs(z[b] - o["logZ"]), TOL[name]["logz"])
                    rec(tag + "/logz_backward", abs(zb[b] - o["logZ"]), TOL[name]["logz"])
                    rec(tag + "/posterior", np.max(np.abs(post[a0:a0 + l.n_arcs] - o["posterior"])), TOL[name]["post"])
                if name == "float32":
                    with _lib.tuning(precise=0, tw=0):
                        q = ops.forward_backward(lat, th, arc_scores=t, want_me=True, **kw)
                        torch.cuda.synchronize()
                    for k in FIELDS:
                        x, y = getattr(f, k).cpu().numpy(), getattr(q, k).cpu().numpy()
                        if k == "beta_me":  # (an exact zero: the mantissa is 0 in both, the exponent word is each flavour's own)
                            x, y = x.copy(), y.copy()
                            zero = (x[:, 0] == 0.0) & (y[:, 0] == 0.0)
                            x[zero, 1] = 0.0
                            y[zero, 1] = 0.0
                        rec(tag + "/bits_differ_from_tw0/" + k, 0.0 if x.tobytes() == y.tobytes() else 1.0, 0.0)
            if ex != "weights+scores":  # (Viterbi takes the same extras through its own tile waves: one case of them is enough)
                v = ops.viterbi(lat, th, arc_scores=t)
                torch.cuda.synchronize()
                best, arcs, lens = v.best.cpu().numpy(), v.arcs.cpu().numpy(), v.lengths.cpu().numpy()
                for b, l in enumerate(lats):
                    sc, (obest, _, oarcs) = c["vit"][b]
                    bound = len(oarcs) * 2.0 ** -23 * float(np.sum(np.abs(sc[oarcs]))) + 1e-7
                    rec(f"viterbi/{ex}/best", abs(float(best[b]) - obest), bound)
                    own = arcs[b, :lens[b]] - int(lat.arc_off[b])
                    rec(f"viterbi/{ex}/path_score", abs(float(np.sum(sc[own])) - obest), bound)
    return err, bad, {k: sorted(v) for k, v in ran.items()}


def _write(name, doc):
    # the directory of run outputs at the repository's root (a run that wants the figures creates it)
    for out in sorted(glob.glob(os.path.join(ROOT, "*_out"))):
        if os.path.isdir(out):
            with open(os.path.join(out, name), "w") as f:
                json.dump(doc, f, indent=1)


def _check(reserve_kb, err, bad, ran):
    assert set(LENGTHS) <= set(ran["lengths"]), ran["lengths"]
    want32, wantp = DEPTHS[reserve_kb]
    depths = [tuple(d) for d in ran["depths"]]
    assert ("float32", want32) in depths and ("precise", wantp) in depths, (reserve_kb, depths)
    # extras are staged in LDS where eight slots are left and gathered from memory where not: both occur over the reserves
    assert ran["staged"] == ([True] if want32 >= 8 else [False]), ran["staged"]
    assert not bad, bad[:8]
    assert len(err) >= 30, sorted(err)  # (nothing skipped silently: every instantiation left its checks)


def test_every_program_length_at_twelve_slots(dev):
    assert os.environ.get("NFST_LDS_RESERVE_KB", "0") in ("", "0"), "the in-process cases expect the default ring depth"
    err, bad, ran = run_all(dev, 0)
    _write("tile_wave_loop_errors.json", {"reserve_kb_0": dict(sorted(err.items())), "ran": ran})
    _check(0, err, bad, ran)


@pytest.mark.parametrize("reserve_kb", [48, 80, 96])
def test_every_program_length_at_shallower_rings(dev, reserve_kb):
    """8 and 4 slots per sweep: reached only with LDS held back, which the library reads once -- a fresh child process."""
    env = dict(os.environ, NFST_LDS_RESERVE_KB=str(reserve_kb))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(reserve_kb)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    doc = json.loads(p.stdout.strip().splitlines()[-1])
    _write(f"tile_wave_loop_errors_reserve{reserve_kb}.json", doc)
    _check(reserve_kb, doc["errors"], [tuple(b) for b in doc["failures"]], doc["ran"])


if __name__ == "__main__":
    e, b, r = run_all(torch.device("cuda:0"), int(sys.argv[1]))
    print(json.dumps({"errors": dict(sorted(e.items())), "failures": b, "ran": r}))

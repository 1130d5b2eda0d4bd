"""The tile-wave step where its instruction stream was tightened (``-m gpu``): the segmented sum of ``tile_math3`` /
``tile_math3p`` with the window test in its wait states and the exact path's own pack, and -- unchanged, but next in line
for the same treatment -- the posterior pass of the kernel with preloaded label weights.

Every case is held two ways:

* to the float64 oracle at the bounds of tests/test_gpu_parity.py for the same outputs (log Z 1e-5, row outputs 1e-5 + half
  a float32 spacing, posteriors 2e-6; under ``precise=1`` log Z 1e-8, tests/test_gpu_tile_wave_edges.py);
* bit for bit -- the raw bytes of logz64, logalpha, logbeta, beta_me and posterior -- to the same call under
  ``_lib.tuning(tw=0)``: loader + decoder + sweep waves (``tile_sweep`` / ``tile_math``, which this change leaves alone and
  which ``tile_math3`` is documented to match).  The parent commit's library agrees bit for bit on every input of this file
  but for the exponent word of exact zeros in ``beta_me`` (test_a_forbidden_label_stores_exact_zeros; profiles/sweep_slots.json,
  "flavours_agree_on_parent").  ``precise=1`` is held to the oracle only: ``tw=0`` does not
  select another kernel there.

The largest error of every check goes to sweep_slots_errors.json in the directory of run outputs (profiles/README.md).
"""
import glob
import json
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from nfst_amd import ops, synth, _lib
from nfst_amd.lattice import LatticeBatch

pytestmark = pytest.mark.gpu
TOL_Z, TOL_ROWS, TOL_POST, TOL_Z_PRECISE = 1e-5, 1e-5, 2e-6, 1e-8
FIELDS = ("logz64", "logalpha", "logbeta", "beta_me", "posterior")

_ERR = {}


def rec(tag, err):
    err = float(err)
    _ERR[tag] = max(_ERR.get(tag, 0.0), err)
    return err


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    # the directory of run outputs at the repository's root, as in test_gpu_neural_edges.py (a run that wants the figures
    # creates it; nothing is written without it)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for out in sorted(glob.glob(os.path.join(root, "*_out"))):
        if _ERR and os.path.isdir(out):
            with open(os.path.join(out, "sweep_slots_errors.json"), "w") as f:
                json.dump(dict(sorted(_ERR.items())), f, indent=1)


# ----------------------------------------------------------------------------- lattices
DEGREES = (1, 5, 9, 17)  # 1, 2, 3 (a group of 4) and 5 (a group of 8) lanes of four slots
N_LEVELS = 7
# arcs from the k-th state of a level (out-degree DEGREES[k]) to the j-th state of the next (in-degree DEGREES[j])
LEVEL_ARCS = ((0, 0, 0, 1), (0, 0, 0, 5), (0, 0, 0, 9), (1, 5, 9, 2))
MIX_V = synth.N_SPECIAL + 32 + N_LEVELS * 17


def mixed_degree_lattice():
    """0 --bos--> 1, state 1 fans out (32 arcs, eight lanes) to the first of N_LEVELS levels of four states whose in-degrees
    and out-degrees are 1, 5, 9 and 17 (parallel arcs with distinct labels), the last level leaves by eos.  The labels of
    a level's out-arcs are the level's own: ``level_labels(k)``."""
    assert [sum(r) for r in LEVEL_ARCS] == list(DEGREES) and [sum(c) for c in zip(*LEVEL_ARCS)] == list(DEGREES)
    src, lab, dst = [0], [synth.BOS], [1]
    first = lambda k: 2 + 4 * k  # first state of level k
    j = 0
    for t, d in enumerate(DEGREES):  # the fan-out of state 1
        for _ in range(d):
            src.append(1), lab.append(synth.N_SPECIAL + j), dst.append(first(0) + t)
            j += 1
    for k in range(N_LEVELS - 1):
        for s in range(4):
            j = 0
            for t in range(4):
                for _ in range(LEVEL_ARCS[s][t]):
                    src.append(first(k) + s), lab.append(level_labels(k)[j]), dst.append(first(k + 1) + t)
                    j += 1
    n_states = first(N_LEVELS)
    for s in range(4):
        src.append(first(N_LEVELS - 1) + s), lab.append(synth.EOS), dst.append(n_states)
    return synth._finish(n_states + 1, MIX_V, src, lab, dst)


def level_labels(k):
    return np.arange(synth.N_SPECIAL + 32 + 17 * k, synth.N_SPECIAL + 32 + 17 * (k + 1))


def tiny_chain(n_states, vocab=24):
    """0 --bos--> 1 ==(two parallel arcs)==> 2 ... --eos--> sink: a program of n_states tiles in either direction."""
    src, lab, dst = [], [], []
    for s in range(n_states - 1):
        for l in ([synth.BOS] if s == 0 else [synth.N_SPECIAL + s, synth.N_SPECIAL + 9 + s]):
            src.append(s), lab.append(l), dst.append(s + 1)
    src.append(n_states - 1), lab.append(synth.EOS), dst.append(n_states)
    return synth._finish(n_states + 1, vocab, src, lab, dst)


def _csrc_constants():
    """the ring constants of csrc/tile_pipeline.h and the LDS size of csrc/kernels.hip, read from the sources"""
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nfst_amd", "csrc")
    text = open(os.path.join(csrc, "tile_pipeline.h")).read() + open(os.path.join(csrc, "kernels.hip")).read()
    text = re.sub(r"//[^\n]*", "", text)
    env = {}
    for name in ("kDmaAheadDeep", "kRawSlotsDeep", "kRawWords", "kSlotWords", "kSlotWords2", "kMinRing", "kSweepFlags", "kMaxLds"):
        m = re.search(r"\b" + name + r"\s*=\s*([^,;]+)[,;]", text)
        assert m, name
        env[name] = int(eval(m.group(1), {"__builtins__": {}}, dict(env)))
    return env


def largest_tile_wave_rows(vocab):
    """The launcher's LDS budget (plan_forward_backward, ring_config in csrc/kernels.hip): forward-backward takes tile waves
    while the deep rings of the loader + decoder pipeline -- per sweep kRawSlotsDeep staging slots of kRawWords words and at
    least kMinRing decoded slots of kSlotWords words -- fit the CU's LDS beside alpha and beta (8 B per row each, rows
    rounded up to even), the label weights, the label histogram, the flag words and 1 KiB of trash (LdsPlan::fb_bytes);
    one row more and it falls back to the self-loading pipeline with the smallest rings."""
    c = _csrc_constants()
    v2, v4 = (vocab + 3) & ~1, (vocab + 3) & ~3
    fixed = v2 * 8 + v4 * 4 + 2 * c["kRawSlotsDeep"] * c["kRawWords"] * 4 + 2 * c["kSweepFlags"] * 4 + 1024
    room = c["kMaxLds"] - fixed - c["kMinRing"] * 2 * c["kSlotWords"] * 4
    rows = (room // 16) & ~1
    # (and the tile waves' own rings fit there: at least four slots of kSlotWords2 words per sweep)
    assert (c["kMaxLds"] - (16 * rows + fixed - 2 * c["kRawSlotsDeep"] * c["kRawWords"] * 4)) // (2 * c["kSlotWords2"] * 4) >= 4
    return rows


# ----------------------------------------------------------------------------- the two comparisons
def oracle_of(l, theta):
    return O.forward_backward(l.n_rows, l.src, l.dst, theta[l.label].astype(np.float64))


def check_rows(got, ref, tag):
    got = np.asarray(got, np.float64)
    inf = np.isneginf(ref)
    assert np.array_equal(np.isneginf(got), inf), tag
    if inf.all():
        return
    err = np.abs(got[~inf] - ref[~inf])
    half_ulp = 0.5 * np.spacing(np.abs(ref[~inf]).astype(np.float32)).astype(np.float64)
    rec(tag, err.max())
    assert np.all(err <= TOL_ROWS + half_ulp), (tag, err.max())


def run_fb(lat, theta, **kw):
    r = ops.forward_backward(lat, torch.from_numpy(theta), want_me=True, **kw)
    torch.cuda.synchronize()
    return r


def check_case(tag, lats, lat, theta, refs, precise=False, oracle_only=(), **kw):
    """forward_backward (precise=0, or precise=1) against the oracle; unless precise, its bytes against tw=0 (but for the
    outputs named in ``oracle_only``)."""
    if precise:
        with _lib.tuning(precise=1):
            r = run_fb(lat, theta, **kw)
    else:
        with _lib.tuning(precise=0):
            r = run_fb(lat, theta, **kw)
    z, la, lb, post = (getattr(r, k).cpu().numpy() for k in ("logz64", "logalpha", "logbeta", "posterior"))
    me = r.beta_me.cpu()
    with np.errstate(divide="ignore"):  # (an exact zero: mantissa 0 -> -inf)
        lb_me = np.log(me[:, 0].numpy().astype(np.float64)) + me[:, 1].contiguous().view(torch.int32).numpy().astype(np.float64) * np.log(2.0)
    for b, (l, o) in enumerate(zip(lats, refs)):
        r0, a0 = int(lat.row_off[b]), int(lat.arc_off[b])
        assert rec(tag + "/logz", abs(z[b] - o["logZ"])) <= (TOL_Z_PRECISE if precise else TOL_Z), (tag, b)
        check_rows(la[r0:r0 + l.n_rows], o["logalpha"], tag + "/logalpha")
        check_rows(lb[r0:r0 + l.n_rows], o["logbeta"], tag + "/logbeta")
        check_rows(lb_me[r0:r0 + l.n_rows], o["logbeta"], tag + "/beta_me")
        assert rec(tag + "/posterior", np.max(np.abs(post[a0:a0 + l.n_arcs] - o["posterior"]))) <= TOL_POST, (tag, b)
    if not precise:
        with _lib.tuning(precise=0, tw=0):
            q = run_fb(lat, theta, **kw)
        for k in FIELDS:
            x, y = getattr(r, k).cpu().numpy(), getattr(q, k).cpu().numpy()
            same = x.tobytes() == y.tobytes()
            if not same:  # (where, for the log)
                bad = np.flatnonzero(x.reshape(-1).view(np.uint32 if x.itemsize == 4 else np.uint64) != y.reshape(-1).view(np.uint32 if x.itemsize == 4 else np.uint64))
                print(tag, k, "differs from tw=0 at", bad[:8], x.reshape(-1)[bad[:8]], y.reshape(-1)[bad[:8]])
            if k in oracle_only:
                continue
            rec(tag + "/bits_differ_from_tw0/" + k, 0.0 if same else 1.0)
            assert same, (tag, k)
    return r


# ----------------------------------------------------------------------------- the sweep loop
@pytest.fixture(scope="module")
def mix():
    return mixed_degree_lattice()


def mix_theta(seed, low_level=None, dead_label=None):
    th = np.random.default_rng(seed).normal(0.0, 0.3, size=MIX_V).astype(np.float32)
    if low_level is not None:
        th[level_labels(low_level)] = -80.0 + th[level_labels(low_level)]
    if dead_label is not None:
        th[dead_label] = -np.inf
    return th


def test_groups_of_one_two_four_and_eight_lanes_in_one_tile(dev, mix):
    """Distinct weights on states of in-degree and out-degree 1, 5, 9 and 17: a stage of the segmented sum that read its
    source too early shows in exactly those sums."""
    deg_out = np.bincount(mix.src, minlength=mix.n_rows)
    deg_in = np.bincount(mix.dst[mix.src != mix.dst], minlength=mix.n_rows)
    assert set(DEGREES) <= set(deg_out) and set(DEGREES) <= set(deg_in) and max(deg_out.max(), deg_in.max()) <= 32
    lat = LatticeBatch.from_synth([mix], device=dev)
    for seed in (1, 2):
        theta = mix_theta(seed)
        check_case(f"mixed_degrees/seed{seed}", [mix], lat, theta, [oracle_of(mix, theta)])
        check_case(f"mixed_degrees_precise/seed{seed}", [mix], lat, theta, [oracle_of(mix, theta)], precise=True)


def test_a_level_far_below_the_reference_takes_the_exact_path(dev, mix):
    """One level's label scores at -80 between levels near 0: that level's terms lie 2^-115 from the reference exponent of
    the tiles before it (the window is 2^+-64), and the next trip's reference is 2^-115 from the levels behind it: the exact
    path with its own pack-and-store, in both sweeps."""
    lat = LatticeBatch.from_synth([mix], device=dev)
    for low in (1, 3, 4):
        theta = mix_theta(3, low_level=low)
        check_case(f"exact_path/level{low}", [mix], lat, theta, [oracle_of(mix, theta)])
        check_case(f"exact_path_precise/level{low}", [mix], lat, theta, [oracle_of(mix, theta)], precise=True)


def test_a_forbidden_label_stores_exact_zeros(dev, mix):
    """-inf on the label of the one out-arc of a level's first state: its beta is an exact zero, and so is the alpha of a state
    on the way.  ``beta_me`` is held to the oracle only: the two flavours give an exact zero different exponent words, in the
    parent commit's library as well -- ``tile_math3`` stores kEZero, the exponent that never wins a maximum, ``me_pack`` of
    the loader + decoder + sweep pipeline the largest term exponent -- while mantissa 0 and log beta = -inf are the same."""
    lat = LatticeBatch.from_synth([mix], device=dev)
    for k in (2, 3):
        theta = mix_theta(4, dead_label=level_labels(k)[0])
        o = oracle_of(mix, theta)
        assert np.isneginf(o["logbeta"]).any() and np.isfinite(o["logZ"])
        check_case(f"exact_zeros/level{k}", [mix], lat, theta, [o], oracle_only=("beta_me",))
        check_case(f"exact_zeros_precise/level{k}", [mix], lat, theta, [o], precise=True)


@pytest.mark.parametrize("precise", [False, True])
def test_programs_of_one_to_nine_tiles(dev, precise):
    """Shorter than a trip, every tail length and the first whole trips."""
    lats = [tiny_chain(n) for n in range(1, 10)]
    lat = LatticeBatch.from_synth(lats, device=dev)
    m = lat.meta_host
    assert sorted(int(x) for x in m[:, _lib.META_BWD_TILES]) == list(range(1, 10))
    assert sorted(int(x) for x in m[:, _lib.META_FWD_TILES]) == list(range(1, 10))
    theta = synth.label_scores(11, 24, mean=-1.0, std=1.0)
    check_case("tiles_1_to_9" + ("_precise" if precise else ""), lats, lat, theta, [oracle_of(l, theta) for l in lats], precise=precise)


# ----------------------------------------------------------------------------- the posterior pass
def test_arc_ranges_at_every_alignment(dev):
    """Lattices whose canonical arc ranges begin and end at 0, 1, 2 and 3 (mod 4): the unaligned head and tail beside the
    16-byte groups; every lattice ends in its sink's self loop (posterior 0 by definition)."""
    lats = [tiny_chain(2 + (i % 5)) for i in range(12)] + [synth.layered_lattice(40 + i, n_states=30 + i, avg_degree=3.0, vocab=24, width=3, span=2)
                                                            for i in range(8)]
    lat = LatticeBatch.from_synth(lats, device=dev)
    begin = {int(a) % 4 for a in lat.arc_off[:len(lats)]}
    end = {(int(lat.arc_off[b]) + l.n_arcs) % 4 for b, l in enumerate(lats)}
    assert begin == {0, 1, 2, 3} and end == {0, 1, 2, 3}
    theta = synth.label_scores(12, 24, mean=-1.0, std=1.0)
    r = check_case("arc_alignment", lats, lat, theta, [oracle_of(l, theta) for l in lats])
    post = r.posterior.cpu().numpy()
    for b, l in enumerate(lats):
        loops = np.flatnonzero(l.src == l.dst)
        assert loops.size >= 1 and np.all(post[int(lat.arc_off[b]) + loops].view(np.uint32) == 0)  # +0.0, bit for bit


def test_more_arcs_than_the_preloaded_groups_hold(dev):
    """More than 7 x 768 x 4 = 21,504 arcs: the remainder loop behind the preloaded groups."""
    l = synth.layered_lattice(51, n_states=1900, avg_degree=12.5, vocab=64, width=16, span=4)
    assert l.n_arcs > 21504 + 2 * 1024  # (the remainder loop runs for more than half of the block's threads)
    theta = synth.label_scores(13, 64)
    check_case("remainder_loop", [l], LatticeBatch.from_synth([l], device=dev), theta, [oracle_of(l, theta)])


def test_largest_lattice_of_the_tile_wave_kernel(dev):
    """The largest row count at which the launcher still takes tile waves, and the first beyond it (the self-loading
    pipeline): 6972 and 6973 rows at 40 labels, (160 KiB - 32,304 B beside the rows - 3 x 2 x 3328 B of decoded slots) / 16."""
    V = 40
    n_max = largest_tile_wave_rows(V)
    assert n_max == 6972 and 8 * n_max < 65536
    theta = synth.label_scores(14, V)
    for n_rows in (n_max, n_max + 1):
        l = synth.layered_lattice(52, n_states=n_rows - 1, avg_degree=3.0, vocab=V, width=24, span=3)
        lat = LatticeBatch.from_synth([l], device=dev)
        assert l.n_rows == n_rows and lat.max_rows == n_rows
        check_case(f"largest_lattice/rows{n_rows}", [l], lat, theta, [oracle_of(l, theta)])


def test_launch_with_label_sums_is_unchanged(dev, mix):
    """``want_grad_theta=True`` selects the kernel without preloaded label weights."""
    lats = [mix, synth.layered_lattice(53, n_states=200, avg_degree=6.0, vocab=MIX_V, width=6, span=3)]
    lat = LatticeBatch.from_synth(lats, device=dev)
    theta = mix_theta(5)
    refs = [oracle_of(l, theta) for l in lats]
    r = check_case("with_label_sums", lats, lat, theta, refs, want_grad_theta=True)
    g = r.grad_theta.cpu().numpy()
    for b, (l, o) in enumerate(zip(lats, refs)):
        assert rec("with_label_sums/grad_theta", np.max(np.abs(g[b] - np.bincount(l.label, weights=o["posterior"], minlength=MIX_V)))) <= 1e-4

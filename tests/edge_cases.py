"""Inputs of the edge-case tests of the expectation, k-best and positional kernels (test helper, not a test module).

tests/test_gpu_expectation.py and tests/test_gpu_kbest.py run the kernels on these inputs; tests/test_expectation_cpu.py
and tests/test_kbest_cpu.py prove on the references alone that the inputs are what their tests need (posteriors that
have not collapsed to one path, a lattice with fewer than k finite paths, scores that really tie).  Both sides build
their inputs here, so they cannot drift apart.  The positional section at the end serves tests/test_gpu_positional.py
and tests/test_positional_cpu.py in the same way.
"""
from __future__ import annotations

import numpy as np

from nfst_amd import synth
from tests import expectation_ref as X
from tests import kbest_ref as R

F32 = np.float32
PAD, BOS, EOS = synth.PAD, synth.BOS, synth.EOS
V_MIXED, V_WEIGHTED = 64, 48
DEAD = np.array([4, 9, 15, 22, 30, 41])  # the labels test_viterbi_labels_at_minus_infinity puts at -inf


def arc_slices(lats):
    """The slice of every lattice in the batch's canonical arc order."""
    off = np.concatenate([[0], np.cumsum([l.n_arcs for l in lats])])
    return [slice(int(off[b]), int(off[b + 1])) for b in range(len(lats))]


def score64(l, theta_b, asc=None):
    s = np.asarray(theta_b, F32)[l.label].astype(np.float64)
    if l.weight is not None:
        s = s + l.weight.astype(np.float64)
    if asc is not None:
        s = s + np.asarray(asc, np.float64)
    return s


# ----------------------------------------------------------------------------- lattices
def mixed_batch():  # (the mixed batch of test_gpu_parity.py)
    V = V_MIXED
    return [
        synth.layered_lattice(3, n_states=30, avg_degree=3.0, vocab=V, width=4, span=2),
        synth.layered_lattice(4, n_states=300, avg_degree=8.0, vocab=V, width=9, span=5),
        synth.layered_lattice(5, n_states=90, avg_degree=5.0, vocab=V, width=1, span=6),
        synth.edit_lattice([10, 11, 12, 13, 14], [20, 21, 22, 23], vocab=V, seed=2),
        synth.layered_lattice(6, n_states=700, avg_degree=10.0, vocab=V, width=16, span=8),
        synth._finish(2, V, [0], [EOS], [1]),
    ]


def weighted_batch(n=4, vocab=V_WEIGHTED):
    return [synth.layered_lattice(s, n_states=150 + 20 * s, avg_degree=6.0, vocab=vocab, width=7, span=3, weighted=True)
            for s in range(n)]


def weighted_lats(weighted, vocab=V_WEIGHTED):  # (the batch of the Viterbi edge tests of test_gpu_paths.py)
    return [synth.layered_lattice(s, n_states=n, avg_degree=6.0, vocab=vocab, width=7, span=3, weighted=weighted)
            for s, n in enumerate((150, 170, 190, 210, 700))]


def star():  # a state with 200 out-arcs: four chunks of the k-best sweep, tree-summed or wide groups in the tile programs
    src = [0] + [1] * 200 + list(range(2, 202)) + [202]
    lab = [BOS] + list(range(3, 203)) + [5] * 200 + [EOS]
    dst = [1] + list(range(2, 202)) + [202] * 200 + [203]
    return synth._finish(204, 256, src, lab, dst)


def double_funnel():  # fan-out 200, fan-in, fan-out, fan-in (test_beta_neural_grad_funnels)
    src = [0] + [1] * 200 + list(range(2, 202)) + [202] * 200 + list(range(203, 403)) + [403]
    lab = [BOS] + list(range(3, 203)) + [5] * 200 + list(range(3, 203)) + [6] * 200 + [EOS]
    dst = [1] + list(range(2, 202)) + [202] * 200 + list(range(203, 403)) + [403] * 200 + [404]
    return synth._finish(405, 256, src, lab, dst)


# the ten packings the edge-case tests run: narrow and wide groups, one, two and four slots per lane, compact tiles or not
STAR_PACKINGS = [dict(), dict(group_mode=1), dict(group_mode=2), dict(group_mode=1, slots_per_lane=1), dict(group_mode=2, slots_per_lane=1),
                 dict(group_mode=1, slots_per_lane=2), dict(group_mode=2, slots_per_lane=2), dict(slots_per_lane=4),
                 dict(group_mode=1, slots_per_lane=4, no_compact=True), dict(group_mode=2, slots_per_lane=4, no_compact=True)]


def packing_lattices():
    """The lattices run under every packing: the star, the double funnel and a layered lattice with states of up to 40
    out-arcs (vocabulary 256: compact tiles unless the options forbid them)."""
    return [star(), double_funnel(), synth.layered_lattice(31, n_states=300, avg_degree=8.0, vocab=256, width=24, max_degree=40)]


def large_pair(n_states):
    """The lattices of test_viterbi_large_lattice: n_states + 1 rows beside a 200-state neighbour."""
    big = synth.layered_lattice(77, n_states=n_states, avg_degree=4.0, vocab=64, width=16, span=4, weighted=True)
    small = synth.layered_lattice(78, n_states=200, avg_degree=4.0, vocab=64, width=8, span=4, weighted=True)
    return [big, small]


def beyond_lds_batch():
    """A batch of 8192 rows that forward_backward takes: the lattice of large_pair(8191) without table weights beside
    300 single-arc lattices (more lattices than compute units and no per-arc extras: the fused sweeps, 16 bytes of LDS
    per row and no rings)."""
    big = synth.layered_lattice(77, n_states=8191, avg_degree=4.0, vocab=64, width=16, span=4)
    return [big] + [synth._finish(2, 64, [0], [EOS], [1]) for _ in range(300)]


def many_small():
    """The 330 lattices and per-lattice label scores of test_viterbi_more_lattices_than_compute_units."""
    rng = np.random.default_rng(6)
    lats = [synth.layered_lattice(2000 + i, n_states=int(rng.integers(8, 60)), avg_degree=3.0, vocab=40, width=int(rng.choice([1, 2, 4])),
                                  span=2, max_degree=8, weighted=True) for i in range(330)]
    theta = rng.normal(-1.0, 1.0, size=(len(lats), 40)).astype(F32)
    asc = np.random.default_rng(7).normal(0.0, 0.3, size=sum(l.n_arcs for l in lats)).astype(F32)
    return lats, theta, asc


# ----------------------------------------------------------------------------- labels at -inf, no finite path
def dead_label_theta(seed=10, vocab=V_WEIGHTED, shape=None):
    theta = np.random.default_rng(seed).normal(-2.0, 0.7, size=shape or vocab).astype(F32)
    theta[..., DEAD] = -np.inf
    return theta


def no_path_case(weighted):
    """test_viterbi_without_a_finite_path: every path of lattice 1 ends by eos and every path of lattice 3 starts by
    bos, both at -inf there."""
    lats = weighted_lats(weighted)
    theta = np.random.default_rng(12).normal(-2.0, 0.7, size=(len(lats), V_WEIGHTED)).astype(F32)
    theta[1, EOS] = -np.inf
    theta[3, BOS] = -np.inf
    return lats, theta


def few_paths_case():
    """(lats, theta [B, V], b, n): the mixed batch with per-lattice label scores; lattice b keeps n finite paths,
    0 < n < 64, after the labels of a fixed draw are put at -inf for it alone."""
    lats = mixed_batch()
    theta = np.stack([synth.label_scores(40 + b, V_MIXED) for b in range(len(lats))])
    b = 0
    labels = np.arange(synth.N_SPECIAL, V_MIXED)
    dead = np.random.default_rng(FEW_PATHS_SEED).choice(labels, size=FEW_PATHS_DEAD, replace=False)
    theta[b, dead] = -np.inf
    l = lats[b]
    n = R.count_finite_paths(l.n_rows, l.src, l.dst, score64(l, theta[b]), l.n_rows - 1)
    return lats, theta, b, n


FEW_PATHS_SEED, FEW_PATHS_DEAD = 1, 30  # (chosen on the reference: tests/test_kbest_cpu.py asserts 0 < n < 64)


# ----------------------------------------------------------------------------- exponent range and cancellation
SPREAD_MIN = 20  # arcs per lattice with a posterior in (0.01, 0.99): the distribution has not collapsed to one path
RANGE_CASES = ("scale30", "scale3000", "shift")
RANGE_SPREAD = RANGE_CASES  # (every case meets the condition: none is held for log Z and E[V] only)
RANGE_SEED = {"scale30": 6, "scale3000": 9}  # chosen on the reference: tests/test_expectation_cpu.py asserts the spread
RANGE_LOGZ = {"scale30": 8.0e2, "scale3000": 5.0e4, "shift": 1.0e5}  # |log Z| of some lattice of the case exceeds this


def range_case(name):
    """(lats, theta [V], arc_scores, arc_values): label scores N(0, 1) * 30 or * 3000 with per-arc scores of +-40 (path
    weights around e^+-1e3 and e^+-5e4), or ordinary scores shifted by -2e4 per label (e^-4e5); values +-1e3 with
    random signs, so that |E[V]| << M = E[sum |v|]."""
    if name == "shift":
        lats = weighted_batch()
        rng = np.random.default_rng(21)
        theta = (rng.normal(-2.0, 0.7, size=V_WEIGHTED) - 2.0e4).astype(F32)
        n = sum(l.n_arcs for l in lats)
        asc = rng.normal(0.0, 0.3, size=n).astype(F32)
    else:
        scale, seed = {"scale30": 30.0, "scale3000": 3000.0}[name], RANGE_SEED[name]
        # edit lattices: many paths over the same marks, which tie in the label scores and differ in the +-40 only
        lats = [synth.edit_lattice(list(range(10, 19)), list(range(20, 28)), vocab=V_MIXED, seed=seed),
                synth.edit_lattice(list(range(10, 17)), list(range(20, 30)), vocab=V_MIXED, seed=seed + 1)]
        rng = np.random.default_rng(seed)
        theta = (rng.normal(0.0, 1.0, size=V_MIXED) * scale).astype(F32)
        n = sum(l.n_arcs for l in lats)
        asc = (40.0 * rng.choice([-1.0, 1.0], size=n)).astype(F32)
    av = (1.0e3 * rng.choice([-1.0, 1.0], size=n)).astype(F32)
    return lats, theta, asc, av


def posterior_spread(l, theta_b, asc=None):
    """Arcs of l whose reference posterior lies in (0.01, 0.99)."""
    p = X.expectation(l.n_rows, l.src, l.dst, score64(l, theta_b, asc), np.zeros(l.n_arcs))["posterior"]
    return int(np.sum((p > 0.01) & (p < 0.99)))


# ----------------------------------------------------------------------------- exact ties
def quarter(x):
    return (np.round(np.asarray(x, np.float64) * 4) / 4).astype(F32)


def tie_cases():
    """{name: (lats, theta, arc_scores or None, pack options)} with every score on a grid of 0.25: float32 sums are
    exact and whole paths tie."""
    out = {}
    for tag, opts in (("star", dict()), ("star wide", dict(group_mode=2)), ("star one slot", dict(slots_per_lane=1))):
        out[tag] = ([star()], np.full(256, -0.25, F32), None, opts)  # all 200 paths score -1.0
    out["funnel"] = ([double_funnel()], quarter(np.random.default_rng(14).normal(-2.0, 0.4, size=256)), None, dict())
    for extras in (False, True):  # (test_viterbi_exact_ties)
        lats = weighted_lats(extras) + [synth.edit_lattice([10, 11, 12, 13, 14], [20, 21, 22, 23], vocab=V_WEIGHTED, seed=2)]
        asc = None
        if extras:
            for l in lats[:-1]:
                l.weight = quarter(l.weight)
            lats[-1].weight = np.zeros(lats[-1].n_arcs, F32)
            n = sum(l.n_arcs for l in lats)
            asc = quarter(np.random.default_rng(9).normal(0.0, 0.5, size=n))
        theta = quarter(np.random.default_rng(8).normal(-2.0, 0.7, size=V_WEIGHTED))
        out["grid extras" if extras else "grid"] = (lats, theta, asc, dict())
    return out


def kbest_refs(lats, theta, asc=None, k=64):
    """kbest_ref.k_best per lattice of a batch (theta [V] or [B, V], asc over the batch's arcs)."""
    out = []
    for b, (l, sl) in enumerate(zip(lats, arc_slices(lats))):
        th, e = R.arc_terms(l, theta[b] if theta.ndim == 2 else theta, None if asc is None else asc[sl])
        with np.errstate(invalid="ignore"):  # (+inf + -inf: no candidate)
            out.append(R.k_best(l.n_rows, l.src, l.dst, th, e, k, l.n_rows - 1))
    return out


def tied_entries(ref):
    """Entries of a reference list that share their score with another one."""
    best = ref["best"][:ref["n_paths"]]
    _, c = np.unique(best, return_counts=True)
    return int(c[c > 1].sum())


def sweep_chunk(l, a):
    """The chunk of the k-best sweep that takes canonical arc a of lattice l: a state's first 64 out-arcs, then 63 at a
    time beside the carry lane."""
    i = int(a) - int(np.searchsorted(l.src, l.src[a]))
    return 0 if i < 64 else 1 + (i - 64) // 63


def reachable_dead_arc(l, dead=DEAD):
    """A canonical arc of l with a dead label (every state of a layered lattice is reachable from state 0, so the sweep
    reads the arc's candidate)."""
    a = np.nonzero(np.isin(l.label, dead) & (l.src != l.dst))[0]
    return int(a[len(a) // 2])


# ----------------------------------------------------------------------------- positional sweeps (nfst_positional*)
# tests/test_gpu_positional.py runs these; tests/test_positional_cpu.py proves, on the reference and the host-side plan
# query alone, that they are what their cases need (which flavour a batch takes, the group sizes, the exponent range, the
# limits, scores that really tie).  Builders return fresh lattices: callers may change them.
POS_V = 140
POS_LARGE = {"big": 480, "mid": 440}  # n_states: (unstaged, unstaged) and (sum-product unstaged, max-plus staged)
# (n_states, avg_degree) -> (G by the mean degree alone, G after the widening loop), from the packed meta words
POS_DEGREE_CLASSES = {(120, 12.0): (8, 8), (120, 20.0): (16, 16), (120, 44.0): (32, 32), (30, 20.0): (16, 16),
                      (60, 6.0): (4, 8), (60, 12.0): (8, 16), (30, 24.0): (16, 32)}
# n_states of pos_rowmax whose batch packs to the most rows nfst_positional takes beside 256 labels: 24 * 6442 + 20 * 256 +
# 4112 = 163840 (chosen on the packed batch's own max_rows, which counts the packer's scratch rows)
POS_ROWMAX_STATES = 6437
POS_LDS_LIMIT = 160 * 1024
POS_WIDE_VOCAB = 32767  # NFST_MAX_VOCAB
# seeds of the position scores of the tie cases, chosen on the reference, and the lattices of each case whose walk
# meets a state at which two or more live arcs attain vb_t(state) (tests/test_positional_cpu.py asserts them)
POS_TIE_SEED = {"star": 4, "star wide": 4, "star one slot": 4, "funnel": 4, "grid": 7, "grid extras": 135}
POS_TIE_LATTICES = {"star": 1, "star wide": 1, "star one slot": 1, "funnel": 1, "grid": 5, "grid extras": 6}


def pos_large(name, weighted=False):
    return synth.layered_lattice(27, n_states=POS_LARGE[name], avg_degree=90.0, vocab=POS_V, width=8, span=3, max_degree=130,
                                 weighted=weighted)


def pos_neighbour(vocab=POS_V, weighted=False):  # 13 rows
    return synth.layered_lattice(3, n_states=12, avg_degree=2.0, vocab=vocab, width=3, span=3, max_degree=4, weighted=weighted)


def pos_degree_classes():
    return [synth.layered_lattice(92, n_states=n, avg_degree=d, vocab=POS_V, width=8, span=3, max_degree=130)
            for n, d in POS_DEGREE_CLASSES]


def pos_rowmax_batch(over=0):
    """[pos_rowmax lattice, 13-row neighbour]: the most rows nfst_positional takes at vocabulary 256, or ``over`` more."""
    return [pos_rowmax(POS_ROWMAX_STATES + over), pos_neighbour(256)]


def pos_rowmax(n_states=POS_ROWMAX_STATES):
    return synth.layered_lattice(91, n_states=n_states, avg_degree=4.0, vocab=256, width=128, span=4)


def pos_wide(vocab=POS_WIDE_VOCAB):  # 13 rows, 28 arcs
    return synth.layered_lattice(26, n_states=12, avg_degree=2.0, vocab=vocab, width=3, span=3, max_degree=4)


def pos_sum_lds(max_rows, vocab):
    """Dynamic LDS of nfst_positional without staged arcs (include/nfst_hip.h)."""
    return 24 * int(max_rows) + 20 * int(vocab) + 4112


def pos_vocab_limit(max_rows):
    """The largest vocabulary nfst_positional takes beside ``max_rows`` rows."""
    return (POS_LDS_LIMIT - 4112 - 24 * int(max_rows)) // 20


def pos_range_inputs(name):
    """(lats, theta [V], arc_scores, pos [B, T, V], T) of a range case under position scores: T is the batch's longest
    path, pos of lattice b is drawn from default_rng(90 + b)."""
    from tests import positional_ref as P

    lats, theta, asc, _ = range_case(name)
    T = max(P.min_max_len(l)[1] for l in lats)
    V = lats[0].vocab
    pos = np.stack([np.random.default_rng(90 + b).normal(0.0, 1.0, size=(T, V)) for b in range(len(lats))]).astype(F32)
    return lats, theta, asc, pos, T


def pos_tie_inputs(name):
    """(lats, theta, arc_scores or None, pos [B, T, V], T) of a tie case: ``tie_cases()[name]`` with position scores on
    the 0.25 grid, T the batch's longest path."""
    from tests import positional_ref as P

    lats, theta, asc, _ = tie_cases()[name]
    T = max(P.min_max_len(l)[1] for l in lats)
    V = lats[0].vocab
    rng = np.random.default_rng(POS_TIE_SEED[name])
    pos = quarter(rng.normal(0.0, 1.0, size=(len(lats), T, V)))
    return lats, theta, asc, pos, T

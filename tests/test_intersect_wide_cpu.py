"""The sparse automata of up to 4096 states (nfst_amd.constraints.WideDFA): every builder against brute-force runs, the
dense round trip, validation; the vectorised restatement of the product (tests/intersect_wide_ref.py) against the
pure-Python one; the weight lookup of IntersectResult.scores on CPU tensors; the three C entry points' declarations and
their argument checks (host side, before any launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from nfst_amd import synth
from nfst_amd.constraints import MAX_WIDE_STATES, ConstraintDFA, WideDFA
from nfst_amd.lattice import IntersectResult, LatticeBatch
from tests import intersect_ref as R
from tests import intersect_wide_ref as RW

V = 64
ERR_ARG, ERR_LIMIT = -1, -6  # (include/nfst_hip.h)


def _strings(rng, n, vocab, length, alphabet=None):
    for _ in range(n):
        k = int(rng.integers(0, length + 1))
        yield [int(x) for x in (rng.integers(0, vocab, k) if alphabet is None else rng.choice(alphabet, k))]


def _dense_run(delta, final, labels):
    return R.run(delta, final, labels)


def _same_language(w, delta, final, strings):
    """The sparse automaton, its dense form and the given dense table accept the same of ``strings``."""
    d2, f2 = w.to_dense()
    assert np.array_equal(d2, delta) and np.array_equal(f2, np.asarray(final, bool))
    n_acc = 0
    for s in strings:
        want = _dense_run(delta, final, s)
        assert w.accepts(s) == want, s
        n_acc += want
    return n_acc


# ----------------------------------------------------------------------------- builders
def test_from_dense_round_trip_and_default_choice():
    rng = np.random.default_rng(0)
    for Q in (1, 2, 7, 65, 130):
        delta = rng.integers(-1, Q, size=(Q, 9))
        delta[rng.random((Q, 9)) < 0.5] = int(rng.integers(-1, Q))  # a frequent target, so that defaults matter
        final = rng.random(Q) < 0.5
        w = WideDFA.from_dense(delta, final)
        assert w.n_states == Q and w.n_lattices is None and w.vocab == 9
        _same_language(w, delta, final, list(_strings(rng, 50, 9, 6)))
        for q in range(Q):  # the most frequent target, ties to the smallest; the exceptions are exactly the others
            vals, cnt = np.unique(delta[q], return_counts=True)
            assert w.dflt[q] == vals[cnt == cnt.max()].min()
            assert w.exc_off[q + 1] - w.exc_off[q] == int((delta[q] != w.dflt[q]).sum())
    tie = WideDFA.from_dense(np.array([[1, 0, 1, 0]]).repeat(2, 0), [1, 1])
    assert list(tie.dflt) == [0, 0] and list(tie.exc_label) == [0, 2, 0, 2]


@pytest.mark.parametrize("name", ["accept_all", "count_at_most", "forbid_bigram", "parity", "contains", "marked_sequence"])
def test_from_constraint_keeps_the_table(name):
    c = {"accept_all": ConstraintDFA.accept_all(V), "count_at_most": ConstraintDFA.count_at_most(V, range(3, 30), 63),
         "forbid_bigram": ConstraintDFA.forbid_bigram(V, 3, 10), "parity": ConstraintDFA.parity(V, range(3, 34)),
         "contains": ConstraintDFA.contains(V, [4, 20, 4]), "marked_sequence": ConstraintDFA.marked_sequence(V, 4, [20, 21, 20])}[name]
    w = WideDFA.from_constraint(c)
    d, f = w.to_dense()
    assert np.array_equal(d, c.delta) and np.array_equal(f, c.final) and w.n_states == c.n_states
    assert w.exc_label.size < c.delta.size / 2  # (sparse: these tables are mostly their defaults)


def test_from_constraint_per_lattice_and_weighted():
    cs = [ConstraintDFA.marked_sequence(V, 4, y) for y in ([20, 21], [22], [23, 24, 25])]
    w = WideDFA.from_constraint(ConstraintDFA.stack(cs))
    assert w.n_lattices == 3 and w.n_states == 8 and list(np.diff(w.q_off)) == [8, 8, 8]  # (stack pads the narrow ones)
    for b, (d, f) in enumerate(w.to_dense()):
        assert np.array_equal(d[:cs[b].n_states], cs[b].delta) and np.array_equal(f[:cs[b].n_states], cs[b].final)
    weight = torch.randn(2, V)
    ww = WideDFA.from_constraint(ConstraintDFA(ConstraintDFA.parity(V, [5]).delta, [1, 0], weight))
    assert ww.weighted and ww.exc_label.size == 2 * V and torch.equal(ww.weight_exc, weight.reshape(-1))


def test_sequence():
    rng = np.random.default_rng(1)
    seq = [1, 7, 7, 3, 2]
    w = WideDFA.sequence(8, seq)
    assert w.n_states == 6 and w.accepts(seq) and not w.accepts(seq[:-1]) and not w.accepts(seq + [2]) and not w.accepts([])
    for s in _strings(rng, 300, 8, 6):
        assert w.accepts(s) == (s == seq)
    long = [int(x) for x in rng.integers(0, 8, 4095)]
    wl = WideDFA.sequence(8, long)
    assert wl.n_states == MAX_WIDE_STATES and wl.accepts(long) and wl.run(long) == 4095 and not wl.accepts(long[:-1])


def _marked_ok(marker, seq, s):
    return [s[i + 1] for i in range(len(s) - 1) if s[i] == marker] == list(seq) and (not s or s[-1] != marker)


def test_marked_sequence_is_the_narrow_automaton_and_goes_beyond_it():
    for n in (0, 1, 5, 31):
        seq = [3 + (7 * j) % 11 for j in range(n)]
        c, w = ConstraintDFA.marked_sequence(V, 4, seq), WideDFA.marked_sequence(V, 4, seq)
        d, f = w.to_dense()
        assert np.array_equal(d, c.delta) and np.array_equal(f, c.final), n
    rng = np.random.default_rng(2)
    seq = [int(x) for x in rng.integers(0, 4, 40)]  # 40 symbols over {0 .. 3}, marker 4: beyond the narrow 31
    with pytest.raises(ValueError, match="at most 31"):
        ConstraintDFA.marked_sequence(6, 4, seq)
    w = WideDFA.marked_sequence(6, 4, seq)
    assert w.n_states == 82 and w.exc_label.size == 81
    good = []
    for y in seq:
        good += [5] * int(rng.integers(0, 3)) + [4, y]
    assert w.accepts(good) and w.accepts(good + [5, 5]) and w.run(good) == 80
    n_acc = 0
    for _ in range(400):  # mutations of an accepted string, judged by the definition
        s = list(good)
        for _ in range(int(rng.integers(0, 3))):
            i = int(rng.integers(0, len(s)))
            if rng.random() < 0.5:
                s[i] = int(rng.integers(0, 6))
            else:
                del s[i]
        assert w.accepts(s) == _marked_ok(4, seq, s), s
        n_acc += w.accepts(s)
    assert 20 < n_acc < 380
    assert WideDFA.marked_sequence(6, 4, [1] * 2047).n_states == MAX_WIDE_STATES


def test_projected_sequence():
    rng = np.random.default_rng(3)
    keep, seq = [1, 2, 5], [5, 1, 1, 2]
    w = WideDFA.projected_sequence(8, keep, seq)
    assert w.n_states == 5
    n_acc = 0
    for s in list(_strings(rng, 600, 8, 8)) + list(_strings(rng, 600, 8, 9, alphabet=[5, 1, 2, 0])) + [[0, 5, 3, 1, 1, 7, 2, 4]]:
        want = [x for x in s if x in keep] == seq
        assert w.accepts(s) == want, s
        n_acc += want
    assert n_acc >= 1
    assert WideDFA.projected_sequence(8, keep, []).accepts([0, 3, 4]) and not WideDFA.projected_sequence(8, keep, []).accepts([1])
    with pytest.raises(ValueError):
        WideDFA.projected_sequence(8, keep, [3])


def test_bigram():
    logp, start = torch.randn(5, 5), torch.randn(5)
    w = WideDFA.bigram(logp, start)
    assert w.n_states == 6 and w.vocab == 5 and w.weighted
    s = [3, 0, 0, 4, 1]
    assert w.accepts(s) and w.run(s) == 2 and not w.accepts([])
    q = torch.tensor([0, 4, 1, 1, 5])  # the states in front of every label of s
    got = w.arc_weights(q, torch.tensor(s), 5)
    want = torch.stack([start[3], logp[3, 0], logp[0, 0], logp[0, 4], logp[4, 1]])
    assert torch.equal(got, want)
    assert torch.equal(WideDFA.bigram(logp).arc_weights(torch.tensor([0]), torch.tensor([2]), 5), torch.zeros(1))


def test_stack_is_ragged():
    parts = [WideDFA.accept_all(V), WideDFA.sequence(V, [5, 6, 7]), WideDFA.marked_sequence(V, 4, list(range(10, 50)))]
    w = WideDFA.stack(parts)
    assert w.n_lattices == 3 and w.n_states == 82 and list(w.q_off) == [0, 1, 5, 87]
    assert w.dflt.size == 87 and w.exc_label.size == 0 + 3 + 81  # no padding
    for b, (d, f) in enumerate(w.to_dense()):
        d0, f0 = parts[b].to_dense()
        assert np.array_equal(d, d0) and np.array_equal(f, f0)
    assert w.accepts([5, 6, 7], b=1) and not w.accepts([5, 6, 7], b=2) and w.accepts([9, 9], b=0)
    w.check(V, 3)
    with pytest.raises(ValueError):
        w.check(V, 4)
    with pytest.raises(ValueError):
        WideDFA.stack([w, w])  # already per-lattice
    with pytest.raises(ValueError):
        WideDFA.stack([WideDFA.accept_all(V), WideDFA.accept_all(V + 1)])
    with pytest.raises(ValueError):
        WideDFA.stack([WideDFA.accept_all(5), WideDFA.bigram(torch.zeros(5, 5))])  # weighted beside unweighted
    with pytest.raises(ValueError):
        WideDFA.stack([])


def test_device_arrays_are_cached():
    w = WideDFA.accept_all(V)
    t = w.to("cpu")
    assert w.to("cpu") is t and [x.dtype for x in t] == [torch.int32] * 5 + [torch.uint8]
    assert t[3].numel() == 1 and t[4].numel() == 1  # (valid pointers although there is no exception)


# ----------------------------------------------------------------------------- validation
def test_every_validation_error():
    ok = dict(dflt=[0, -1], exc_off=[0, 1, 2], exc_label=[3, 5], exc_dst=[1, 0], final=[0, 1])
    WideDFA(**ok)

    def bad(**kw):
        with pytest.raises(ValueError):
            WideDFA(**{**ok, **kw})

    bad(dflt=[0, 2])                 # a default outside -1 .. Q-1
    bad(dflt=[0, -2])
    bad(exc_dst=[1, 2])              # an exception's target outside
    bad(exc_dst=[-2, 0])
    bad(exc_label=[3, -1])           # a negative label
    bad(exc_off=[0, 2, 2], exc_label=[5, 3])  # descending inside a state
    bad(exc_off=[0, 2, 2], exc_label=[5, 5])  # a repeated label
    bad(exc_off=[0, 1])              # too short
    bad(exc_off=[1, 1, 2])           # does not start at 0
    bad(exc_off=[0, 2, 1])           # not ascending
    bad(exc_off=[0, 1, 3])           # beyond the exceptions
    bad(exc_dst=[1])                 # lengths differ
    bad(final=[1])
    bad(dflt=[0.5, 0.0])             # not integers
    bad(q_off=[0, 1])                # does not end at the number of states
    bad(q_off=[1, 2])
    bad(q_off=[0, 0, 2])             # an automaton without a state
    bad(q_off=[0, 1, 2])             # state 0's exception leads to state 1 of a one-state automaton
    bad(vocab=5)                     # label 5 with five labels
    bad(weight_dflt=torch.zeros(2))  # one weight tensor without the other
    bad(weight_dflt=torch.zeros(2), weight_exc=torch.zeros(3))
    bad(weight_dflt=torch.zeros(2, dtype=torch.int64), weight_exc=torch.zeros(2))
    WideDFA(**ok, weight_dflt=torch.zeros(2), weight_exc=torch.zeros(2))
    n = MAX_WIDE_STATES + 1
    with pytest.raises(ValueError, match="4096"):
        WideDFA(np.zeros(n, int), np.zeros(n + 1, int), [], [], np.ones(n))
    with pytest.raises(ValueError):
        WideDFA([], [0], [], [], [])
    WideDFA(np.zeros(n - 1, int), np.zeros(n, int), [], [], np.ones(n - 1))
    # labels beyond the batch's vocabulary are refused at check()
    w = WideDFA(**ok)
    w.check(6, 3)
    with pytest.raises(ValueError):
        w.check(5, 3)
    with pytest.raises(ValueError):
        WideDFA.sequence(V, [1, 2]).check(V + 1, 3)  # another vocabulary
    with pytest.raises(ValueError):
        WideDFA.sequence(V, [V])
    with pytest.raises(ValueError):
        WideDFA.sequence(V, list(range(3)) * 1366)  # 4098 labels
    with pytest.raises(ValueError):
        WideDFA.marked_sequence(V, 4, [1] * 2048)
    with pytest.raises(ValueError):
        WideDFA.marked_sequence(V, V, [1])
    with pytest.raises(ValueError):
        WideDFA.bigram(torch.zeros(3, 4))
    with pytest.raises(ValueError):
        WideDFA.bigram(torch.zeros(3, 3), torch.zeros(4))
    with pytest.raises(ValueError):
        WideDFA.from_dense(np.array([[0, 1]]), [1])
    with pytest.raises(ValueError):
        w.to_dense()  # no vocabulary known
    assert w.to_dense(6)[0].shape == (2, 6)


# ----------------------------------------------------------------------------- the vectorised restatement
def _small_lattices():
    return [
        synth.layered_lattice(3, n_states=30, avg_degree=3.0, vocab=V, width=4, span=2),
        synth.edit_lattice([10, 11, 12, 13, 14], [20, 21, 22, 23], vocab=V, seed=2),
        synth.edit_lattice([10, 11, 12], [20, 21, 20], vocab=V, seed=5),
    ]


def _small_automata():
    return {
        "accept_all": ConstraintDFA.accept_all(V), "count_at_most": ConstraintDFA.count_at_most(V, [5], 1),
        "count_many": ConstraintDFA.count_at_most(V, range(3, 30), 4), "forbid_bigram": ConstraintDFA.forbid_bigram(V, 3, 10),
        "parity": ConstraintDFA.parity(V, range(3, 34)), "contains": ConstraintDFA.contains(V, [4, 20]),
        "marked_sequence": ConstraintDFA.marked_sequence(V, 4, [20, 21, 20]), "reject_all": ConstraintDFA(np.full((1, V), -1), [1]),
    }


@pytest.mark.parametrize("name", sorted(_small_automata()))
def test_vectorised_restatement_equals_the_python_one(name):
    c = _small_automata()[name]
    some = 0
    for l in _small_lattices():
        a, b = R.intersect(l, c.delta, c.final), RW.intersect(l, *WideDFA.from_constraint(c).to_dense())
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]) and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype, (name, k)
        some += a["n_rows"]
    assert (some > 0) == (name != "reject_all")


def test_the_gpu_tests_numerator_grid_stays_under_the_row_limit():
    """The denominator grid of tests/test_gpu_intersect_wide.py (|x| = 12, four output symbols, at most 40 of them) and
    its product with marked_sequence(y), |y| = 40, by the restatement: both under 8192 rows, and the product is the
    machine of synth.edit_lattice(x, y) row for row and arc for arc."""
    from tests import test_gpu_intersect_wide as G

    den, dfa = G._headline()
    assert den.n_rows == 3467 <= 8192 and dfa.n_states == 82
    ref = RW.intersect(den, *dfa.to_dense())
    num = synth.edit_lattice(list(G.X12), list(G.Y40), vocab=V)
    assert (ref["n_rows"], ref["n_arcs"]) == (num.n_rows, num.n_arcs) == (3467, 4427)
    assert sorted(ref["label"]) == sorted(num.label)


# ----------------------------------------------------------------------------- IntersectResult.scores on CPU tensors
@pytest.mark.parametrize("per_lattice", [False, True])
def test_scores_look_the_weights_up_as_a_dense_gather_does(per_lattice):
    rng = np.random.default_rng(5)
    lats = _small_lattices()
    lat = LatticeBatch.from_synth(lats)  # on the host: scores() is torch only
    parts, dense_w = [], []
    for b in range(3 if per_lattice else 1):
        Q = 3 + 2 * b
        delta = rng.integers(-1, Q, size=(Q, V))
        delta[:, rng.random(V) < 0.7] = 0  # (mostly the default)
        base = WideDFA.from_dense(delta, np.ones(Q))
        wd, we = torch.randn(Q, requires_grad=True), torch.randn(base.exc_label.size, requires_grad=True)
        parts.append(WideDFA(base.dflt, base.exc_off, base.exc_label, base.exc_dst, base.final, weight_dflt=wd, weight_exc=we, vocab=V))
        dw = wd.detach()[:, None].repeat(1, V)
        dw[torch.from_numpy(base._state_of), torch.from_numpy(base.exc_label.astype(np.int64))] = we.detach()
        dense_w.append(dw)
    dfa = WideDFA.stack(parts) if per_lattice else parts[0]
    if per_lattice:  # (stack concatenates the weights: leaves of their own)
        dfa.weight_dflt, dfa.weight_exc = dfa.weight_dflt.detach().requires_grad_(True), dfa.weight_exc.detach().requires_grad_(True)
    arc_b = lat.arc_lattice()
    q_hi = torch.tensor([p.n_states for p in parts])[arc_b if per_lattice else torch.zeros_like(arc_b)]
    arc_q = (torch.from_numpy(rng.integers(0, 1 << 30, lat.total_arcs)) % q_hi).to(torch.int32)
    res = IntersectResult(lat, torch.arange(lat.total_arcs), arc_q, None, None, dfa)
    asc = torch.randn(lat.total_arcs)
    got = res.scores(asc)
    lab = lat.arc_label.to(torch.int64)
    want = asc + torch.stack([dense_w[int(b) if per_lattice else 0][int(q), int(l)] for b, q, l in zip(arc_b, arc_q, lab)])
    assert got.dtype == torch.float32 and torch.equal(got, want)
    got.sum().backward()  # every arc's gradient lands on the entry it was gathered from
    n_exc, n_dflt = int(dfa.weight_exc.grad.sum()), int(dfa.weight_dflt.grad.sum())
    assert n_exc > 0 and n_dflt > 0 and n_exc + n_dflt == lat.total_arcs
    assert torch.equal(IntersectResult(lat, torch.arange(lat.total_arcs), arc_q, None, None, WideDFA.accept_all(V)).scores(asc), asc)


def test_scores_of_an_automaton_without_a_vocabulary_on_labels_beyond_its_exceptions():
    """The stride of the lookup key is the BATCH's vocabulary: a hand-built automaton (no ``vocab``) whose largest
    exception label is 1, on arcs with labels up to V - 1, against the dense gather.  With the stride taken from the
    automaton, label 3 in state 0 would land on state 1's exception."""
    wd, we = torch.tensor([10.0, 20.0], requires_grad=True), torch.tensor([1.0, 2.0], requires_grad=True)
    dfa = WideDFA([0, 1], [0, 1, 2], [1, 1], [1, 0], [1, 1], weight_dflt=wd, weight_exc=we)
    assert dfa.vocab is None
    dfa.check(8, 1)
    got = dfa.arc_weights(torch.tensor([0, 0, 0, 1]), torch.tensor([0, 1, 3, 3]), 8)
    assert got.tolist() == [10.0, 1.0, 10.0, 20.0]
    with pytest.raises(ValueError):
        dfa.arc_weights(torch.tensor([0]), torch.tensor([0]), 1)  # a vocabulary below the automaton's own labels
    # through IntersectResult.scores on a host batch, every (state, label) pair of the batch
    lat = LatticeBatch.from_synth(_small_lattices())
    rng = np.random.default_rng(6)
    arc_q = torch.from_numpy(rng.integers(0, 2, lat.total_arcs)).to(torch.int32)
    res = IntersectResult(lat, torch.arange(lat.total_arcs), arc_q, None, None, dfa)
    got = res.scores()
    dense = wd.detach()[:, None].repeat(1, V)
    dense[0, 1], dense[1, 1] = 1.0, 2.0
    lab = lat.arc_label.to(torch.int64)
    assert int(lab.max()) > 1 and torch.equal(got, dense[arc_q.to(torch.int64), lab])
    got.sum().backward()
    n1 = lab == 1
    assert we.grad.tolist() == [float((n1 & (arc_q == 0)).sum()), float((n1 & (arc_q == 1)).sum())]
    assert wd.grad.tolist() == [float((~n1 & (arc_q == 0)).sum()), float((~n1 & (arc_q == 1)).sum())]
    assert dfa._score_keys(lab.device, V)[0] is dfa._score_keys(lab.device, V)[0]  # built once per device and vocabulary


# ----------------------------------------------------------------------------- the C entry points
NAMES = ("nfst_intersect_wide_ws_bytes", "nfst_intersect_wide_count", "nfst_intersect_wide_write")


def test_lib_and_header_declare_the_three_entry_points_at_abi_7():
    from nfst_amd import _lib

    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nfst_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert hasattr(_lib.lib, name) and getattr(_lib.lib, name).argtypes is not None and name in _lib.EXPORTS
        assert re.search(r"^int(64_t)? " + name + r"\(const nfst_batch \*lat,", header, re.M), name
    assert _lib.ABI_VERSION == 7 and _lib.lib.nfst_abi_version() == 7


def test_argument_checks_return_before_any_launch():
    from nfst_amd import _lib

    lat = LatticeBatch.from_synth(_small_lattices())  # host-packed: the checks run before anything touches a device
    assert lat.device.type == "cpu"
    lib = _lib.lib
    bs = C.byref(lat.c_struct())
    B, Q = lat.n_lattices, 130
    assert lib.nfst_intersect_wide_ws_bytes(bs, 0) == ERR_ARG
    assert lib.nfst_intersect_wide_ws_bytes(bs, 4097) == ERR_LIMIT
    assert lib.nfst_intersect_wide_ws_bytes(None, Q) == ERR_ARG
    ws_bytes = lib.nfst_intersect_wide_ws_bytes(bs, Q)
    assert ws_bytes >= lat.total_rows * (16 * 3 + 12) + B * 8 * 8192  # W = 3
    assert lib.nfst_intersect_wide_ws_bytes(bs, 4096) >= lat.total_rows * 16 * 64 > ws_bytes
    assert lib.nfst_intersect_wide_ws_bytes(bs, 128) < ws_bytes == lib.nfst_intersect_wide_ws_bytes(bs, 192)
    ws = np.zeros(ws_bytes // 8 + 2, np.float64)  # (16-byte aligned by numpy)
    a32 = np.zeros(Q + 1, np.int32)
    fin = np.ones(Q, np.uint8)
    counts, status = np.full((B, 2), 77, np.int32), np.full(B, 77, np.int32)
    off = np.zeros(B, np.int64)
    i32, i64 = np.full(8, 77, np.int32), np.full(8, 77, np.int64)
    p = lambda a: None if a is None else a.ctypes.data
    auto = ("q_off", "dflt", "exc_off", "exc_label", "exc_dst", "fin")

    def count(q=Q, n_dfa=1, q_off=a32, dflt=a32, exc_off=a32, exc_label=a32, exc_dst=a32, fin=fin, ws=ws, wsb=ws_bytes, counts=counts,
              status=status, lat=bs):
        return lib.nfst_intersect_wide_count(lat, p(q_off), p(dflt), p(exc_off), p(exc_label), p(exc_dst), p(fin), n_dfa, q, p(ws), wsb,
                                             p(counts), p(status), None)

    def write(q=Q, n_dfa=1, q_off=a32, dflt=a32, exc_off=a32, exc_label=a32, exc_dst=a32, fin=fin, ws=ws, wsb=ws_bytes, roff=off,
              aoff=off, src=i32, label=i32, dst=i32, arc_map=i64, arc_q=i32, row_state=i32, row_q=i32, lat=bs):
        return lib.nfst_intersect_wide_write(lat, p(q_off), p(dflt), p(exc_off), p(exc_label), p(exc_dst), p(fin), n_dfa, q, p(ws), wsb,
                                             p(roff), p(aoff), p(src), p(label), p(dst), p(arc_map), p(arc_q), p(row_state), p(row_q), None)

    for fn in (count, write):
        assert fn(4097) == ERR_LIMIT
        assert fn(0) == ERR_ARG and fn(-1) == ERR_ARG
        for name in auto:
            assert fn(**{name: None}) == ERR_ARG, name
        assert fn(n_dfa=0) == ERR_ARG and fn(n_dfa=2) == ERR_ARG and fn(n_dfa=B + 1) == ERR_ARG
        assert fn(ws=None) == ERR_ARG
        assert fn(wsb=ws_bytes - 1) == ERR_ARG
        assert fn(q=193) == ERR_ARG  # (four words per state: the workspace is short)
        assert fn(lat=None) == ERR_ARG
    assert count(counts=None) == ERR_ARG and count(status=None) == ERR_ARG
    for name in ("roff", "aoff", "src", "label", "dst", "arc_map", "arc_q", "row_state", "row_q"):
        assert write(**{name: None}) == ERR_ARG, name
    # nothing was launched: every output is as it was
    assert (counts == 77).all() and (status == 77).all() and (i32 == 77).all() and (i64 == 77).all() and not ws.any()


def test_a_host_batch_raises_as_the_other_ops_do():
    from nfst_amd import ops

    lat = LatticeBatch.from_synth(_small_lattices())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.intersect(lat, WideDFA.accept_all(V))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.constraint_log_prob(lat, torch.zeros(V), WideDFA.accept_all(V))

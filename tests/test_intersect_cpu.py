"""The product of a lattice with a constraint automaton: the pure-Python restatement (tests/intersect_ref.py) that the
GPU tests of ops.intersect rely on, checked against path enumeration, the oracle's log Z and the host packer; the
automaton builders of nfst_amd.constraints; the C entry points' argument checks (host side, before any launch)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from nfst_amd import synth
from nfst_amd.constraints import ConstraintDFA
from nfst_amd.lattice import LatticeBatch
from oracle import oracle as O
from tests import intersect_ref as R
from tests import kbest_ref as K

V = 64
ERR_ARG, ERR_LIMIT = -1, -6  # (include/nfst_hip.h)


def _small_lattices():
    return [
        synth.layered_lattice(3, n_states=30, avg_degree=3.0, vocab=V, width=4, span=2),
        synth.edit_lattice([10, 11, 12, 13, 14], [20, 21, 22, 23], vocab=V, seed=2),
        synth.edit_lattice([10, 11, 12], [20, 21, 20], vocab=V, seed=5),
    ]


N_PATHS = (3267, 681, 63)


def _automata():
    return {
        "accept_all": ConstraintDFA.accept_all(V),
        "count_at_most": ConstraintDFA.count_at_most(V, [5], 1),
        "count_many": ConstraintDFA.count_at_most(V, range(3, 30), 4),
        "forbid_bigram": ConstraintDFA.forbid_bigram(V, 3, 10),
        "parity": ConstraintDFA.parity(V, range(3, 34)),
        "contains": ConstraintDFA.contains(V, [4, 20]),
        "marked_sequence": ConstraintDFA.marked_sequence(V, 4, [20, 21, 20]),
    }


_PATHS = {}


def _paths(i):
    """(label tuple, arc tuple) of every path of small lattice i, computed once."""
    if i not in _PATHS:
        l = _small_lattices()[i]
        ps = K.enumerate_paths(l.n_rows, l.src, l.dst, np.zeros(l.n_arcs), l.n_rows - 1)
        _PATHS[i] = (l, [(tuple(int(x) for x in l.label[p]), tuple(p)) for _, p in ps])
    return _PATHS[i]


@pytest.mark.parametrize("i", range(3))
def test_small_lattices_have_the_stated_path_counts(i):
    assert len(_paths(i)[1]) == N_PATHS[i]


@pytest.mark.parametrize("name", list(_automata()))
@pytest.mark.parametrize("i", range(3))
def test_reference_product_equals_the_accepted_paths(i, name):
    l, paths = _paths(i)
    dfa = _automata()[name]
    accepted = [(labs, arcs) for labs, arcs in paths if dfa.accepts(labs)]
    assert all(dfa.accepts(labs) == R.run(dfa.delta, dfa.final, labs) for labs, _ in paths[:50])
    p = R.intersect(l, dfa.delta, dfa.final)
    got = R.product_paths(p)
    # one product path per accepted path: the same label sequences, over the same lattice arcs
    assert len(got) == len(accepted)
    assert sorted(got) == sorted(accepted)
    if not accepted:
        assert p["n_rows"] == 0 and p["n_arcs"] == 0
        return
    assert p["row_state"][0] == 0 and p["row_q"][0] == 0
    # sorted by (src, label), deterministic, trim: every row has an arc out and (but row 0) an arc in
    key = p["src"].astype(np.int64) * V + p["label"]
    assert np.all(np.diff(key) > 0)
    assert set(p["src"]) == set(range(p["n_rows"])) and set(p["dst"]) | {0} == set(range(p["n_rows"]))
    assert np.array_equal(l.label[p["arc_map"]], p["label"])
    assert np.array_equal(p["row_state"][p["src"]], l.src[p["arc_map"]])
    assert np.array_equal(p["row_state"][p["dst"]], l.dst[p["arc_map"]])
    # the oracle's float64 log Z of the product = the log-sum over the accepted paths
    theta = synth.label_scores(7, V).astype(np.float64)
    s64 = theta[p["label"]]
    o = O.forward_backward(p["n_rows"], p["src"], p["dst"], s64)
    want = np.logaddexp.reduce([theta[list(labs)].sum() for labs, _ in accepted])
    assert abs(o["logZ"] - want) <= 1e-9
    # the host packer keeps every arc and every row
    lat = LatticeBatch.from_arcs(np.array([p["n_rows"]], np.int32), np.array([0, p["n_arcs"]], np.int64), p["src"], p["label"],
                                 p["dst"], V)
    lat.validate()
    assert lat.total_arcs == p["n_arcs"] and lat.total_rows == p["n_rows"]
    assert int(lat.meta_host[0, 9]) == p["n_rows"] and int(lat.sink[0]) == p["n_rows"] - 1  # (NFST_META_N_REACH)
    for k in ("src", "label", "dst"):
        assert np.array_equal(lat._t["arc_" + k].numpy(), p[k])


def test_marked_sequence_is_the_identity_on_its_own_edit_lattice_and_empty_on_another():
    x, y = [10, 11, 12], [20, 21, 20]
    l = synth.edit_lattice(x, y, vocab=V, seed=5)
    dfa = ConstraintDFA.marked_sequence(V, 4, y)
    assert dfa.n_states == 2 * (len(y) + 1)
    p = R.intersect(l, dfa.delta, dfa.final)
    assert p["n_rows"] == l.n_rows and p["n_arcs"] == l.n_arcs
    assert np.array_equal(p["src"], l.src) and np.array_equal(p["label"], l.label) and np.array_equal(p["dst"], l.dst)
    assert np.array_equal(p["arc_map"], np.arange(l.n_arcs)) and np.array_equal(p["row_state"], np.arange(l.n_rows))
    for other in ([20, 21, 21], [20, 21], [20, 21, 20, 20]):
        d2 = ConstraintDFA.marked_sequence(V, 4, other)
        q = R.intersect(l, d2.delta, d2.final)
        assert q["n_rows"] == 0 and q["n_arcs"] == 0


def test_contains_against_brute_force_search():
    rng = np.random.default_rng(0)
    for trial in range(60):
        n = int(rng.integers(1, 5))
        seq = [int(x) for x in rng.integers(0, 3, size=n)]
        dfa = ConstraintDFA.contains(4, seq)
        assert dfa.n_states == n + 1
        for _ in range(40):
            s = [int(x) for x in rng.integers(0, 3, size=int(rng.integers(0, 12)))]
            want = any(s[i:i + n] == seq for i in range(len(s) - n + 1))
            assert dfa.accepts(s) == want, (seq, s)


def test_builders_on_short_strings():
    for s in itertools.product(range(4), repeat=5):
        assert ConstraintDFA.accept_all(4).accepts(s)
        assert ConstraintDFA.count_at_most(4, [1, 2], 2).accepts(s) == (sum(x in (1, 2) for x in s) <= 2)
        assert ConstraintDFA.forbid_bigram(4, 1, 3).accepts(s) == all((a, b) != (1, 3) for a, b in zip(s, s[1:]))
        assert ConstraintDFA.forbid_bigram(4, 2, 2).accepts(s) == all((a, b) != (2, 2) for a, b in zip(s, s[1:]))
        assert ConstraintDFA.parity(4, [0, 3]).accepts(s) == (sum(x in (0, 3) for x in s) % 2 == 0)
        follow = [b for a, b in zip(s, s[1:]) if a == 0] if s[-1] != 0 else None
        assert ConstraintDFA.marked_sequence(4, 0, [1, 2]).accepts(s) == (follow == [1, 2])


def test_stack_pads_to_a_common_size():
    a, b = ConstraintDFA.parity(V, [5]), ConstraintDFA.count_at_most(V, [5], 3)
    st = ConstraintDFA.stack([a, b])
    assert st.n_lattices == 2 and st.n_states == 4 and st.vocab == V
    for s in ([5, 5, 6], [5], [5, 5, 5, 5, 7]):
        assert st.accepts(s, 0) == a.accepts(s) and st.accepts(s, 1) == b.accepts(s)
    wa = ConstraintDFA(a.delta, a.final, torch.zeros(2, V))
    with pytest.raises(ValueError):
        ConstraintDFA.stack([wa, b])
    with pytest.raises(ValueError):
        ConstraintDFA.stack([a, ConstraintDFA.parity(V + 1, [5])])


def test_device_layout_is_label_major():
    dfa = ConstraintDFA.stack([ConstraintDFA.count_at_most(V, [5, 6], 40), ConstraintDFA.parity(V, [7])])
    t, mask = dfa.to("cpu")
    assert t.dtype == torch.int8 and tuple(t.shape) == (2, V, 64) and mask.dtype == torch.int64 and tuple(mask.shape) == (2,)
    assert np.array_equal(t.numpy()[:, :, :41], np.swapaxes(dfa.delta, 1, 2)) and bool((t[:, :, 41:] == -1).all())
    assert int(mask[0]) == (1 << 41) - 1 and int(mask[1]) == 1
    assert dfa.to("cpu")[0] is t  # cached
    full = ConstraintDFA.count_at_most(V, [5], 63)
    assert int(full.to("cpu")[1][0]) == -1  # all 64 bits


def test_validation_errors():
    ok = np.zeros((2, V), np.int64)
    ConstraintDFA(ok, [1, 0])
    bad = ok.copy()
    bad[1, 3] = 2
    for delta, final in ((bad, [1, 0]), (-2 * np.ones((2, V), np.int64), [1, 0]), (np.zeros((65, V), np.int64), np.ones(65)),
                         (np.zeros((0, V), np.int64), np.ones(0)), (ok, [1, 0, 1]), (np.zeros(V, np.int64), 1),
                         (np.zeros((2, V)), [1, 0])):
        with pytest.raises(ValueError):
            ConstraintDFA(delta, final)
    with pytest.raises(ValueError):
        ConstraintDFA(ok, [1, 0], weight=torch.zeros(3, V))
    with pytest.raises(ValueError):
        ConstraintDFA.count_at_most(V, [V], 1)
    with pytest.raises(ValueError):
        ConstraintDFA.count_at_most(V, [5], 64)
    with pytest.raises(ValueError):
        ConstraintDFA.marked_sequence(V, 4, list(range(3, 35)))
    with pytest.raises(ValueError):  # wrong vocabulary / wrong number of automata for the batch
        ConstraintDFA.parity(V, [5]).check(V + 1, 3)
    with pytest.raises(ValueError):
        ConstraintDFA.stack([ConstraintDFA.parity(V, [5])] * 2).check(V, 3)


# ----------------------------------------------------------------------------- the C entry points
def test_lib_declares_and_exports_the_new_symbols():
    from nfst_amd import _lib

    for name in ("nfst_intersect_ws_bytes", "nfst_intersect_count", "nfst_intersect_write"):
        assert hasattr(_lib.lib, name)
        assert getattr(_lib.lib, name).argtypes is not None
        assert name in _lib.EXPORTS


def test_argument_checks_return_before_any_launch():
    from nfst_amd import _lib

    lats = _small_lattices()
    lat = LatticeBatch.from_synth(lats)  # host-packed: the checks run before anything touches a device
    assert lat.device.type == "cpu"
    lib = _lib.lib
    bs = C.byref(lat.c_struct())
    B, Q = lat.n_lattices, 3
    assert lib.nfst_intersect_ws_bytes(bs, 0) == ERR_ARG
    assert lib.nfst_intersect_ws_bytes(bs, 65) == ERR_LIMIT
    assert lib.nfst_intersect_ws_bytes(None, Q) == ERR_ARG
    ws_bytes = lib.nfst_intersect_ws_bytes(bs, Q)
    assert ws_bytes >= lat.total_rows * 24 + B * 8 * 8192
    ws = np.zeros(ws_bytes // 8 + 2, np.float64)  # (16-byte aligned by numpy)
    delta = np.full((B, V, 64), -1, np.int8)
    fin = np.ones(B, np.uint64)
    counts, status = np.zeros((B, 2), np.int32), np.zeros(B, np.int32)
    off = np.zeros(B, np.int64)
    i32, i64 = np.zeros(8, np.int32), np.zeros(8, np.int64)
    p = lambda a: None if a is None else a.ctypes.data

    def count(q=Q, delta=delta, ds=0, fin=fin, fs=0, ws=ws, wsb=ws_bytes, counts=counts, status=status, lat=bs):
        return lib.nfst_intersect_count(lat, p(delta), ds, p(fin), fs, q, p(ws), wsb, p(counts), p(status), None)

    assert count(0) == ERR_ARG
    assert count(-1) == ERR_ARG
    assert count(65) == ERR_LIMIT
    assert count(delta=None) == ERR_ARG
    assert count(fin=None) == ERR_ARG
    assert count(ds=V * 64 - 1) == ERR_ARG
    assert count(ds=-1) == ERR_ARG
    assert count(fs=-1) == ERR_ARG
    assert count(ws=None) == ERR_ARG
    assert count(wsb=ws_bytes - 1) == ERR_ARG
    assert count(counts=None) == ERR_ARG
    assert count(status=None) == ERR_ARG
    assert count(lat=None) == ERR_ARG

    def write(q=Q, delta=delta, ds=0, ws=ws, wsb=ws_bytes, roff=off, aoff=off, src=i32, label=i32, dst=i32, arc_map=i64,
              arc_q=i32, row_state=i32, row_q=i32, lat=bs):
        return lib.nfst_intersect_write(lat, p(delta), ds, q, p(ws), wsb, p(roff), p(aoff), p(src), p(label), p(dst), p(arc_map),
                                        p(arc_q), p(row_state), p(row_q), None)

    assert write(0) == ERR_ARG
    assert write(65) == ERR_LIMIT
    assert write(delta=None) == ERR_ARG
    assert write(ds=5) == ERR_ARG
    assert write(ws=None) == ERR_ARG
    assert write(wsb=ws_bytes - 1) == ERR_ARG
    assert write(lat=None) == ERR_ARG
    for name in ("roff", "aoff", "src", "label", "dst", "arc_map", "arc_q", "row_state", "row_q"):
        assert write(**{name: None}) == ERR_ARG, name


def test_a_host_batch_raises_as_the_other_ops_do():
    from nfst_amd import ops

    lat = LatticeBatch.from_synth(_small_lattices())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.intersect(lat, ConstraintDFA.accept_all(V))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lat.intersect(ConstraintDFA.accept_all(V))

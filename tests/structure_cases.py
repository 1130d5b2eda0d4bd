"""Lattices with the structure the engine promises to take and ``nfst_amd.synth`` never builds (test helper, not a test
module; pure numpy on tests/pack_cases.py): a sink that is not the last row, reachable states above it, self loops at
inner states, at state 0 and at the edges of a state's 64-arc chunks, unreachable rows below and above reachable ones
(so that canonical arc ids differ from the caller's), a lattice whose state 0 is the sink.

``entries()`` is the corpus, every entry named after the thing it exists for; ``features`` evaluates the structural
predicates on ``pack_cases.analyse``; ``batches()`` deals the corpus into the few batches the GPU tests launch on
(weighted and unweighted lattices do not share a batch; one vocabulary per batch).  The references of tests/*_ref.py
take one lattice in the engine's numbering: ``canonical(l)`` is the lattice with the arcs of unreachable states dropped
(``pack_cases.reachable_arcs``), over the same rows.

Every lattice has at most a few dozen paths, except the ``self_loop_in_chunks`` ones: a state with 129 arcs that leave it
lies on at least 129 paths (still instant to enumerate).  tests/test_structure_cpu.py holds the corpus to its claims and
every reference to plain enumeration on it; tests/test_gpu_structure.py holds the path-side ops to those references.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np

from tests import pack_cases as PC
from tests.expectation_ref import sink_of

F32 = np.float32
PAD, BOS, EOS = PC.PAD, PC.BOS, PC.EOS
V = 140           # one vocabulary for every entry but many_with_junk (labels 3 .. 132 leave the 130-arc states)
HI = 9            # the label of highest score: the self loops of self_loop_only_alternative carry it
CHUNK = 64        # arcs that the path-side kernels deal to the lanes of a wave in one trip
DEGREE = 130      # out-arcs of the chunked state: three chunks
CHUNK_POSITIONS = (0, 63, 64, 129)

# every structural feature that the corpus must cover (test_structure_cpu.py: the union over the corpus)
FEATURES = (
    "sink_not_last",                # the sink is not row n_rows - 1
    "reachable_above_sink",         # a reachable state has an id above the sink's
    "inner_self_loop",              # a self loop at a reachable state that is neither state 0 nor the sink
    "self_loop_at_0",               # a self loop at state 0 (which is not the sink)
    "self_loop_at_chunk_edge",      # a self loop first or last in a 64-arc chunk of a state with more than 64 arcs
    "unreachable_below_reachable",  # an unreachable row below a reachable one
    "unreachable_above_reachable",  # an unreachable row above every reachable one (padding behind the lattice)
    "arc_ids_shifted",              # a dropped arc in front of a kept one: canonical ids differ from the caller's
    "state0_is_sink",               # the one path is the empty path
)


def features(l) -> set:
    a = PC.analyse(l)
    assert len(a["sinks"]) == 1 and a["acyclic"], "not a lattice the packers take"
    sink, reach = a["sinks"][0], a["reach"]
    ids = np.flatnonzero(reach)
    got = set()
    if sink != l.n_rows - 1:
        got.add("sink_not_last")
    if ids.max() > sink:
        got.add("reachable_above_sink")
    src, dst = l.src[a["canon"]], l.dst[a["canon"]]
    loops = np.flatnonzero(src == dst)
    if np.any((src[loops] != 0) & (src[loops] != sink)):
        got.add("inner_self_loop")
    if np.any(src[loops] == 0) and sink != 0:
        got.add("self_loop_at_0")
    first = np.searchsorted(src, np.arange(l.n_rows + 1))
    for k in loops:
        s = int(src[k])
        deg, p = int(first[s + 1] - first[s]), int(k - first[s])
        if deg > CHUNK and (p % CHUNK in (0, CHUNK - 1) or p == deg - 1):
            got.add("self_loop_at_chunk_edge")
    unreach = np.flatnonzero(~reach)
    if unreach.size and unreach.min() < ids.max():
        got.add("unreachable_below_reachable")
    if unreach.size and unreach.max() > ids.max():
        got.add("unreachable_above_reachable")
    if not np.array_equal(a["canon"], np.arange(len(a["canon"]))):
        got.add("arc_ids_shifted")
    if sink == 0:
        got.add("state0_is_sink")
    return got


@dataclasses.dataclass
class Entry:
    name: str
    lats: list             # the lattices of the entry (one batch: all weighted or none)
    features: frozenset    # what the entry is named after: its lattices have these between them (names of FEATURES)
    dense: Optional[tuple] = None  # (emission, transition) tables whose arcs the lattices spell out


# ---------------------------------------------------------------- helpers
def with_vocab(l, vocab=V, weight_seed=None):
    """``l`` over another vocabulary (its labels must fit), with fresh weights if asked for"""
    assert l.n_arcs == 0 or int(l.label.max()) < vocab
    w = l.weight
    if weight_seed is not None:
        w = np.random.default_rng(weight_seed).normal(-0.5, 0.7, size=l.n_arcs).astype(F32)
    return dataclasses.replace(l, vocab=int(vocab), weight=w)


def canonical(l):
    """The lattice as the engine numbers it: the arcs of the states that state 0 reaches, over the same rows."""
    src, label, dst, w = PC.reachable_arcs(l)
    return PC.Lat(l.n_rows, l.vocab, src, label, dst, w)


def sink(l) -> int:
    return sink_of(l.n_rows, l.src, l.dst)


def theta(vocab=V, seed=17) -> np.ndarray:
    """Label scores ~ N(-2.3, 0.5) with label HI far above every other, and positive: a path that took a self loop of
    that label would score higher than any real path."""
    t = np.random.default_rng(seed).normal(-2.3, 0.5, size=vocab).astype(F32)
    t[HI] = 1.5
    return t


def arcs_of_dense(em, tr) -> list:
    """The arc lists that one batch of dense tables spells out, rows of padding included: one Lat per lattice."""
    out = []
    for e, t in zip(em, tr):
        weighted = np.issubdtype(e.dtype, np.floating)
        r, v = np.nonzero(e > -np.inf) if weighted else np.nonzero(e)
        out.append(PC.Lat(int(e.shape[0]), int(e.shape[1]), r.astype(np.int32), v.astype(np.int32), t[r, v].astype(np.int32),
                          e[r, v].astype(F32) if weighted else None))
    return out


# ---------------------------------------------------------------- the new lattices
def _sink_below_reachable(weight_seed=None):
    # seven reachable rows, the sink is row 3: states 4, 5 and 6 lie above it
    return PC.make(7, V, [(0, BOS, 1), (1, 3, 2), (1, 4, 4), (2, 5, 5), (4, 5, 5), (4, 6, 6), (5, EOS, 3), (6, EOS, 3), (3, PAD, 3)],
                   weight_seed=weight_seed)


def _chunked(position: int, at_state_0: bool = False, weight_seed=None):
    """A hub with DEGREE out-arcs by the labels 3 .. 132, the arc at ``position`` of its sorted list a self loop; the
    others lead to two states in turn, which meet in one that ends the path.  The hub is state 1 behind a bos arc, or
    state 0 itself.  Row 2 is an unreachable dead end, so the sink is row 3 and every arc of the hub has another id in
    the packed batch than in the caller's list when junk sits in front (it owns one arc)."""
    hub = 0 if at_state_0 else 1
    a, b, meet, snk, junk = 4, 5, 6, 3, 2
    arcs = [] if at_state_0 else [(0, BOS, 1)]
    for p in range(DEGREE):
        arcs.append((hub, 3 + p, hub if p == position else (a, b)[p % 2]))
    arcs += [(a, 5, meet), (b, 6, meet), (b, 7, b), (meet, EOS, snk), (snk, PAD, snk), (junk, 3, a)]
    if at_state_0:
        arcs.append((1, 3, a))  # state 1 is unreachable here, and its arc sits right behind the hub's
    return PC.make(7, V, arcs, weight_seed=weight_seed)


def _self_loop_only_alternative(weight_seed=None):
    # states 1 and 2 carry a self loop by the label of highest score; the sink (row 5 of 7) has reachable row 6 above it
    l = PC.make(7, V, [(0, BOS, 1), (1, 3, 2), (1, 4, 4), (1, HI, 1), (2, 5, 6), (2, HI, 2), (4, 5, 6), (4, 6, 6), (6, EOS, 5), (5, PAD, 5)],
                weight_seed=weight_seed)
    if l.weight is not None:  # the loops' weights on top of their label: the highest of their states by far
        l.weight[l.src == l.dst] = 2.0
    return l


def _dense_pair(weighted: bool):
    """Two lattices of 7 and 5 rows collated as the scorer's loader does: the shorter one gets two rows of padding
    behind its sink.  Unweighted tables are padded with the id 6 (all-True rows whose arcs lead to row 6, a padding row
    itself), weighted ones with 0 (arcs of weight 0.0 into state 0)."""
    big = _sink_below_reachable(weight_seed=31 if weighted else None)
    small = PC.make(5, V, [(0, BOS, 1), (1, 3, 2), (1, 4, 3), (1, 8, 1), (2, 5, 3), (3, EOS, 4), (4, PAD, 4)], weight_seed=32 if weighted else None)
    from nfst_amd import synth
    return synth.collate_dense([big.dense(weighted=weighted), small.dense(weighted=weighted)], pad=0 if weighted else 6)


def one_row(weighted=False):
    return PC.Lat(1, V, *(np.zeros(0, np.int32) for _ in range(3)), np.zeros(0, F32) if weighted else None)


def no_arcs(weighted=False):
    return PC.Lat(3, V, *(np.zeros(0, np.int32) for _ in range(3)), np.zeros(0, F32) if weighted else None)


# ---------------------------------------------------------------- the corpus
def entries() -> dict:
    j = PC._junk_cases()
    c = PC.cases()
    f = frozenset
    em, tr = _dense_pair(False)
    em_w, tr_w = _dense_pair(True)
    out = [
        Entry("sink_below_reachable", [_sink_below_reachable()], f({"sink_not_last", "reachable_above_sink"})),
        Entry("sink_below_reachable_weighted", [_sink_below_reachable(21)], f({"sink_not_last", "reachable_above_sink"})),
        Entry("self_loop_in_chunks", [_chunked(p) for p in CHUNK_POSITIONS], f({"self_loop_at_chunk_edge", "inner_self_loop", "arc_ids_shifted"})),
        Entry("self_loop_in_chunks_at_0", [_chunked(64, at_state_0=True)], f({"self_loop_at_chunk_edge", "self_loop_at_0", "arc_ids_shifted"})),
        Entry("self_loop_in_chunks_weighted", [_chunked(63, weight_seed=22), _chunked(129, at_state_0=True, weight_seed=23)],
              f({"self_loop_at_chunk_edge", "arc_ids_shifted"})),
        Entry("self_loop_only_alternative", [_self_loop_only_alternative()], f({"inner_self_loop", "sink_not_last", "reachable_above_sink"})),
        Entry("self_loop_only_alternative_weighted", [_self_loop_only_alternative(24)], f({"inner_self_loop", "sink_not_last"})),
        Entry("pad_rows_behind_sink", arcs_of_dense(em, tr), f({"unreachable_above_reachable"}), dense=(em, tr)),
        Entry("pad_rows_behind_sink_weighted", arcs_of_dense(em_w, tr_w), f({"unreachable_above_reachable"}), dense=(em_w, tr_w)),
        Entry("one_row", [one_row()], f({"state0_is_sink"})),
        Entry("no_arcs", [no_arcs()], f({"state0_is_sink", "unreachable_above_reachable"})),
        # the entries of tests/pack_cases.py, over this corpus's vocabulary
        Entry("junk_acyclic", [with_vocab(j["junk_acyclic"])], f({"sink_not_last", "unreachable_above_reachable"})),
        Entry("junk_cycle", [with_vocab(j["junk_cycle"])], f({"sink_not_last", "unreachable_above_reachable"})),
        Entry("junk_self_loop", [with_vocab(j["junk_self_loop"])], f({"sink_not_last", "unreachable_above_reachable"})),
        Entry("junk_dead_end", [with_vocab(j["junk_dead_end"])], f({"sink_not_last", "unreachable_above_reachable"})),
        Entry("junk_low_ids", [with_vocab(j["junk_low_ids"])], f({"unreachable_below_reachable", "arc_ids_shifted"})),
        Entry("junk_weighted", [with_vocab(j["junk_weighted"])], f({"unreachable_below_reachable", "arc_ids_shifted"})),
        Entry("inner_self_loops", [with_vocab(l) for l in c["inner_self_loops"].lats], f({"inner_self_loop", "self_loop_at_0"})),
        Entry("inner_self_loops_weighted", [with_vocab(l) for l in c["inner_self_loops_weighted"].lats], f({"inner_self_loop", "self_loop_at_0"})),
    ]
    return {e.name: e for e in out}


def many_with_junk() -> list:
    """``pack_cases._many()``: 300 tiny lattices over 12 labels, a few of them with junk -- more than there are compute
    units, for the ops whose launch differs beyond one workgroup per compute unit."""
    return PC._many()


def batches() -> dict:
    """name -> lattices: the corpus dealt into the batches the GPU tests launch on.  ``one_row`` and ``no_arcs`` sit
    between ordinary members of the two big batches, and alone in a batch without any arc."""
    e = entries()
    plain = [l for x in e.values() for l in x.lats if l.weight is None and l.n_arcs and x.dense is None]
    heavy = [l for x in e.values() for l in x.lats if l.weight is not None and l.n_arcs and x.dense is None]
    plain = plain[:2] + [one_row()] + plain[2:5] + [no_arcs()] + plain[5:] + e["pad_rows_behind_sink"].lats  # (mixed_with_junk: the pair as arc lists)
    heavy = heavy[:1] + [no_arcs(True)] + heavy[1:3] + [one_row(True)] + heavy[3:] + e["pad_rows_behind_sink_weighted"].lats
    return {"unweighted": plain, "weighted": heavy, "zero_arcs": [no_arcs(), one_row(), no_arcs()], "many_with_junk": many_with_junk()}


def n_paths(l) -> int:
    from tests import kbest_ref
    c = canonical(l)
    return len(kbest_ref.enumerate_paths(c.n_rows, c.src, c.dst, np.zeros(c.n_arcs), sink(c)))

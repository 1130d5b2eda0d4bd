"""Random ragged batches for the path-side ops, products and pruned sub-lattices (test helper, not a test module; numpy on
tests/pack_cases.py, tests/structure_cases.py and the references of tests/*_ref.py).

``draw(seed, it)`` is a pure function of its two arguments: lattices from ``synth.layered_lattice`` with the parameter
ranges of tests/test_gpu_fuzz.py's ``_draw_batch`` and ``SIZES`` states, one member in four with a structural change
that tests/structure_cases.py spells by hand (the sink renumbered away from the last row, junk rows appended, an inner
self loop), one batch in eight with a member whose state 0 is the sink; label scores shared or per lattice, caller
scores, labels at -inf; the packing; the parameters of the ops; constraint automata.  The last iteration of every seed
draws more lattices than the device has compute units, of 4 .. 9 states each.  The lattices with their scores, the
strings and the automata come from three random streams of their own, so that a change to one leaves the others as they
are.  One leg is narrowed for the sake of a bound, and says why: ``LOG_PROB_K`` / ``LOG_PROB_MAGNITUDE``.

``derived(d)`` builds, from the references alone, the batches that ``ops.intersect`` and ``ops.prune`` must produce on
the draw: the product with an automaton, the pruned sub-lattice, the prune of the product and the product of the
product.  tests/test_fuzz_cases_cpu.py pins a digest of every draw and holds the corpus to its claims;
tests/test_gpu_fuzz_paths.py runs the ops on it.
"""
from __future__ import annotations

import dataclasses
import hashlib
from typing import Optional

import numpy as np

from nfst_amd import synth
from tests import intersect_ref, intersect_wide_ref, pack_cases as PC, slack_ref, structure_cases as S
from tests.expectation_ref import levels

F32 = np.float32
NEG = -np.inf
PAD, BOS, EOS = PC.PAD, PC.BOS, PC.EOS
SIZES = (4, 5, 6, 9, 17, 40, 65, 90, 130, 200, 257)
SMALL = (4, 5, 6, 9)
VOCABS = (24, 40, 256, 700)
KS = (1, 2, 7, 20, 64)                      # tests/test_gpu_kbest.py's KS
BEAMS = (0.0, 0.5, 3.0, float("inf"))       # tests/test_gpu_slack.py's BEAMS, taking turns per lattice
NARROW_Q = (1, 2, 5, 17, 64)
WIDE_Q = (65, 130, 300)
MAX_ROWS = PC.MAX_ROWS
N_CUS = PC.N_CUS
SEEDS = tuple(range(6))
ITERS = 4                                   # iterations per seed; the last one is the batch of more lattices than compute units
ENUMERABLE = 10_000                         # members with at most this many paths are held to enumeration
DERIVED_ROWS = 2048                         # the product that the derived legs run on has no member above this many rows


# ---------------------------------------------------------------- structural changes
def _sorted(n_rows, vocab, src, label, dst, w):
    order = np.lexsort((label, src))
    key = src[order].astype(np.int64) * vocab + label[order]
    assert np.all(np.diff(key) > 0), "not deterministic"
    return PC.Lat(int(n_rows), int(vocab), src[order].astype(np.int32), label[order].astype(np.int32), dst[order].astype(np.int32),
                  None if w is None else w[order].astype(F32))


def renumbered(l, rng):
    """The states 1 .. n - 1 permuted so that the sink is not the last row."""
    n = l.n_rows
    perm = np.arange(n, dtype=np.int64)
    perm[1:] = 1 + rng.permutation(n - 1)
    if perm[n - 1] == n - 1:  # (synth's sink is its last row)
        j = int(rng.integers(1, n - 1))
        perm[n - 1], perm[j] = perm[j], perm[n - 1]
    return _sorted(n, l.vocab, perm[l.src], l.label.astype(np.int64), perm[l.dst], l.weight)


def with_junk(l, rng):
    """One to three rows behind the lattice that state 0 does not reach: their arcs lead into the lattice, to each other
    and to themselves."""
    n, j = l.n_rows, int(rng.integers(1, 4))
    src, label, dst = [], [], []
    for s in range(n, n + j):
        labs = 3 + rng.choice(l.vocab - 3, size=int(rng.integers(0, 4)), replace=False)
        for lab in labs:
            src.append(s), label.append(int(lab)), dst.append(int(rng.integers(1, n + j)))
    w = None if l.weight is None else np.concatenate([l.weight, rng.normal(-0.5, 0.25, size=len(src)).astype(F32)])
    cat = lambda a, b: np.concatenate([np.asarray(a, np.int64), np.asarray(b, np.int64)])
    return _sorted(n + j, l.vocab, cat(l.src, src), cat(l.label, label), cat(l.dst, dst), w)


def with_self_loop(l, rng):
    """A self loop at an inner state (neither state 0 nor the sink), by a label that the state does not use yet."""
    sink = S.sink(l)
    inner = [s for s in np.unique(l.src) if s not in (0, sink)]
    if not inner:
        return l
    s = int(inner[int(rng.integers(0, len(inner)))])
    free = np.setdiff1d(np.arange(3, l.vocab), l.label[l.src == s])
    lab = int(free[int(rng.integers(0, len(free)))])
    w = None if l.weight is None else np.concatenate([l.weight, [F32(1.0)]])
    cat = lambda a, b: np.concatenate([np.asarray(a, np.int64), [b]])
    return _sorted(l.n_rows, l.vocab, cat(l.src, s), cat(l.label, lab), cat(l.dst, s), w)


CHANGES = {"renumbered": renumbered, "junk": with_junk, "self_loop": with_self_loop}


def _layered(rng, n, V, weighted):
    md = min(int(rng.choice([8, 24, 60])), (V - 12) // 2)
    for _attempt in range(50):  # (the generator refuses a state whose arcs outnumber the labels: draw again)
        try:
            l = synth.layered_lattice(int(rng.integers(1, 1 << 30)), n_states=n, avg_degree=min(float(rng.choice([1.5, 3.0, 6.0, 12.0])), md / 2),
                                      vocab=V, width=int(rng.choice([1, 2, 4, 8, 16, 32])), span=int(rng.choice([1, 2, 4, 8])), max_degree=md,
                                      weighted=weighted)
            return PC.Lat(l.n_rows, l.vocab, l.src, l.label, l.dst, l.weight)
        except AssertionError:
            continue
    raise AssertionError("no lattice in 50 attempts")


# ---------------------------------------------------------------- paths of one lattice
def out_lists(l):
    out = [[] for _ in range(l.n_rows)]
    for a in range(l.n_arcs):
        if l.src[a] != l.dst[a]:
            out[int(l.src[a])].append(a)
    return out


def random_path(l, rng, out=None):
    """arc ids of one path from state 0 to the sink (empty where state 0 is the sink)"""
    out = out or out_lists(l)
    s, arcs = 0, []
    while out[s]:
        a = out[s][int(rng.integers(0, len(out[s])))]
        arcs.append(a)
        s = int(l.dst[a])
    return np.asarray(arcs, np.int64)


def count_paths(l, cap=ENUMERABLE + 1) -> int:
    """paths from state 0 to the sink, saturating at ``cap``"""
    depth = levels(l.n_rows, l.src, l.dst)
    order = sorted((s for s in range(l.n_rows) if depth[s] >= 0), key=lambda s: -depth[s])
    out = out_lists(l)
    cnt = {}
    for s in order:
        cnt[s] = 1 if not out[s] else min(cap, sum(cnt[int(l.dst[a])] for a in out[s]))
    return cnt[0]


def all_paths(l):
    """every path as a tuple of arc ids (small lattices)"""
    out = out_lists(l)
    res = []

    def walk(s, arcs):
        if not out[s]:
            res.append(tuple(arcs))
            return
        for a in out[s]:
            walk(int(l.dst[a]), arcs + [a])

    walk(0, [])
    return res


def min_max_len(l):
    """(shortest, longest) path length in arcs"""
    depth = levels(l.n_rows, l.src, l.dst)
    order = sorted((s for s in range(l.n_rows) if depth[s] >= 0), key=lambda s: depth[s])
    lo = np.full(l.n_rows, np.iinfo(np.int64).max)
    lo[0] = 0
    first = np.searchsorted(l.src, np.arange(l.n_rows + 1))
    for s in order:
        for a in range(int(first[s]), int(first[s + 1])):
            if l.dst[a] != s:
                lo[l.dst[a]] = min(lo[l.dst[a]], lo[s] + 1)
    sink = S.sink(l)
    return int(lo[sink]), int(depth[sink])


# ---------------------------------------------------------------- automata
@dataclasses.dataclass
class Auto:
    """One constraint of a draw.  ``tables``: one ``(delta [Q, V] int64, final [Q] bool, weight [Q, V] float32 | None)`` for
    the batch, or one per lattice.  ``kind``: "narrow" (ConstraintDFA), "wide" (WideDFA.from_dense), "sequence" /
    "marked" (the sparse builders, ``seqs``: one label sequence per table, ``marker`` for "marked")."""
    kind: str
    tables: list
    seqs: Optional[list] = None
    marker: int = -1

    @property
    def per_lattice(self) -> bool:
        return len(self.tables) > 1

    def table(self, b):
        return self.tables[b if self.per_lattice else 0]

    @property
    def weighted(self) -> bool:
        return self.tables[0][2] is not None

    def build(self):
        """the ``nfst_amd.constraints`` object"""
        import torch
        from nfst_amd.constraints import ConstraintDFA, WideDFA
        V = self.tables[0][0].shape[1]
        if self.kind == "narrow":
            if not self.per_lattice:
                d, f, w = self.tables[0]
                return ConstraintDFA(d, f, None if w is None else torch.from_numpy(w))
            w = None if not self.weighted else torch.from_numpy(np.stack([t[2] for t in self.tables]))
            return ConstraintDFA(np.stack([t[0] for t in self.tables]), np.stack([t[1] for t in self.tables]), w)
        if self.kind == "wide":
            one = [WideDFA.from_dense(d, f, None if w is None else torch.from_numpy(w)) for d, f, w in self.tables]
        elif self.kind == "sequence":
            one = [WideDFA.sequence(V, s) for s in self.seqs]
        else:
            one = [WideDFA.marked_sequence(V, self.marker, s) for s in self.seqs]
        return one[0] if not self.per_lattice else WideDFA.stack(one)


def random_table(rng, Q, V, miss, weighted):
    delta = rng.integers(0, Q, size=(Q, V)).astype(np.int64)
    if miss > 0:
        delta[rng.random((Q, V)) < miss] = -1
    final = rng.random(Q) < 0.5
    final[int(rng.integers(0, Q))] = True
    w = rng.normal(0.0, 0.3, size=(Q, V)).astype(F32) if weighted else None
    return delta, final, w


def sequence_table(V, seq):
    """``WideDFA.sequence``: state j = j labels read"""
    n = len(seq)
    delta = np.full((n + 1, V), -1, np.int64)
    delta[np.arange(n), np.asarray(seq, np.int64)] = np.arange(1, n + 1)
    final = np.zeros(n + 1, bool)
    final[n] = True
    return delta, final, None


def marked_table(V, marker, seq):
    """``marked_sequence``: state 2 j = j marked labels read, 2 j + 1 = the marker read after them"""
    n = len(seq)
    delta = np.full((2 * (n + 1), V), -1, np.int64)
    for j in range(n + 1):
        delta[2 * j] = 2 * j
        delta[2 * j, marker] = 2 * j + 1
        if j < n:
            delta[2 * j + 1, seq[j]] = 2 * j + 2
    final = np.zeros(2 * (n + 1), bool)
    final[2 * n] = True
    return delta, final, None


def _draw_automata(rng, canon, V, many):
    B = len(canon)
    autos = []
    for kind, qs in (("narrow", NARROW_Q), ("wide", WIDE_Q)):
        Q = int(rng.choice(qs))
        miss = float(rng.choice([0.0, 0.0, 0.02, 0.1, 0.3]))
        weighted = bool(rng.integers(0, 2))
        per = bool(rng.integers(0, 2)) and not many and Q * V * B <= 4_000_000
        autos.append(Auto(kind, [random_table(rng, Q, V, miss, weighted) for _ in range(B if per else 1)]))
    # the labels of a random path of every lattice: a thin numerator (a member without arcs accepts the empty sequence only
    # through an automaton whose state 0 is final: marked_sequence of no label)
    paths = [random_path(c, rng) for c in canon]
    marked = bool(rng.integers(0, 2)) or any(len(p) == 0 for p in paths)
    if marked:
        first = canon[0].label[paths[0]]  # the marker: a label inside the first member's path, where it has one
        marker = int(first[int(rng.integers(1, len(first) - 1))]) if len(first) >= 3 else int(rng.integers(3, V))
        seqs = []
        for c, p in zip(canon, paths):
            labs = c.label[p]
            seqs.append([int(labs[i + 1]) for i in range(len(labs) - 1) if labs[i] == marker])
        if many:  # the batch of many lattices takes one automaton for all: "no marker on the path" (an empty marked sequence), which
            # is a filter and no thin numerator; its thin numerators are the per-lattice ``sequence`` automata of the other branch
            seqs = [[]]
        autos.append(Auto("marked", [marked_table(V, marker, s) for s in seqs], seqs=seqs, marker=marker))
    else:
        # one exact sequence per lattice, in the batch of many lattices too: 260 - 300 automata of 5 - 10 states are small, unlike
        # per-lattice tables of up to 300 x 700 entries, which ``many`` rules out above
        seqs = [[int(x) for x in c.label[p]] for c, p in zip(canon, paths)]
        autos.append(Auto("sequence", [sequence_table(V, s) for s in seqs], seqs=seqs))
    second = Auto("narrow", [random_table(rng, int(rng.choice([2, 5])), V, 0.0, bool(rng.integers(0, 2)))])  # for the product of a product
    return autos, second


def keep_labels(V: int) -> set:
    """the output tape of the string ops: the odd labels and eos (tests/test_gpu_strings.py's structure test)"""
    return set(range(3, V, 2)) | {EOS}


# ---------------------------------------------------------------- a draw
@dataclasses.dataclass
class Draw:
    seed: int
    it: int
    vocab: int
    weighted: bool
    lats: list              # the caller's arc lists (PC.Lat)
    canon: list             # S.canonical of them: what the engine numbers
    changes: list           # per member: None or a name of CHANGES / "state0_is_sink"
    theta: np.ndarray       # [V] or [B, V] float32
    asc: Optional[np.ndarray]  # float32 over the canonical arcs of the batch, or None
    dead: bool              # labels at -inf
    route: str              # "host" / "device"
    gm: int
    chunks: bool
    k: int
    T: int
    refs: list              # reference strings for lattice edit distance, one per lattice (int64 arrays)
    cands: list             # candidate strings for string_log_prob, four per lattice, on the tape of ``keep_labels``
    autos: list             # [narrow, wide, thin]
    second: Auto
    states: list = None     # the drawn number of states of every member (before junk rows; the rows of a member without arcs)

    @property
    def B(self):
        return len(self.lats)

    def theta_of(self, b):
        return self.theta[b] if self.theta.ndim == 2 else self.theta

    def slices(self):
        off = np.concatenate([[0], np.cumsum([c.n_arcs for c in self.canon])])
        return [slice(int(off[b]), int(off[b + 1])) for b in range(self.B)]

    def asc_of(self, b):
        return None if self.asc is None else self.asc[self.slices()[b]]

    def score64(self, b, c=None, asc=None):
        """float64 arc scores of member b (or of a derived lattice ``c`` over the same labels with its own caller scores)"""
        c = c or self.canon[b]
        asc = self.asc_of(b) if c is self.canon[b] and asc is None else asc
        s = self.theta_of(b)[c.label].astype(np.float64)
        if c.weight is not None:
            s = s + c.weight.astype(np.float64)
        if asc is not None:
            s = s + asc.astype(np.float64)
        return s


def draw(seed: int, it: int) -> Draw:
    rng = np.random.default_rng([0xF022, seed, it])
    many = it == ITERS - 1
    V = int(rng.choice(VOCABS))
    weighted = bool(rng.integers(0, 2))
    B = int(rng.integers(N_CUS + 4, N_CUS + 45)) if many else int(rng.integers(1, 13))
    lats, changes, states = [], [], []
    for _ in range(B):
        states.append(int(rng.choice(SMALL if many else SIZES)))
        l = _layered(rng, states[-1], V, weighted)
        change = None
        if rng.integers(0, 4) == 0:
            change = str(rng.choice(sorted(CHANGES)))
            l = CHANGES[change](l, rng)
        lats.append(l), changes.append(change)
    if rng.integers(0, 8) == 0:  # a member whose state 0 is the sink: one row, or rows without any arc
        b = int(rng.integers(0, B))
        lats[b] = (S.one_row if rng.integers(0, 2) else S.no_arcs)(weighted)
        lats[b] = dataclasses.replace(lats[b], vocab=V)
        changes[b], states[b] = "state0_is_sink", lats[b].n_rows
    canon = [S.canonical(l) for l in lats]
    A = sum(c.n_arcs for c in canon)
    mean, std = float(rng.choice([-2.3, 0.0, -8.0])), float(rng.choice([0.5, 2.0]))
    per_lattice = bool(rng.integers(0, 2))
    theta = rng.normal(mean, std, size=(B, V) if per_lattice else V).astype(F32)
    asc = rng.normal(0.0, 0.5, size=A).astype(F32) if rng.integers(0, 2) else None
    dead = rng.integers(0, 4) == 0
    if dead:
        labs = 3 + rng.choice(V - 3, size=max(1, V // 20), replace=False)
        theta[..., labs] = NEG
        if rng.integers(0, 3) == 0:  # eos at -inf for one lattice (per-lattice scores) or for all: no finite path
            theta[(int(rng.integers(0, B)), EOS) if per_lattice else EOS] = NEG
    route = str(rng.choice(["host", "device"]))
    gm = int(rng.choice([0, 0, 0, 1, 2]))
    chunks = rng.integers(0, 3) == 0
    k = int(rng.choice(KS))
    spans = [min_max_len(c) for c in canon]
    T = int(rng.integers(max(1, min(s[0] for s in spans) - 1), max(1, max(s[1] for s in spans)) + 1))
    outs = [out_lists(c) for c in canon]
    refs, cands = [], []
    rng = np.random.default_rng([0xF022, seed, it, 1])  # the strings have a stream of their own, and so have the automata
    for b, c in enumerate(canon):
        if rng.integers(0, 2):  # the labels of a random path with a few edits
            y = [int(x) for x in c.label[random_path(c, rng, outs[b])]][:40]
            for _ in range(int(rng.integers(0, 4))):
                p = int(rng.integers(0, len(y) + 1))
                kind = int(rng.integers(0, 3))
                if kind == 0:
                    y.insert(p, int(rng.integers(0, V)))
                elif y and kind == 1:
                    del y[min(p, len(y) - 1)]
                elif y:
                    y[min(p, len(y) - 1)] = int(rng.integers(0, V))
        else:
            y = [int(x) for x in rng.integers(0, V, size=int(rng.integers(0, 13)))]
        refs.append(np.asarray(y, np.int64))
        keep = keep_labels(V)  # candidates: the projections of three random paths, and one that no path spells (a label behind eos)
        cs = [np.asarray([x for x in c.label[random_path(c, rng, outs[b])] if int(x) in keep], np.int64) for _ in range(3)]
        cs.append(np.concatenate([cs[0], [V - 1]]))
        cands.append(cs)
    autos, second = _draw_automata(np.random.default_rng([0xF022, seed, it, 2]), canon, V, many)
    return Draw(seed, it, V, weighted, lats, canon, changes, theta, asc, bool(dead), route, gm, bool(chunks), k, T, refs, cands, autos, second, states)


def digest(d: Draw) -> str:
    h = hashlib.sha256()

    def put(x):
        if x is None:
            h.update(b"none")
        elif isinstance(x, np.ndarray):
            h.update(str(x.dtype).encode() + str(x.shape).encode() + np.ascontiguousarray(x).tobytes())
        elif isinstance(x, (list, tuple)):
            h.update(b"[%d" % len(x))
            for y in x:
                put(y)
        else:
            h.update(repr(x).encode())

    put([d.seed, d.it, d.vocab, d.weighted, d.changes, d.theta, d.asc, d.dead, d.route, d.gm, d.chunks, d.k, d.T, d.refs, d.cands])
    for l in d.lats:
        put([l.n_rows, l.vocab, l.src, l.label, l.dst, l.weight])
    for a in d.autos + [d.second]:
        put([a.kind, a.marker, a.seqs, [list(t) for t in a.tables]])
    return h.hexdigest()


# ---------------------------------------------------------------- packing
def pack(d: Draw, dev, chunks=None):
    """The draw's batch as it asks to be packed: host or device packer, group mode, chunked programs on request."""
    from nfst_amd.lattice import LatticeBatch
    chunks = d.chunks if chunks is None else chunks
    n_rows, arc_off, src, label, dst, w = PC.batch_arcs(d.lats)
    if d.route == "host" or dev is None:
        lat = LatticeBatch.from_arcs(n_rows, arc_off, src, label, dst, d.vocab, arc_w=w, group_mode=d.gm)
        if chunks:
            lat.build_chunks()
        return lat if dev is None else lat.to(dev, auto_chunks=False)
    return LatticeBatch.from_arcs_device(n_rows, arc_off, src, label, dst, d.vocab, arc_w=w, device=dev, group_mode=d.gm, chunks=chunks)


# ---------------------------------------------------------------- derived corpora, from the references alone
def product_ref(c, auto: Auto, b: int) -> dict:
    delta, final, _ = auto.table(b)
    fn = intersect_ref.intersect if auto.kind == "narrow" else intersect_wide_ref.intersect
    return fn(c, delta, final)


def outcome(products) -> tuple:
    """What ``ops.intersect`` must do with these products: ("ok", None), ("limit", b) -- the first product of more than
    8192 rows, NFST_ERR_LIMIT from the counting launch -- or ("empty", b), the first empty one (reported after the
    launch: a limit anywhere in the batch comes first)."""
    big = [b for b, p in enumerate(products) if p["n_rows"] > MAX_ROWS]
    if big:
        return "limit", big[0]
    empty = [b for b, p in enumerate(products) if p["n_rows"] == 0]
    return ("empty", empty[0]) if empty else ("ok", None)


@dataclasses.dataclass
class Derived:
    """A batch made from another by the references: ``lats`` over canonical numbering, ``arc_map`` per member into the
    parent's canonical arcs (relative to the member), ``asc`` per member (caller scores of the derived arcs, or None)."""
    lats: list
    arc_map: list
    asc: list
    products: Optional[list] = None  # the reference dictionaries of a product


def product_of(lats, ascs, auto: Auto) -> Optional[Derived]:
    """The product of every lattice with the automaton, or None where ``ops.intersect`` refuses the batch."""
    prods = [product_ref(c, auto, b) for b, c in enumerate(lats)]
    if outcome(prods)[0] != "ok":
        return None
    out, maps, new_asc = [], [], []
    for b, (c, p) in enumerate(zip(lats, prods)):
        am = p["arc_map"]
        out.append(PC.Lat(p["n_rows"], c.vocab, p["src"], p["label"], p["dst"], None if c.weight is None else c.weight[am]))
        a = None if ascs[b] is None else ascs[b][am].astype(F32)
        w = auto.table(b)[2]
        if w is not None:
            wa = w[p["arc_q"], p["label"]].astype(F32)
            a = wa if a is None else (a + wa).astype(F32)
        maps.append(am), new_asc.append(a)
    return Derived(out, maps, new_asc, prods)


def pruned_of(lats, ascs, thetas) -> Derived:
    """``slack_ref.arc_slack``'s keep mask applied to every arc list (beams taking turns): the kept arcs over the same
    rows, the states they no longer reach left as junk rows."""
    out, maps = [], []
    for b, c in enumerate(lats):
        if c.n_arcs == 0:
            out.append(c), maps.append(np.zeros(0, np.int64))
            continue
        keep = slack_ref.arc_slack(c, thetas[b], ascs[b], beam=BEAMS[b % len(BEAMS)])["keep"]
        am = np.flatnonzero(keep)
        out.append(PC.Lat(c.n_rows, c.vocab, c.src[am], c.label[am], c.dst[am], None if c.weight is None else c.weight[am]))
        maps.append(am)
    return Derived(out, maps, [None if a is None else a[m] for a, m in zip(ascs, maps)])


def finite(d: Draw) -> bool:
    """every member has a path of finite score (the beam of a lattice without one keeps nothing: ``prune`` refuses it)"""
    from tests import kbest_ref
    for b, c in enumerate(d.canon):
        if c.n_arcs and kbest_ref.count_finite_paths(c.n_rows, c.src, c.dst, d.score64(b), S.sink(c)) == 0:
            return False
    return True


def derived(d: Draw) -> dict:
    """{"auto": index of the automaton of the product (the first that ``ops.intersect`` takes on the whole batch),
    "product", "pruned", "pruned_product", "second": the automaton of the second product (``d.second``, or the same with every
    state final where ``d.second`` leaves a product empty), "product_product"}; entries are None where the draw has none."""
    thetas = [d.theta_of(b) for b in range(d.B)]
    ascs = [d.asc_of(b) for b in range(d.B)]
    out = {"auto": None, "product": None, "pruned": None, "pruned_product": None, "second": None, "product_product": None}
    fin = finite(d)
    if fin:
        out["pruned"] = pruned_of(d.canon, ascs, thetas)
    for i, auto in enumerate(d.autos):  # (the Python references of every leg run on the product: the first of moderate size)
        p = product_of(d.canon, ascs, auto)
        if p is not None and max(l.n_rows for l in p.lats) <= DERIVED_ROWS:
            out["auto"], out["product"] = i, p
            break
    p = out["product"]
    if p is not None:
        out["second"] = d.second
        out["product_product"] = product_of(p.lats, p.asc, d.second)
        if out["product_product"] is None:  # the same transitions with every state final: nothing is refused
            out["second"] = all_final(d.second)
            out["product_product"] = product_of(p.lats, p.asc, out["second"])
        if fin and all(_has_finite(d, b, c, a) for b, (c, a) in enumerate(zip(p.lats, p.asc))):
            out["pruned_product"] = pruned_of(p.lats, p.asc, thetas)
    return out


def all_final(a: Auto) -> Auto:
    return Auto(a.kind, [(d, np.ones_like(f), w) for d, f, w in a.tables], a.seqs, a.marker)


def _has_finite(d, b, c, asc):
    from tests import kbest_ref
    return c.n_arcs == 0 or kbest_ref.count_finite_paths(c.n_rows, c.src, c.dst, d.score64(b, c, asc), S.sink(c)) > 0


# ---------------------------------------------------------------- inputs that the CPU and the GPU tests share
SAMPLE_K = 8           # walks per lattice of the samplers
# The gradient check of ``swor.log_prob`` is narrowed twice, for one reason.  The gradient to theta is assembled in float32
# from one term per label of every drawn path (``ops._path_score_grads``: ``index_add_``; a table shared by the batch: one
# more sum over the lattices).  With the draw's k = 64 the summed gradient of a shared table missed the 1e-5 of
# tests/test_gpu_swor.py by 1.44e-5 on draw (2, 3), 265 lattices over one table, and by 1.76e-5 on the product of draw
# (0, 2), paths of up to 240 arcs over 24 labels; at that test's own k = 7 still by 2.4e-5 on the batches of hundreds of
# lattices, in the entries of bos and eos, which every path adds to: their terms sum to thousands in magnitude, where half
# a float32 ulp alone is above 1e-5 (2^-24 * 128 = 7.6e-6), and every error stayed inside the classical bound of a
# float32 sum, n 2^-23 times the summed magnitudes.  So (i) the leg runs at that test's k, not the draw's, and (ii) it
# holds to 1e-5 the entries whose terms sum to less than LOG_PROB_MAGNITUDE in magnitude (half an ulp there: 3.8e-6) and
# the others to that rounding bound.  tests/test_gpu_fuzz_paths.py keeps draw (2, 3) at k = 64 as a named test
# (tests/golden/fuzz_swor_log_prob_k64.json).  The draws without replacement themselves run at the draw's k.
LOG_PROB_K = 7
LOG_PROB_MAGNITUDE = 64.0
SAMPLE_SEED = 7        # seed of the uniforms of ``sample_paths``
POS_SWOR_SEED = 13     # seed of the uniforms of the positional draws without replacement


def pos_inputs(lats, T: int, seed=21) -> np.ndarray:
    """[B, T, V] position scores ~ N(0, 1), NaN in the pad column (it enters no output): tests/test_gpu_structure.py's"""
    pos = np.random.default_rng([seed, T]).normal(0.0, 1.0, size=(len(lats), T, lats[0].vocab)).astype(F32)
    pos[..., PAD] = np.nan
    return pos


def theta_rows(theta, b):
    return theta[b] if np.ndim(theta) == 2 else theta


def arc_parts(lats, asc):
    off = np.concatenate([[0], np.cumsum([l.n_arcs for l in lats])])
    return [None if asc is None else asc[int(off[b]):int(off[b + 1])] for b in range(len(lats))]


def sample_walks(lats, theta, asc, K=SAMPLE_K):
    """(uniforms [B, K, L], per lattice None (no arcs) or ``paths_ref.oracle_walks`` on them)"""
    from tests import paths_ref
    L = max(int(levels(l.n_rows, l.src, l.dst).max()) for l in lats) + 1
    u = np.random.default_rng(SAMPLE_SEED).random((len(lats), K, L)).astype(F32)
    out = []
    for b, (l, a) in enumerate(zip(lats, arc_parts(lats, asc))):
        out.append(paths_ref.oracle_walks(l, paths_ref.score64(l, theta_rows(theta, b), l.weight, a), u[b]) if l.n_arcs else None)
    return u, out


def positional_walks(lats, theta, asc, T: int, K=SAMPLE_K):
    """(pos, uniforms [B, K, T], samplers, walks) of ``positional_sample_ref`` as tests/test_gpu_structure.py draws them"""
    from tests import positional_ref as P, positional_sample_ref as PS
    pos = pos_inputs(lats, T)
    U = np.stack([PS.uniforms(100 * T + b, K, T) for b in range(len(lats))])
    smp = [PS.Sampler(l, P.arc_score64(l, theta_rows(theta, b), a), pos[b], T) for b, (l, a) in enumerate(zip(lats, arc_parts(lats, asc)))]
    walks = [s.walks(U[b]) if l.n_arcs and np.isfinite(s.logz) else None for b, (l, s) in enumerate(zip(lats, smp))]
    return pos, U, smp, walks


def positional_swor_refs(tag, lats, theta, asc, k: int, T: int):
    """(case, pos, uniforms [B, T, k, D], ``positional_swor_ref.search`` per lattice on float64 beta rows)"""
    from tests import positional_swor_ref as PW, swor_ref
    case = swor_ref.Case(str(tag), lats, theta, asc, ks=(k,), seed=POS_SWOR_SEED)
    es = case.scores()
    D = max(swor_ref.degree(lats), 1)
    pos = pos_inputs(lats, T)
    pos[..., PAD] = 0.0
    betas = PW.beta_rows(case, T, pos)
    u = np.stack([np.random.default_rng([POS_SWOR_SEED, b, T]).random((T, k, D), dtype=F32) for b in range(len(lats))])
    refs = [PW.search(l, es[b], pos[b], betas[b][0], betas[b][1], k, T, u[b]) for b, l in enumerate(lats)]
    return case, pos, u, refs

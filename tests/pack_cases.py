"""Lattices that reach every launch branch of the device packer (``k_pack_lattice``, pack_kernels.h), each named after
the branch it exists for.  Pure numpy: explicit arc lists, no library, no GPU, no randomness beyond fixed seeds.

``cases()`` returns the corpus; ``analyse`` is the plain-Python reference of what a packer must find in an arc list
(reachable states, canonical arcs, sink, depth, degrees); ``branches`` evaluates the kernel's own predicates on that
analysis with the kernel's constants (``nfst_pack_device_limits``) passed in, so that a predicate cannot drift from the
kernel.  tests/test_pack_cases_cpu.py holds the corpus to its claims and the host packer to the float64 oracle on it;
tests/test_gpu_pack.py holds the device packer to the host packer on it, bit for bit."""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

PAD, BOS, EOS = 0, 1, 2
MAX_ROWS = 8192          # NFST_MAX_ROWS
NARROW_G, WIDE_G, SLOTS = 3, 6, 4  # tile_format.h: largest group of a narrow / wide program, slots per lane of a compact tile
N_CUS = 256

# every branch of the packer that the corpus must reach (test_pack_cases_cpu.py: the union over the corpus covers them)
BRANCHES = (
    "arcs_beyond_lds",        # sd_in_lds false: the relaxation reads src / dst from global memory
    "ranks_in_global",        # t_lds false while c_lds holds: `place` aliases in_tmp
    "counters_in_global",     # c_lds false: counters and the unordered in-arc lists in global memory
    "count_falls_back",       # (D + 1)(2 P + 1) beyond the LDS table: pk_count_layout -> pk_layout<false>
    "count_falls_back_wide",  # ... for a program of 64-lane groups: the fallback's count of wide tiles feeds the cost model
    "second_relaxation",      # a cycle among unreachable states: the first relaxation attempt does not settle
    "junk_arcs",              # unreachable states own arcs: the dep[src] >= 0 compaction has something to drop
    "junk_into_reachable",    # ... arcs into reachable states: in-degrees must ignore them
    "junk_self_loop",         # ... a self loop of an unreachable state
    "junk_dead_end",          # an unreachable state without out-arcs is not a second sink
    "junk_low_ids",           # unreachable states at ids below reachable ones: canonical arc ids shift
    "junk_weighted",          # arc weights follow the compaction
    "inner_self_loops",       # self loops at inner reachable states
    "self_loop_at_0",         # ... and at state 0
    "one_row",                # n_rows = 1, no arcs
    "no_arcs_mid_batch",      # a lattice without arcs between lattices with arcs
    "zero_arcs",              # a batch whose total arc count is 0
    "many",                   # more workgroups than CUs at one workgroup per CU
    "limit_pieces",           # more pieces of one direction than sort keys fit LDS: NFST_ERR_LIMIT from inside the kernel
    "limit_rows",             # n_rows + scratch rows beyond NFST_MAX_ROWS: NFST_ERR_LIMIT from inside the kernel
)


@dataclass
class Lat:
    """One lattice as an arc list sorted by (src, label); the fields of ``nfst_amd.synth.SynthLattice``."""
    n_rows: int
    vocab: int
    src: np.ndarray
    label: np.ndarray
    dst: np.ndarray
    weight: Optional[np.ndarray] = None

    @property
    def n_arcs(self) -> int:
        return int(self.src.shape[0])

    def dense(self, weighted: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        if weighted:
            em = np.full((self.n_rows, self.vocab), -np.inf, dtype=np.float32)
            em[self.src, self.label] = self.weight if self.weight is not None else np.zeros(self.n_arcs, np.float32)
        else:
            em = np.zeros((self.n_rows, self.vocab), dtype=np.bool_)
            em[self.src, self.label] = True
        tr = np.zeros((self.n_rows, self.vocab), dtype=np.int64)
        tr[self.src, self.label] = self.dst
        return em, tr


@dataclass
class Case:
    name: str
    lats: list            # one batch
    branches: frozenset   # what the entry exists for (names of BRANCHES)
    group_modes: tuple    # the packer's group modes the entry is run under
    small: bool           # small enough to replay tile by tile in Python
    only: frozenset = frozenset()  # launch branches that must be the ONLY ones of their kind the entry reaches ("isolated")


def make(n_rows, vocab, arcs, weight_seed=None) -> Lat:
    """arcs: (src, label, dst) triples in any order; sorted by (src, label) here"""
    a = np.asarray(arcs, dtype=np.int64).reshape(-1, 3)
    order = np.lexsort((a[:, 1], a[:, 0]))
    a = a[order]
    assert np.all(np.diff(a[:, 0] * vocab + a[:, 1]) > 0), "not deterministic"
    assert a.size == 0 or (a.min() >= 0 and a[:, [0, 2]].max() < n_rows and a[:, 1].max() < vocab)
    w = None
    if weight_seed is not None:
        w = np.random.default_rng(weight_seed).normal(-0.5, 0.7, size=a.shape[0]).astype(np.float32)
    return Lat(int(n_rows), int(vocab), a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32), w)


def chain(par, vocab=None, skip_label=0) -> Lat:
    """states 0 .. len(par); step i has par[i] parallel arcs i -> i + 1 with labels 3, 4, ...; the last state is the sink
    with its pad self loop.  ``skip_label``: one more arc i -> i + 2 with that label from every state that has room."""
    par = np.asarray(par, dtype=np.int64)
    n = int(par.shape[0]) + 1
    vocab = int(vocab if vocab is not None else par.max() + 3)
    src = np.repeat(np.arange(n - 1), par)
    first = np.repeat(np.cumsum(par) - par, par)
    label = 3 + np.arange(src.shape[0]) - first
    dst = src + 1
    parts = [np.stack([src, label, dst], axis=1), np.array([[n - 1, PAD, n - 1]])]
    if skip_label:
        s = np.arange(n - 2)
        parts.append(np.stack([s, np.full_like(s, skip_label), s + 2], axis=1))
    return make(n, vocab, np.concatenate(parts))


# ---------------------------------------------------------------- the plain reference of what a packer finds
def analyse(l: Lat) -> dict:
    n = l.n_rows
    src, dst = l.src.tolist(), l.dst.tolist()
    out = [[] for _ in range(n)]
    for a, s in enumerate(src):
        out[s].append(a)
    reach = [False] * n
    reach[0] = True
    queue = [0]
    for s in queue:  # breadth first from state 0
        for a in out[s]:
            if not reach[dst[a]]:
                reach[dst[a]] = True
                queue.append(dst[a])
    canon = [a for a in range(len(src)) if reach[src[a]]]
    dp = [a for a in canon if src[a] != dst[a]]
    indeg, outdeg = [0] * n, [0] * n
    for a in dp:
        indeg[dst[a]] += 1
        outdeg[src[a]] += 1
    sinks = [s for s in range(n) if reach[s] and outdeg[s] == 0]
    # longest paths by Kahn's order over the arcs of reachable states (self loops are not part of the sweeps)
    depth, height, rem, order = [0] * n, [0] * n, list(indeg), [0]
    for s in order:
        for a in out[s]:
            d = dst[a]
            if d == s:
                continue
            depth[d] = max(depth[d], depth[s] + 1)
            rem[d] -= 1
            if rem[d] == 0:
                order.append(d)
    acyclic = indeg[0] == 0 and len(order) == sum(reach)
    if acyclic:
        for s in reversed(order):
            for a in out[s]:
                if dst[a] != s:
                    height[s] = max(height[s], height[dst[a]] + 1)
    # the unreachable part
    junk = [a for a in range(len(src)) if not reach[src[a]]]
    jrem = [0] * n
    for a in junk:
        if src[a] != dst[a] and not reach[dst[a]]:
            jrem[dst[a]] += 1
    jorder = [s for s in range(n) if not reach[s] and jrem[s] == 0]
    for s in jorder:
        for a in out[s]:
            d = dst[a]
            if d != s and not reach[d]:
                jrem[d] -= 1
                if jrem[d] == 0:
                    jorder.append(d)
    return dict(n=n, A=len(src), reach=np.array(reach), n_reach=sum(reach), canon=np.array(canon, dtype=np.int64), n_arcs=len(canon),
                n_dp=len(dp), sinks=sinks, acyclic=acyclic, depth=np.array(depth), height=np.array(height),
                D=depth[sinks[0]] if len(sinks) == 1 and acyclic else -1, indeg=np.array(indeg), outdeg=np.array(outdeg),
                junk=junk, junk_cyclic=len(jorder) != n - sum(reach), src=l.src, dst=l.dst, weighted=l.weight is not None)


# ---------------------------------------------------------------- tile_format.h, the few formulas the predicates need
def _chain_pieces(length, cap):
    return 1 if length <= cap else 1 + (length - 2) // (cap - 1)


def _tree_parts(deg, max_g, cap):
    return (deg + cap - 1) // cap if (max_g == NARROW_G and deg > 2 * cap) else 0


def _passes_pieces(deg, max_g):
    cap = (1 << max_g) * SLOTS
    parts = _tree_parts(deg, max_g, cap)
    if parts:
        return 1 + _chain_pieces(parts, cap), parts + _chain_pieces(parts, cap), parts
    return _chain_pieces(deg, cap), _chain_pieces(deg, cap), 0


def programs_tried(a: dict, group_mode: int):
    """(direction, wide) of every layout that the planning pass counts"""
    out = []
    for direction, deg in (("fwd", a["indeg"]), ("bwd", a["outdeg"])):
        for wide in (0, 1):
            if (group_mode == 1 and wide) or (group_mode == 2 and not wide):
                continue
            if wide and group_mode != 2 and int(deg.max()) <= (1 << NARROW_G) * SLOTS:
                continue
            out.append((direction, wide))
    return out


def layout_figures(a: dict, direction: str, wide: int):
    """(P, pieces, scratch rows) of one direction's layout: the passes of the longest chain, the pieces of the levels
    1 .. D, the partial groups of the fullest level"""
    deg, lev, first = (a["indeg"], a["depth"], 0) if direction == "fwd" else (a["outdeg"], a["height"], a["sinks"][0])
    max_g = WIDE_G if wide else NARROW_G
    P, pieces, per_level = 1, 0, {}
    for s in np.flatnonzero(a["reach"]).tolist():
        if s == first:
            continue
        p, k, parts = _passes_pieces(int(deg[s]), max_g)
        P, pieces = max(P, p), pieces + k
        if parts:
            per_level[int(lev[s])] = per_level.get(int(lev[s]), 0) + parts
    return P, pieces, max(per_level.values(), default=0)


def branches(a: dict, n_lattices: int, group_mode: int, lds_bytes: int, max_keys: int) -> set:
    """The names of BRANCHES that this lattice (in a batch of ``n_lattices``) reaches under ``group_mode``, by the
    predicates of k_pack_lattice.  The lattice must be one that the packers accept (one sink, acyclic)."""
    n, A, n_dp, D = a["n"], a["A"], a["n_dp"], a["D"]
    got = set()
    if 4 * A + 8 * n > lds_bytes:
        got.add("arcs_beyond_lds")
    c_lds = 20 * n <= lds_bytes
    if not c_lds:
        got.add("counters_in_global")
    if c_lds and 4 * (5 * n + n_dp) > lds_bytes:
        got.add("ranks_in_global")
    for direction, wide in programs_tried(a, group_mode):
        P, pieces, scratch = layout_figures(a, direction, wide)
        if pieces > max_keys:
            got.add("limit_pieces")
            break
        if (D + 1) * (2 * P + 1) > lds_bytes // 4:
            got.add("count_falls_back_wide" if wide else "count_falls_back")
        if n + scratch > MAX_ROWS:
            got.add("limit_rows")
            break
    src, dst, reach = a["src"], a["dst"], a["reach"]
    if a["junk"]:
        got.add("junk_arcs")
        j = np.array(a["junk"])
        if np.any(reach[dst[j]]):
            got.add("junk_into_reachable")
        if np.any(src[j] == dst[j]):
            got.add("junk_self_loop")
        if a["canon"].size and int(j.min()) < int(a["canon"].max()):  # (dropped arcs in front of kept ones)
            got.add("junk_low_ids")
        if a["weighted"]:
            got.add("junk_weighted")
    if a["junk_cyclic"]:
        got.add("second_relaxation")
    unreach_dead = [s for s in range(n) if not reach[s] and not np.any((src == s) & (dst != s))]
    if unreach_dead and np.any(np.isin(dst, unreach_dead) & ~reach[src]):  # (a dead end that junk arcs lead to, not a padding row)
        got.add("junk_dead_end")
    loops = np.flatnonzero((src == dst) & reach[src])
    if np.any((src[loops] != a["sinks"][0]) & (src[loops] != 0)):
        got.add("inner_self_loops")
    if np.any(src[loops] == 0) and a["sinks"][0] != 0:
        got.add("self_loop_at_0")
    if n == 1 and A == 0:
        got.add("one_row")
    if n_lattices > N_CUS:
        got.add("many")
    return got


def batch_branches(lats, group_mode: int, lds_bytes: int, max_keys: int, analyses=None) -> set:
    """``branches`` of every lattice of a batch, and what only a batch can be"""
    analyses = analyses if analyses is not None else [analyse(l) for l in lats]
    got = set()
    for a in analyses:
        got |= branches(a, len(lats), group_mode, lds_bytes, max_keys)
    arcs = [l.n_arcs for l in lats]
    if any(arcs[b] == 0 and arcs[b - 1] > 0 and arcs[b + 1] > 0 for b in range(1, len(lats) - 1)):
        got.add("no_arcs_mid_batch")
    if sum(arcs) == 0:
        got.add("zero_arcs")
    return got


# ---------------------------------------------------------------- the corpus
def _junk_cases():
    V = 12
    # the reachable part of every entry: 0 -bos-> a -> ... -eos-> sink, a diamond in the middle
    def core(a, b, c, d, sink):
        return [(0, BOS, a), (a, 3, b), (a, 4, c), (b, 5, d), (c, 5, d), (c, 6, d), (d, EOS, sink), (sink, PAD, sink)]
    out = {}
    # unreachable 6, 7, 8: acyclic arcs among themselves and into the reachable 3, 4 and the sink (counted, they would put
    # state 3 in front of state 2 in the order of their level: in-degree falling, then id)
    out["junk_acyclic"] = make(9, V, core(1, 2, 3, 4, 5) + [(6, 3, 7), (6, 4, 8), (7, 3, 8), (7, 5, 3), (8, 3, 4), (8, 4, 4), (6, 7, 5)])
    # unreachable 6 -> 7 -> 8 -> 6, and 7 -> 3 into the reachable part
    out["junk_cycle"] = make(9, V, core(1, 2, 3, 4, 5) + [(6, 3, 7), (7, 3, 8), (8, 3, 6), (7, 4, 3)])
    # unreachable 6 with a self loop and an arc into the reachable part; 7 with a self loop alone
    out["junk_self_loop"] = make(8, V, core(1, 2, 3, 4, 5) + [(6, 3, 6), (6, 4, 2), (7, 9, 7)])
    # unreachable 6 -> 7, and 7 has no out-arcs: not a second sink
    out["junk_dead_end"] = make(8, V, core(1, 2, 3, 4, 5) + [(6, 3, 7), (6, 4, 4)])
    # unreachable 1, 3 and 5 between the reachable states 0, 2, 4, 6, 7, 8: their arcs sit in the middle of the list
    out["junk_low_ids"] = make(9, V, core(2, 4, 6, 7, 8) + [(1, 3, 2), (1, 4, 3), (3, 3, 4), (3, 4, 5), (3, 5, 8), (5, 3, 6), (5, 7, 5)])
    # the same with weights, and a cycle 1 -> 3 -> 1 on top
    out["junk_weighted"] = make(9, V, core(2, 4, 6, 7, 8) + [(1, 3, 2), (1, 4, 3), (3, 3, 4), (3, 4, 5), (3, 5, 8), (3, 6, 1), (5, 3, 6), (5, 7, 5)],
                                weight_seed=11)
    return out


def _many():
    """about 300 tiny lattices, a few of them with junk"""
    junk = _junk_cases()
    V = 12
    rng = np.random.default_rng(5)
    out = []
    for i in range(300):
        if i % 37 == 5:
            out.append(junk[("junk_acyclic", "junk_cycle", "junk_self_loop", "junk_dead_end", "junk_low_ids")[(i // 37) % 5]])
            continue
        k = int(rng.integers(1, 7))
        par = rng.integers(1, 5, size=k)
        out.append(chain(par, vocab=V, skip_label=int(rng.integers(0, 2)) * 9))
    return out


def cases():
    """name -> Case.  The big entries hold one lattice each and are packed once per group mode."""
    j = _junk_cases()
    V = 12
    one_row = make(1, V, [])
    no_arcs = make(3, V, [])  # three rows, no arcs: state 0 is the sink, rows 1 and 2 are padding
    tiny = chain([2, 1, 3], vocab=V)
    loops = make(7, V, [(0, BOS, 1), (0, 7, 0), (1, 3, 2), (1, 4, 3), (1, 8, 1), (2, 5, 4), (2, 9, 2), (3, 5, 4), (3, 6, 5), (4, 3, 5), (4, 0, 4),
                        (5, EOS, 6), (6, PAD, 6)])
    loops_w = make(7, V, [(0, BOS, 1), (0, 7, 0), (1, 3, 2), (1, 4, 3), (1, 8, 1), (2, 5, 4), (3, 5, 4), (3, 6, 5), (4, 3, 5), (5, EOS, 6),
                          (5, 11, 5), (6, PAD, 6)], weight_seed=12)
    f = frozenset
    all_modes = (0, 1, 2)
    out = [
        # 300 states, 130 parallel arcs per step: 4 A + 8 n = 157 884 > 155 648; 5 n + n_dp beyond LDS as well
        Case("arcs_beyond_lds", [chain([130] * 299)], f({"arcs_beyond_lds"}), all_modes, False),
        # 4000 states, 3 .. 5 parallel arcs per step and a skip arc: A + 2 n = 27 996 <= 38 912 < 5 n + n_dp = 39 991
        Case("ranks_in_global", [chain([3 + i % 3 for i in range(3999)], vocab=24, skip_label=20)], f({"ranks_in_global"}), all_modes, False,
             only=f({"ranks_in_global"})),
        # 8000 states; one step of 33 parallel arcs: two passes under 8-lane groups, 8000 levels x 5 words beyond the table
        Case("counters_in_global", [chain([1] * 4000 + [33] + [1] * 3998 + [2])], f({"counters_in_global", "count_falls_back"}), all_modes, False),
        # 5600 levels; state 3001 has exactly 64 in-arcs (and 3000 as many out-arcs): three passes both ways, 5600 x 7 > 38 912
        Case("count_falls_back", [chain([1] * 3000 + [64] + [1] * 2599)], f({"count_falls_back"}), (0, 1), False, only=f({"count_falls_back"})),
        # 7800 levels; one step of 257 parallel arcs: two passes under 64-lane groups as well (and a tree of 9 partial groups
        # under 8-lane groups), so both programs of both directions are counted by laying them out: 7800 x 5 > 38 912.
        # (No more rows: alpha and beta of 7800 + 9 rows and 260 labels are what fits the sweeps' LDS beside four ring slots.)
        Case("count_falls_back_wide", [chain([1] * 5000 + [257] + [1] * 2798)], f({"count_falls_back", "count_falls_back_wide", "counters_in_global"}),
             (0, 2), False),
        Case("junk_acyclic", [j["junk_acyclic"]], f({"junk_arcs", "junk_into_reachable"}), all_modes, True),
        Case("junk_cycle", [j["junk_cycle"]], f({"junk_arcs", "second_relaxation", "junk_into_reachable"}), all_modes, True),
        Case("junk_self_loop", [j["junk_self_loop"]], f({"junk_arcs", "junk_self_loop"}), all_modes, True),
        Case("junk_dead_end", [j["junk_dead_end"]], f({"junk_arcs", "junk_dead_end"}), all_modes, True),
        Case("junk_low_ids", [j["junk_low_ids"]], f({"junk_arcs", "junk_low_ids"}), all_modes, True),
        Case("junk_weighted", [j["junk_weighted"]], f({"junk_arcs", "junk_weighted", "junk_low_ids", "second_relaxation"}), all_modes, True),
        Case("inner_self_loops", [loops], f({"inner_self_loops", "self_loop_at_0"}), all_modes, True),
        Case("inner_self_loops_weighted", [loops_w], f({"inner_self_loops", "self_loop_at_0"}), all_modes, True),
        Case("one_row", [one_row], f({"one_row", "zero_arcs"}), all_modes, True),
        Case("no_arcs_mid_batch", [tiny, no_arcs, j["junk_low_ids"], one_row, tiny], f({"no_arcs_mid_batch", "one_row"}), all_modes, True),
        Case("zero_arcs", [no_arcs, one_row, no_arcs], f({"zero_arcs", "one_row"}), all_modes, True),
        Case("many", _many(), f({"many", "junk_arcs"}), (0,), False),
        # 5500 states of fan-in 64 under 8-lane groups: 3 pieces each, 16 500 > 16 384 sort keys
        Case("limit_pieces", [chain([64] * 5500)], f({"limit_pieces"}), (1,), False),
        # 8190 rows, one state of fan-in 65 under 8-lane groups: a tree of 3 partial groups, 8190 + 3 > 8192
        Case("limit_rows", [chain([1] * 4000 + [65] + [1] * 4188)], f({"limit_rows"}), (1,), False),
    ]
    return {c.name: c for c in out}


def batch_arcs(lats):
    """(n_rows [B], arc_off [B + 1], src, label, dst, weight | None) of a batch"""
    n_rows = np.array([l.n_rows for l in lats], dtype=np.int32)
    arc_off = np.zeros(len(lats) + 1, dtype=np.int64)
    arc_off[1:] = np.cumsum([l.n_arcs for l in lats])
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    w = cat([l.weight for l in lats], np.float32) if all(l.weight is not None for l in lats) else None
    return n_rows, arc_off, cat([l.src for l in lats], np.int32), cat([l.label for l in lats], np.int32), cat([l.dst for l in lats], np.int32), w


def reachable_arcs(l: Lat):
    """(src, label, dst, weight | None) of the arcs whose source state 0 reaches, by the breadth-first search of
    ``analyse``: what the float64 oracle is given"""
    keep = analyse(l)["canon"]
    return l.src[keep], l.label[keep], l.dst[keep], None if l.weight is None else l.weight[keep]


# ---------------------------------------------------------------- what the packers refuse
ERR_ARG, ERR_INDEX, ERR_CYCLE, ERR_SINK, ERR_DETERMINISM, ERR_LIMIT = -1, -2, -3, -4, -5, -6
ERROR_VOCAB = 8


def error_rows():
    """(name, [(n_rows, src, label, dst), ...], code, lattice): batches of raw arc lists (as given: not sorted here) and
    the refusal both packers owe them -- the first offending arc of the first bad lattice decides, a lattice that is
    cyclic and has not exactly one sink is refused for its sinks.  code None: accepted."""
    good = (4, [0, 1, 2, 3], [1, 3, 2, 0], [1, 2, 3, 3])
    good2 = (5, [0, 0, 1, 2, 3], [1, 3, 4, 4, 2], [1, 2, 3, 3, 4])
    cyc = (4, [0, 1, 2, 2], [1, 3, 3, 4], [1, 2, 1, 3])  # 0 -> 1 -> 2 -> 1, 2 -> 3
    dup = (3, [0, 0, 1], [3, 3, 2], [1, 1, 2])
    one = lambda name, lat, code: (name, [lat], code, 0)
    return [
        one("source beyond the rows", (3, [0, 5], [1, 3], [1, 2]), ERR_INDEX),
        one("destination beyond the rows", (2, [0], [3], [5]), ERR_INDEX),
        one("destination = n_rows", (2, [0], [3], [2]), ERR_INDEX),
        one("label = vocab", (2, [0], [ERROR_VOCAB], [1]), ERR_INDEX),
        one("negative source", (2, [-1], [3], [1]), ERR_INDEX),
        one("negative destination", (2, [0], [3], [-1]), ERR_INDEX),
        one("negative label", (2, [0], [-2], [1]), ERR_INDEX),
        one("unsorted sources", (3, [0, 1, 0], [1, 2, 4], [1, 2, 2]), ERR_ARG),
        one("repeated (state, label)", dup, ERR_DETERMINISM),
        one("falling label inside a state", (3, [0, 0, 1], [4, 3, 2], [1, 1, 2]), ERR_DETERMINISM),
        one("repeated label, then a bad destination", (4, [0, 0, 0, 1], [1, 1, 3, 2], [1, 1, 9, 2]), ERR_DETERMINISM),
        one("bad destination, then a repeated label", (4, [0, 0, 0, 1], [1, 3, 3, 2], [1, 9, 1, 2]), ERR_INDEX),
        one("unsorted source, then a repeated label", (4, [0, 1, 0, 0], [1, 2, 3, 3], [1, 2, 2, 2]), ERR_ARG),
        one("repeated label, then an unsorted source", (4, [0, 0, 1, 0], [3, 3, 2, 4], [1, 1, 2, 2]), ERR_DETERMINISM),
        one("a cycle", cyc, ERR_CYCLE),
        one("a cycle and two sinks", (5, [0, 0, 0, 1, 2], [3, 4, 5, 3, 3], [1, 3, 4, 2, 1]), ERR_SINK),
        one("two sinks", (3, [0, 0], [3, 4], [1, 2]), ERR_SINK),
        one("no sink at all", (3, [0, 1, 2], [3, 3, 3], [1, 2, 1]), ERR_SINK),
        one("an arc back into state 0", (3, [0, 1, 1], [3, 3, 4], [1, 0, 2]), ERR_CYCLE),
        one("a cycle among unreachable states only", (6, [0, 1, 3, 4, 5], [1, 2, 3, 3, 3], [1, 2, 4, 5, 3]), None),
        one("a state whose only out-arc is a self loop, beside the sink", (4, [0, 0, 1, 2], [3, 4, 5, 3], [1, 2, 1, 3]), ERR_SINK),
        one("n_rows = 0", (0, [], [], []), ERR_ARG),
        one("more rows than the engine takes", (9000, [0], [3], [1]), ERR_LIMIT),
        ("a bad lattice at b = 2 of 6", [good, good2, cyc, good, good2, good], ERR_CYCLE, 2),
        ("two bad lattices: the first is reported", [good, cyc, good2, dup, good], ERR_CYCLE, 1),
        ("two bad lattices, the other order", [good, dup, good2, cyc, good], ERR_DETERMINISM, 1),
    ]


def raw_batch(lats):
    """(n_rows, arc_off, src, label, dst) of raw (n_rows, src, label, dst) tuples"""
    n_rows = np.array([l[0] for l in lats], dtype=np.int32)
    arc_off = np.zeros(len(lats) + 1, dtype=np.int64)
    arc_off[1:] = np.cumsum([len(l[1]) for l in lats])
    cat = lambda k: np.concatenate([np.asarray(l[k], dtype=np.int32) for l in lats])
    return n_rows, arc_off, cat(1), cat(2), cat(3)

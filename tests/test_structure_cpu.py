"""The structural corpus of tests/structure_cases.py and the references of tests/*_ref.py on it (no GPU).

The corpus is held to its claims: the union of its features covers ``FEATURES``, every entry has the features it is named
after.  Then every reference that tests/test_gpu_structure.py compares a kernel with is held to plain enumeration of all
paths on every lattice of the corpus, in the engine's numbering (``structure_cases.canonical``): integers, arcs and paths
exactly, float64 sums to 1e-12 relative (a float64 reference against a float64 enumeration, not a kernel tolerance),
float32 restatements to the rounding of their own adds (``paths_ref.path_guard``: depth * 2^-23 * the largest partial
sum).  A choice between paths is compared where the enumeration's gap between them exceeds GAP, far above that rounding.
"""
import json
import os

import numpy as np
import pytest

from nfst_amd import synth
from tests import beam_ref, edge_cases as E, expectation_ref as X, intersect_ref, intersect_wide_ref, kbest_ref, lattice_edit_ref
from tests import pack_cases as PC
from tests import paths_ref, positional_expectation_ref as PE, positional_kbest_ref as PK, positional_ref as P
from tests import positional_sample_ref as PS, positional_swor_ref as PW, slack_ref, structure_cases as S, swor_ref

F32 = np.float32
RTOL = 1e-12   # float64 reference against float64 enumeration
GAP = 1e-3     # two paths whose float64 scores differ by more are told apart by every float32 restatement here
ENTRIES = S.entries()
THETA = S.theta()


def lattices():
    """(name, canonical lattice) of every lattice of the corpus"""
    out = []
    for name, e in ENTRIES.items():
        for i, l in enumerate(e.lats):
            out.append((f"{name}[{i}]", S.canonical(l)))
    return out


LATS = lattices()
IDS = [n for n, _ in LATS]


def close(a, b, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    both_inf = np.isinf(a) & (a == b)
    with np.errstate(invalid="ignore"):
        err = np.where(both_inf, 0.0, np.abs(a - b))
    assert np.all(err <= RTOL * np.maximum(np.abs(b), 1.0)), (what, float(np.max(err)))


def paths_of(l, score64):
    """[(score, arcs)] best first, by plain enumeration with the helper's sink"""
    return kbest_ref.enumerate_paths(l.n_rows, l.src, l.dst, score64, S.sink(l))


def arc_extra(l, seed=3):
    return np.random.default_rng(seed).normal(0.0, 0.4, size=l.n_arcs).astype(F32)


def pos_scores(T, V, seed=5):
    return np.random.default_rng(seed).normal(0.0, 0.5, size=(T, V)).astype(F32)


# ----------------------------------------------------------------------------- the corpus
def test_corpus_covers_the_features():
    got = set()
    for name, e in ENTRIES.items():
        per = [S.features(l) for l in e.lats]
        assert e.features <= set().union(*per), (name, e.features - set().union(*per))
        got |= set().union(*per)
    assert got >= set(S.FEATURES), set(S.FEATURES) - got
    for l in S.many_with_junk():
        S.features(l)  # (asserts one sink, no cycle)
    assert len(S.many_with_junk()) > PC.N_CUS


def test_entries_are_what_they_are_named_after():
    # sink_below_reachable: the example of the corpus's docstring
    l = ENTRIES["sink_below_reachable"].lats[0]
    a = PC.analyse(l)
    assert a["sinks"] == [3] and a["reach"].all() and l.n_rows == 7
    # self_loop_in_chunks: 130 out-arcs, the loop at each of the four positions of the sorted list; the sibling at state 0
    for l, p, hub in [(x, q, 1) for x, q in zip(ENTRIES["self_loop_in_chunks"].lats, S.CHUNK_POSITIONS)] + [(ENTRIES["self_loop_in_chunks_at_0"].lats[0], 64, 0)]:
        c = S.canonical(l)
        own = np.flatnonzero(c.src == hub)
        assert len(own) == S.DEGREE == 130 and np.all(np.diff(c.label[own]) > 0)
        assert np.flatnonzero(c.dst[own] == hub).tolist() == [p]
    # pad_rows_behind_sink: rows behind the shorter lattice's sink, and the arc lists are the tables'
    for name in ("pad_rows_behind_sink", "pad_rows_behind_sink_weighted"):
        e = ENTRIES[name]
        small = PC.analyse(e.lats[1])
        assert small["sinks"] == [4] and not small["reach"][5:].any() and len(small["junk"]) == 2 * S.V
        for l, (em, tr) in zip(e.lats, zip(*e.dense)):
            em2, tr2 = l.dense(weighted=l.weight is not None)
            assert np.array_equal(em2, em) and np.array_equal(tr2[em2 > -np.inf] if l.weight is not None else tr2[em2], tr[em > -np.inf] if l.weight is not None else tr[em])
    # state 0 is the sink
    for l in (S.one_row(), S.no_arcs()):
        assert S.sink(l) == 0 and S.n_paths(l) == 1
    # sizes
    for name, e in ENTRIES.items():
        for l in e.lats:
            assert l.n_rows < 300 and l.n_arcs < 400 and S.n_paths(l) <= (129 if "chunks" in name else 36), name
    b = S.batches()
    assert sum(l.n_arcs for l in b["zero_arcs"]) == 0
    for name in ("unweighted", "weighted"):
        arcs = [l.n_arcs for l in b[name]]
        zero = [i for i, n in enumerate(arcs) if n == 0]
        assert len(zero) == 2 and all(0 < i < len(arcs) - 1 and arcs[i - 1] and arcs[i + 1] for i in zero)
        assert len({l.weight is None for l in b[name]}) == 1 and len({l.vocab for l in b[name]}) == 1
        assert {l.n_rows for l in b[name] if l.n_arcs == 0} == {1, 3}


@pytest.mark.parametrize("name", ["self_loop_only_alternative", "self_loop_only_alternative_weighted"])
def test_self_loop_is_the_best_candidate_by_raw_score(name):
    """Without the ``src != dst`` filter the answer changes: at both looped states the loop has the largest raw score of
    the state's arcs, and a path that took a loop once would beat the best real path."""
    l = S.canonical(ENTRIES[name].lats[0])
    sc = E.score64(l, THETA)
    loops = np.flatnonzero(l.src == l.dst)
    inner = [a for a in loops if l.src[a] not in (0, S.sink(l))]
    assert len(inner) == 2
    for a in inner:
        own = np.flatnonzero(l.src == l.src[a])
        assert int(own[np.argmax(sc[own])]) == a and sc[a] > 0
    best = paths_of(l, sc)[0]
    on_best = [a for a in inner if l.src[a] in l.src[best[1]]]
    assert on_best, "no looped state on the best path"
    unfiltered = best[0] + max(sc[a] for a in on_best)  # the best walk that may take each loop once
    assert unfiltered > best[0] + GAP
    v = paths_ref.viterbi_f64(l, sc)
    assert v["arcs"].tolist() == best[1] and not set(v["arcs"].tolist()) & set(loops.tolist())


def test_the_helper_is_the_last_row_on_synth_lattices():
    """... so every reference returns on them what it returned with ``n_rows - 1``."""
    lats = E.mixed_batch() + E.weighted_batch() + [E.star(), E.double_funnel(), swor_ref.small_lattice(), swor_ref.over_cap_lattice(),
                                                   synth.edit_lattice([10, 11, 12], [20, 21], vocab=64, seed=1)]
    for l in lats:
        assert X.sink_of(l.n_rows, l.src, l.dst) == l.n_rows - 1
    with pytest.raises(AssertionError):
        X.sink_of(3, [0, 0], [1, 2])  # two states without an out-arc
    with pytest.raises(AssertionError):
        X.sink_of(3, [0, 1, 2], [1, 2, 1])  # none
    assert X.sink_of(4, [0, 1, 1, 2, 3], [1, 1, 2, 2, 0]) == 2  # self loops do not count, junk into state 0 is ignored


def fingerprint(l, theta):
    """A few numbers of every reference that took ``n_rows - 1`` for the sink, on one lattice; floats as hex strings."""
    h = lambda x: float(x).hex()
    out = {}
    v = paths_ref.viterbi_ref(l, theta, l.weight)
    out["viterbi_ref"] = [h(v["best"]), int(np.sum(v["arcs"])), v["length"]]
    sc = E.score64(l, theta)
    out["viterbi_f64"] = h(paths_ref.viterbi_f64(l, sc)["best"])
    r = slack_ref.arc_slack(l, theta, beam=1.0)
    out["arc_slack"] = [h(r["best"]), h(np.sum(r["slack"][np.isfinite(r["slack"])], dtype=np.float64)), r["n_kept"], bool(slack_ref.is_trim(l, r["keep"]))]
    out["vbeta"] = h(np.sum(beam_ref.vbeta(l, theta), dtype=np.float64))
    lb, z = swor_ref.backward64(l, sc)
    out["backward64"] = [h(z), h(lb.sum())]
    ref = l.label[v["arcs"]][::2].astype(np.int64)
    e = lattice_edit_ref.of_lattice(l, ref, theta)
    out["lattice_edit"] = [e["distance"], h(e["score"]), int(np.sum(e["arcs"])), list(e["counts"])]
    V = l.vocab
    d = np.stack([np.zeros(V, np.int64), np.ones(V, np.int64)]); d[0, 5], d[1, 5] = 1, 0
    f = np.array([1, 0])
    p, w = intersect_ref.intersect(l, d, f), intersect_wide_ref.intersect(l, d, f)
    out["intersect"] = [p["n_rows"], p["n_arcs"], int(p["arc_map"].sum()), int(p["row_q"].sum())]
    out["intersect_wide"] = [w["n_rows"], w["n_arcs"], int(w["arc_map"].sum()), int(w["row_q"].sum())]
    lo, hi = P.min_max_len(l)
    out["min_max_len"] = [lo, hi]
    T = (lo + hi) // 2 + 1
    pos = np.random.default_rng(T).normal(0.0, 0.5, size=(T, V)).astype(np.float32)
    s = P.sum_product(l, P.arc_score64(l, theta), pos, T)
    out["sum_product"] = [T, h(s["logz"]), h(np.sum(s["len_logz"][np.isfinite(s["len_logz"])])), h(s["arc_post"].sum())]
    m = P.max_plus(l, theta, pos, T)
    out["max_plus"] = [h(m["best"]), int(np.sum(m["arcs"]))]
    kb = PK.k_best(l, theta, pos, T, 3)
    out["positional_k_best"] = [[h(x) for x in kb["best"]], kb["n_paths"], int(sum(map(sum, kb["arcs"])))]
    pe = PE.expectation(l, P.arc_score64(l, theta), pos, T, label_values=np.arange(V) / V, coef=0.5)
    out["positional_expectation"] = [h(pe["logz"]), h(pe["ev"]), h(pe["arc_cov"].sum())]
    smp = PS.Sampler(l, P.arc_score64(l, theta), pos, T)
    wk = smp.walk(PS.uniforms(3, 1, T)[0])
    out["positional_sample"] = [h(smp.logz), int(sum(wk["arcs"])), h(wk["logq"])]
    D = int(np.diff(swor_ref.out_arcs(l)).max())
    u = np.random.default_rng(4).random((T, 2, D), dtype=np.float32)
    sw = PW.search(l, swor_ref.arc_score32(l, theta), pos, smp.beta, smp.logz, 2, T, u)
    out["positional_swor"] = [sw["n_paths"], int(sum(map(sum, sw["arcs"]))), h(sw["kappa"])]
    return out


def test_references_return_what_they_returned_on_the_mixed_batch(golden_dir):
    """tests/golden/structure_refs_mixed_batch.json was written by ``fingerprint`` with the references as they were when
    they took ``n_rows - 1`` for the sink: every number is the same now, bit for bit."""
    with open(os.path.join(golden_dir, "structure_refs_mixed_batch.json")) as f:
        before = json.load(f)
    theta = synth.label_scores(8, E.V_MIXED)
    lats = E.mixed_batch()
    assert len(before) == len(lats)
    for b, l in enumerate(lats):
        now = json.loads(json.dumps(fingerprint(l, theta)))
        assert now == before[b], (b, {k: (now[k], before[b][k]) for k in now if now[k] != before[b][k]})


# ----------------------------------------------------------------------------- max-plus: Viterbi, k-best, slack, beam
@pytest.mark.parametrize("name,l", LATS, ids=IDS)
def test_max_plus_references(name, l):
    asc = arc_extra(l)
    sc = E.score64(l, THETA, asc)
    paths = paths_of(l, sc)
    sink = S.sink(l)
    best, n = paths_ref.brute_force_best(l, sc)
    assert n == len(paths) == S.n_paths(l) and best == paths[0][0]
    v64 = paths_ref.viterbi_f64(l, sc)
    close(v64["best"], best, "viterbi_f64")
    decided = len(paths) < 2 or paths[0][0] - paths[1][0] > GAP
    assert decided, "the corpus's scores leave the best path undecided"
    assert v64["arcs"].tolist() == paths[0][1]
    for order in ("general", "tile_waves"):
        v = paths_ref.viterbi_ref(l, THETA, l.weight, asc, order=order)
        assert v["arcs"].tolist() == paths[0][1] and v["length"] == len(paths[0][1]), order
        gap, bound = paths_ref.path_guard(l, sc, v["arcs"])
        assert gap <= bound and abs(float(v["best"]) - best) <= max(bound, 0.0) + 2.0 ** -23 * abs(best), order
    # k-best: k = 1, and more than there are paths (or the top 64 of the 129)
    th, e = kbest_ref.arc_terms(l, THETA, asc)
    for k in (1, 64):
        r = kbest_ref.k_best(l.n_rows, l.src, l.dst, th, e, k, sink)
        m = min(k, len(paths))
        assert r["n_paths"] == m
        np.testing.assert_allclose(r["best"][:m], [s for s, _ in paths[:m]], rtol=0, atol=1e-5)
        cut = m == len(paths) or paths[m - 1][0] - paths[m][0] > GAP
        if cut:
            assert sorted(map(tuple, r["arcs"])) == sorted(tuple(p) for _, p in paths[:m])
        sure = [i for i in range(m) if (i == 0 or paths[i - 1][0] - paths[i][0] > GAP) and (i + 1 >= len(paths) or paths[i][0] - paths[i + 1][0] > GAP)]
        assert all(r["arcs"][i] == paths[i][1] for i in sure) and (sure or not paths or len(paths) > 3)
    assert kbest_ref.count_finite_paths(l.n_rows, l.src, l.dst, sc, sink) == len(paths)
    # slack against the float64 max-marginals by enumeration
    mm = slack_ref.max_marginals64(l, THETA, asc)
    r = slack_ref.arc_slack(l, THETA, asc, beam=1.0)
    loop = l.src == l.dst
    assert np.all(np.isneginf(mm[loop]))
    if l.n_arcs:
        on = ~loop
        np.testing.assert_allclose(r["slack"][on], best - mm[on], rtol=0, atol=1e-5)
        assert np.array_equal(r["keep"][on], (best - mm[on]) <= 1.0) or np.min(np.abs(best - mm[on] - 1.0)) < 1e-5
        assert slack_ref.is_trim(l, r["keep"])
    depth = X.levels(l.n_rows, l.src, l.dst)
    assert np.all(np.isneginf(r["vbeta"][depth < 0])) and np.all(np.isposinf(r["state_slack"][depth < 0]))
    assert r["vbeta"][sink] == 0.0 and abs(float(r["best"]) - best) <= 1e-5
    # the beam search's look-ahead (no arc scores): the same recursion
    vb = beam_ref.vbeta(l, THETA)
    r0 = slack_ref.arc_slack(l, THETA)
    assert np.array_equal(vb, r0["vbeta"]) and np.all(np.isneginf(vb[depth < 0]))


# ----------------------------------------------------------------------------- sum-product: expectation, backward, SWOR
@pytest.mark.parametrize("name,l", LATS, ids=IDS)
def test_sum_product_references(name, l):
    asc = arc_extra(l)
    sc = E.score64(l, THETA, asc)
    val = np.random.default_rng(9).normal(0.0, 1.0, size=l.n_arcs)
    sink = S.sink(l)
    b = X.brute_force(l.n_rows, l.src, l.dst, sc, val, sink)
    assert b["n_paths"] == S.n_paths(l)
    if l.n_arcs:  # (the float64 oracle takes lattices with arcs)
        r = X.expectation(l.n_rows, l.src, l.dst, sc, val)
        for key in ("logZ", "ev", "posterior", "cov"):
            close(r[key], b[key], key)
        assert np.all(r["posterior"][l.src == l.dst] == 0.0)
        h = X.entropy(l.n_rows, l.src, l.dst, sc)
        assert abs(h["H"] - b["H"]) <= 1e-11 * max(1.0, abs(b["logZ"]))
    depth = X.levels(l.n_rows, l.src, l.dst)
    assert depth[sink] == max(depth) and depth[0] == 0
    lb, z = swor_ref.backward64(l, sc)
    close(z, b["logZ"], "backward64")
    assert np.all(np.isneginf(lb[depth < 0])) and lb[sink] == 0.0 and np.all(np.isfinite(lb[depth >= 0]))
    listed = swor_ref.enumerate_paths(l, sc)
    assert sorted(a for a, _ in listed) == sorted(tuple(p) for _, p in paths_of(l, sc))
    # without replacement: k at or above the number of paths returns every path once
    n = len(listed)
    if n <= 64:
        k = 64
        u = swor_ref.uniforms_for([l], k, seed=1, max_len=int(depth.max()) + 1)[0] if l.n_arcs else np.zeros((1, k, 1), F32)
        s = swor_ref.search(l, swor_ref.arc_score32(l, THETA, asc), lb, z, k, u.shape[0], u)
        assert s["status"] == 0 and s["n_paths"] == n and s["kappa"] == -np.inf
        assert sorted(map(tuple, s["arcs"])) == sorted(a for a, _ in listed)
        want = {a: x - z for a, x in listed}
        np.testing.assert_allclose(s["logp64"], [want[tuple(a)] for a in s["arcs"]], rtol=0, atol=1e-5)  # (float32 arc scores)


# ----------------------------------------------------------------------------- lattice edit distance
@pytest.mark.parametrize("name,l", LATS, ids=IDS)
def test_lattice_edit_reference(name, l):
    sc = E.score64(l, THETA)
    paths = paths_of(l, sc)
    longest = max(len(p) for _, p in paths)
    best_labels = l.label[paths[-1][1]].astype(np.int64)  # the worst path's labels: the oracle path is not the Viterbi path
    refs = [np.zeros(0, np.int64), np.full(longest + 3, S.HI, np.int64), best_labels,
            np.concatenate([best_labels[:1], [S.HI, 8, 7], best_labels[1:]])]  # (the labels the self loops carry, inserted)
    for ref in refs:
        bf = lattice_edit_ref.brute_force(l, ref, sc)
        for scored in (False, True):
            r = lattice_edit_ref.of_lattice(l, ref, THETA if scored else None)
            assert r["distance"] == bf["distance"] and sum(r["counts"]) == r["distance"], (name, len(ref))
            assert not set(r["arcs"]) & set(np.flatnonzero(l.src == l.dst).tolist())
            n_sub, n_ins, n_del = r["counts"]
            assert len(r["arcs"]) == len(ref) + n_ins - n_del
            if scored:
                assert abs(float(r["score"]) - bf["best"]) <= 1e-5
                if len(bf["ties"]) < 2 or bf["ties"][-1] - bf["ties"][-2] > GAP:
                    assert r["arcs"] == bf["best_arcs"]
            if not len(paths[0][1]):  # state 0 is the sink: le_fold's sink cell
                assert r["distance"] == len(ref) and r["counts"] == (0, 0, len(ref)) and r["arcs"] == [] and float(r["score"]) == 0.0


# ----------------------------------------------------------------------------- intersection
def automata(V):
    """name -> (delta [Q, V], final [Q]): everything, nothing, no label HI (the loops of self_loop_only_alternative), no
    label 8 (loops of inner_self_loops and of the padded pair), an even number of label 5 (two states)."""
    everything = (np.zeros((1, V), np.int64), np.ones(1, np.int64))
    nothing = (np.zeros((1, V), np.int64), np.zeros(1, np.int64))
    out = {"everything": everything, "nothing": nothing}
    for lab in (S.HI, 8, 4):
        d = np.zeros((1, V), np.int64)
        d[0, lab] = -1
        out[f"no label {lab}"] = (d, np.ones(1, np.int64))
    d = np.stack([np.zeros(V, np.int64), np.ones(V, np.int64)])
    d[0, 5], d[1, 5] = 1, 0
    out["even number of 5"] = (d, np.array([1, 0]))
    return out


@pytest.mark.parametrize("name,l", LATS, ids=IDS)
def test_intersect_references(name, l):
    paths = P.enumerate_paths(l)
    depth = X.levels(l.n_rows, l.src, l.dst)
    for tag, (delta, final) in automata(l.vocab).items():
        p = intersect_ref.intersect(l, delta, final)
        w = intersect_wide_ref.intersect(l, delta, final)
        for key in p:
            assert np.array_equal(p[key], w[key]), (tag, key)
        want = sorted((tuple(int(x) for x in l.label[q]), tuple(q)) for q in paths if intersect_ref.run(delta, final, l.label[q]))
        if l.n_arcs == 0 and want:  # state 0 is the sink: the product is the one row, when the start state is final
            assert p["n_rows"] == 1 and p["n_arcs"] == 0 and p["row_state"].tolist() == [0]
            continue
        assert sorted(intersect_ref.product_paths(p)) == want, tag
        assert np.all(depth[p["row_state"]] >= 0)  # no row for a state that state 0 does not reach
        if tag == "everything":  # every reachable state, every canonical arc, self loops included
            assert p["row_state"].tolist() == np.flatnonzero(depth >= 0).tolist() and p["arc_map"].tolist() == list(range(l.n_arcs))


# ----------------------------------------------------------------------------- the positional references
def budgets(l):
    lo, hi = P.min_max_len(l)
    return sorted({max(hi - 1, 0), hi, hi + 2})


@pytest.mark.parametrize("name,l", LATS, ids=IDS)
def test_positional_references(name, l):
    paths = P.enumerate_paths(l)
    lens = sorted({len(p) for p in paths})
    assert P.min_max_len(l) == (lens[0], lens[-1])
    sc = P.arc_score64(l, THETA)
    sink = S.sink(l)
    depth = X.levels(l.n_rows, l.src, l.dst)
    for T in budgets(l):
        pos = pos_scores(T, l.vocab)
        b = P.brute_force(l, sc, pos, T, paths)
        r = P.sum_product(l, sc, pos, T)
        for key in ("logz", "len_logz", "pos_post", "arc_post"):
            close(r[key], b[key], (key, T))
        # max-plus: the best path that fits, the loops never
        m = P.max_plus(l, THETA, pos, T)
        assert np.all(np.isneginf(m["vb"][:, depth < 0])) and np.all(m["vb"][:, sink] == 0.0)
        if np.isfinite(b["best"]):
            assert abs(float(m["best"]) - b["best"]) <= 1e-5
            if b["best"] - b["runner_up"] > GAP:
                assert m["arcs"] == b["best_arcs"]
        else:
            assert np.isneginf(m["best"]) and m["arcs"] == []
        # k-best
        fit = sorted((x for x in ((sum(sc[a] + float(pos[t, l.label[a]]) for t, a in enumerate(p)), p) for p in paths if len(p) <= T)), key=lambda x: -x[0])
        for k in (1, 64):
            kb = PK.k_best(l, THETA, pos, T, k)
            n = min(k, len(fit))
            assert kb["n_paths"] == n
            np.testing.assert_allclose(kb["best"][:n], [x for x, _ in fit[:n]], rtol=0, atol=1e-5)
            if n == len(fit) or fit[n - 1][0] - fit[n][0] > GAP:
                assert sorted(map(tuple, kb["arcs"])) == sorted(tuple(p) for _, p in fit[:n])
        # expectation
        rng = np.random.default_rng(T)
        pv, lv, av = rng.normal(size=(T, l.vocab)), rng.normal(size=l.vocab), rng.normal(size=l.n_arcs)
        be = PE.brute_force(l, sc, pos, T, pv, lv, av, 0.3, paths)
        re = PE.expectation(l, sc, pos, T, pv, lv, av, 0.3)
        for key in PE.KEYS:
            close(re[key], be[key], (key, T))
        # the sampler: its beta rows, and every walk is a path that fits, at its exact probability
        beta = PS.beta_rows(l, sc, pos, T)
        close(beta[0, 0], b["logz"], "beta rows")
        assert np.all(np.isneginf(beta[:, depth < 0]))
        if np.isfinite(b["logz"]):
            sm = PS.Sampler(l, sc, pos, T)
            U = PS.uniforms(11, 16, max(T, 1))
            for wk in sm.walks(U):
                assert wk["arcs"] in [list(p) for p in paths] and wk["length"] <= T
                want = sum(sc[a] + float(pos[t, l.label[a]]) for t, a in enumerate(wk["arcs"])) - b["logz"]
                assert abs(wk["logq"] - want) <= 1e-11 * max(1.0, abs(want))
                assert abs(sm.path_logprob(wk["arcs"]) - want) <= 1e-11 * max(1.0, abs(want))
            # without replacement: k above the number of paths that fit returns each of them once
            if len(fit) <= 64:
                D = max(int(np.diff(swor_ref.out_arcs(l)).max()), 1) if l.n_arcs else 1
                u = np.random.default_rng([3, T]).random((max(T, 1), 64, D), dtype=F32)
                s = PW.search(l, swor_ref.arc_score32(l, THETA), pos, beta, b["logz"], 64, T, u)
                assert s["status"] == 0 and sorted(map(tuple, s["arcs"])) == sorted(tuple(p) for _, p in fit)

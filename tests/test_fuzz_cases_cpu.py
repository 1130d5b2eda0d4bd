"""The random corpus of tests/fuzz_cases.py and the references of tests/*_ref.py on it (no GPU).

The draws are pinned (a digest of every draw in tests/golden/fuzz_cases_digests.json); the references that
tests/test_gpu_fuzz_paths.py compares kernels with are held to plain enumeration on every drawn member of at most
``fuzz_cases.ENUMERABLE`` paths, with the comparisons of tests/test_structure_cpu.py (float64 against float64 at 1e-12
relative, a choice between paths where the enumeration's gap exceeds GAP); the derived corpora are what they claim to be;
and the draws reach, by name, the branches the corpus exists for."""
import dataclasses
import json
import os

import numpy as np
import pytest

from tests import beam_ref, expectation_ref as X, fuzz_cases as F, intersect_ref, kbest_ref, lattice_edit_ref, paths_ref
from tests import positional_expectation_ref as PE, positional_kbest_ref as PK, positional_ref as P, positional_sample_ref as PS
from tests import positional_swor_ref as PW, slack_ref, strings_ref as SR, structure_cases as S, swor_ref

RTOL = 1e-12   # float64 reference against float64 enumeration
GAP = 1e-3     # two paths whose float64 scores differ by more are told apart by every float32 restatement here
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_cases_digests.json")
ALL = [(s, i) for s in F.SEEDS for i in range(F.ITERS)]
_DRAWS, _DERIVED = {}, {}


def draw(seed, it):
    if (seed, it) not in _DRAWS:
        _DRAWS[seed, it] = F.draw(seed, it)
    return _DRAWS[seed, it]


def derived(seed, it):
    if (seed, it) not in _DERIVED:
        _DERIVED[seed, it] = F.derived(draw(seed, it))
    return _DERIVED[seed, it]


def close(a, b, what="", scale=1.0):
    """``scale``: the magnitude that the compared sums cancel from (the M of an expectation), where it exceeds 1"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    both_inf = np.isinf(a) & (a == b)
    with np.errstate(invalid="ignore"):
        err = np.where(both_inf, 0.0, np.abs(a - b))
    assert np.all(err <= RTOL * np.maximum(np.abs(b), max(1.0, scale))), (what, float(np.max(err)))


def enumerable(l) -> bool:
    return F.count_paths(l) <= F.ENUMERABLE


# ----------------------------------------------------------------------------- determinism
def test_every_draw_is_pinned():
    got = {f"{s}.{i}": F.digest(F.draw(s, i)) for s, i in ALL}  # (drawn afresh: not the cached objects)
    assert got == {f"{s}.{i}": F.digest(draw(s, i)) for s, i in ALL}
    with open(GOLDEN) as f:
        assert got == json.load(f)


# ----------------------------------------------------------------------------- the references against enumeration
@pytest.mark.parametrize("seed", F.SEEDS)
def test_references_against_enumeration(seed):
    """Expectation, k best, Viterbi (both add orders) and arc slack on every enumerable member of the seed's draws."""
    done = small = small_done = 0
    for it in range(F.ITERS):
        d = draw(seed, it)
        for b, l in enumerate(d.canon):
            is_small = d.states[b] <= 40  # (the drawn number of states: junk rows do not move a member out of the count)
            small += is_small
            if not enumerable(l):
                continue
            done += 1
            small_done += is_small
            theta, asc, sink = d.theta_of(b), d.asc_of(b), S.sink(l)
            sc = d.score64(b)
            paths = kbest_ref.enumerate_paths(l.n_rows, l.src, l.dst, sc, sink)
            assert kbest_ref.count_finite_paths(l.n_rows, l.src, l.dst, sc, sink) == len(paths) <= F.count_paths(l)
            # sum-product
            if l.n_arcs and np.isfinite(sc[l.src != l.dst]).all():
                val = np.random.default_rng(9).normal(0.0, 1.0, size=l.n_arcs)
                bf = X.brute_force(l.n_rows, l.src, l.dst, sc, val, sink)
                r = X.expectation(l.n_rows, l.src, l.dst, sc, val)
                assert bf["n_paths"] == len(paths)
                for key in ("logZ", "ev", "posterior", "cov"):
                    close(r[key], bf[key], key)
                assert np.all(r["posterior"][l.src == l.dst] == 0.0)
            # max-plus
            best = paths[0][0] if paths else -np.inf
            v64 = paths_ref.viterbi_f64(l, sc)
            close(v64["best"], best, "viterbi_f64")
            for order in ("general", "tile_waves"):
                v = paths_ref.viterbi_ref(l, theta, l.weight, asc, order=order)
                if paths:
                    gap, bound = paths_ref.path_guard(l, sc, v["arcs"])
                    assert -bound <= gap <= bound, (seed, it, b, order)
                    if len(paths) < 2 or paths[0][0] - paths[1][0] > GAP:
                        assert v["arcs"].tolist() == paths[0][1]
                else:
                    assert v["length"] == 0 and v["best"] == -np.inf
            th, e = kbest_ref.arc_terms(l, theta, asc)
            for k in sorted({d.k, 64}):
                r = kbest_ref.k_best(l.n_rows, l.src, l.dst, th, e, k, sink)
                m = min(k, len(paths))
                assert r["n_paths"] == m, (seed, it, b, k)
                scale = max([1.0] + [abs(s) for s, _ in paths[:m]])
                np.testing.assert_allclose(r["best"][:m], [s for s, _ in paths[:m]], rtol=0, atol=1e-5 * scale)
                if m == len(paths) or paths[m - 1][0] - paths[m][0] > GAP * scale:
                    assert sorted(map(tuple, r["arcs"])) == sorted(tuple(p) for _, p in paths[:m])
            if l.n_arcs and paths:
                mm = slack_ref.max_marginals64(l, theta, asc)
                beam = F.BEAMS[b % len(F.BEAMS)]
                r = slack_ref.arc_slack(l, theta, asc, beam=beam)
                on = (l.src != l.dst) & np.isfinite(mm)
                scale = max(1.0, abs(best))
                np.testing.assert_allclose(r["slack"][on], best - mm[on], rtol=0, atol=1e-5 * scale)
                assert np.all(np.isposinf(r["slack"][(l.src != l.dst) & ~np.isfinite(mm)]))
                assert slack_ref.is_trim(l, r["keep"])
    assert done >= 1 and 2 * small_done >= small, (done, small_done, small)


@pytest.mark.parametrize("seed", F.SEEDS)
def test_products_are_the_filtered_enumeration(seed):
    """Every automaton of every draw on every enumerable member: the product's paths, mapped through ``arc_map``, are
    exactly the paths that ``intersect_ref.run`` accepts; the wide and the narrow reference agree."""
    done = 0
    for it in range(F.ITERS):
        d = draw(seed, it)
        for b, l in enumerate(d.canon):
            if not enumerable(l) or (it == F.ITERS - 1 and b >= 24):
                continue
            paths = F.all_paths(l)
            for auto in d.autos + [d.second]:
                delta, final, _ = auto.table(b)
                p = F.product_ref(l, auto, b)
                if p["n_rows"] > 3000:
                    continue
                want = sorted((tuple(int(x) for x in l.label[list(q)]), tuple(q)) for q in paths if intersect_ref.run(delta, final, l.label[list(q)]))
                if l.n_arcs == 0:
                    assert p["n_rows"] == (1 if want else 0) and p["n_arcs"] == 0
                    continue
                assert sorted(intersect_ref.product_paths(p)) == want, (seed, it, b, auto.kind)
                done += 1
                if delta.shape[0] <= 64 and auto.kind != "narrow":
                    q = intersect_ref.intersect(l, delta, final)
                    assert all(np.array_equal(p[k], q[k]) for k in p)
    assert done >= 1


@pytest.mark.parametrize("seed", F.SEEDS)
def test_positional_and_lattice_edit_references_against_enumeration(seed):
    """``positional_ref.sum_product`` / ``max_plus``, ``positional_kbest_ref.k_best`` at the draw's T and
    ``lattice_edit_ref.of_lattice`` on the draw's reference strings, on every enumerable member (the first 24 of the
    batch of tiny lattices) with finite scores."""
    done = 0
    for it in range(F.ITERS):
        d = draw(seed, it)
        T = d.T
        for b, l in enumerate(d.canon):
            if not enumerable(l) or (it == F.ITERS - 1 and b >= 24):
                continue
            done += 1
            theta, asc = d.theta_of(b), d.asc_of(b)
            paths = P.enumerate_paths(l)
            lens = sorted({len(p) for p in paths})
            assert P.min_max_len(l) == (lens[0], lens[-1]) == F.min_max_len(l)
            sc = P.arc_score64(l, theta, asc)
            pos = np.random.default_rng([5, T]).normal(0.0, 1.0, size=(T, l.vocab)).astype(np.float32)
            bf = P.brute_force(l, sc, pos, T, paths)
            r = P.sum_product(l, sc, pos, T)
            for key in ("logz", "len_logz", "pos_post", "arc_post"):
                close(r[key], bf[key], (key, T))
            m = P.max_plus(l, theta, pos, T, asc)
            if np.isfinite(bf["best"]):
                assert abs(float(m["best"]) - bf["best"]) <= 1e-5 * max(1.0, abs(bf["best"]))
                if bf["best"] - bf["runner_up"] > GAP * max(1.0, abs(bf["best"])):
                    assert m["arcs"] == bf["best_arcs"]
            else:
                assert np.isneginf(m["best"]) and m["arcs"] == []
            fit = sorted((x for x in ((sum(sc[a] + float(pos[t, l.label[a]]) for t, a in enumerate(p)), p) for p in paths if len(p) <= T)
                          if x[0] > -np.inf), key=lambda x: -x[0])  # (paths of finite score)
            for k in sorted({d.k, 64}):
                kb = PK.k_best(l, theta, pos, T, k, asc)
                n = min(k, len(fit))
                scale = max([1.0] + [abs(x) for x, _ in fit[:n]])
                assert kb["n_paths"] == n
                np.testing.assert_allclose(kb["best"][:n], [x for x, _ in fit[:n]], rtol=0, atol=1e-5 * scale)
                if n == len(fit) or fit[n - 1][0] - fit[n][0] > GAP * scale:
                    assert sorted(map(tuple, kb["arcs"])) == sorted(tuple(p) for _, p in fit[:n])
            # lattice edit distance
            s64 = d.score64(b)
            ref = d.refs[b]
            for scored in (False, True):  # (scored: over the paths of finite score; unscored: over every path)
                be = lattice_edit_ref.brute_force(l, ref, s64 if scored else None)
                r = lattice_edit_ref.of_lattice(l, ref, theta if scored else None, asc if scored else None)
                assert r["distance"] == be["distance"], (seed, it, b)
                if be["distance"] < 0:
                    continue
                n_sub, n_ins, n_del = r["counts"]
                assert sum(r["counts"]) == r["distance"] and len(r["arcs"]) == len(ref) + n_ins - n_del
                if scored:
                    assert abs(float(r["score"]) - be["best"]) <= 1e-5 * max(1.0, abs(be["best"]))
    assert done >= 1


def test_draws_without_replacement_stay_inside_the_cap():
    """With the reference alone (the rounded float64 backward pass for the op's beta), every lattice of every draw is
    decided at the uniforms' seed that tests/test_gpu_fuzz_paths.py uses: none is left out, which is inside
    ``swor_ref.CAP``."""
    left_out = runs = 0
    margin = np.inf
    for s, i in ALL:
        d = draw(s, i)
        if not swor_ref.degree(d.canon):
            continue
        refs = swor_ref.Case("fuzz", d.canon, d.theta, d.asc, ks=(d.k,), seed=11).references(d.k)
        runs += len(refs)
        left_out += sum(not swor_ref.decided(r) for r in refs)
        margin = min([margin] + [r["margin"] for r in refs])
    print(f"{left_out} of {runs} lattice runs undecided, smallest margin {margin:.3g} (DECIDED = {swor_ref.DECIDED:g})")
    assert left_out == 0 <= swor_ref.CAP * runs


def test_sample_paths_walks_stay_inside_the_cap():
    """``paths_ref.oracle_walks`` on the uniforms that tests/test_gpu_fuzz_paths.py uses: in every draw more than
    ``paths_ref.CAP`` of the walks stay ``paths_ref.MARGIN`` clear of every CDF boundary."""
    left_out = walks = 0
    for s, i in ALL:
        d = draw(s, i)
        if not F.finite(d):  # (no walk where a lattice has no path of finite score)
            continue
        _, w = F.sample_walks(d.canon, d.theta, d.asc)
        safe = sum(int((x[0]["margin"] > paths_ref.MARGIN).sum()) for x in w if x is not None)
        n = sum(len(x[0]["margin"]) for x in w if x is not None)
        assert n == 0 or safe > paths_ref.CAP * n, (s, i, safe, n)
        left_out, walks = left_out + n - safe, walks + n
    print(f"{left_out} of {walks} walks within MARGIN of a boundary")
    assert walks > 10000


def test_positional_draws_stay_inside_their_caps():
    """``positional_sample_ref``: no draw leaves out more than CAP of its walks as undecided; ``positional_swor_ref``: every
    lattice of every draw is decided (none left out: inside its CAP), at the seeds that tests/test_gpu_fuzz_paths.py uses."""
    und = walks = left_out = runs = 0
    margin = np.inf
    for s, i in ALL:
        d = draw(s, i)
        _, _, _, w = F.positional_walks(d.canon, d.theta, d.asc, d.T)
        a, n = sum(PS.undecided(x) for x in w if x is not None), sum(len(x) for x in w if x is not None)
        assert a <= PS.CAP * n, (s, i, a, n)
        und, walks = und + a, walks + n
        _, _, _, refs = F.positional_swor_refs("fuzz", d.canon, d.theta, d.asc, d.k, d.T)
        left_out += sum(not PW.decided(r) for r in refs)
        runs += len(refs)
        margin = min([margin] + [r["margin"] for r in refs])
    print(f"{und} of {walks} positional walks undecided; {left_out} of {runs} lattice runs undecided, smallest margin {margin:.3g}")
    assert left_out == 0 <= PW.CAP * runs and walks > 10000


@pytest.mark.parametrize("seed", F.SEEDS)
def test_sampling_string_and_beam_references_against_enumeration(seed):
    """On the enumerable members of the seed's draws (the first 24 of the batch of tiny lattices): ``swor_ref.search`` and
    ``positional_swor_ref.search`` with k at or above the number of finite paths return each of them once at its exact
    probability; every walk of ``positional_sample_ref.Sampler`` is a path that fits, at its exact probability;
    ``positional_expectation_ref.expectation`` is its brute force; ``strings_ref.string_log_prob`` and ``strings_ref.merge``
    are ``strings_ref.brute_force``; a beam of 64 slots through ``beam_ref.decode`` finds every path of a lattice of at
    most 64 paths (scores on a grid of 1/4: exact sums)."""
    done = {"swor": 0, "positional": 0, "strings": 0, "beam": 0}
    for it in range(F.ITERS):
        d = draw(seed, it)
        T, keep = d.T, F.keep_labels(d.vocab)
        for b, l in enumerate(d.canon):
            if not enumerable(l) or l.n_arcs == 0 or (it == F.ITERS - 1 and b >= 24):
                continue
            theta, asc, sc = d.theta_of(b), d.asc_of(b), d.score64(b)
            listed = swor_ref.enumerate_paths(l, sc)
            depth = X.levels(l.n_rows, l.src, l.dst)
            # draws without replacement: k at or above the number of finite paths returns every path once
            if 0 < len(listed) <= 64:
                lb, z = swor_ref.backward64(l, sc)
                u = swor_ref.uniforms_for([l], 64, seed=1, max_len=int(depth.max()) + 1)[0]
                r = swor_ref.search(l, swor_ref.arc_score32(l, theta, asc), lb, z, 64, u.shape[0], u)
                assert r["status"] == 0 and r["n_paths"] == len(listed) and r["kappa"] == -np.inf
                assert sorted(map(tuple, r["arcs"])) == sorted(a for a, _ in listed)
                want = {a: x - z for a, x in listed}
                np.testing.assert_allclose(r["logp64"], [want[tuple(a)] for a in r["arcs"]], rtol=0, atol=1e-5 * max(1.0, abs(z)))
                done["swor"] += 1
            # the positional references
            paths = P.enumerate_paths(l)
            ps = P.arc_score64(l, theta, asc)
            pos = np.random.default_rng([5, T]).normal(0.0, 1.0, size=(T, l.vocab)).astype(np.float32)
            bf = P.brute_force(l, ps, pos, T, paths)
            if np.isfinite(ps[l.src != l.dst]).all():
                rng = np.random.default_rng(T)
                pv, lv, av = rng.normal(size=(T, l.vocab)), rng.normal(size=l.vocab), rng.normal(size=l.n_arcs)
                be, re = PE.brute_force(l, ps, pos, T, pv, lv, av, 0.3, paths), PE.expectation(l, ps, pos, T, pv, lv, av, 0.3)
                for key in PE.KEYS:  # (E[V] and the covariances are differences of sums of magnitude M: the GPU checker's scale)
                    close(re[key], be[key], (key, T), scale=be["M"])
            beta = PS.beta_rows(l, ps, pos, T)
            close(beta[0, 0], bf["logz"], "beta rows")
            fit = [(sum(ps[a] + float(pos[t, l.label[a]]) for t, a in enumerate(q)), q) for q in paths if len(q) <= T]
            fit = [x for x in fit if x[0] > -np.inf]
            if np.isfinite(bf["logz"]):
                sm = PS.Sampler(l, ps, pos, T)
                for wk in sm.walks(PS.uniforms(11, 8, max(T, 1))):
                    assert wk["arcs"] in [list(q) for _, q in fit] and wk["length"] <= T
                    want = sum(ps[a] + float(pos[t, l.label[a]]) for t, a in enumerate(wk["arcs"])) - bf["logz"]
                    assert abs(wk["logq"] - want) <= 1e-11 * max(1.0, abs(want))
                if len(fit) <= 64:
                    D = max(int(np.diff(swor_ref.out_arcs(l)).max()), 1)
                    u = np.random.default_rng([3, T]).random((max(T, 1), 64, D), dtype=np.float32)
                    r = PW.search(l, swor_ref.arc_score32(l, theta, asc), pos, beta, bf["logz"], 64, T, u)
                    assert r["status"] == 0 and sorted(map(tuple, r["arcs"])) == sorted(tuple(q) for _, q in fit)
                done["positional"] += 1
            # strings: every candidate against the enumeration's table, and merge of the whole path set
            by, z, ranked = SR.brute_force(l, sc, keep=keep)
            for y in d.cands[b]:
                num, zz = SR.string_log_prob(l, sc, y, keep=keep)
                close(zz, z, "string logz")
                close(num, by.get(SR.project(y, keep), -np.inf), "string log_num")
            if 0 < len(ranked) <= 64:
                L = max(len(q) for _, q in ranked)
                rows = np.zeros((1, len(ranked), L), np.int64)
                lens = np.array([[len(q) for _, q in ranked]])
                for j, (_, q) in enumerate(ranked):
                    rows[0, j, :len(q)] = l.label[q]
                m = SR.merge(rows, lens, np.array([[x for x, _ in ranked]]), pad=0, keep=keep)
                n = int(m["n_strings"][0])
                assert n == len(by)
                got = {tuple(int(x) for x in m["strings"][0, j, :m["lengths"][0, j]]): float(m["log_weights"][0, j]) for j in range(n)}
                assert set(got) == set(by)
                for y, w in got.items():
                    assert abs(w - by[y]) <= 1e-9 * max(1.0, abs(by[y])), (seed, it, b, y)
            done["strings"] += 1
            # the beam: wide enough, it finds every path (the structure alone: no table weights, no self loop)
            n_all = F.count_paths(l)
            loops = (l.src == l.dst) & (l.src != S.sink(l))
            if n_all <= 64 and not loops.any() and beam_ref.first_state(l) != 0:
                plain = dataclasses.replace(l, weight=None)
                th = (np.round(np.where(np.isfinite(theta), theta, -8.0).astype(np.float64) * 4) / 4).astype(np.float32)
                ref = kbest_ref.enumerate_paths(l.n_rows, l.src, l.dst, th[l.label].astype(np.float64), S.sink(l))
                want = {tuple(int(x) for x in l.label[q][1:]): x - float(th[F.BOS]) for x, q in ref}
                dd = beam_ref.decode([plain], 64, beam_ref.stateless(th, 64), max_length=l.n_rows)
                got = {tuple(int(x) for x in dd["paths"][0, j, :dd["lengths"][0, j]]): float(dd["scores"][0, j])
                       for j in range(64) if dd["scores"][0, j] > -np.inf}
                assert got == want, (seed, it, b)
                done["beam"] += 1
    assert all(v >= 1 for v in done.values()), done


# ----------------------------------------------------------------------------- the derived corpora
@pytest.mark.parametrize("seed", F.SEEDS)
def test_derived_corpora(seed):
    n_prod = n_pruned = n_nested = 0
    for it in range(F.ITERS):
        d, der = draw(seed, it), derived(seed, it)
        if der["pruned"] is not None:
            for l, k, am in zip(d.canon, der["pruned"].lats, der["pruned"].arc_map):
                keep = np.zeros(l.n_arcs, bool)
                keep[am] = True
                assert slack_ref.is_trim(l, keep) and k.n_rows == l.n_rows
                assert S.canonical(k).n_arcs == k.n_arcs and (l.n_arcs == 0 or S.sink(k) == S.sink(l))
                n_pruned += 1
        prod = der["product"]
        if prod is None:
            continue
        for l, k, am in zip(d.canon, prod.lats, prod.arc_map):
            assert np.array_equal(k.label, l.label[am]) and S.canonical(k).n_arcs == k.n_arcs
            assert (k.weight is None) == (l.weight is None) and (k.weight is None or np.array_equal(k.weight, l.weight[am]))
            n_prod += 1
        for name in ("pruned_product", "product_product"):  # nested maps compose: labels (and weights) of the original's arcs
            nest = der[name]
            if nest is None:
                continue
            for b, (l, mid, k) in enumerate(zip(d.canon, prod.lats, nest.lats)):
                am = prod.arc_map[b][nest.arc_map[b]]
                assert np.array_equal(k.label, l.label[am]) and (l.weight is None or np.array_equal(k.weight, l.weight[am]))
                if name == "pruned_product":
                    keep = np.zeros(mid.n_arcs, bool)
                    keep[nest.arc_map[b]] = True
                    assert slack_ref.is_trim(mid, keep)
                elif enumerable(l) and b < 24:  # intersect(intersect(L, A), B) has the paths that A and B both accept
                    auto, second = d.autos[der["auto"]], der["second"]
                    accept = lambda a, q: intersect_ref.run(a.table(b)[0], a.table(b)[1], l.label[list(q)])
                    want = sorted(tuple(q) for q in F.all_paths(l) if accept(auto, q) and accept(second, q))
                    got = sorted(tuple(int(prod.arc_map[b][a]) for a in arcs) for _, arcs in
                                 intersect_ref.product_paths(nest.products[b])) if k.n_arcs else [()]
                    assert got == want, (seed, it, b)
                n_nested += 1
    assert n_prod and n_pruned and n_nested


# ----------------------------------------------------------------------------- reach
REACH = ("rows <= 64", "rows 65 .. 256", "rows > 256", "per-lattice theta", "weights with caller scores", "a -inf label on a path",
         "a lattice with no finite path", "k above the number of paths", "T below the shortest path", "state 0 is the sink",
         "more lattices than 256", "host packer", "device packer", "group mode 0", "group mode 1", "group mode 2",
         "a batch that gets chunked programs", "narrow Q = 64", "wide Q > 64", "a per-lattice automaton", "a missing transition on a path",
         "an empty product", "a product over 8192 rows", "a product whose sink row is not its last", "sink not the last row", "junk rows",
         "an inner self loop")


def reach_of(d, der) -> set:
    got = set()
    rows = [l.n_rows for l in d.canon]
    got |= {"rows <= 64"} if min(rows) <= 64 else set()
    got |= {"rows 65 .. 256"} if any(65 <= r <= 256 for r in rows) else set()
    got |= {"rows > 256"} if max(rows) > 256 else set()
    if d.theta.ndim == 2:
        got.add("per-lattice theta")
    if d.weighted and d.asc is not None:
        got.add("weights with caller scores")
    paths = [F.count_paths(l) for l in d.canon]
    for b, l in enumerate(d.canon):
        sc = d.score64(b)
        if np.any(np.isneginf(sc[l.src != l.dst])):
            got.add("a -inf label on a path")  # (every arc of a canonical lattice lies on a path: layered_lattice is trim)
            if kbest_ref.count_finite_paths(l.n_rows, l.src, l.dst, sc, S.sink(l)) == 0:
                got.add("a lattice with no finite path")
        if l.n_arcs and d.T < F.min_max_len(l)[0]:
            got.add("T below the shortest path")
    if d.k > min(paths):
        got.add("k above the number of paths")
    for name, change in (("state 0 is the sink", "state0_is_sink"), ("sink not the last row", "renumbered"), ("junk rows", "junk"),
                         ("an inner self loop", "self_loop")):
        if change in d.changes:
            got.add(name)
    if d.B > 256:
        got.add("more lattices than 256")
    got.add(f"{d.route} packer")
    got.add(f"group mode {d.gm}")
    if d.chunks and F.pack(d, None).chunks is not None:
        got.add("a batch that gets chunked programs")
    for auto in d.autos:
        Q = max(t[0].shape[0] for t in auto.tables)
        if auto.kind == "narrow" and Q == 64:
            got.add("narrow Q = 64")
        if auto.kind != "narrow" and Q > 64:
            got.add("wide Q > 64")
        if auto.per_lattice:
            got.add("a per-lattice automaton")
        prods = [F.product_ref(l, auto, b) for b, l in enumerate(d.canon)]
        what, _ = F.outcome(prods)
        if any(p["n_rows"] == 0 for p in prods):
            got.add("an empty product")
        if any(p["n_rows"] > F.MAX_ROWS for p in prods):
            got.add("a product over 8192 rows")
        for b, (l, p) in enumerate(zip(d.canon, prods)):
            if 0 < p["n_rows"] and l.n_arcs and int(np.flatnonzero(p["row_state"] == S.sink(l))[0]) != p["n_rows"] - 1:
                got.add("a product whose sink row is not its last")
            if l.n_arcs and p["n_arcs"] < l.n_arcs and np.any(auto.table(b)[0][:, l.label] < 0):
                got.add("a missing transition on a path")
    return got


def test_the_draws_reach_what_they_exist_for():
    got = set()
    for s, i in ALL:
        got |= reach_of(draw(s, i), derived(s, i))
    missing = [r for r in REACH if r not in got]
    assert not missing, missing

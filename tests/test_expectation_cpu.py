"""The float64 reference of the expectation semiring (tests/expectation_ref.py) that the GPU tests of
ops.expectation / entropy / kl_divergence and of the double backward of log_z rely on: against path enumeration,
against central differences of the oracle's float64 log Z and posteriors, and on closed-form cases."""
import numpy as np
import pytest

from nfst_amd import synth
from oracle import oracle as O
from tests import edge_cases as E
from tests import expectation_ref as X
from tests import kbest_ref as R

V = 16


def _small_lattices():
    out = [
        synth.layered_lattice(11, n_states=10, avg_degree=2.5, vocab=V, width=3, span=2),
        synth.layered_lattice(12, n_states=12, avg_degree=3.0, vocab=V, width=4, span=3),
        synth.layered_lattice(13, n_states=9, avg_degree=2.0, vocab=V, width=1, span=4, weighted=True),
        synth.edit_lattice([6, 7], [8, 9], vocab=V, seed=3),
    ]
    # parallel-free: drop the arcs that duplicate a (src, dst) pair
    out.append(synth.without_parallel_arcs(synth.layered_lattice(14, n_states=12, avg_degree=3.0, vocab=V, width=3, span=2)))
    return out


def _score_value(l, seed):
    rng = np.random.default_rng(seed)
    theta = rng.normal(-1.0, 0.8, size=V)
    score = theta[l.label] + (0.0 if l.weight is None else l.weight.astype(np.float64))
    value = rng.normal(0.0, 2.0, size=l.n_arcs)
    return score, value


def test_small_lattices_exist_as_intended():
    for l in _small_lattices():
        assert l.n_rows <= 40  # (the edit lattice spells its marks out: 39 rows)
        assert X.brute_force(l.n_rows, l.src, l.dst, np.zeros(l.n_arcs), np.zeros(l.n_arcs), l.n_rows - 1)["n_paths"] >= 2


@pytest.mark.parametrize("i", range(5))
def test_helper_equals_path_enumeration(i):
    l = _small_lattices()[i]
    score, value = _score_value(l, i)
    sink = l.n_rows - 1
    ref = X.brute_force(l.n_rows, l.src, l.dst, score, value, sink)
    got = X.expectation(l.n_rows, l.src, l.dst, score, value)
    assert abs(got["logZ"] - ref["logZ"]) <= 1e-12
    assert abs(got["ev"] - ref["ev"]) <= 1e-12
    assert np.max(np.abs(got["posterior"] - ref["posterior"])) <= 1e-12
    assert np.max(np.abs(got["cov"] - ref["cov"])) <= 1e-12
    # both directions give the same E[V]
    assert abs(got["r_alpha"][sink] - got["ev"]) <= 1e-12
    h = X.entropy(l.n_rows, l.src, l.dst, score)
    assert abs(h["H"] - ref["H"]) <= 1e-12


@pytest.mark.parametrize("i", [0, 1, 3])
def test_helper_equals_central_differences_of_the_oracle(i):
    """E[V] = d log Z(s + t v) / dt and c_a = d p_a(s + t v) / dt at t = 0 (the Hessian of log Z along v)."""
    l = _small_lattices()[i]
    score, value = _score_value(l, 10 + i)
    h = 1e-5
    up = O.forward_backward(l.n_rows, l.src, l.dst, score + h * value)
    dn = O.forward_backward(l.n_rows, l.src, l.dst, score - h * value)
    got = X.expectation(l.n_rows, l.src, l.dst, score, value)
    assert abs((up["logZ"] - dn["logZ"]) / (2 * h) - got["ev"]) <= 1e-7
    fd = (np.asarray(up["posterior"]) - np.asarray(dn["posterior"])) / (2 * h)
    loop = l.src == l.dst
    fd[loop] = 0.0
    assert np.max(np.abs(fd - got["cov"])) <= 1e-7


def test_single_path_has_zero_entropy_and_zero_covariance():
    l = synth._finish(4, V, [0, 1, 2], [3, 4, 5], [1, 2, 3])
    score = np.array([0.3, -1.2, 2.0, 0.0])[: l.n_arcs]
    e = X.entropy(l.n_rows, l.src, l.dst, score)
    assert abs(e["H"]) <= 1e-12
    assert np.max(np.abs(e["grad"])) <= 1e-12


@pytest.mark.parametrize("n", [2, 3, 7])
def test_n_equally_weighted_paths_have_entropy_log_n(n):
    n_rows, src, dst, sink = X.all_paths_equal(n)
    score = np.full(len(src), -0.7)  # every path has the same score
    e = X.entropy(n_rows, src, dst, score)
    assert abs(e["H"] - np.log(n)) <= 1e-12
    assert np.max(np.abs(e["grad"])) <= 1e-12  # (all paths equal: no arc covaries with the score)


def test_label_sums():
    assert np.allclose(X.label_sums([0, 2, 2, 1], [1.0, 2.0, 3.0, 4.0], 4), [1.0, 4.0, 5.0, 0.0])


def test_build_guard_covers_the_expectation_sweep():
    from nfst_amd.build import check_resources

    assert check_resources({"k_expect_sweep": {"vgpr_spill": 4, "agprs": 0}})
    assert not check_resources({"k_expect_sweep": {"vgpr_spill": 0, "agprs": 0}})


# ----------------------------------------------------------------------------- the edges the GPU tests lean on
def _quiet_expectation(l, score, value):
    """X.expectation with every NumPy warning turned into an error: the helper silences what it expects itself."""
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return X.expectation(l.n_rows, l.src, l.dst, score, value)


@pytest.mark.parametrize("i", range(5))
def test_one_label_at_minus_infinity_equals_path_enumeration(i):
    l = _small_lattices()[i]
    score, value = _score_value(l, 20 + i)
    sink = l.n_rows - 1
    total = R.count_finite_paths(l.n_rows, l.src, l.dst, score, sink)
    for lab in np.argsort(-np.bincount(l.label, minlength=V), kind="stable"):  # the commonest label that leaves a path
        dead = l.label == lab
        if 0 < R.count_finite_paths(l.n_rows, l.src, l.dst, np.where(dead, -np.inf, score), sink) < total:
            break
    else:
        pytest.fail("no label kills some paths and not all")
    score = np.where(dead, -np.inf, score)
    with np.errstate(divide="ignore", invalid="ignore"):  # (the enumerator's entropy term takes log 0)
        ref = X.brute_force(l.n_rows, l.src, l.dst, score, value, sink)
    assert np.isfinite(ref["logZ"]) and 0 < np.sum(ref["posterior"] > 0) < l.n_arcs
    got = _quiet_expectation(l, score, value)
    assert abs(got["logZ"] - ref["logZ"]) <= 1e-12
    assert abs(got["ev"] - ref["ev"]) <= 1e-12
    assert np.max(np.abs(got["posterior"] - ref["posterior"])) <= 1e-12
    assert np.max(np.abs(got["cov"] - ref["cov"])) <= 1e-12
    assert abs(got["r_alpha"][sink] - got["ev"]) <= 1e-12
    assert np.all(got["posterior"][dead] == 0.0) and np.all(got["cov"][dead] == 0.0)
    # a dead arc has no value: whatever stands there is ignored
    for junk in (np.inf, np.nan):
        again = _quiet_expectation(l, score, np.where(dead, junk, value))
        for key in ("ev", "posterior", "cov"):
            assert np.array_equal(again[key], got[key])


@pytest.mark.parametrize("i", range(5))
def test_all_paths_dead(i):
    l = _small_lattices()[i]
    score, value = _score_value(l, 30 + i)
    score = np.where(l.label == synth.EOS, -np.inf, score)  # every path ends by eos
    got = _quiet_expectation(l, score, value)
    assert got["logZ"] == -np.inf and got["ev"] == 0.0
    assert np.all(got["posterior"] == 0.0) and np.all(got["cov"] == 0.0)
    for key in ("posterior", "cov", "r_alpha", "r_beta"):
        assert not np.isnan(got[key]).any()


@pytest.mark.parametrize("i", range(8))
def test_uniform_shift_of_the_scores_changes_log_z_only(i):
    """-2e4 on every arc of a lattice whose paths all have the same length (span=1: every arc goes to the next layer),
    and on the file's small lattices -2e4 per level an arc crosses (a potential: their paths differ in length, so a shift
    per arc would favour the short ones): every path is shifted by the same amount, so only log Z moves."""
    if i < 3:
        l = synth.layered_lattice(15 + i, n_states=14, avg_degree=2.5, vocab=V, width=3, span=1)
        hops = np.ones(l.n_arcs)
    else:
        l = _small_lattices()[i - 3]
        depth = X.levels(l.n_rows, l.src, l.dst)
        hops = (depth[l.dst] - depth[l.src]).astype(np.float64)
    score, value = _score_value(l, 40 + i)
    paths = X.brute_force(l.n_rows, l.src, l.dst, hops, np.zeros(l.n_arcs), l.n_rows - 1)
    assert paths["n_paths"] >= 2 and abs(paths["H"] - np.log(paths["n_paths"])) <= 1e-12  # (all paths: the same total)
    a = X.expectation(l.n_rows, l.src, l.dst, score, value)
    b = X.expectation(l.n_rows, l.src, l.dst, score - 2.0e4 * hops, value)
    assert abs(a["ev"] - b["ev"]) <= 1e-9
    assert np.max(np.abs(a["posterior"] - b["posterior"])) <= 1e-9
    assert np.max(np.abs(a["cov"] - b["cov"])) <= 1e-9
    assert b["logZ"] < a["logZ"] - 2.0e4


@pytest.mark.parametrize("name", E.RANGE_CASES)
def test_range_cases_have_not_collapsed_to_one_path(name):
    """The condition of test_gpu_expectation.test_exponent_range_and_cancelling_values, on the reference alone and for
    the seeds that test uses: at least 20 arcs per lattice with a posterior in (0.01, 0.99), values that cancel, and
    a log Z as large as the case is meant to be."""
    lats, theta, asc, av = E.range_case(name)
    big = 0.0
    for l, sl in zip(lats, E.arc_slices(lats)):
        if name in E.RANGE_SPREAD:
            assert E.posterior_spread(l, theta, asc[sl]) >= E.SPREAD_MIN
        s = E.score64(l, theta, asc[sl])
        e = X.expectation(l.n_rows, l.src, l.dst, s, av[sl].astype(np.float64))
        assert np.isfinite(e["logZ"]) and np.isfinite(e["ev"])
        assert abs(e["ev"]) <= 0.5 * float(np.sum(e["posterior"] * np.abs(av[sl])))
        big = max(big, abs(e["logZ"]))
    assert big > E.RANGE_LOGZ[name]


def test_dead_label_case_has_over_120_dead_arcs_per_lattice():
    for l in E.weighted_batch():
        assert np.isin(l.label, E.DEAD).sum() > 120


def test_no_path_case_on_the_reference():
    lats, theta = E.no_path_case(True)
    for b, l in enumerate(lats):
        e = _quiet_expectation(l, E.score64(l, theta[b]), np.ones(l.n_arcs))
        assert np.isneginf(e["logZ"]) == (b in (1, 3))
        if b in (1, 3):
            assert e["ev"] == 0.0 and not e["posterior"].any() and not e["cov"].any()

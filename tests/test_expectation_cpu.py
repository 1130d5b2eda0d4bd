"""The float64 reference of the expectation semiring (tests/expectation_ref.py) that the GPU tests of
ops.expectation / entropy / kl_divergence and of the double backward of log_z rely on: against path enumeration,
against central differences of the oracle's float64 log Z and posteriors, and on closed-form cases."""
import numpy as np
import pytest

from nfst_amd import synth
from oracle import oracle as O
from tests import expectation_ref as X

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

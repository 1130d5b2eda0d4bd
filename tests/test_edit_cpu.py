"""The yardstick of the edit-distance op (tests/edit_ref.py) against hand cases and the metric's properties, the C
entry point's host-side checks on host pointers, and ``decoders.mbr_select`` on CPU tensors against its restatement.
Runs without a GPU; tests/test_gpu_edit.py holds the kernel to the same reference."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import edit_ref as R

ERR_ARG, ERR_LIMIT = -1, -6


# ----------------------------------------------------------------------------- the reference
def _codes(s):
    return [ord(c) for c in s]


@pytest.mark.parametrize("fn", [R.levenshtein, R.levenshtein_fast])
def test_hand_cases(fn):
    assert fn(_codes("kitten"), _codes("sitting")) == 3
    assert fn(_codes("sitting"), _codes("kitten")) == 3
    assert fn(_codes("flaw"), _codes("lawn")) == 2
    assert fn(_codes("intention"), _codes("execution")) == 5
    assert fn([], []) == 0
    for n in (1, 2, 7, 65):
        assert fn([], list(range(n))) == n and fn(list(range(n)), []) == n
        assert fn(list(range(n)), list(range(n))) == 0
    for la, lb in ((1, 1), (3, 5), (5, 3), (64, 70)):  # disjoint alphabets: substitute min, insert the rest
        assert fn(list(range(la)), list(range(1000, 1000 + lb))) == max(la, lb)
    assert fn([5] * 9, [5] * 4) == 5  # one symbol: |la - lb|
    assert fn([7, -1, 3], [7, 3]) == 1  # tokens are plain integers, negative ones too


def _random_pairs(n, seed, alphabet=3, longest=24):
    rng = np.random.default_rng(seed)
    return [tuple(rng.integers(0, alphabet, size=int(rng.integers(0, longest + 1))) for _ in range(3)) for _ in range(n)]


def test_properties_on_random_triples():
    for x, y, z in _random_pairs(60, 11):
        dxy, dyx = R.levenshtein(x, y), R.levenshtein(y, x)
        assert dxy == dyx
        assert abs(len(x) - len(y)) <= dxy <= max(len(x), len(y))
        assert (dxy == 0) == (len(x) == len(y) and np.array_equal(x, y))
        assert R.levenshtein(x, z) <= dxy + R.levenshtein(y, z)


def test_the_row_sweep_is_the_table():
    """``levenshtein_fast``, which the GPU tests use on their long rows, equals the plain table."""
    for alphabet in (1, 2, 3, 50):
        for x, y, _ in _random_pairs(40, 5 + alphabet, alphabet=alphabet, longest=40):
            assert R.levenshtein_fast(x, y) == R.levenshtein(x, y)
    rng = np.random.default_rng(3)
    x, y = rng.integers(0, 3, 150), rng.integers(0, 3, 131)
    assert R.levenshtein_fast(x, y) == R.levenshtein(x, y)


def test_distance_table():
    a = np.array([[[1, 2, 3, 9], [1, 2, 9, 9]]])
    b = np.array([[[1, 3, 9], [9, 9, 9], [1, 2, 3]]])
    D = R.distance_table(a, [[3, 2]], b, [[2, 0, 3]])
    assert D.dtype == np.int32 and D.tolist() == [[[1, 3, 0], [1, 2, 1]]]
    assert np.array_equal(R.distance_table(a, [[3, 2]], b, [[2, 0, 3]], fn=R.levenshtein), D)


@pytest.mark.parametrize("alphabet", [1, 3])
def test_the_set_by_set_table_is_the_pair_by_pair_one(alphabet):
    """The form the GPU tests use on their large tables, on rows with a tail that must not be read."""
    rng = np.random.default_rng(20 + alphabet)
    for B, Ka, Kb, La, Lb in ((2, 5, 4, 30, 22), (1, 1, 6, 9, 40), (3, 2, 1, 1, 1)):
        a, b = rng.integers(0, alphabet, (B, Ka, La)), rng.integers(0, alphabet, (B, Kb, Lb))
        al, bl = rng.integers(0, La + 1, (B, Ka)), rng.integers(0, Lb + 1, (B, Kb))
        al[0, 0], bl[0, 0] = La, 0
        for s in range(B):
            for i in range(Ka):
                a[s, i, al[s, i]:] = 9
            for j in range(Kb):
                b[s, j, bl[s, j]:] = 9
        D = R.distance_table(a, al, b, bl)
        assert D.dtype == np.int32 and np.array_equal(D, R.distance_table(a, al, b, bl, fn=R.levenshtein))
        assert np.array_equal(R.distance_table(b, bl, a, al), D.transpose(0, 2, 1))
    assert R.distance_table(np.zeros((2, 3, 4), int), np.zeros((2, 3), int), np.zeros((2, 0, 4), int), np.zeros((2, 0), int)).shape == (2, 3, 0)


# ----------------------------------------------------------------------------- the library
def test_export_is_declared():
    from nfst_amd import _lib, ops

    assert "nfst_edit_distance" in _lib.EXPORTS
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "nfst_hip.h")).read()
    assert "int nfst_edit_distance(" in header
    assert _lib.ABI_VERSION == 7 and _lib.lib.nfst_abi_version() == 7  # functions were added, no struct changed
    limit = int(re.search(r"#define\s+NFST_EDIT_MAX_LEN\s+(\d+)", header).group(1))
    assert limit >= 1024 and limit == ops.EDIT_MAX_LEN


def test_argument_checks_return_before_any_launch():
    """Every host-side check of nfst_edit_distance on host pointers: had anything been launched, or read on the host,
    the outputs would not be untouched (and without a GPU the launch itself would have returned NFST_ERR_HIP)."""
    from nfst_amd import _lib, ops

    lib = _lib.lib
    S, Ka, La, Kb, Lb = 2, 3, 5, 4, 7
    a, al = np.zeros((S, Ka, La), np.int32), np.zeros((S, Ka), np.int32)
    b, bl = np.zeros((S, Kb, Lb), np.int32), np.zeros((S, Kb), np.int32)
    out, status = np.full((S, Ka, Kb), 77, np.int32), np.zeros(1, np.int32)
    p = lambda x: None if x is None else x.ctypes.data

    def call(a=a, al=al, Ka=Ka, La=La, b=b, bl=bl, Kb=Kb, Lb=Lb, S=S, sym=0, out=out, status=status):
        return lib.nfst_edit_distance(p(a), p(al), Ka, La, p(b), p(bl), Kb, Lb, S, sym, p(out), p(status), None)

    for name in ("a", "al", "b", "bl", "out", "status"):
        assert call(**{name: None}) == ERR_ARG, name
    for name in ("S", "Ka", "Kb"):
        assert call(**{name: -1}) == ERR_ARG, name
    for name in ("La", "Lb"):
        assert call(**{name: 0}) == ERR_ARG, name
        assert call(**{name: -3}) == ERR_ARG, name
        assert call(**{name: ops.EDIT_MAX_LEN + 1}) == ERR_LIMIT, name
    # symmetric mode is the table of one set
    assert call(sym=1) == ERR_ARG  # b is not a
    assert call(sym=1, b=a, bl=al, Kb=Ka) == ERR_ARG  # Lb != La
    assert call(sym=1, b=a, bl=al, Lb=La) == ERR_ARG  # kb != ka
    assert call(sym=1, b=a, bl=bl, Kb=Ka, Lb=La) == ERR_ARG  # other lengths
    # nothing to do is not an error, whatever the data pointers
    for name in ("S", "Ka", "Kb"):
        assert call(**{name: 0}) == 0, name
        assert call(**{name: 0, "a": None, "b": None, "out": None}) == 0, name
    assert call(S=0, status=None) == ERR_ARG
    assert status[0] == 0 and np.all(out == 77)  # nothing ran


def test_wrappers_validate_before_any_launch():
    from nfst_amd import ops

    a, al = torch.zeros((2, 3, 5), dtype=torch.int32), torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.edit_distance(a, al, a, al)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.pairwise_edit_distance(a, al)


# ----------------------------------------------------------------------------- mbr_select
def _select(D, lw, n=None):
    from nfst_amd import decoders

    index, risk = decoders.mbr_select(torch.as_tensor(D), torch.as_tensor(lw), None if n is None else torch.as_tensor(n))
    assert index.dtype == torch.int64 and risk.dtype == torch.float64 and index.shape == (len(lw),) and risk.shape == np.shape(lw)
    return index.numpy(), risk.numpy()


def _tables(seed, B=5, K=7, longest=9):
    """Distance tables of random strings (a real metric) and float32 log weights."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, longest + 1, size=(B, K))
    rows = rng.integers(0, 3, size=(B, K, longest))
    return R.distance_table(rows, lens, rows, lens, fn=R.levenshtein), rng.normal(size=(B, K)).astype(np.float32) * 3


def _same(got, ref):
    assert np.array_equal(got[0], ref[0])
    assert np.array_equal(np.isinf(got[1]), np.isinf(ref[1]))
    fin = np.isfinite(ref[1])
    assert np.all(np.abs(got[1][fin] - ref[1][fin]) <= 1e-12 * np.maximum(1.0, np.abs(ref[1][fin])))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_mbr_select_against_the_restatement(seed):
    D, lw = _tables(seed)
    _same(_select(D, lw), R.mbr_select(D, lw))
    n = np.array([7, 3, 1, 0, 5])
    got, ref = _select(D, lw, n), R.mbr_select(D, lw, n)
    _same(got, ref)
    assert got[0][3] == -1 and np.all(np.isinf(got[1][3]))  # a lattice with no valid entry
    assert got[0][2] == 0 and got[1][2, 0] == 0.0 and np.all(np.isinf(got[1][2, 1:]))  # one entry: itself, at no risk
    for b in range(5):
        assert got[0][b] < n[b] and np.all(np.isinf(got[1][b, n[b]:])) and np.all(np.isfinite(got[1][b, :n[b]]))


def test_mbr_select_by_hand():
    # three candidates on a line at 0, 1, 4 (distances |x - y|), weights 0.4, 0.3, 0.3: the weighted median wins
    D = np.array([[[0, 1, 4], [1, 0, 3], [4, 3, 0]]])
    lw = np.log(np.array([[4.0, 3.0, 3.0]])) + 5.0  # (unnormalised)
    index, risk = _select(D, lw)
    assert index[0] == 1
    assert np.all(np.abs(risk[0] - np.array([1.5, 1.3, 2.5])) <= 1e-12)


def test_mbr_select_ties_go_to_the_first_index():
    D = np.array([[[0, 2, 2, 2], [2, 0, 2, 2], [2, 2, 0, 2], [2, 2, 2, 0]]] * 2)
    lw = np.array([[0.0, 0.0, 0.0, 0.0], [-1.0, 0.5, 0.5, -1.0]])  # risks all equal; then entries 1 and 2 tie
    index, risk = _select(D, lw)
    assert index.tolist() == [0, 1] and risk[0, 0] == risk[0, 3] and risk[1, 1] == risk[1, 2]
    index, _ = _select(D, lw, np.array([4, 4]))
    assert index.tolist() == [0, 1]
    assert np.array_equal(index, R.mbr_select(D, lw, np.array([4, 4]))[0])


def test_mbr_select_weights_at_minus_infinity():
    ninf = -np.inf
    D, _ = _tables(4, B=4, K=5)
    lw = np.array([[0.0, ninf, -1.0, ninf, -2.0], [ninf] * 5, [ninf, ninf, ninf, 1.5, ninf], [0.3, 0.2, 0.1, 0.0, -0.1]])
    got = _select(D, lw)
    _same(got, R.mbr_select(D, lw))
    assert got[0][1] == -1 and np.all(np.isinf(got[1][1]))
    assert got[0][2] == 3 and got[1][2, 3] == 0.0
    assert np.all(np.isinf(got[1][0, [1, 3]])) and got[0][0] in (0, 2, 4)
    # with n_paths an entry at -inf is a candidate of no weight: it can be chosen, it attracts nothing
    n = np.array([5, 5, 5, 2])
    got = _select(D, lw, n)
    _same(got, R.mbr_select(D, lw, n))
    assert np.all(np.isfinite(got[1][0])) and got[0][1] == -1 and np.all(np.isfinite(got[1][2]))
    assert np.array_equal(got[1][2], D[2, :, 3].astype(np.float64))
    assert not np.any(np.isnan(got[1]))


def test_mbr_select_rejects_bad_shapes():
    from nfst_amd import decoders

    with pytest.raises(ValueError):
        decoders.mbr_select(torch.zeros(2, 3, 4), torch.zeros(2, 3))
    with pytest.raises(ValueError):
        decoders.mbr_select(torch.zeros(3, 3), torch.zeros(3))

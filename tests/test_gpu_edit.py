"""ops.edit_distance / ops.pairwise_edit_distance (nfst_edit_distance: one wave64 per pair, the shorter row on the lanes
in strips of 64, a skewed wavefront per strip) and decoders.mbr_decode against tests/edit_ref.py.  Every comparison of
distances is exact: the op computes integers.

The kernel has no flavours and the grid is not capped; what changes with the sizes is the number of strips (columns
beyond 64, 128: the boundary column goes through LDS), which side lies on the lanes (the shorter), the last strip's
width, and whether a workgroup's four waves all have a pair."""
import numpy as np
import pytest
import torch

from nfst_amd import _lib, decoders, ops, swor, synth
from nfst_amd.lattice import LatticeBatch
from tests import edge_cases as E
from tests import edit_ref as R

pytestmark = pytest.mark.gpu
PAD = synth.PAD
GRID = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
TAIL = 9  # the token behind every row's end, on both sides: reading it would find matches that are not there


def _rows(rng, lens, L, alphabet):
    """int32 [*lens.shape, L]: random tokens below ``alphabet`` up to every row's length, TAIL behind it"""
    x = rng.integers(0, alphabet, size=(*np.shape(lens), L)).astype(np.int32)
    x[np.arange(L) >= np.asarray(lens)[..., None]] = TAIL
    return x


def _dev(dev, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def _op(dev, a, al, b, bl):
    return ops.edit_distance(*_dev(dev, a, al, b, bl)).cpu().numpy()


# ----------------------------------------------------------------------------- every length class against every other
@pytest.mark.parametrize("alphabet", [3, 1])
def test_length_grid(dev, alphabet):
    """All pairs of lengths of GRID in one launch (100 pairs: a strip, two, three, four; either side the shorter; the
    last strip one lane, 63 lanes, full), rows of 203 with a tail that would change the answer if read.  Three symbols:
    substitutions, insertions and deletions all occur; one symbol: d = |la - lb|.  The other way round is the transpose."""
    rng = np.random.default_rng(alphabet)
    lens = np.array([GRID], dtype=np.int32)
    a, b = _rows(rng, lens, 203, alphabet), _rows(rng, lens, 203, alphabet)
    ref = R.distance_table(a, lens, b, lens)
    if alphabet == 1:
        assert np.array_equal(ref[0], np.abs(lens[0][:, None] - lens[0][None, :]))
    else:
        assert np.all(ref[0] >= np.abs(lens[0][:, None] - lens[0][None, :])) and (ref[0] > np.abs(lens[0][:, None] - lens[0][None, :])).sum() > 30
    D = _op(dev, a, lens, b, lens)
    assert D.dtype == np.int32 and np.array_equal(D, ref)
    assert np.array_equal(_op(dev, b, lens, a, lens), ref.transpose(0, 2, 1))
    # the reading of garbage would have shown: the same rows with another tail give the same table
    a2, b2 = a.copy(), b.copy()
    a2[a2 == TAIL], b2[b2 == TAIL] = -1, 0
    assert np.array_equal(_op(dev, a2, lens, b2, lens), ref)


@pytest.mark.parametrize("S,Ka,Kb", [(1, 1, 1), (1, 3, 3), (1, 1, 3), (3, 3, 1), (2, 64, 1), (2, 1, 64), (1, 64, 3), (1, 3, 64),
                                     (1, 64, 64), (5, 3, 5)])
def test_set_sizes(dev, S, Ka, Kb):
    """ka, kb in {1, 3, 64} and one set: the pair -> (set, i, j) arithmetic, pair counts that leave waves of the last
    workgroup without a pair (1, 3, 9, 75), and different L on the two sides."""
    rng = np.random.default_rng(100 * S + 10 * Ka + Kb)
    al, bl = rng.integers(0, 14, (S, Ka)).astype(np.int32), rng.integers(0, 18, (S, Kb)).astype(np.int32)
    a, b = _rows(rng, al, 13, 2), _rows(rng, bl, 19, 2)
    D = _op(dev, a, al, b, bl)
    assert D.shape == (S, Ka, Kb) and np.array_equal(D, R.distance_table(a, al, b, bl))


def test_two_dimensional_sides_and_dtypes(dev):
    """A 2-D side is K = 1 with its axis squeezed; int64 marks and non-contiguous tensors give what contiguous int32
    gives."""
    rng = np.random.default_rng(5)
    al, bl = rng.integers(0, 71, (4, 6)).astype(np.int32), rng.integers(0, 80, (4, 1)).astype(np.int32)
    a, b = _rows(rng, al, 70, 3), _rows(rng, bl, 80, 3)
    ref = R.distance_table(a, al, b, bl)
    ta, tal, tb, tbl = _dev(dev, a, al, b, bl)
    D = ops.edit_distance(ta, tal, tb, tbl)
    assert D.dtype == torch.int32 and np.array_equal(D.cpu().numpy(), ref)
    flat = ops.edit_distance(ta, tal, tb[:, 0], tbl[:, 0])
    assert flat.shape == (4, 6) and torch.equal(flat, D[:, :, 0])
    flat = ops.edit_distance(tb[:, 0], tbl[:, 0], ta, tal)
    assert flat.shape == (4, 6) and torch.equal(flat, D[:, :, 0])
    both = ops.edit_distance(ta[:, 2], tal[:, 2], tb[:, 0], tbl[:, 0])
    assert both.shape == (4,) and torch.equal(both, D[:, 2, 0])
    assert torch.equal(ops.edit_distance(ta.long(), tal.long(), tb.long(), tbl.long()), D)
    wide = torch.full((4, 6, 140), 5, dtype=torch.int64, device=dev)
    wide[:, :, ::2] = ta.long()
    nc, ncl = wide[:, :, ::2], torch.stack((tal, tal), dim=2)[:, :, 1]
    assert not nc.is_contiguous() and not ncl.is_contiguous()
    assert torch.equal(ops.edit_distance(nc, ncl, tb.transpose(0, 1).contiguous().transpose(0, 1), tbl), D)
    with pytest.raises(ValueError):
        ops.edit_distance(ta, tal, tb[:3], tbl[:3])
    with pytest.raises(ValueError):
        ops.edit_distance(ta, tal, tb.cpu(), tbl.cpu())
    assert ops.edit_distance(ta[:, :0], tal[:, :0], tb, tbl).shape == (4, 0, 1)  # nothing to do


# ----------------------------------------------------------------------------- the symmetric mode
@pytest.mark.parametrize("K", [1, 2, 5, 64])
def test_pairwise(dev, K):
    """The symmetric mode gives the general mode's bits, a zero diagonal and D == D^T, on lengths of every strip class."""
    rng = np.random.default_rng(K)
    lens = rng.choice(np.array(GRID[:-1] + (100, 140)), size=(2, K)).astype(np.int32)
    lens[0, 0] = 140
    x = _rows(rng, lens, 141, 3)
    tx, tl = _dev(dev, x, lens)
    D = ops.pairwise_edit_distance(tx, tl)
    assert D.dtype == torch.int32 and D.shape == (2, K, K)
    assert torch.equal(D, ops.edit_distance(tx, tl, tx, tl))
    assert torch.equal(D, ops.edit_distance(tx, tl, tx.clone(), tl.clone()))
    assert torch.equal(D, D.transpose(1, 2)) and not D.diagonal(dim1=1, dim2=2).any()
    assert np.array_equal(D.cpu().numpy(), R.distance_table(x, lens, x, lens))


# ----------------------------------------------------------------------------- limits and bad lengths
def test_rows_at_the_limit_and_beyond(dev):
    """A row of NFST_EDIT_MAX_LEN tokens on either side (sixteen strips against itself; against a short and an empty row);
    one token more is NFST_ERR_LIMIT on the host, before any launch."""
    M = ops.EDIT_MAX_LEN
    rng = np.random.default_rng(8)
    al, bl = np.array([[M]], dtype=np.int32), np.array([[M, 70, 0]], dtype=np.int32)
    a, b = _rows(rng, al, M, 3), _rows(rng, bl, M, 3)
    ref = R.distance_table(a, al, b, bl)
    assert ref[0, 0, 2] == M and ref[0, 0, 1] >= M - 70
    assert np.array_equal(_op(dev, a, al, b, bl), ref)
    assert np.array_equal(_op(dev, b, bl, a, al), ref.transpose(0, 2, 1))
    long = torch.zeros((1, 1, M + 1), dtype=torch.int32, device=dev)
    one = torch.ones((1, 1), dtype=torch.int32, device=dev)
    short = torch.zeros((1, 1, 4), dtype=torch.int32, device=dev)
    for args in ((long, one, short, one), (short, one, long, one)):
        with pytest.raises(_lib.NfstError) as e:
            ops.edit_distance(*args)
        assert e.value.code == -6
    with pytest.raises(_lib.NfstError) as e:
        ops.pairwise_edit_distance(long, one)
    assert e.value.code == -6


def _raw(a, al, b, bl, symmetric=0):
    """The entry point itself, for the launches whose status the wrapper would raise: (return code, out, status)"""
    S, Ka, La = a.shape
    Kb, Lb = b.shape[1], b.shape[2]
    out = torch.full((S, Ka, Kb), 77, dtype=torch.int32, device=a.device)
    status = torch.zeros(1, dtype=torch.int32, device=a.device)
    rc = _lib.lib.nfst_edit_distance(a.data_ptr(), al.data_ptr(), Ka, La, b.data_ptr(), bl.data_ptr(), Kb, Lb, S, symmetric,
                                     out.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), int(status.item())


def test_a_length_outside_its_row(dev):
    """-1 and L + 1 are found on the device: the status word reports the length error, the pairs of that row hold -1
    (no token of theirs was read), every other pair of the launch is right, and the wrapper raises."""
    rng = np.random.default_rng(9)
    al, bl = rng.integers(0, 71, (2, 5)).astype(np.int32), rng.integers(0, 67, (2, 4)).astype(np.int32)
    a, b = _rows(rng, al, 70, 3), _rows(rng, bl, 66, 3)
    ref = R.distance_table(a, al, b, bl)
    ta, tal, tb, tbl = _dev(dev, a, al, b, bl)
    rc, out, status = _raw(ta, tal, tb, tbl)
    assert (rc, status) == (0, 0) and np.array_equal(out, ref)
    for side, (s, r), bad in (("a", (0, 3), -1), ("a", (1, 0), 71), ("b", (1, 2), -1), ("b", (0, 0), 67), ("a", (1, 4), 2 ** 31 - 1)):
        la, lb = tal.clone(), tbl.clone()
        (la if side == "a" else lb)[s, r] = bad
        rc, out, status = _raw(ta, la, tb, lb)
        want = ref.copy()
        if side == "a":
            want[s, r, :] = -1
        else:
            want[s, :, r] = -1
        assert rc == 0 and status == _lib.ERR_LENGTH and np.array_equal(out, want), (side, s, r, bad)
        with pytest.raises(_lib.NfstError) as e:
            ops.edit_distance(ta, la, tb, lb)
        assert e.value.code == _lib.ERR_LENGTH
    # the symmetric mode marks the row and the column, the diagonal entry included, as the general mode does
    la = tal.clone()
    la[1, 2] = 71
    rc, out, status = _raw(ta, la, ta, la, symmetric=1)
    pair = R.distance_table(a, al, a, al)
    pair[1, 2, :] = pair[1, :, 2] = -1
    assert rc == 0 and status == _lib.ERR_LENGTH and np.array_equal(out, pair)
    assert np.array_equal(_raw(ta, la, ta.clone(), la.clone())[1], pair)
    with pytest.raises(_lib.NfstError):
        ops.pairwise_edit_distance(ta, la)


def test_two_launches_give_the_same_bits(dev):
    rng = np.random.default_rng(10)
    lens = rng.integers(0, 201, (3, 16)).astype(np.int32)
    tx, tl = _dev(dev, _rows(rng, lens, 200, 3), lens)
    first, pair = ops.edit_distance(tx, tl, tx[:, :5], tl[:, :5]), ops.pairwise_edit_distance(tx, tl)
    assert torch.equal(ops.edit_distance(tx, tl, tx[:, :5], tl[:, :5]), first)
    assert torch.equal(ops.pairwise_edit_distance(tx, tl), pair)
    assert torch.equal(first, pair[:, :, :5])


# ----------------------------------------------------------------------------- real path sets
def _mixed(dev):
    lats = E.mixed_batch()
    return LatticeBatch.from_synth(lats, device=dev), torch.from_numpy(synth.label_scores(7, E.V_MIXED)).to(dev)


def _few(dev):
    lats, theta, b, n = E.few_paths_case()
    return LatticeBatch.from_synth(lats, device=dev), torch.from_numpy(theta).to(dev), b, n


def _check_set(r):
    """Distances of the set to one gold row per lattice (its last path, as a 2-D side) and pairwise, against the
    reference on the copied-back paths.  Slots beyond n_paths have length 0: they are at distance ``len`` from the rest."""
    paths, lens, n = r.paths.cpu().numpy(), r.lengths.cpu().numpy(), r.n_paths.cpu().numpy()
    B, K = lens.shape
    assert all(np.all(lens[b, n[b]:] == 0) for b in range(B))
    last = torch.clamp(r.n_paths.long() - 1, min=0)
    rows = torch.arange(B, device=r.paths.device)
    gold, gold_len = r.paths[rows, last], r.lengths[rows, last]
    D = ops.edit_distance(r.paths, r.lengths, gold, gold_len)
    ref = R.distance_table(paths, lens, gold.cpu().numpy()[:, None, :], gold_len.cpu().numpy()[:, None])[:, :, 0]
    assert D.shape == (B, K) and np.array_equal(D.cpu().numpy(), ref)
    P = ops.pairwise_edit_distance(r.paths, r.lengths)
    pref = R.distance_table(paths, lens, paths, lens)
    assert np.array_equal(P.cpu().numpy(), pref)
    for b in range(B):
        assert np.array_equal(pref[b, :n[b], n[b]:], np.repeat(lens[b, :n[b], None], K - n[b], axis=1))
        off = pref[b, :n[b], :n[b]][~np.eye(n[b], dtype=bool)]
        assert np.all(off > 0)  # distinct paths of a deterministic lattice: distinct mark sequences
    return D, P, pref


def test_k_best_sets(dev):
    lat, theta = _mixed(dev)
    _check_set(ops.k_best(lat, theta, 64, pad=PAD))
    lat, theta, b, n = _few(dev)
    r = ops.k_best(lat, theta, 64, pad=PAD)
    assert int(r.n_paths[b]) == n < 64
    _check_set(r)


def test_swor_sets(dev):
    lat, theta = _mixed(dev)
    _check_set(swor.sample(lat, theta, 64, seed=3, pad=PAD))
    lat, theta, b, n = _few(dev)
    r = swor.sample(lat, theta, 64, seed=4, pad=PAD)
    assert int(r.n_paths[b]) == n < 64
    _check_set(r)


def test_positional_k_best_set(dev):
    lat, theta = _mixed(dev)
    T = 24
    pos = torch.from_numpy(np.random.default_rng(6).normal(size=(lat.n_lattices, T, lat.vocab)).astype(np.float32)).to(dev)
    r = ops.positional_k_best(lat, theta, 16, pos, pad=PAD)
    assert r.paths.shape == (lat.n_lattices, 16, T) and int(r.n_paths.sum()) > 16
    _check_set(r)


def test_expected_distance_and_mbr_on_a_lattice_drawn_whole(dev):
    """few_paths_case with k = 64 above the lattice's number of paths: the Horvitz-Thompson estimate of the expected
    distance to a gold row is the formula of swor.log_weights written out in NumPy on r.logp, r.kappa and the
    reference's distances (on the lattice drawn whole the weights are the probabilities and the estimate is the exact
    expectation), and mbr_decode picks what the restatement picks."""
    lat, theta, b, n = _few(dev)
    r = swor.sample(lat, theta, 64, seed=11, pad=PAD)
    npaths = r.n_paths.cpu().numpy()
    assert npaths[b] == n and float(r.kappa[b]) == -np.inf
    gold, gold_len = r.paths[:, 0], r.lengths[:, 0]
    D = ops.edit_distance(r.paths, r.lengths, gold, gold_len)
    ref = R.distance_table(r.paths.cpu().numpy(), r.lengths.cpu().numpy(), gold.cpu().numpy()[:, None], gold_len.cpu().numpy()[:, None])[:, :, 0]
    assert np.array_equal(D.cpu().numpy(), ref)
    logp, kappa = r.logp.cpu().numpy().astype(np.float64), r.kappa.cpu().numpy()
    want, norm = np.zeros(lat.n_lattices), np.zeros(lat.n_lattices)
    for s in range(lat.n_lattices):
        for i in range(npaths[s]):
            logw = logp[s, i] if kappa[s] == -np.inf else logp[s, i] - np.log(-np.expm1(-np.exp(logp[s, i] - kappa[s])))
            w = np.exp(logw)
            want[s] += w * ref[s, i]
            norm[s] += w
    got = swor.expectation(r, D.double()).cpu().numpy()
    print("expected distance, estimate and formula:", got, want)
    assert np.all(np.abs(got - want) <= 1e-12)
    assert abs(want[b] - float((np.exp(logp[b, :n]) * ref[b, :n]).sum())) <= 1e-12
    got = swor.expectation(r, D.double(), normalize=True).cpu().numpy()
    assert np.all(np.abs(got - want / norm) <= 1e-12)

    index, risk, P = decoders.mbr_decode(r)
    pref = R.distance_table(r.paths.cpu().numpy(), r.lengths.cpu().numpy(), r.paths.cpu().numpy(), r.lengths.cpu().numpy())
    assert P.dtype == torch.int32 and np.array_equal(P.cpu().numpy(), pref)
    logw = swor.log_weights(r).cpu().numpy()
    ref_index, ref_risk = R.mbr_select(pref, logw, npaths)
    risk = risk.cpu().numpy()
    fin = np.isfinite(ref_risk)
    assert np.array_equal(np.isfinite(risk), fin) and np.all(np.abs(risk[fin] - ref_risk[fin]) <= 1e-12 * np.maximum(1.0, ref_risk[fin]))
    # the choice is compared where the restatement's two least risks are further apart than the risks' rounding
    gap = np.array([np.diff(np.sort(ref_risk[s, :npaths[s]])[:2])[0] if npaths[s] > 1 else np.inf for s in range(lat.n_lattices)])
    clear = gap > 1e-9
    assert clear[b] and clear.sum() >= lat.n_lattices - 1
    assert np.array_equal(index.cpu().numpy()[clear], ref_index[clear])
    # the k-best list of the same lattice, weighed by its scores, holds every path too: the same choice
    kb = ops.k_best(lat, theta, 64, pad=PAD)
    kindex, krisk, _ = decoders.mbr_decode(kb)
    chosen = lambda res, idx: res.paths[b, int(idx[b]), :int(res.lengths[b, int(idx[b])])].tolist()
    # (float32 scores against float32 logp: log weights within 2^-24 * 2 |score|, |score| below 100, so weights within
    # 2e-5 of themselves and the risk, a weighted mean of distances, within 1e-4 of itself)
    least = float(ref_risk[b, ref_index[b]])
    assert abs(float(krisk[b, int(kindex[b])]) - least) <= 1e-4 * max(1.0, least)
    if gap[b] > 1e-3 * max(1.0, least):
        assert chosen(kb, kindex) == chosen(r, index)


def test_scorer_entry_point(dev):
    from nfst_amd.scorers import LatticeScorer

    lats, theta, b, n = E.few_paths_case()
    m = LatticeScorer(E.V_MIXED, pad=PAD, theta=theta[b]).to(dev)
    m.set_lattice(LatticeBatch.from_synth(lats, device=dev))
    out = m.mbr(64)
    kb = ops.k_best(m.lattice, m.theta.detach(), 64, pad=PAD)
    index, risk, _ = decoders.mbr_decode(kb)
    assert len(out) == len(lats)
    for s, (rk, marks) in enumerate(out):
        i = int(index[s])
        if i < 0:  # (the dead labels of lattice b may leave another lattice without a path)
            assert int(kb.n_paths[s]) == 0 and (rk, marks) == (float("inf"), [])
        else:
            assert marks == kb.paths[s, i, :int(kb.lengths[s, i])].tolist() and rk == float(risk[s, i])
    assert int(index[b]) >= 0 and len(out[b][1]) > 0
    assert len(m.mbr(8, draws="swor", seed=5)) == len(lats)
    with pytest.raises(ValueError):
        m.mbr(8, draws="beam")


def _entries(r):
    """What LatticeScorer.mbr must return for the draw ``r``: mbr_decode's choice, its marks and its risk"""
    index, risk, _ = decoders.mbr_decode(r)
    out = []
    for s in range(index.shape[0]):
        i = int(index[s])
        out.append((float("inf"), []) if i < 0 else (float(risk[s, i]), r.paths[s, i, :int(r.lengths[s, i])].tolist()))
    return out


def test_scorer_entry_points_on_every_draw(dev):
    """mbr(draws="swor") and both branches of positional_mbr against mbr_decode on the same draw (the draws are
    deterministic: a seed, or no noise at all), with the arguments they forward."""
    from nfst_amd.scorers import LatticeScorer

    lats = E.mixed_batch()
    m = LatticeScorer(E.V_MIXED, pad=PAD, theta=synth.label_scores(7, E.V_MIXED)).to(dev)
    m.set_lattice(LatticeBatch.from_synth(lats, device=dev))
    lat, theta = m.lattice, m.theta.detach()
    L = int(lat.depth.max()) + 3
    assert m.mbr(8, draws="swor", seed=5, max_len=L) == _entries(swor.sample(lat, theta, 8, seed=5, max_len=L, pad=PAD))
    assert m.mbr(8, draws="swor", seed=6) != m.mbr(8, draws="swor", seed=5)  # (the seed arrives)
    assert m.mbr(5, max_len=L) == _entries(ops.k_best(lat, theta, 5, max_len=L, pad=PAD))
    T = 24
    pos = torch.from_numpy(np.random.default_rng(6).normal(size=(lat.n_lattices, T, lat.vocab)).astype(np.float32)).to(dev)
    want = _entries(ops.positional_k_best(lat, theta, 16, pos, pad=PAD))
    assert m.positional_mbr(pos, 16) == want and m.positional_mbr(pos, 16, T=T) == want
    assert sum(1 for rk, marks in want if marks) >= 3
    short = m.positional_mbr(pos[:, :3].contiguous(), 4)  # three arcs: the one-arc lattice has a path, the deep ones none
    assert short == _entries(ops.positional_k_best(lat, theta, 4, pos[:, :3].contiguous(), pad=PAD))
    assert short[5][1] and (float("inf"), []) in short
    got = m.positional_mbr(pos, 16, draws="swor", seed=9)
    assert got == _entries(swor.positional_sample(lat, theta, 16, pos, seed=9, pad=PAD))
    assert all(marks for _, marks in got)
    with pytest.raises(ValueError):
        m.positional_mbr(pos, 4, draws="beam")

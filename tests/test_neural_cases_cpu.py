"""The inputs of tests/test_gpu_neural_edges.py reach the branches they are named for -- CPU only.

The launchers' predicates are restated in tests/neural_cases.py (``with_hid``, ``pack_wh``, the path choice of
``neu_phase_b``, ``NeuLds`` / ``NeuGradLds`` / ``lds_small0``, ``gx_in_lds``); the tile programs are the host packer's,
decoded here.  A hidden-size list, a packing or a lattice changed so that a branch is no longer reached fails here."""
import numpy as np
import pytest

from nfst_amd import synth
from nfst_amd.lattice import LatticeBatch
from tests import neural_cases as NC


def _parity_hidden(name):
    """The hidden sizes tests/test_gpu_parity.py runs `name` at."""
    from tests import test_gpu_parity as P
    marks = [m for m in getattr(P, name).pytestmark if m.name == "parametrize" and m.args[0] == "H"]
    return tuple(marks[0].args[1])


def test_restated_formulas_in_figures():
    assert NC.row_stride(512) == 516 and NC.row_stride(500) == 516 and NC.row_stride(1) == 20
    assert NC.planes_bytes(512) == 49920
    # H = 512: 8 bytes a row + two staged tiles + 32 rows of 516 floats + the three bfloat16 planes
    assert NC.neu_lds_bytes(5340, 512) == 5340 * 8 + 5152 + 66048 + 49920 == NC.MAX_LDS
    assert NC.neu_grad_lds_bytes(3388, 512) == 3388 * 12 + 7200 + 66048 + 16 + 49920 == NC.MAX_LDS
    assert NC.lds_small0(217) == 218 * 8 + 220 * 4 + 7200 + 16
    assert [NC.with_hid(h) for h in (1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512)] == [
        c for c in NC.CLASSES for _ in (0, 1)]
    assert [NC.phase_b_path(h) for h in (48, 64, 100, 128, 192, 256, 272, 300, 448, 500)] == [
        "f32_tail16", "f32", "scalar", "f32", "f32", "packed", "f32_tail16", "scalar", "packed", "scalar"]
    assert NC.class_paths(("two_phase", 1)) == NC.class_paths(("two_phase", 2)) == {"f32_tail16", "f32", "scalar"}
    assert NC.class_paths(("two_phase", 4)) == {"f32_tail16", "f32", "scalar", "packed"}
    assert NC.class_paths(("two_phase", 8)) == {"f32_tail16", "scalar", "packed"}


def test_hidden_sizes_cover_every_class_and_phase_b_path():
    new = set(NC.HIDDEN) | set(NC.GROUPS_HIDDEN)
    # the new lists alone: every class, the first size above every boundary, H = 1, the 16-wide tail in every two-phase
    # class, <8> packed and unpacked
    assert {NC.with_hid(h) for h in NC.HIDDEN} == set(NC.CLASSES)
    assert {1, 9, 17, 33, 65, 129, 257} <= set(NC.HIDDEN)
    for cls in NC.CLASSES[3:]:
        assert any(NC.with_hid(h) == cls and NC.phase_b_path(h) == "f32_tail16" for h in NC.HIDDEN), cls
    assert {(NC.wh_packed(h)) for h in NC.HIDDEN if NC.with_hid(h) == ("two_phase", 8)} == {False, True}
    # together with the sizes tests/test_gpu_parity.py runs (128 and 192 are the float32 path without a tail in <2> and
    # <4>), forward and gradient each: every path every class can take
    for name in ("test_beta_neural_against_oracle", "test_beta_neural_grad_against_autograd"):
        sizes = new | set(_parity_hidden(name))
        for cls in NC.CLASSES[3:]:
            got = {NC.phase_b_path(h) for h in sizes if NC.with_hid(h) == cls}
            assert got == NC.class_paths(cls), (name, cls, NC.class_paths(cls) - got)
    # many groups per tile: every two-phase class, every path
    assert {NC.with_hid(h) for h in NC.GROUPS_HIDDEN} == set(NC.CLASSES[3:])
    assert {NC.phase_b_path(h) for h in NC.GROUPS_HIDDEN} == {"scalar", "f32", "packed", "f32_tail16"}
    # the gradient kernels' table and the dead-row and range cases: small and two-phase kernels
    assert all(h <= 8 for h in NC.GX_HIDDEN) and 8 in NC.GX_HIDDEN and any(h < 8 for h in NC.GX_HIDDEN)
    for hs in (NC.DEAD_HIDDEN, NC.RANGE_HIDDEN):
        assert {NC.with_hid(h)[0] for h in hs} == {"small", "two_phase"}
    assert all(NC.with_hid(h) == ("two_phase", 8) for h in NC.LIMIT_HIDDEN)
    assert {NC.wh_packed(h) for h in NC.LIMIT_HIDDEN} == {False, True}


def test_many_groups_per_tile_under_the_packings_used():
    for name, l in NC.groups_lattices().items():
        for opts in NC.GROUPS_PACKINGS:
            lat = LatticeBatch.from_synth([l], **opts)
            for direction in ("fwd", "bwd"):  # (the gradient kernel walks the alpha program, the forward kernel the beta program)
                n = max(NC.leaders_per_tile(lat, 0, direction))
                if name == "wide":
                    assert n > 31, (name, opts, direction, n)        # round 2 of neu_group_of
                else:
                    assert n >= NC.FETCH_BACK_LEADERS, (name, opts, direction, n)
                    assert n > NC.ROWS_LDS  # a pass of phase B with g0 + 16 > kNeuRows: rows fetched back from the workspace
    # the scratch rows of the double funnel's partial groups are written at two levels under two of the packings
    for opts, scratch in zip(NC.GROUPS_PACKINGS, (True, True, False)):
        lat = LatticeBatch.from_synth([NC.double_funnel()], **opts)
        assert (int(lat.max_rows) > NC.double_funnel().n_rows) == scratch, opts
    # the hidden-size sweep's star: the same under its packings; its batch stays below round 2 (at most 20 groups a tile)
    for opts in NC.HIDDEN_PACKINGS:
        lat = LatticeBatch.from_synth([NC.star()], **opts)
        assert min(NC.max_leaders(lat, "fwd"), NC.max_leaders(lat, "bwd")) >= NC.FETCH_BACK_LEADERS
        lat = LatticeBatch.from_synth(list(NC.grad_batch()), **opts)
        assert max(NC.max_leaders(lat, "fwd"), NC.max_leaders(lat, "bwd")) <= 31


@pytest.mark.parametrize("H", NC.GX_HIDDEN)
def test_gx_vocabularies_fall_on_both_sides(H):
    v_in, v_out, rows = NC.gx_pair(H)
    assert v_out == v_in + 1
    for V, side in ((v_in, True), (v_out, False)):
        lat = LatticeBatch.from_synth(NC.gx_lattices(V))
        assert int(lat.max_rows) == rows and int(lat.vocab) == V
        assert bool(NC.gx_in_lds(rows, H, V)) == side
        # what the kernel is launched with fits either way
        assert NC.lds_small0(rows) + (V * H * 4 if side else 0) <= NC.MAX_LDS
        used = np.unique(np.concatenate([l.label for l in NC.gx_lattices(V)]))
        assert 200 < used.shape[0] < V // 10 and used.max() < V   # most rows of emb get no gradient
    if H == 8:
        assert 4700 <= v_in <= 5000
    # the 200 arcs of one label that meet in one row of the LDS table (V = 256 fits at both sizes)
    for l in (NC.star(), NC.double_funnel()):
        assert np.bincount(l.label[l.dst == 202]).max() == 200
        lat = LatticeBatch.from_synth([l])
        assert NC.gx_in_lds(int(lat.max_rows), H, l.vocab)


@pytest.mark.parametrize("H", NC.LIMIT_HIDDEN)
def test_limit_lattices_have_the_rows_claimed(H):
    r = NC.limit_rows(H)
    if H == 512:
        assert (r["fwd_fits"], r["grad_fits"]) == (5340, 3388)
    assert r["grad_refused"] < r["fwd_fits"]  # the window where the forward op runs and its gradient is refused
    for k, rows in r.items():
        l = NC.limit_lattice(rows)
        lat = LatticeBatch.from_synth([l])
        assert int(lat.max_rows) == rows == l.n_rows, (k, rows, int(lat.max_rows))
        fwd, grad = NC.neu_lds_bytes(rows, H) <= NC.MAX_LDS, NC.neu_grad_lds_bytes(rows, H) <= NC.MAX_LDS
        assert (fwd, grad) == dict(fwd_fits=(True, False), fwd_refused=(False, False), grad_fits=(True, True),
                                   grad_refused=(True, False))[k], k
    # at the largest size the three bfloat16 planes end with the workgroup's LDS (to the 16 bytes of its alignment)
    assert NC.MAX_LDS - NC.neu_lds_bytes(r["fwd_fits"], H) < 16 and NC.MAX_LDS - NC.neu_grad_lds_bytes(r["grad_fits"], H) < 16
    # the small call after a refusal is thousands of rows from either limit
    lat = LatticeBatch.from_synth([NC.small_lattice()])
    assert NC.neu_grad_lds_bytes(int(lat.max_rows), H) < NC.MAX_LDS - 32 * 1024


def test_dead_rows_are_where_the_case_says():
    l, live, dead, partial = NC.dead_case()
    assert 1 < dead < l.n_rows - 1 and 1 < partial < l.n_rows - 1
    assert np.all(np.isneginf(l.weight[l.src == dead])) and np.any(l.dst == dead)
    wp = l.weight[l.src == partial]
    assert np.count_nonzero(np.isneginf(wp)) == 1 and np.count_nonzero(np.isfinite(wp)) >= 2
    assert np.count_nonzero(np.isneginf(l.weight)) == np.count_nonzero(l.src == dead) + 1
    assert not np.any(np.isneginf(live.weight))
    for H in NC.DEAD_HIDDEN:
        p = NC.dead_params(H)
        logb, bhat = NC.oracle_forward(l, p)
        assert np.array_equal(np.nonzero(np.isneginf(logb))[0], [dead]) and not np.any(bhat[dead])
        # the oracle on the pruned lattice -- what the gradients are held to -- has one sink and the same values
        pl = NC.pruned(l, logb)
        assert pl.n_arcs == l.n_arcs - np.count_nonzero(l.src == dead) - np.count_nonzero(l.dst == dead) - 1
        lb2, bh2 = NC.oracle_forward(pl, p)
        fin = np.isfinite(logb)
        assert np.array_equal(np.isfinite(lb2), fin)
        assert np.max(np.abs(lb2[fin] - logb[fin])) <= 1e-12 and np.max(np.abs(bh2 - bhat)) <= 1e-12
        # the -inf arcs matter: with them at weight 0 the values differ
        full = synth.SynthLattice(n_rows=l.n_rows, vocab=l.vocab, src=l.src, label=l.label, dst=l.dst,
                                  weight=np.where(np.isneginf(l.weight), 0.0, l.weight).astype(np.float32))
        assert abs(NC.oracle_forward(full, p)[0][0] - logb[0]) > 1e-3


@pytest.mark.parametrize("H", NC.RANGE_HIDDEN)
def test_range_lattice_has_siblings_on_both_sides_of_the_drop(H):
    l = NC.range_lattice()
    p = NC.range_params(H)
    assert set(np.unique(l.weight)) == set(NC.RANGE_WEIGHTS)
    lat = LatticeBatch.from_synth([l])
    assert int(lat.meta_host[0][NC._lib.META_DEPTH]) <= 12
    logb, bhat = NC.oracle_forward(l, p)
    assert np.all(np.isfinite(logb)) and np.max(np.abs(logb)) < NC.ME_LOG32_EXACT
    z = NC.arc_logits(l, p, logb, bhat)
    real = l.src != l.dst
    below = []
    for s in range(l.n_rows - 1):
        zs = z[real & (l.src == s)]
        below.extend(zs.max() - zs[zs < zs.max()])
    below = np.array(below)
    # siblings more than 120 binary orders below their state's largest term (dropped by neu_scale), and less
    assert np.count_nonzero(below > NC.DROP_NATS + 1.0) >= 20 and np.count_nonzero((below > 20.0) & (below < NC.DROP_NATS - 1.0)) >= 20
    # tanh saturates: the pre-activations of a good part of the components lie beyond +-4
    x = p["emb"].astype(np.float64) @ p["Wx"].T.astype(np.float64) + p["bias"]
    assert np.mean(np.abs(x) > 4.0) > 0.25


def test_float32_recurrences_follow_the_oracle():
    """The float32 restatements the limit-size cases take their allowance from are the oracle's recurrence: on small
    lattices (plain, and with table weights) they agree with it to float32 accuracy."""
    for l, V in ((NC.small_lattice(), 256), (NC.grad_batch()[0], NC.V_BATCH)):
        for H in (8, 64):
            p = NC.neural_params(70 + H, V, H)
            c, ch = NC.coefficients(71 + H, l, H)
            logb, bhat, g = NC.oracle_grad(l, p, c, ch)
            lb32, bh32 = NC.beta_neural_f32(l, p)
            assert np.max(np.abs(lb32 - logb)) <= 1e-5 and np.max(np.abs(bh32 - bhat)) <= 1e-5
            g32 = NC.grad_f32(l, p, c, ch)
            for k in NC.PARAMS:
                assert g32[k].shape == g[k].shape
                assert np.max(np.abs(g32[k] - g[k])) <= 1e-5 * np.max(np.abs(g[k])), (H, k)

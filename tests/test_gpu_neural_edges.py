"""The neuralised beta kernels (csrc/neural_kernels.h) against the float64 oracle at every branch of their launchers.
Needs a real MI355X: run with ``pytest -m gpu``.

The inputs come from tests/neural_cases.py; tests/test_neural_cases_cpu.py proves on the host that they reach the
branches named here.  Bounds, the ones tests/test_gpu_parity.py holds these kernels to: log beta <= 3e-5 + half a float32
spacing at its magnitude, beta_hat <= 3e-5 absolute, each of the five parameter gradients <= 1e-4 of the largest entry
of the float64 gradient; every forward runs twice and must give the same bits.  Gradients enter through log beta AND
beta_hat.  The largest errors seen are written to neural_edge_errors.json in the directory of run outputs
(profiles/README.md; DESIGN.md section 5 quotes them)."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

from nfst_amd import ops, _lib
from nfst_amd.lattice import LatticeBatch
from tests import neural_cases as NC

pytestmark = pytest.mark.gpu
PARAMS = NC.PARAMS
TOL_ROWS, TOL_HAT, TOL_GRAD = 3e-5, 3e-5, 1e-4
ERR_LIMIT = -6  # NFST_ERR_LIMIT

_ERR = {}


def rec(tag, err):
    err = float(err)
    _ERR[tag] = max(_ERR.get(tag, 0.0), err)
    print(f"{tag}: {err:.3e}")
    return err


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    # the directory of run outputs at the repository's root, as in test_gpu_paths.py (a run that wants the figures
    # creates it; nothing is written without it)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for out in sorted(glob.glob(os.path.join(root, "*_out"))):
        if _ERR and os.path.isdir(out):
            import json
            with open(os.path.join(out, "neural_edge_errors.json"), "w") as f:
                json.dump(dict(sorted(_ERR.items())), f, indent=1)


def forward_twice(lat, p):
    t = [torch.from_numpy(p[k]) for k in PARAMS]
    r, again = ops.backward_neural(lat, *t), ops.backward_neural(lat, *t)
    assert torch.equal(r.log_beta, again.log_beta) and torch.equal(r.beta_hat, again.beta_hat)  # no race, no stale line
    return r


def check_rows(tag, lat, r, lats, refs, tol_rows=TOL_ROWS, tol_hat=TOL_HAT):
    """log beta by cmp_rows's rule (-inf on exactly the oracle's rows), beta_hat absolutely; refs[b] = (log beta, beta_hat, ...)."""
    lb, bh = r.log_beta.detach().cpu().numpy().astype(np.float64), r.beta_hat.detach().cpu().numpy().astype(np.float64)
    for b, (l, ref) in enumerate(zip(lats, refs)):
        r0 = int(lat.row_off[b])
        got, logb, bhat = lb[r0:r0 + l.n_rows], ref[0], ref[1]
        inf = np.isneginf(logb)
        assert np.array_equal(np.isneginf(got), inf), (tag, b)
        assert not np.any(bh[r0:r0 + l.n_rows][inf]), (tag, b)
        err = np.abs(got[~inf] - logb[~inf])
        half_ulp = 0.5 * np.spacing(np.abs(logb[~inf]).astype(np.float32)).astype(np.float64)
        rec(tag + "_log_beta", err.max())
        beyond = rec(tag + "_log_beta_beyond_f32_rounding", np.maximum(err - half_ulp, 0.0).max())
        hat = rec(tag + "_beta_hat", np.max(np.abs(bh[r0:r0 + l.n_rows] - bhat)))
        assert beyond <= tol_rows and hat <= tol_hat, (tag, b, beyond, hat, tol_rows, tol_hat)


def grads(lat, p, lats, coefs):
    """The loss sum coef . log beta + sum coef_hat . beta_hat through ops.backward_neural: (NeuralBeta, {name: grad})."""
    H = p["Wh"].shape[0]
    rows, hat = np.zeros(lat.total_rows), np.zeros((lat.total_rows, H))
    for b, (l, (c, ch)) in enumerate(zip(lats, coefs)):
        r0 = int(lat.row_off[b])
        rows[r0:r0 + l.n_rows], hat[r0:r0 + l.n_rows] = c, ch
    t = {k: torch.from_numpy(p[k]).to(lat.device).requires_grad_(True) for k in PARAMS}
    r = ops.backward_neural(lat, *(t[k] for k in PARAMS))
    c = torch.from_numpy(rows.astype(np.float32)).to(lat.device)
    loss = (c[c != 0] * r.log_beta[c != 0]).sum() + (torch.from_numpy(hat.astype(np.float32)).to(lat.device) * r.beta_hat).sum()
    loss.backward()
    return r, {k: t[k].grad.detach().cpu().numpy().astype(np.float64) for k in PARAMS}


def rel_err(got, ref):
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-30))


def check_grads(tag, got, refs, tol_grad=None):
    ref = {k: sum(r[2][k] for r in refs) for k in PARAMS}
    for k in PARAMS:
        assert np.all(np.isfinite(got[k])), (tag, k)
        rel = rec(tag + "_grad_rel", rel_err(got[k], ref[k]))
        assert rel <= (tol_grad[k] if tol_grad else TOL_GRAD), (tag, k, rel, tol_grad)


def check_case(dev, tag, lats, p, coefs, refs, packings, tol_grad=None, **tol):
    """Forward (twice) and gradient of one batch under every packing against refs[b] = (log beta, beta_hat, gradients)."""
    out = None
    for opts in packings:
        lat = LatticeBatch.from_synth(list(lats), device=dev, **opts)
        check_rows(tag, lat, forward_twice(lat, p), lats, refs, **tol)
        r, got = grads(lat, p, lats, coefs)
        check_rows(tag, lat, r, lats, refs, **tol)
        check_grads(tag, got, refs, tol_grad)
        out = got
    return out


def references(lats, p, seed):
    H = p["Wh"].shape[0]
    coefs = [NC.coefficients(seed + b, l, H) for b, l in enumerate(lats)]
    return coefs, [NC.oracle_grad(l, p, c, ch) for l, (c, ch) in zip(lats, coefs)]


# ----------------------------------------------------------------------------- hidden sizes
@pytest.mark.parametrize("H", NC.HIDDEN)
def test_every_hidden_size_class_and_phase_b_path(dev, H):
    """The first size above every with_hid boundary, H = 1, the 16-wide tail of phase B's float32 path, <8> with and
    without the packed Wh: the weighted three-lattice batch (V = 64) and the star (V = 256), forward and gradient."""
    for name, lats, V in (("batch", NC.grad_batch(), NC.V_BATCH), ("star", (NC.star(),), NC.V_STAR)):
        p = NC.neural_params(H + 1, V, H)
        coefs, refs = references(lats, p, 100 + H)
        check_case(dev, f"hidden_H{H}", lats, p, coefs, refs, NC.HIDDEN_PACKINGS)


# ----------------------------------------------------------------------------- many groups per tile
@pytest.mark.parametrize("H", NC.GROUPS_HIDDEN)
def test_two_phase_kernels_with_many_groups_per_tile(dev, H):
    """Tiles of 64 (star, double funnel) and 48 groups (the wide lattice) in the two-phase kernels: rounds >= 2 of
    neu_group_of and the fetch-back pass of phase B, forward and gradient; the double funnel's scratch rows are rewritten
    at its second level."""
    p = NC.neural_params(H + 3, 256, H)
    for name, l in NC.groups_lattices().items():
        coefs, refs = references((l,), p, 200 + H)
        check_case(dev, f"groups_{name}", (l,), p, coefs, refs, NC.GROUPS_PACKINGS)


# ----------------------------------------------------------------------------- the dL/dx table of the small gradient kernel
@pytest.mark.parametrize("H", NC.GX_HIDDEN)
def test_label_gradient_table_on_both_sides_of_its_limit(dev, H):
    """k_backward_neural_grad_small sums dL/dx in LDS while [V, H] floats fit (gx_in_lds) and with global atomics
    beyond: the largest vocabulary that fits and the next one.  Rows of emb whose label no arc carries get exactly zero."""
    v_in, v_out, rows = NC.gx_pair(H)
    for V, side in ((v_in, True), (v_out, False)):
        lats = NC.gx_lattices(V)
        lat = LatticeBatch.from_synth(lats)
        assert int(lat.max_rows) == rows and bool(NC.gx_in_lds(rows, H, V)) == side
        p = NC.neural_params(H + 4, V, H)
        coefs, refs = references(lats, p, 300 + H)
        got = check_case(dev, f"gx_{'lds' if side else 'global'}", lats, p, coefs, refs, (dict(),))
        unused = np.setdiff1d(np.arange(V), np.concatenate([l.label for l in lats]))
        assert unused.shape[0] > V // 2 and not np.any(got["emb"][unused])
        assert np.count_nonzero(np.any(got["emb"] != 0, axis=1)) > 200


@pytest.mark.parametrize("H", NC.GX_HIDDEN)
def test_label_gradient_table_with_200_arcs_of_one_label(dev, H):
    """The star's and the double funnel's gradient in the small kernel at H <= 8: 200 arcs of one label add into one
    row of the LDS table."""
    p = NC.neural_params(H + 5, 256, H)
    for name, l in (("star", NC.star()), ("double_funnel", NC.double_funnel())):
        coefs, refs = references((l,), p, 400 + H)
        check_case(dev, f"gx_collisions_{name}", (l,), p, coefs, refs, NC.GROUPS_PACKINGS)


# ----------------------------------------------------------------------------- LDS limits
@functools.lru_cache(maxsize=None)
def _small_reference(H):
    l = NC.small_lattice()
    p = NC.neural_params(H + 6, 256, H)
    coefs, refs = references((l,), p, 500 + H)
    return l, p, coefs, refs


def small_call_is_right(dev, H, tag):
    l, p, coefs, refs = _small_reference(H)
    check_case(dev, tag, (l,), p, coefs, refs, (dict(),))


def limit_batch(dev, H, which):
    rows = NC.limit_rows(H)[which]
    l = NC.limit_lattice(rows)
    lat = LatticeBatch.from_synth([l], device=dev)
    assert int(lat.max_rows) == rows
    return l, lat, NC.neural_params(H + 7, 256, H)


def float32_allowance(tag, l, p, logb, bhat):
    """The forward bounds of a limit-size case.  Its lattices are 55 to 87 levels of 64 states with two arcs a state:
    beta_hat is a mean over two messages, and Wh (scale 2) carries a rounding error from level to level with a gain above
    one, so that float32 arithmetic alone leaves more than the 3e-5 of the small batches.  The kernel gets 4 times the
    error of the same recurrence in NumPy float32 (NC.beta_neural_f32) against the float64 oracle -- its sums run in
    another order, and its exp2 / rcp tanh adds up to 2e-7 per component -- and never less than the usual bounds."""
    lb32, bh32 = NC.beta_neural_f32(l, p)
    e_rows = rec(tag + "_float32_recurrence_log_beta", np.max(np.abs(lb32 - logb)))
    e_hat = rec(tag + "_float32_recurrence_beta_hat", np.max(np.abs(bh32 - bhat)))
    return dict(tol_rows=max(TOL_ROWS, 4.0 * e_rows), tol_hat=max(TOL_HAT, 4.0 * e_hat))


def float32_gradient_allowance(tag, l, p, coefs, ref):
    """The same for the gradients: 4 times what torch.autograd over the recurrence in float32 (NC.grad_f32) leaves of the
    float64 gradients, per parameter, and never less than the usual 1e-4."""
    g32 = NC.grad_f32(l, p, *coefs)
    return {k: max(TOL_GRAD, 4.0 * rec(tag + "_float32_recurrence_grad_rel", rel_err(g32[k], ref[k]))) for k in PARAMS}


@pytest.mark.parametrize("H", NC.LIMIT_HIDDEN)
def test_forward_at_the_largest_row_count_that_fits(dev, H):
    """NeuLds(max_rows, H).bytes() within 16 bytes of the 160 KiB: the three bfloat16 planes end where LDS ends.
    Measured (log beta beyond float32 rounding / beta_hat): H = 512, 5340 rows: kernel 2.8e-4 / 4.5e-4, the float32
    recurrence 1.6e-4 / 2.1e-4; H = 500, 5484 rows: kernel 3.9e-4 / 4.1e-4, the float32 recurrence 2.8e-4 / 3.1e-4."""
    l, lat, p = limit_batch(dev, H, "fwd_fits")
    assert NC.MAX_LDS - NC.neu_lds_bytes(int(lat.max_rows), H) < 16
    ref = NC.oracle_forward(l, p)
    check_rows(f"limit_forward_H{H}", lat, forward_twice(lat, p), (l,), [ref], **float32_allowance(f"limit_forward_H{H}", l, p, *ref))


@pytest.mark.parametrize("H", NC.LIMIT_HIDDEN)
def test_gradient_at_the_largest_row_count_that_fits(dev, H):
    """NeuGradLds(max_rows, H).bytes() within 16 bytes of the 160 KiB.  Measured (log beta / beta_hat / worst gradient):
    H = 512, 3388 rows: kernel 6.0e-5 / 6.8e-5 / 2.0e-4, the float32 recurrence 8.1e-5 / 1.2e-4 / 5.4e-4; H = 500, 3484
    rows: kernel 7.3e-5 / 1.3e-4 / 8.5e-5, the float32 recurrence 3.7e-5 / 6.8e-5 / 1.1e-4."""
    l, lat, p = limit_batch(dev, H, "grad_fits")
    assert NC.MAX_LDS - NC.neu_grad_lds_bytes(int(lat.max_rows), H) < 16
    coefs, refs = references((l,), p, 600 + H)
    tol = float32_allowance(f"limit_gradient_H{H}", l, p, refs[0][0], refs[0][1])
    tol_grad = float32_gradient_allowance(f"limit_gradient_H{H}", l, p, coefs[0], refs[0][2])
    check_case(dev, f"limit_gradient_H{H}", (l,), p, coefs, refs, (dict(),), tol_grad=tol_grad, **tol)


@pytest.mark.parametrize("H", NC.LIMIT_HIDDEN)
def test_beyond_the_lds_limits_the_ops_refuse_before_any_launch(dev, H):
    """One state beyond the forward limit the op raises NFST_ERR_LIMIT; one state beyond the gradient's limit the
    forward succeeds and loss.backward() raises it.  Either refusal is a return code before the launch: a small call
    after it gives the right answer."""
    l, lat, p = limit_batch(dev, H, "fwd_refused")
    with pytest.raises(_lib.NfstError) as e:
        ops.backward_neural(lat, *(torch.from_numpy(p[k]) for k in PARAMS))
    assert e.value.code == ERR_LIMIT
    small_call_is_right(dev, H, f"after_refusal_H{H}")

    l, lat, p = limit_batch(dev, H, "grad_refused")
    t = {k: torch.from_numpy(p[k]).to(dev).requires_grad_(True) for k in PARAMS}
    r = ops.backward_neural(lat, *(t[k] for k in PARAMS))
    assert bool(torch.all(torch.isfinite(r.log_beta)))
    with pytest.raises(_lib.NfstError) as e:
        r.log_beta.sum().backward()
    assert e.value.code == ERR_LIMIT
    small_call_is_right(dev, H, f"after_refusal_H{H}")


# ----------------------------------------------------------------------------- dead rows
@pytest.mark.parametrize("H", NC.DEAD_HIDDEN)
def test_dead_rows(dev, H):
    """A state whose every out-arc has table weight -inf, and one with a single such arc, beside a live lattice: log beta
    is -inf and beta_hat 0 on exactly the oracle's rows; with coefficients of zero there, every gradient is finite and
    equals the oracle's on the lattice without the -inf arcs and without the arcs that touch a dead state."""
    l, live, dead, partial = NC.dead_case()
    p = NC.dead_params(H)
    logb, bhat = NC.oracle_forward(l, p)
    gone = np.nonzero(np.isneginf(logb))[0]
    assert dead in gone
    c, ch = NC.coefficients(700 + H, l, H, zero_rows=gone)
    plb, pbh, pg = NC.oracle_grad(NC.pruned(l, logb), p, c, ch)
    fin = np.isfinite(logb)
    assert np.array_equal(np.isfinite(plb), fin) and np.max(np.abs(plb[fin] - logb[fin])) <= 1e-12
    c2, ch2 = NC.coefficients(710 + H, live, H)
    refs = [(logb, bhat, pg), NC.oracle_grad(live, p, c2, ch2)]
    check_case(dev, "dead_rows", (l, live), p, [(c, ch), (c2, ch2)], refs, NC.GROUPS_PACKINGS)


# ----------------------------------------------------------------------------- exponent range
@pytest.mark.parametrize("H", NC.RANGE_HIDDEN)
def test_table_weights_across_the_exponent_range(dev, H):
    """Table weights from {0, -30, -80, -100}: siblings less and more than 120 binary orders apart (the latter dropped by
    neu_scale, clamped by the gradient's ldexpf), embeddings times 8 so that tanh saturates."""
    l = NC.range_lattice()
    p = NC.range_params(H)
    coefs, refs = references((l,), p, 800 + H)
    check_case(dev, "exponent_range", (l,), p, coefs, refs, NC.GROUPS_PACKINGS)

"""Draws without replacement: k distinct paths per lattice from p(path) = exp S(path) / Z by stochastic beam search
(Gumbel top-k; Kool, van Hoof and Welling 2019), the Horvitz-Thompson weights that turn the drawn set into an unbiased
estimate of any expectation, and the differentiable log-probabilities of the drawn paths (DESIGN.md sections 2 and 4.15).

``sample`` is one launch of ``nfst_swor`` (include/nfst_hip.h) behind the beta sweep, ``positional_sample`` its twin
under per-position scores and a length budget (``nfst_positional_swor``); everything else is
torch arithmetic on their result.  There is no CPU implementation of the search.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import ops
from .lattice import LatticeBatch
from .ops import _call, _check_k, _max_len, _path_outputs, _path_score_grads, _raise_status, _scores, _workspace


class SworResult(NamedTuple):
    paths: torch.Tensor  # [B, k, max_len] int32 labels, pad-terminated
    arcs: Optional[torch.Tensor]  # [B, k, max_len] int32 canonical arc ids, -1 padded
    lengths: torch.Tensor  # [B, k] int32 arcs per path (0 beyond n_paths)
    logp: torch.Tensor  # [B, k] float32 = path score - log Z (-inf beyond n_paths)
    gumbel: torch.Tensor  # [B, k] float64 perturbed scores, non-increasing (-inf beyond n_paths)
    kappa: torch.Tensor  # [B] float64 the largest perturbed score that was dropped (-inf: nothing was)
    n_paths: torch.Tensor  # [B] int32 min(k, paths of score > -inf)
    logz: torch.Tensor  # [B] float32


def max_degree(lat: LatticeBatch) -> int:
    """The batch's largest out-degree (self loops counted): the last dimension of ``sample``'s ``uniforms``."""
    return int(torch.diff(lat.row_ptr).max())


def sample(lat: LatticeBatch, theta, k: int, arc_scores=None, max_len: Optional[int] = None,
           uniforms: Optional[torch.Tensor] = None, seed: int = 0, pad: int = 0,
           beta: Optional["ops.BackwardResult"] = None, want_arcs: bool = True) -> SworResult:
    """k distinct paths per lattice, drawn without replacement from the exact posterior, ranked by their perturbed
    scores: what ``ops.sample_paths`` draws with replacement (Sampler.sample, modules/samplers.py:137-335), without the
    copies of the best path that K draws from a peaked posterior mostly are.  1 <= k <= 64.  ``beta``: the
    ``ops.backward`` result of the same scores (with ``logbeta``), computed here if absent.  ``uniforms`` [B, max_len,
    k, D] float32 in [0, 1), D the batch's largest out-degree (``max_degree``): entry [b, t, j, r] perturbs the arc of
    rank r out of slot j's state at step t; without them the noise comes from Philox keyed by ``seed``.  ``max_len``
    defaults to the longest path + 1; a longer draw raises ``NfstError`` (NFST_ERR_LENGTH)."""
    ops._need_gpu(lat)
    _check_k(k)
    sc, keep = _scores(lat, theta, arc_scores)
    max_len = _max_len(lat, max_len)
    if beta is None or beta.logbeta is None:
        beta = ops.backward(lat, theta, arc_scores)
    dev, B = lat.device, lat.n_lattices
    degree = 0
    if uniforms is not None:
        uniforms = uniforms.to(device=dev, dtype=torch.float32).contiguous()
        if uniforms.dim() != 4 or uniforms.shape[:3] != (B, max_len, k) or uniforms.shape[3] < 1:
            raise ValueError(f"uniforms must be [{B}, {max_len}, {k}, largest out-degree]")
        degree = int(uniforms.shape[3])
    ws, ws_bytes = _workspace(lat, "nfst_swor_ws_bytes", k, int(max_len))
    _, paths, arcs, lens, n_paths, logp = _path_outputs(lat, (B, k), max_len, arcs=want_arcs, n_paths=True, logq=True)
    gumbel = torch.empty((B, k), dtype=torch.float64, device=dev)
    kappa = torch.empty(B, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _call("nfst_swor", lat, sc, beta.logbeta, beta.logz64, int(k), int(max_len), uniforms, degree, C.c_uint64(seed & (2 ** 64 - 1)),
          int(pad), ws, ws_bytes, paths, arcs, lens, logp, gumbel, kappa, n_paths, status)
    _raise_status(status, "nfst_swor")  # the length budget, or uniforms narrower than a state's out-arcs
    return SworResult(paths, arcs, lens, logp, gumbel, kappa, n_paths, beta.logz)


def positional_sample(lat: LatticeBatch, theta, k: int, pos_scores=None, T: Optional[int] = None, arc_scores=None,
                      uniforms: Optional[torch.Tensor] = None, seed: int = 0, pad: int = 0, want_arcs: bool = True) -> SworResult:
    """``sample`` under the scores of ``ops.positional_forward_backward``: k distinct paths per lattice drawn without
    replacement from p_T(path) = exp(S_T(path)) / Z_T over the paths of at most ``T`` arcs, where the arc at position t
    also scores ``pos_scores[(b,) t, label]`` (``nfst_positional_swor``; DESIGN.md sections 2 and 4.16).  What
    ``ops.positional_sample_paths`` draws with replacement, without the copies of ``positional_viterbi``'s path: the
    weighted path set that a sequence-level loss needs.  1 <= k <= 64.  ``T`` defaults as in ``ops.positional_k_best``: to
    ``pos_scores.shape[-2]``, without ``pos_scores`` to the longest path of the batch.  ``uniforms`` [B, T, k, D] as in
    ``sample``.  No draw overruns ``T`` and there is no length error: a prefix that cannot finish within ``T`` has no
    mass.  ``paths`` / ``arcs`` are [B, k, T] and ``logz`` is log Z_T; ``log_weights`` and ``expectation`` work on the
    result unchanged.  One backward pass with every beta row stored (12 (T + 1) total_rows bytes of workspace), then
    the search."""
    ops._need_gpu(lat)
    _check_k(k)
    sc, keep, pos, stride, T = ops._score_args(lat, theta, arc_scores, pos_scores, T)
    dev, B = lat.device, lat.n_lattices
    degree = 0
    if uniforms is not None:
        if not isinstance(uniforms, torch.Tensor) or uniforms.dim() != 4 or uniforms.shape[:3] != (B, T, k) or uniforms.shape[3] < 1:
            raise ValueError(f"uniforms must be a tensor of shape [{B}, {T}, {k}, largest out-degree]")
        uniforms = uniforms.detach().to(device=dev, dtype=torch.float32).contiguous()
        degree = int(uniforms.shape[3])
    ws, ws_bytes = _workspace(lat, "nfst_positional_swor_ws_bytes", T, int(k))
    z64 = torch.empty(B, dtype=torch.float64, device=dev)
    z32 = torch.empty(B, dtype=torch.float32, device=dev)
    _, paths, arcs, lens, n_paths, logp = _path_outputs(lat, (B, k), T, arcs=want_arcs, n_paths=True, logq=True)
    gumbel = torch.empty((B, k), dtype=torch.float64, device=dev)
    kappa = torch.empty(B, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _call("nfst_positional_swor", lat, sc, pos, stride, T, int(k), uniforms, degree, C.c_uint64(seed & (2 ** 64 - 1)), int(pad),
          ws, ws_bytes, z64, z32, paths, arcs, lens, logp, gumbel, kappa, n_paths, status)
    _raise_status(status, "nfst_positional_swor")  # uniforms narrower than a state's out-arcs
    return SworResult(paths, arcs, lens, logp, gumbel, kappa, n_paths, z32)


def log_weights(r: SworResult) -> torch.Tensor:
    """log w [B, k] float64 of the Horvitz-Thompson weights w_i = p_i / q_i, q_i = 1 - exp(-exp(log p_i - kappa)) the
    probability that path i's perturbed score exceeds the threshold kappa: log w = logp - log(-expm1(-exp(logp - kappa))).
    w = p where kappa = -inf (every path of the lattice was drawn); -inf beyond ``n_paths``."""
    logp = r.logp.double()
    kappa = r.kappa[:, None].expand_as(logp)
    ok = torch.arange(logp.shape[1], device=logp.device)[None, :] < r.n_paths[:, None]
    all_drawn = torch.isinf(kappa) & (kappa < 0)
    d = torch.where(ok & ~all_drawn, logp - kappa, torch.zeros_like(logp))
    logq = torch.log(-torch.expm1(-torch.exp(d)))
    logw = torch.where(all_drawn, logp, logp - logq)
    return torch.where(ok, logw, torch.full_like(logw, float("-inf")))


def expectation(r: SworResult, values: torch.Tensor, normalize: bool = False) -> torch.Tensor:
    """sum_i w_i values[b, i] per lattice, float64 [B]: an unbiased estimate of E_p[value], exact once k reaches the
    lattice's number of paths.  ``normalize=True`` divides by sum_i w_i (biased, lower variance).  Entries beyond
    ``n_paths`` do not count, whatever their values.  The expected edit distance to a gold sequence ``gold`` [B, L] of
    lengths ``gold_len`` [B], a sequence-level risk, is::

        cost = ops.edit_distance(r.paths, r.lengths, gold, gold_len).double()
        risk = swor.expectation(r, cost, normalize=True)
    """
    w = torch.exp(log_weights(r))
    v = torch.where(w > 0, values.to(device=w.device, dtype=torch.float64), torch.zeros_like(w))
    tot = (w * v).sum(dim=1)
    return tot / w.sum(dim=1) if normalize else tot


class _PathScore(torch.autograd.Function):
    """score[b, i] = the sum of the scores of path i's arcs (float64 from ``ops.score_paths``' sum, rounded once):
    d / d arc_scores[a] = 1 on the path's arcs, d / d theta counts its labels."""

    @staticmethod
    def forward(ctx, lat, theta, arc_scores, paths, arcs):
        tot, _ = ops.score_paths(lat, theta.detach(), paths, arc_scores=None if arc_scores is None else arc_scores.detach())
        ctx.lat = lat
        ctx.like = (theta, arc_scores)
        ctx.save_for_backward(arcs)
        return tot

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (arcs,) = ctx.saved_tensors
        nt, na = ctx.needs_input_grad[1:3]
        theta, arc_scores = ctx.like
        d_theta, d_arc, _ = _path_score_grads(ctx.lat, arcs, g, theta if nt else None, arc_scores if na else None)
        return None, d_theta, d_arc, None, None


class _PositionalPathScore(torch.autograd.Function):
    """``_PathScore`` under positional scores (``ops.positional_score_paths``): the arc at position t of a path also marks
    (t, label) in d / d pos_scores."""

    @staticmethod
    def forward(ctx, lat, theta, pos_scores, arc_scores, paths, arcs, T):
        tot, _, _ = ops.positional_score_paths(lat, theta.detach(), paths, ops._det(pos_scores), T, ops._det(arc_scores))
        ctx.lat = lat
        ctx.like = (theta, pos_scores, arc_scores)
        ctx.save_for_backward(arcs)
        return tot

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (arcs,) = ctx.saved_tensors
        nt, npos, na = ctx.needs_input_grad[1:4]
        theta, pos_scores, arc_scores = ctx.like
        d_theta, d_arc, d_pos = _path_score_grads(ctx.lat, arcs, g, theta if nt else None, arc_scores if na else None,
                                                  pos_like=pos_scores if npos else None)
        return None, d_theta, d_pos, d_arc, None, None, None


def positional_log_prob(lat: LatticeBatch, theta: torch.Tensor, r: SworResult, pos_scores: Optional[torch.Tensor] = None,
                        T: Optional[int] = None, arc_scores: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``log_prob`` for a result of ``positional_sample`` under the same scores and ``T``: the path's score
    (``ops.positional_score_paths``) minus ``ops.positional_log_z``, float32 [B, k], the numbers of ``r.logp``,
    differentiable in ``theta``, ``arc_scores`` and ``pos_scores``: the gradient is the path's label / arc / (position,
    label) counts minus the posteriors of ``ops.positional_forward_backward``.  -inf beyond ``n_paths`` (no gradient
    there)."""
    if r.arcs is None:
        raise ValueError("positional_log_prob needs the paths' arcs: positional_sample(..., want_arcs=True)")
    if pos_scores is None and T is None:
        T = int(r.paths.shape[2])
    _, _, T = ops._positions(lat, pos_scores, T)
    if r.paths.shape[2] != T:
        raise ValueError(f"the paths have {r.paths.shape[2]} positions, T = {T}")
    score = _PositionalPathScore.apply(lat, theta, pos_scores, arc_scores, r.paths, r.arcs, T)
    # (log Z_T without pos_scores: a table of zeros adds +0.0 to every label score)
    table = pos_scores if pos_scores is not None else torch.zeros((T, lat.vocab), dtype=torch.float32, device=lat.device)
    logz = ops.positional_log_z(lat, theta, table, arc_scores)
    ok = torch.arange(score.shape[1], device=score.device)[None, :] < r.n_paths[:, None]
    return torch.where(ok, score - logz[:, None], torch.full_like(score, float("-inf")))


def log_prob(lat: LatticeBatch, theta: torch.Tensor, r: SworResult, arc_scores: Optional[torch.Tensor] = None) -> torch.Tensor:
    """log p [B, k] float32 of the drawn paths, the numbers of ``r.logp``, differentiable in ``theta`` and ``arc_scores``:
    the path's score minus ``ops.log_z``, so the gradient is the path's label / arc counts minus the posteriors.  What a
    score-function gradient over the drawn set needs.  -inf beyond ``n_paths`` (no gradient there)."""
    if r.arcs is None:
        raise ValueError("log_prob needs the paths' arcs: sample(..., want_arcs=True)")
    score = _PathScore.apply(lat, theta, arc_scores, r.paths, r.arcs)
    logz = ops.log_z(lat, theta, arc_scores)
    ok = torch.arange(score.shape[1], device=score.device)[None, :] < r.n_paths[:, None]
    return torch.where(ok, score - logz[:, None], torch.full_like(score, float("-inf")))

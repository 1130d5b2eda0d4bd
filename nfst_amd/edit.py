"""Unit-cost edit distance between the rows of path sets: the wrappers of ``nfst_edit_distance`` (include/nfst_hip.h;
DESIGN.md sections 2 and 4.17).  ``ops.edit_distance`` and ``ops.pairwise_edit_distance`` are these functions; minimum-
Bayes-risk selection on top of them is in ``decoders``.  ``lattice_edit_distance`` (``nfst_lattice_edit``) is the distance between a
reference string and a whole lattice, with the oracle path.  There is no CPU implementation.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

EDIT_MAX_LEN = 1024  # NFST_EDIT_MAX_LEN of include/nfst_hip.h: the longest row of a path set


def _edit_side(x: torch.Tensor, lengths: torch.Tensor, name: str) -> tuple:
    """``(rows [B, K, L] int32 contiguous, lengths [B, K] int32 contiguous, the side was 2-D)`` of one side of
    ``edit_distance``; an empty last dimension gets one column that no length reaches."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3) or x.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name} must be an int32 or int64 tensor [B, K, L] or [B, L]")
    flat = x.dim() == 2
    if flat:
        x = x[:, None, :]
    if not isinstance(lengths, torch.Tensor) or lengths.device != x.device:
        raise ValueError(f"{name}_lengths must be a tensor on {name}'s device")
    if lengths.dtype not in (torch.int32, torch.int64) or lengths.numel() != x.shape[0] * x.shape[1]:
        raise ValueError(f"{name}_lengths must hold one integer per row of {name}")
    if x.shape[2] == 0:
        x = x.new_zeros((x.shape[0], x.shape[1], 1))
    return x.to(torch.int32).contiguous(), lengths.reshape(x.shape[:2]).to(torch.int32).contiguous(), flat


def edit_distance(a: torch.Tensor, a_lengths: torch.Tensor, b: torch.Tensor, b_lengths: torch.Tensor) -> torch.Tensor:
    """Unit-cost edit distances (Levenshtein) int32 [B, Ka, Kb] between the rows of two path sets, one launch of
    ``nfst_edit_distance``: entry [s, i, j] is the distance of ``a[s, i, :a_lengths[s, i]]`` and ``b[s, j,
    :b_lengths[s, j]]``.  ``a`` is [B, Ka, La] or [B, La] and ``b`` [B, Kb, Lb] or [B, Lb], int32 or int64 (the
    reference's LongTensor samples; cast to int32); a 2-D side counts as K = 1 and its axis is squeezed from the result.
    Nothing beyond a row's length is read, so the paths of ``k_best``, ``sample_paths`` or ``swor.sample`` go in with
    their pads, and an entry beyond ``n_paths`` (length 0) is at distance ``len`` from everything.  A row may be
    ``EDIT_MAX_LEN`` long.  A length outside [0, L] raises ``NfstError`` (NFST_ERR_LENGTH) after the launch."""
    if not isinstance(a, torch.Tensor) or a.device.type != "cuda":
        raise RuntimeError("nfst_amd: edit_distance runs on the MI355X only (no CPU fallback)")
    if not isinstance(b, torch.Tensor) or b.device != a.device:
        raise ValueError("a and b must be on the same device")
    a, al, a_flat = _edit_side(a, a_lengths, "a")
    b, bl, b_flat = _edit_side(b, b_lengths, "b")
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"a holds {a.shape[0]} sets and b {b.shape[0]}")
    out = _edit_launch(a, al, b, bl, 0)
    if a_flat:
        out = out.squeeze(1)
    return out.squeeze(-1) if b_flat else out


def pairwise_edit_distance(paths: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
    """The edit distances int32 [B, K, K] between the rows of every set of ``paths`` [B, K, L]: ``edit_distance(paths,
    lengths, paths, lengths)`` bit for bit at half the work (``nfst_edit_distance`` in symmetric mode computes i < j and
    writes both halves; the diagonal is 0).  The table ``decoders.mbr_select`` takes."""
    if not isinstance(paths, torch.Tensor) or paths.device.type != "cuda":
        raise RuntimeError("nfst_amd: pairwise_edit_distance runs on the MI355X only (no CPU fallback)")
    if paths.dim() != 3:
        raise ValueError("paths must be [B, K, L]")
    a, al, _ = _edit_side(paths, lengths, "paths")
    return _edit_launch(a, al, a, al, 1)


def _edit_launch(a, al, b, bl, symmetric: int) -> torch.Tensor:
    from .ops import _call, _raise_status  # (ops re-exports this module's functions: it is imported here, not at the top)

    B, Ka, La = a.shape
    Kb, Lb = b.shape[1], b.shape[2]
    out = torch.empty((B, Ka, Kb), dtype=torch.int32, device=a.device)
    if out.numel() == 0:
        return out
    status = torch.zeros(1, dtype=torch.int32, device=a.device)
    _call("nfst_edit_distance", None, a, al, Ka, La, b, bl, Kb, Lb, B, symmetric, out, status)  # (L > EDIT_MAX_LEN: NFST_ERR_LIMIT)
    _raise_status(status, "nfst_edit_distance")  # a length outside its row
    return out


class LatticeEditResult(NamedTuple):
    distance: torch.Tensor  # [B] int32: the least edit distance of a path to the reference; -1 without a path
    score: Optional[torch.Tensor]  # [B] float32: the oracle path's score (-inf without a path); None without theta
    paths: torch.Tensor  # [B, max_len] int32 labels (bos .. eos), pad-terminated
    path_arcs: torch.Tensor  # [B, max_len] int32 canonical arc ids, -1 padded
    align: torch.Tensor  # [B, max_len] int32: the reference position an arc was matched or substituted with, -1: insertion
    lengths: torch.Tensor  # [B] int32 arcs of the oracle path
    counts: torch.Tensor  # [B, 3] int32 (substitutions, insertions, deletions): they sum to distance


def _lattice_edit_terms(lat, ref, ref_lengths, theta=None, arc_scores=None, max_len=None, pad: int = 0) -> LatticeEditResult:
    """One launch of ``nfst_lattice_edit`` (no autograd); see ``lattice_edit_distance``."""
    from .ops import _call, _max_len, _need_gpu, _path_outputs, _raise_status, _scores, _workspace

    _need_gpu(lat)
    B = lat.n_lattices
    if not isinstance(ref, torch.Tensor) or ref.dim() != 2 or ref.shape[0] != B or ref.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"ref must be an int32 or int64 tensor [{B}, R]")
    if not isinstance(ref_lengths, torch.Tensor) or ref_lengths.dtype not in (torch.int32, torch.int64) or ref_lengths.numel() != B:
        raise ValueError("ref_lengths must hold one integer per lattice")
    if theta is None and arc_scores is not None:
        raise ValueError("arc_scores need theta")
    if ref.shape[1] == 0:
        ref = ref.new_zeros((B, 1))  # (one column that no valid length reaches)
    ref = ref.to(device=lat.device, dtype=torch.int32).contiguous()
    ref_lengths = ref_lengths.reshape(B).to(device=lat.device, dtype=torch.int32).contiguous()
    R = ref.shape[1]
    sc, keep = _scores(lat, theta, arc_scores) if theta is not None else (None, None)
    max_len = _max_len(lat, max_len)
    best, paths, arcs, lens, _, _ = _path_outputs(lat, (B,), max_len, best=theta is not None)
    dev = lat.device
    distance = torch.empty(B, dtype=torch.int32, device=dev)
    align = torch.empty((B, max_len), dtype=torch.int32, device=dev)
    counts = torch.empty((B, 3), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace(lat, "nfst_lattice_edit_ws_bytes", R)  # (R > EDIT_MAX_LEN: NFST_ERR_LIMIT)
    _call("nfst_lattice_edit", lat, sc, ref, ref_lengths, R, ws, ws_bytes, distance, best, paths, arcs, align, lens, counts,
          int(max_len), int(pad), status)
    _raise_status(status, "nfst_lattice_edit")  # a reference length outside its row, or an oracle path longer than max_len
    return LatticeEditResult(distance, best, paths, arcs, align, lens, counts)


class _LatticeEdit(torch.autograd.Function):
    """score[b] = the sum of the scores of the oracle path's arcs: the gradients of ``_KBest`` for one path per lattice."""

    @staticmethod
    def forward(ctx, lat, ref, ref_lengths, theta, arc_scores, max_len, pad):
        from .ops import _det

        r = _lattice_edit_terms(lat, ref, ref_lengths, theta.detach(), _det(arc_scores), max_len, pad)
        ctx.lat = lat
        ctx.like = (theta, arc_scores)
        ctx.save_for_backward(r.path_arcs)
        ctx.mark_non_differentiable(r.distance, r.paths, r.path_arcs, r.align, r.lengths, r.counts)
        return r.score, r.distance, r.paths, r.path_arcs, r.align, r.lengths, r.counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *_):
        from .ops import _path_score_grads

        (arcs,) = ctx.saved_tensors
        nt, na = ctx.needs_input_grad[3:5]
        theta, arc_scores = ctx.like
        d_theta, d_arc, _ = _path_score_grads(ctx.lat, arcs[:, None, :], g[:, None], theta if nt else None, arc_scores if na else None)
        return None, None, None, d_theta, d_arc, None, None


def lattice_edit_distance(lat, ref: torch.Tensor, ref_lengths: torch.Tensor, theta=None, arc_scores=None,
                          max_len: Optional[int] = None, pad: int = 0) -> LatticeEditResult:
    """The least unit-cost edit distance between ``ref[b, :ref_lengths[b]]`` and any path of lattice b, with the path
    that attains it: the oracle path (``nfst_lattice_edit``, DESIGN.md sections 2 and 4.18), exact for any number of
    paths.  ``ref`` is [B, R] int32 or int64, R <= ``EDIT_MAX_LEN``; nothing beyond a row's length is read.  Among the
    paths at the least distance the one of the greatest score under ``theta`` [V] or [B, V] and ``arc_scores``
    [total_arcs] wins (``k_best``'s float32 score; paths of score -inf do not count); without ``theta`` every path counts,
    ties go to the smaller label, and ``score`` is None.  ``align`` gives for every arc of the path the reference
    position it was matched or substituted with (-1: an insertion) and ``counts`` the substitutions, insertions and
    deletions.  A lattice without a path gets distance -1, score -inf and length 0.  ``max_len`` defaults to the longest
    path + 1.  A length outside [0, R] or a path longer than ``max_len`` raises ``NfstError`` (NFST_ERR_LENGTH) after
    the launch.  ``score`` is differentiable in ``theta`` and ``arc_scores``: the gradient counts the oracle path's
    labels / marks its arcs."""
    if theta is None:
        return _lattice_edit_terms(lat, ref, ref_lengths, None, arc_scores, max_len, pad)
    if not isinstance(theta, torch.Tensor):
        theta = torch.as_tensor(theta, dtype=torch.float32)
    score, *rest = _LatticeEdit.apply(lat, ref, ref_lengths, theta, arc_scores, max_len, pad)
    return LatticeEditResult(rest[0], score, *rest[1:])

"""Unit-cost edit distance between the rows of path sets: the wrappers of ``nfst_edit_distance`` (include/nfst_hip.h;
DESIGN.md sections 2 and 4.17).  ``ops.edit_distance`` and ``ops.pairwise_edit_distance`` are these functions; minimum-
Bayes-risk selection on top of them is in ``decoders``.  There is no CPU implementation.
"""
from __future__ import annotations

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

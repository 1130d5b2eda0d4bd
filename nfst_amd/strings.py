"""Output strings: the wrappers of ``nfst_merge_paths``, ``nfst_string_logprob``, ``nfst_string_logprob_grad``,
``nfst_string_prefix`` and ``nfst_string_next`` (include/nfst_hip.h; DESIGN.md sections 2 and 4.20 to 4.23).  The path-side ops answer in mark paths; the string of a path is its projection onto the output tape,
given as ``keep`` (a set of labels: the path's labels that belong to it, ``WideDFA.projected_sequence``'s meaning) or as
``marker`` (the labels that directly follow an arc labelled ``marker``, ``WideDFA.marked_sequence``'s meaning).
``ops.merge_paths``, ``ops.string_log_prob``, ``ops.string_arc_posteriors``, ``ops.string_prefix_log_prob`` and
``ops.string_next_log_probs`` are these functions; ``decoders.decode_strings`` puts the first two together and
``decoders.prefix_search`` searches with the last.  ``ops.string_viterbi`` and ``ops.string_sample_paths``
(``nfst_string_viterbi``, ``nfst_string_sample``; section 4.24) hand back the alignments of given strings, the best one and
exact draws, and ``ops.string_alignment_log_prob`` scores given alignments with a gradient.
There is no CPU implementation.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .edit import _edit_side

MERGE_MAX_K = 1024  # nfst_merge_paths: the rows of one set


class StringSet(NamedTuple):
    strings: torch.Tensor      # [B, K, L] int32: one row per distinct string, pad-filled
    lengths: torch.Tensor      # [B, K] int32 (0 beyond n_strings)
    log_weights: torch.Tensor  # [B, K] float64: the logsumexp of the members' weights, descending (-inf beyond n_strings)
    n_strings: torch.Tensor    # [B] int32 distinct strings
    group: torch.Tensor        # [B, K] int32: the entry that input row k went to (-1: an invalid row)
    first: torch.Tensor        # [B, K] int32: per entry the lowest input row among its members of greatest weight (-1 beyond n_strings)


class StringScores(NamedTuple):
    log_num: torch.Tensor   # [B, M] float64: log of the summed weight of the paths that spell the string (-inf: none does)
    logz: torch.Tensor      # [B] float64: the same over all paths
    log_prob: torch.Tensor  # [B, M] float64 = log_num - logz


class _StringScoresWithOffsets(StringScores):
    """``StringScores`` of a call with ``want_arc_grad=True``: ``arc_offsets`` is the float64 zero leaf [total_arcs] whose
    ``.grad`` receives the gradient of the arcs' scores."""


def _tape(keep, marker, vocab: Optional[int], device, need_one: bool) -> tuple:
    """``(keep mask [vocab] uint8 on the device or None, marker or -1, vocab)`` of the two ways to give the tape."""
    if keep is not None and marker is not None:
        raise ValueError("give keep or marker, not both")
    if keep is None and marker is None:
        if need_one:
            raise ValueError("give keep (a set of labels) or marker (a label)")
        return None, -1, 0
    labels = np.asarray([marker] if keep is None else sorted(set(int(x) for x in keep)), np.int64).reshape(-1)
    if vocab is None:
        vocab = int(labels.max()) + 1 if labels.size else 1
    if vocab < 1 or (labels.size and (labels.min() < 0 or labels.max() >= vocab)):
        raise ValueError(f"the labels of keep / marker must lie in 0 .. {vocab - 1}")
    if keep is None:
        return None, int(marker), int(vocab)
    mask = np.zeros(vocab, np.uint8)
    mask[labels] = 1
    return torch.from_numpy(mask).to(device), -1, int(vocab)


def _merge_launch(paths, lengths, logw, n_paths, keep_mask, marker: int, vocab: int, pad: int, hash_bits: int = 64):
    """One launch of ``nfst_merge_paths`` on marshalled inputs: ``(StringSet, status word on the device)``."""
    from .ops import _call

    B, K, L = paths.shape
    dev, i32 = paths.device, torch.int32
    strings = torch.empty((B, K, L), dtype=i32, device=dev)
    out_len = torch.empty((B, K), dtype=i32, device=dev)
    out_w = torch.empty((B, K), dtype=torch.float64, device=dev)
    n_strings = torch.zeros(B, dtype=i32, device=dev)
    group = torch.empty((B, K), dtype=i32, device=dev)
    first = torch.empty((B, K), dtype=i32, device=dev)
    status = torch.zeros(1, dtype=i32, device=dev)
    scratch = torch.empty((B, K, L), dtype=i32, device=dev)
    _call("nfst_merge_paths", None, paths, lengths, logw, n_paths, B, K, L, keep_mask, vocab, marker, hash_bits, int(pad), scratch,
          strings, out_len, out_w, n_strings, group, first, status)  # (K > MERGE_MAX_K, L > EDIT_MAX_LEN: NFST_ERR_LIMIT)
    return StringSet(strings, out_len, out_w, n_strings, group, first), status


class _MergedWeight(torch.autograd.Function):
    """merged[b, g] = logsumexp of the weights of group g's members: d merged[g] / d w[k] = exp(w[k] - merged[g]) for the
    members k of g, from ``group``."""

    @staticmethod
    def forward(ctx, log_weights, merged, group):
        ctx.save_for_backward(log_weights, merged, group)
        return merged.clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        w, merged, group = ctx.saved_tensors
        ok = group >= 0
        idx = group.clamp(min=0).to(torch.int64)
        share = torch.exp(w.to(torch.float64) - merged.gather(1, idx))
        grad = torch.where(ok, share * g.gather(1, idx), torch.zeros_like(share))
        return grad.to(w.dtype), None, None


def merge_paths(paths: torch.Tensor, lengths: torch.Tensor, log_weights: torch.Tensor, n_paths: Optional[torch.Tensor] = None, *,
                keep=None, marker: Optional[int] = None, vocab: Optional[int] = None, pad: int = 0) -> StringSet:
    """The rows of every path set merged by the string they spell ("crunching", ``nfst_merge_paths``): ``paths``
    [B, K, L] int32 or int64 with ``lengths`` [B, K], as ``k_best``, ``swor.sample`` or ``sample_paths`` return them, and
    ``log_weights`` [B, K] float32 or float64 (taken as float64).  Row k counts when k < ``n_paths[b]`` (always without
    ``n_paths``) and its weight is neither -inf nor NaN; only ``paths[b, k, :lengths[b, k]]`` is read.  The string of a
    row is its projection onto the tape ``keep`` or ``marker`` (module docstring; ``vocab`` bounds their labels and
    defaults to the largest of them + 1); with neither it is the row itself, and the op merges plain duplicates.  The
    result has one entry per distinct string, its weight the float64 logsumexp of its members' weights (summed in
    ascending row order around their maximum), ordered by that weight, descending, ties by the lowest member row; the same
    bits at every launch.  K <= 1024, L <= ``EDIT_MAX_LEN``.  A length outside [0, L] raises ``NfstError``
    (NFST_ERR_LENGTH) after the launch.  The weights carry the gradient into ``log_weights``."""
    from .ops import _raise_status

    if not isinstance(paths, torch.Tensor) or paths.device.type != "cuda":
        raise RuntimeError("nfst_amd: merge_paths runs on the MI355X only (no CPU fallback)")
    if paths.dim() != 3:
        raise ValueError("paths must be [B, K, L]")
    rows, lens, _ = _edit_side(paths, lengths, "paths")
    B, K, L = rows.shape
    if not isinstance(log_weights, torch.Tensor) or log_weights.device != rows.device or tuple(log_weights.shape) != (B, K) \
            or log_weights.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"log_weights must be a float32 or float64 tensor [{B}, {K}] on paths' device")
    if n_paths is not None:
        if not isinstance(n_paths, torch.Tensor) or n_paths.numel() != B or n_paths.dtype not in (torch.int32, torch.int64):
            raise ValueError("n_paths must hold one integer per set")
        n_paths = n_paths.reshape(B).to(device=rows.device, dtype=torch.int32).contiguous()
    keep_mask, mk, V = _tape(keep, marker, vocab, rows.device, need_one=False)
    logw = log_weights.detach().to(torch.float64).contiguous()
    out, status = _merge_launch(rows, lens, logw, n_paths, keep_mask, mk, V, pad)
    if B * K:
        _raise_status(status, "nfst_merge_paths")  # a length outside its row
    if log_weights.requires_grad:
        out = out._replace(log_weights=_MergedWeight.apply(log_weights, out.log_weights, out.group))
    return out


class _Candidates(NamedTuple):
    """The marshalled side of one ``string_log_prob`` call: what both entry points take besides the scores."""
    lat: object
    rows: torch.Tensor       # [B, M, N] int32
    lens: torch.Tensor       # [B, M] int32
    keep_mask: Optional[torch.Tensor]
    marker: int
    step: int                # candidates per slice (0: there are none)

    def slices(self):
        M = self.rows.shape[1]
        return [(m0, min(M, m0 + self.step)) for m0 in range(0, max(M, 1), max(self.step, 1))]

    def workspace(self, query: str) -> torch.Tensor:
        """Room for the largest slice as the library's ``query`` sizes it"""
        n = int(getattr(_lib.lib, query)(C.byref(self.lat.c_struct()), self.step, self.rows.shape[2], int(self.marker >= 0)))
        if n < 0:
            _lib.check(n, query)
        return torch.empty(max(n, 16), dtype=torch.uint8, device=self.lat.device)


def _candidates(lat, strings, lengths, keep, marker, max_workspace_bytes: int, query: str = "nfst_string_logprob_ws_bytes") -> _Candidates:
    """Checks and marshals the candidates and the tape, and cuts the candidates into slices whose workspace, as the
    library's ``query`` sizes it (the forward's by default), stays under ``max_workspace_bytes``."""
    from .ops import _need_gpu

    _need_gpu(lat)
    B = lat.n_lattices
    if not isinstance(strings, torch.Tensor) or strings.dim() != 3 or strings.shape[0] != B:
        raise ValueError(f"strings must be an int32 or int64 tensor [{B}, M, N]")
    rows, lens, _ = _edit_side(strings.to(lat.device), lengths.to(lat.device) if isinstance(lengths, torch.Tensor) else lengths, "strings")
    M, N = rows.shape[1], rows.shape[2]
    keep_mask, mk, _ = _tape(keep, marker, lat.vocab, lat.device, need_one=True)
    bs = C.byref(lat.c_struct())

    def ws_bytes(m):
        n = int(getattr(_lib.lib, query)(bs, m, N, int(mk >= 0)))
        if n < 0:
            _lib.check(n, query)  # (N > EDIT_MAX_LEN: NFST_ERR_LIMIT)
        return n

    fixed = ws_bytes(0)
    per = max(ws_bytes(1) - fixed, 1)
    if fixed + per > max_workspace_bytes and M > 0:
        raise ValueError(f"one candidate needs a workspace of {fixed + per} bytes, max_workspace_bytes is {max_workspace_bytes}")
    step = max(1, min(M, (max_workspace_bytes - fixed) // per)) if M else 0
    return _Candidates(lat, rows, lens, keep_mask, mk, step)


def _weights_launches(c: _Candidates, sc) -> tuple:
    """``nfst_string_logprob`` slice by slice: ``(log_num [B, M], logz [B], status word on the device)``"""
    from .ops import _call

    lat, dev = c.lat, c.lat.device
    B, M, N = c.rows.shape
    log_num = torch.empty((B, M), dtype=torch.float64, device=dev)
    logz = torch.empty(B, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = c.workspace("nfst_string_logprob_ws_bytes")
    for m0, m1 in c.slices():
        part_rows = c.rows[:, m0:m1].contiguous()
        part_lens = c.lens[:, m0:m1].contiguous()
        part_num = log_num if (m0, m1) == (0, M) else torch.empty((B, m1 - m0), dtype=torch.float64, device=dev)
        _call("nfst_string_logprob", lat, sc, part_rows, part_lens, m1 - m0, N, c.keep_mask, c.marker, ws, ws.numel(), part_num, logz, status)
        if part_num is not log_num:
            log_num[:, m0:m1] = part_num
    return log_num, logz, status


def _grad_launches(c: _Candidates, sc, g_num: torch.Tensor, g_z: torch.Tensor) -> tuple:
    """``nfst_string_logprob_grad`` over the forward's slices in ascending order, the first with ``accumulate=0`` and the
    rest with ``accumulate=1`` (the bits of one launch): ``(grad_arc [total_arcs] float64, status word on the device)``.
    The workspace is about twice the forward's."""
    from .ops import _call

    lat, dev = c.lat, c.lat.device
    B, M, N = c.rows.shape
    g_num = g_num.to(device=dev, dtype=torch.float64)
    g_z = g_z.to(device=dev, dtype=torch.float64).contiguous()
    grad_arc = torch.zeros(lat.total_arcs, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = c.workspace("nfst_string_logprob_grad_ws_bytes")
    for i, (m0, m1) in enumerate(c.slices()):
        _call("nfst_string_logprob_grad", lat, sc, c.rows[:, m0:m1].contiguous(), c.lens[:, m0:m1].contiguous(), m1 - m0, N, c.keep_mask,
              c.marker, g_num[:, m0:m1].contiguous(), g_z, int(i > 0), ws, ws.numel(), grad_arc, status)
    return grad_arc, status


def _label_sums(lat, grad_arc: torch.Tensor, theta: torch.Tensor) -> torch.Tensor:
    """The gradient of ``theta`` ([V], or [B, V] per lattice) from that of the arcs' scores: summed per label, in
    float64.  ``bincount`` and not ``index_add_``: millions of arcs land on a few hundred labels, and ``index_add_`` sends
    every one of them to global memory as a float64 atomic (270 ms on 5.1 M arcs and 256 labels)."""
    lab = lat.arc_label.to(torch.int64)
    if theta.dim() == 2:
        n_arcs = torch.as_tensor(lat.n_arcs.astype("int64"), device=grad_arc.device)
        lab = lab + torch.repeat_interleave(torch.arange(lat.n_lattices, device=grad_arc.device), n_arcs, output_size=lab.numel()) * lat.vocab
    out = torch.bincount(lab, weights=grad_arc, minlength=theta.numel())
    return out.view(theta.shape).to(dtype=theta.dtype, device=theta.device)


class _StringWeights(torch.autograd.Function):
    """``(log_num, logz)`` of ``nfst_string_logprob`` with the gradient of ``nfst_string_logprob_grad``: d log_num[b, m] /
    d score = the arc's posterior among the paths that spell candidate m, d logz[b] / d score = its posterior among all
    paths.  The backward pass sweeps G again: nothing but the inputs survives between the two."""

    @staticmethod
    def forward(ctx, c, theta, arc_scores):
        from .ops import _det, _raise_status, _scores

        sc, alive = _scores(c.lat, theta.detach(), _det(arc_scores))
        log_num, logz, status = _weights_launches(c, sc)
        _raise_status(status, "nfst_string_logprob")  # a candidate's length outside its row
        del alive
        ctx.c = c
        ctx.save_for_backward(theta, arc_scores)
        return log_num, logz

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_num, g_z):
        from .ops import _det, _scores

        c = ctx.c
        theta, arc_scores = ctx.saved_tensors
        sc, alive = _scores(c.lat, theta.detach(), _det(arc_scores))
        grad_arc, _ = _grad_launches(c, sc, g_num, g_z)  # (the forward has raised on a bad length)
        del alive
        g_theta = _label_sums(c.lat, grad_arc, theta) if ctx.needs_input_grad[1] else None
        g_arc = grad_arc.to(dtype=arc_scores.dtype, device=arc_scores.device).view(arc_scores.shape) if ctx.needs_input_grad[2] else None
        return None, g_theta, g_arc


def string_arc_posteriors(lat, theta, strings: torch.Tensor, lengths: torch.Tensor, *, keep=None, marker: Optional[int] = None,
                          arc_scores=None) -> torch.Tensor:
    """p(arc | x, y) float64 [total_arcs] in canonical arc order, y = ``strings[b, 0, :lengths[b, 0]]`` the one candidate
    of lattice b (``strings`` [B, 1, N]): the share of the weight of the paths that spell y which passes through the arc
    -- the alignment posteriors given the string (``nfst_string_logprob_grad`` with g_num = 1 and g_z = 0, the gradient
    of ``string_log_prob(...).log_num`` in the arc's score).  The out-arcs of state 0 add up to 1; all arcs of a lattice
    that has no path for its y get 0.  A length outside [0, N] raises ``NfstError`` (NFST_ERR_LENGTH) after the launch."""
    from .ops import _raise_status, _scores

    c = _candidates(lat, strings, lengths, keep, marker, 1 << 62)
    if c.rows.shape[1] != 1:
        raise ValueError(f"strings must hold one candidate per lattice, [{lat.n_lattices}, 1, N]")
    if not isinstance(theta, torch.Tensor):
        theta = torch.as_tensor(theta, dtype=torch.float32)
    sc, alive = _scores(lat, theta.detach(), None if arc_scores is None else arc_scores.detach())
    B = lat.n_lattices
    grad_arc, status = _grad_launches(c, sc, torch.ones((B, 1), dtype=torch.float64), torch.zeros(B, dtype=torch.float64))
    _raise_status(status, "nfst_string_logprob_grad")
    del alive
    return grad_arc


def string_log_prob(lat, theta, strings: torch.Tensor, lengths: torch.Tensor, *, keep=None, marker: Optional[int] = None,
                    arc_scores=None, max_workspace_bytes: int = 1 << 30, want_arc_grad: bool = False) -> StringScores:
    """Exact log p(y | x) of candidate strings from the lattice alone (``nfst_string_logprob``): for lattice b and
    candidate m, y = ``strings[b, m, :lengths[b, m]]`` (``strings`` [B, M, N] int32 or int64, N <= ``EDIT_MAX_LEN``),
    ``log_num`` is the log of the summed weight exp(score) of the paths whose projection onto the tape ``keep`` or
    ``marker`` is y, ``logz`` that of all paths and ``log_prob`` their difference, all float64; a string that no path
    spells gets -inf, which is no error.  Scores are those of the other path-side ops (``theta`` [V] or [B, V],
    ``arc_scores`` [total_arcs], the table's weights), acceptance that of ``WideDFA.projected_sequence`` /
    ``marked_sequence``; unlike ``ops.constraint_log_prob`` on those automata, nothing is intersected or packed, the
    arithmetic is float64 and no product has to fit ``NFST_MAX_ROWS``.  The candidates are swept in slices whose workspace
    stays under ``max_workspace_bytes`` (ValueError if one candidate does not fit); the bits do not depend on the
    slicing.  A length outside [0, N] raises ``NfstError`` (NFST_ERR_LENGTH) after the launch.  All three results carry
    exact float64 gradients (``nfst_string_logprob_grad``, once differentiable) into ``theta`` and ``arc_scores`` when
    either requires grad: the gradient of ``arc_scores`` is that of the arcs' scores cast to its dtype, the gradient of
    ``theta`` its sum per label; a candidate of probability 0 passes back zeros through ``log_prob``.  The backward pass
    sweeps the forward's slices again, in a workspace about twice as large.  ``want_arc_grad=True`` asks for the float64
    gradient of every arc's score without a cast and whether or not ``arc_scores`` was given: the result (still a
    ``StringScores``) has one more attribute, ``arc_offsets``, a float64 leaf of zeros [total_arcs] that was added to the
    arcs' scores, and ``arc_offsets.grad`` holds that gradient after a backward pass; the values do not change."""
    from .ops import _raise_status, _scores

    c = _candidates(lat, strings, lengths, keep, marker, max_workspace_bytes)
    if not isinstance(theta, torch.Tensor):
        theta = torch.as_tensor(theta, dtype=torch.float32)
    arc_offsets = None
    if want_arc_grad:
        arc_offsets = torch.zeros(lat.total_arcs, dtype=torch.float64, device=lat.device, requires_grad=True)
        arc_scores = arc_offsets if arc_scores is None else arc_scores.to(device=lat.device, dtype=torch.float64) + arc_offsets
    if torch.is_grad_enabled() and (theta.requires_grad or (isinstance(arc_scores, torch.Tensor) and arc_scores.requires_grad)):
        log_num, logz = _StringWeights.apply(c, theta, arc_scores)
    else:
        sc, alive = _scores(lat, theta.detach(), None if arc_scores is None else arc_scores.detach())
        log_num, logz, status = _weights_launches(c, sc)
        _raise_status(status, "nfst_string_logprob")  # a candidate's length outside its row
        del alive
    neg = torch.full_like(log_num, float("-inf"))
    out = StringScores(log_num, logz, torch.where(torch.isneginf(log_num), neg, log_num - logz[:, None]))
    if arc_offsets is not None:
        out = _StringScoresWithOffsets(*out)
        out.arc_offsets = arc_offsets
    return out


# ----------------------------------------------------------------------------- alignments
class StringAlignment(NamedTuple):
    score: torch.Tensor    # [B, M] float64: the score of the best path that spells the string (-inf: none does)
    paths: torch.Tensor    # [B, M, L] int32 labels, pad-terminated
    arcs: torch.Tensor     # [B, M, L] int32 canonical arc ids, -1 padded
    align: torch.Tensor    # [B, M, L] int32: the position of the string that the arc emitted, -1: none
    lengths: torch.Tensor  # [B, M] int32 arcs of the path


class StringSampleResult(NamedTuple):
    paths: torch.Tensor    # [B, M, K, L] int32 labels, pad-terminated
    arcs: torch.Tensor     # [B, M, K, L] int32 canonical arc ids, -1 padded
    align: torch.Tensor    # [B, M, K, L] int32: the position of the string that the arc emitted, -1: none
    lengths: torch.Tensor  # [B, M, K] int32
    score: torch.Tensor    # [B, M, K] float64: the sum of the path's arc scores (-inf: no path spells the string)
    logq: torch.Tensor     # [B, M, K] float64 = score - log_num: the draw's exact log p(path | x, y) (0 without a path)
    log_num: torch.Tensor  # [B, M] float64: ``string_log_prob``'s, bit for bit
    logz: torch.Tensor     # [B] float64: ``string_log_prob``'s, bit for bit


def _walk_outputs(dev, lead: tuple, L: int) -> tuple:
    """``(paths, arcs, align [*lead, L], lengths [*lead])`` int32, uninitialised"""
    i32 = torch.int32
    return (torch.empty((*lead, L), dtype=i32, device=dev), torch.empty((*lead, L), dtype=i32, device=dev),
            torch.empty((*lead, L), dtype=i32, device=dev), torch.empty(lead, dtype=i32, device=dev))


def _viterbi_launches(c: _Candidates, sc, max_len: int, pad: int) -> StringAlignment:
    """``nfst_string_viterbi`` slice by slice, then the status word (no autograd)"""
    from .ops import _call, _raise_status

    lat, dev = c.lat, c.lat.device
    B, M, N = c.rows.shape
    score = torch.empty((B, M), dtype=torch.float64, device=dev)
    outs = _walk_outputs(dev, (B, M), max_len)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = c.workspace("nfst_string_viterbi_ws_bytes") if M else None
    for m0, m1 in c.slices() if M else ():
        whole = (m0, m1) == (0, M)
        part = (score, *outs) if whole else (torch.empty((B, m1 - m0), dtype=torch.float64, device=dev), *_walk_outputs(dev, (B, m1 - m0), max_len))
        _call("nfst_string_viterbi", lat, sc, c.rows[:, m0:m1].contiguous(), c.lens[:, m0:m1].contiguous(), m1 - m0, N, c.keep_mask,
              c.marker, int(max_len), int(pad), ws, ws.numel(), part[0], part[1], part[2], part[3], part[4], status)
        if not whole:
            for o, q in zip((score, *outs), part):
                o[:, m0:m1] = q
    if B * M:
        _raise_status(status, "nfst_string_viterbi")  # a candidate's length outside its row, or a path longer than max_len
    return StringAlignment(score, *outs)


class _StringViterbi(torch.autograd.Function):
    """score[b, m] = the sum of the scores of the best path's arcs: the gradients of ``_LatticeEdit``, one path per candidate."""

    @staticmethod
    def forward(ctx, c, theta, arc_scores, max_len, pad):
        from .ops import _det, _scores

        sc, alive = _scores(c.lat, theta.detach(), _det(arc_scores))
        r = _viterbi_launches(c, sc, max_len, pad)
        del alive
        ctx.lat = c.lat
        ctx.like = (theta, arc_scores)
        ctx.save_for_backward(r.arcs)
        ctx.mark_non_differentiable(r.paths, r.arcs, r.align, r.lengths)
        return tuple(r)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *_):
        from .ops import _path_score_grads

        (arcs,) = ctx.saved_tensors
        nt, na = ctx.needs_input_grad[1:3]
        theta, arc_scores = ctx.like
        d_theta, d_arc, _ = _path_score_grads(ctx.lat, arcs, g, theta if nt else None, arc_scores if na else None)
        return None, d_theta, d_arc, None, None


def string_viterbi(lat, theta, strings: torch.Tensor, lengths: torch.Tensor, *, keep=None, marker: Optional[int] = None,
                   arc_scores=None, max_len: Optional[int] = None, pad: int = 0, max_workspace_bytes: int = 1 << 30) -> StringAlignment:
    """Forced alignment (``nfst_string_viterbi``; DESIGN.md sections 2 and 4.24): for lattice b and candidate m, the path
    of the greatest score among those whose projection onto the tape ``keep`` or ``marker`` is y = ``strings[b, m,
    :lengths[b, m]]``, from the lattice alone -- no product, float64, any number of paths.  Candidates, tape, scores,
    slicing under ``max_workspace_bytes`` and the length error are ``string_log_prob``'s.  ``score`` [B, M] float64 is
    that path's score, ``paths`` its labels (``pad``-terminated), ``arcs`` its canonical arc ids (-1 padded), ``align``
    the position of y that each arc emitted (-1: none) and ``lengths`` its arcs, all [B, M, max_len] / [B, M]; among
    paths of equal score the one that takes the earlier arc in canonical order at the first difference.  Every output is
    a pure function of the inputs: the same bits at every launch, packing and slicing.  A string that no path of finite
    score spells gets score -inf, length 0, ``pad`` labels and ``align`` -1, which is no error.  ``max_len`` defaults to
    the longest path + 1; a longer path, or a length outside [0, N], raises ``NfstError`` (NFST_ERR_LENGTH) after the
    launch.  ``score`` is differentiable in ``theta`` and ``arc_scores``: the gradient counts the path's labels / marks
    its arcs (float32, as ``lattice_edit_distance``'s); candidates of score -inf pass nothing back."""
    from .ops import _max_len, _scores

    c = _candidates(lat, strings, lengths, keep, marker, max_workspace_bytes, "nfst_string_viterbi_ws_bytes")
    if not isinstance(theta, torch.Tensor):
        theta = torch.as_tensor(theta, dtype=torch.float32)
    max_len = int(_max_len(lat, max_len))
    if max_len < 1:
        raise ValueError("max_len must be at least 1")
    if torch.is_grad_enabled() and (theta.requires_grad or (isinstance(arc_scores, torch.Tensor) and arc_scores.requires_grad)):
        return StringAlignment(*_StringViterbi.apply(c, theta, arc_scores, max_len, int(pad)))
    sc, alive = _scores(lat, theta.detach(), None if arc_scores is None else arc_scores.detach())
    out = _viterbi_launches(c, sc, max_len, int(pad))
    del alive
    return out


def string_sample_paths(lat, theta, strings: torch.Tensor, lengths: torch.Tensor, k: int, *, keep=None, marker: Optional[int] = None,
                        arc_scores=None, uniforms: Optional[torch.Tensor] = None, seed: int = 0, max_len: Optional[int] = None,
                        pad: int = 0, max_workspace_bytes: int = 1 << 30) -> StringSampleResult:
    """``k`` exact draws per lattice and candidate from p(path | x, y), proportional to exp(score) over the paths whose
    projection onto the tape is y = ``strings[b, m, :lengths[b, m]]`` (``nfst_string_sample``; DESIGN.md sections 2 and
    4.24): the proposal over the alignments of a given string, for M candidates at once from the one lattice.
    Candidates, tape, scores, slicing under ``max_workspace_bytes`` and the length error are ``string_log_prob``'s, and
    ``log_num`` / ``logz`` are its results, bit for bit.  Per draw: ``paths``, ``arcs``, ``align`` [B, M, k, max_len] and
    ``lengths`` [B, M, k] as ``string_viterbi``'s, ``score`` the float64 sum of the path's arc scores and ``logq`` =
    ``score - log_num``, the draw's exact log-probability.  ``uniforms`` [B, M, k, max_len] float32 in [0, 1) decide the
    walks (walk (b, m, j) reads its own row only; the rule is ``positional_sample_paths``'s); without them Philox4x32-10
    keyed by ``seed`` and the walk (b, m, j), whatever the slicing.  A string that no path spells gets length 0, ``pad``
    labels, score -inf and ``logq`` 0.  ``max_len`` defaults to the longest path + 1; a longer path raises ``NfstError``
    (NFST_ERR_LENGTH) after the launch.  Not differentiable (``string_alignment_log_prob`` scores given draws with a
    gradient)."""
    from .ops import _call, _check_k, _max_len, _raise_status, _scores

    _check_k(k, bounded=False)
    c = _candidates(lat, strings, lengths, keep, marker, max_workspace_bytes, "nfst_string_sample_ws_bytes")
    if not isinstance(theta, torch.Tensor):
        theta = torch.as_tensor(theta, dtype=torch.float32)
    max_len = int(_max_len(lat, max_len))
    if max_len < 1:
        raise ValueError("max_len must be at least 1")
    dev, f64 = lat.device, torch.float64
    B, M, N = c.rows.shape
    if uniforms is not None:
        if not isinstance(uniforms, torch.Tensor) or tuple(uniforms.shape) != (B, M, k, max_len):
            raise ValueError(f"uniforms must be a tensor of shape [{B}, {M}, {k}, {max_len}]")
        uniforms = uniforms.detach().to(device=dev, dtype=torch.float32).contiguous()
    sc, alive = _scores(lat, theta.detach(), None if arc_scores is None else arc_scores.detach())
    shapes = [((B, M), f64), ((B, M, k), f64), ((B, M, k), f64)]  # log_num, score, logq

    def outputs(m):
        return [torch.empty((B, m) + sh[2:], dtype=dt, device=dev) for sh, dt in shapes] + list(_walk_outputs(dev, (B, m, k), max_len))

    outs = outputs(M)
    logz = torch.empty(B, dtype=f64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    seed64 = C.c_uint64(seed & (2 ** 64 - 1))
    ws = c.workspace("nfst_string_sample_ws_bytes") if M else c.workspace("nfst_string_logprob_ws_bytes")
    if M == 0:  # no candidate: log Z alone
        _call("nfst_string_logprob", lat, sc, None, None, 0, N, c.keep_mask, c.marker, ws, ws.numel(), None, logz, status)
    for m0, m1 in c.slices() if M else ():
        whole = (m0, m1) == (0, M)
        part = outs if whole else outputs(m1 - m0)
        log_num, score, logq, paths, arcs, align, lens = part
        _call("nfst_string_sample", lat, sc, c.rows[:, m0:m1].contiguous(), c.lens[:, m0:m1].contiguous(), m1 - m0, N, c.keep_mask,
              c.marker, int(k), m0, None if uniforms is None else uniforms[:, m0:m1].contiguous(), seed64, max_len, int(pad), ws,
              ws.numel(), log_num, logz, score, logq, paths, arcs, align, lens, status)
        if not whole:
            for o, q in zip(outs, part):
                o[:, m0:m1] = q
    if B:
        _raise_status(status, "nfst_string_sample")  # a candidate's length outside its row, or a path longer than max_len
    del alive
    log_num, score, logq, paths, arcs, align, lens = outs
    return StringSampleResult(paths, arcs, align, lens, score, logq, log_num, logz)


def string_alignment_log_prob(lat, theta, strings: torch.Tensor, lengths: torch.Tensor, arcs: torch.Tensor, path_lengths: torch.Tensor, *,
                              keep=None, marker: Optional[int] = None, arc_scores=None) -> torch.Tensor:
    """log p(path | x, y) float64 [B, M, K] of given alignments, differentiable in ``theta`` and ``arc_scores``: the sum
    of the float64 scores (theta[label] + the table's weight + ``arc_scores``) of ``arcs[b, m, j, :path_lengths[b, m,
    j]]`` (canonical arc ids [B, M, K, L], as ``string_sample_paths`` returns them) less ``string_log_prob(...).log_num``
    of candidate m -- what a score-function estimator over drawn alignments needs, in the role of ``swor.log_prob``.  It
    equals the draws' ``logq`` up to the order of the sum.  Composed from ``string_log_prob`` and a gather: no kernel of
    its own.  An entry with ``path_lengths`` 0 under a string that no path spells is 0, as the draws' ``logq``; the
    caller answers for the paths spelling their strings."""
    from .ops import _need_gpu

    _need_gpu(lat)
    B = lat.n_lattices
    if not isinstance(arcs, torch.Tensor) or arcs.dim() != 4 or arcs.shape[0] != B or arcs.is_floating_point():
        raise ValueError(f"arcs must be an integer tensor [{B}, M, K, L]")
    _, M, K, L = arcs.shape
    if not isinstance(strings, torch.Tensor) or strings.dim() != 3 or strings.shape[1] != M:
        raise ValueError(f"strings must be [{B}, {M}, N]: one candidate per row of arcs")
    if not isinstance(path_lengths, torch.Tensor) or tuple(path_lengths.shape) != (B, M, K) or path_lengths.is_floating_point():
        raise ValueError(f"path_lengths must be an integer tensor [{B}, {M}, {K}]")
    if not isinstance(theta, torch.Tensor):
        theta = torch.as_tensor(theta, dtype=torch.float32)
    dev, f64 = lat.device, torch.float64
    log_num = string_log_prob(lat, theta, strings, lengths, keep=keep, marker=marker, arc_scores=arc_scores).log_num
    a = arcs.to(device=dev, dtype=torch.int64)
    on = (torch.arange(L, device=dev) < path_lengths.to(dev)[..., None]) & (a >= 0)
    idx = a.clamp(min=0)
    lab = lat.arc_label.to(torch.int64)[idx]
    th = theta.to(device=dev, dtype=f64)
    if th.dim() == 2:
        b_of = torch.arange(B, device=dev).view(B, 1, 1, 1).expand_as(lab)
        term = th[b_of, lab]
    else:
        term = th[lab]
    if lat.weighted:
        term = term + lat.arc_w.to(f64)[idx]
    if arc_scores is not None:
        a64 = arc_scores.to(device=dev, dtype=f64)  # (the kernels read float32; the gradient does not pass through the rounding)
        term = term + (a64 + (a64.detach().to(torch.float32).to(f64) - a64.detach()))[idx]
    score = torch.where(on, term, torch.zeros_like(term)).sum(dim=-1)
    has = torch.isfinite(log_num)[..., None]
    return torch.where(has, score - torch.where(has, log_num[..., None], torch.zeros_like(score)), score)


# ----------------------------------------------------------------------------- prefixes
class PrefixScores(NamedTuple):
    log_prefix: torch.Tensor  # [B, M] float64: log of the summed weight of the paths whose string starts with the prefix
    logz: torch.Tensor        # [B] float64: the same over all paths (``string_log_prob``'s, bit for bit)
    log_prob: torch.Tensor    # [B, M] float64 = log_prefix - logz


class NextSymbols(NamedTuple):
    next: torch.Tensor        # [B, M, V] float64: log_prefix of the prefix followed by label v (-inf: v is never on the tape)
    eos: torch.Tensor         # [B, M] float64: the log weight of the paths that spell exactly the prefix
    log_prefix: torch.Tensor  # [B, M] float64: the log-sum of eos and next
    logz: torch.Tensor        # [B] float64


def _prefix_launches(name: str, lat, theta, prefixes, lengths, keep, marker, arc_scores, max_workspace_bytes: int, n_out: int) -> tuple:
    """``nfst_string_prefix`` (``n_out`` = 1) or ``nfst_string_next`` (3) slice by slice: ``(outputs [B, M(, V)] ...,
    logz [B])`` after the status word has been read back."""
    from .ops import _call, _raise_status, _scores

    c = _candidates(lat, prefixes, lengths, keep, marker, max_workspace_bytes, name + "_ws_bytes")
    if not isinstance(theta, torch.Tensor):
        theta = torch.as_tensor(theta, dtype=torch.float32)
    sc, alive = _scores(lat, theta.detach(), None if arc_scores is None else arc_scores.detach())
    dev, f64 = lat.device, torch.float64
    B, M, N = c.rows.shape
    shapes = [(B, M)] if n_out == 1 else [(B, M, lat.vocab), (B, M), (B, M)]
    outs = [torch.empty(sh, dtype=f64, device=dev) for sh in shapes]
    logz = torch.empty(B, dtype=f64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if M == 0:  # no prefix: log Z alone, from the sweep that every slice shares
        ws = c.workspace("nfst_string_logprob_ws_bytes")
        _call("nfst_string_logprob", lat, sc, None, None, 0, N, c.keep_mask, c.marker, ws, ws.numel(), None, logz, status)
    else:
        ws = c.workspace(name + "_ws_bytes")
    for m0, m1 in c.slices() if M else ():
        whole = (m0, m1) == (0, M)
        part = outs if whole else [torch.empty((B, m1 - m0) + sh[2:], dtype=f64, device=dev) for sh in shapes]
        _call(name, lat, sc, c.rows[:, m0:m1].contiguous(), c.lens[:, m0:m1].contiguous(), m1 - m0, N, c.keep_mask, c.marker, ws,
              ws.numel(), *part, logz, status)
        if not whole:
            for o, q in zip(outs, part):
                o[:, m0:m1] = q
    _raise_status(status, name)  # a prefix's length outside its row
    del alive
    return (*outs, logz)


def string_prefix_log_prob(lat, theta, prefixes: torch.Tensor, lengths: torch.Tensor, *, keep=None, marker: Optional[int] = None,
                           arc_scores=None, max_workspace_bytes: int = 1 << 30) -> PrefixScores:
    """The exact probability that the output string starts with a prefix (``nfst_string_prefix``): for lattice b and
    y = ``prefixes[b, m, :lengths[b, m]]`` (``prefixes`` [B, M, N] int32 or int64, N <= ``EDIT_MAX_LEN``), ``log_prefix``
    is the log of the summed weight of the paths whose string on the tape ``keep`` or ``marker`` starts with y, ``logz``
    that of all paths (``string_log_prob``'s, bit for bit) and ``log_prob`` their difference, all float64; a prefix that
    no path spells gets -inf.  A path that ends on a marker with nothing behind it spells no string and counts under no
    prefix: in marker mode the empty prefix has ``log_prob`` = log(1 - those paths' share), in keep mode 0.  The value
    bounds log p of every string that starts with y from above.  Scores, slicing under ``max_workspace_bytes`` and the
    length error are ``string_log_prob``'s.  The results carry no gradient: gradients of prefix masses are out of scope."""
    log_prefix, logz = _prefix_launches("nfst_string_prefix", lat, theta, prefixes, lengths, keep, marker, arc_scores, max_workspace_bytes, 1)
    neg = torch.full_like(log_prefix, float("-inf"))
    return PrefixScores(log_prefix, logz, torch.where(torch.isneginf(log_prefix), neg, log_prefix - logz[:, None]))


def string_next_log_probs(lat, theta, prefixes: torch.Tensor, lengths: torch.Tensor, *, keep=None, marker: Optional[int] = None,
                          arc_scores=None, max_workspace_bytes: int = 1 << 30) -> NextSymbols:
    """The next-symbol masses of prefixes (``nfst_string_next``; arguments as ``string_prefix_log_prob``'s): ``next[b, m,
    v]`` is ``log_prefix`` of the prefix followed by label v, for every label of the vocabulary (-inf for a label that is
    never on the tape: one that ``keep`` does not hold), ``eos[b, m]`` the log weight of the paths that spell exactly the
    prefix (``string_log_prob``'s ``log_num``) and ``log_prefix`` the log-sum of ``eos`` and ``next``, so that
    exp(log_prefix) = exp(eos) + sum_v exp(next[v]); all float64 log weights, not normalised: subtract ``log_prefix`` for
    log p(v | y, x) and ``logz`` for probabilities.  The results carry no gradient: gradients of prefix masses are out
    of scope."""
    return NextSymbols(*_prefix_launches("nfst_string_next", lat, theta, prefixes, lengths, keep, marker, arc_scores, max_workspace_bytes, 3))


# ----------------------------------------------------------------------------- prefix states
STATE_MAX_M = 1024  # nfst_string_prefix_extend: the hypotheses of one state


class PrefixState(NamedTuple):
    cells: torch.Tensor    # opaque float64: one column of the prefix table per lattice row, plane and slot
    lengths: torch.Tensor  # [B, M] int32: the symbols of the slot's prefix, -1 for a dead slot


class PrefixContext:
    """What ``string_next_log_probs`` works out per call from the lattice and the scores alone, worked out once
    (``nfst_string_prefix_open``), and the prefix states that live on it: ``root`` makes the empty prefix, ``extend``
    appends one symbol to chosen parents in one sweep of one column -- O(arcs) per symbol whatever the prefix length --
    and ``next`` gives ``string_next_log_probs``'s results for a state's prefixes, bit for bit.  The caller keeps the
    tokens; a state only knows its lengths.  A decoder that fuses the lattice with an external scorer is this loop::

        ctx = ops.string_prefix_open(lat, theta, marker=4)
        state = ctx.root(k)
        for t in range(max_len):
            ns = ctx.next(state)                         # next [B, k, V], eos, log_prefix
            slot, label = choose(ns.next - ns.log_prefix[:, :, None] + external_scores)   # [B, k] each, -1: none
            state = ctx.extend(state, slot, label)

    The context is a snapshot of the scores: it must be opened again after the parameters change.  No gradient.
    A state is 8 * planes * M * total_rows bytes (planes = 2 with ``marker``), and a step holds two."""

    def __init__(self, lat, sc, alive, keep_mask, marker: int, ws: torch.Tensor, logz: torch.Tensor):
        self.lat, self.marker, self.keep_mask, self.ws, self.logz = lat, marker, keep_mask, ws, logz
        self._sc, self._alive = sc, alive  # (the nfst_scores struct points into the tensors of ``alive``)

    @property
    def planes(self) -> int:
        return 2 if self.marker >= 0 else 1

    def _cells(self, M: int) -> torch.Tensor:
        if isinstance(M, bool) or not isinstance(M, int) or M < 1:
            raise ValueError("a state holds M >= 1 hypotheses")
        n = int(_lib.lib.nfst_string_prefix_state_bytes(C.byref(self.lat.c_struct()), M, int(self.marker >= 0)))
        if n < 0:
            _lib.check(n, "nfst_string_prefix_state_bytes")  # (M > STATE_MAX_M: NFST_ERR_LIMIT)
        return torch.empty(max(n, 16) // 8, dtype=torch.float64, device=self.lat.device)

    def _extend(self, cells, M_in: int, parent: torch.Tensor, symbol: torch.Tensor) -> tuple:
        """One launch of ``nfst_string_prefix_extend``: ``(the children's cells, status word on the device)``"""
        from .ops import _call

        out = self._cells(parent.shape[1])
        status = torch.zeros(1, dtype=torch.int32, device=self.lat.device)
        _call("nfst_string_prefix_extend", self.lat, self._sc, self.keep_mask, self.marker, self.ws, self.ws.numel(), cells,
              0 if cells is None else cells.numel() * 8, M_in, parent, symbol, out, out.numel() * 8, parent.shape[1], status)
        return out, status

    def _slots(self, x, name: str, M_out=None) -> torch.Tensor:
        B = self.lat.n_lattices
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] != B or x.is_floating_point() or (M_out is not None and x.shape[1] != M_out):
            raise ValueError(f"{name} must be an integer tensor [{B}, M_out]")
        return x.to(device=self.lat.device, dtype=torch.int32).contiguous()

    def root(self, M: int = 1) -> PrefixState:
        """A state of ``M`` slots: slot 0 is the empty prefix, the other slots are dead."""
        B, dev = self.lat.n_lattices, self.lat.device
        parent = torch.full((B, M), -1, dtype=torch.int32, device=dev)
        parent[:, 0] = -2
        cells, _ = self._extend(None, 0, parent, torch.zeros_like(parent))
        lengths = torch.full((B, M), -1, dtype=torch.int32, device=dev)
        lengths[:, 0] = 0
        return PrefixState(cells, lengths)

    def extend(self, state: PrefixState, parent: torch.Tensor, symbol: torch.Tensor) -> PrefixState:
        """The state of the prefixes ``state[parent[b, m]] + (symbol[b, m],)`` (``parent`` and ``symbol`` [B, M_out]
        integers, M_out <= 1024; children are independent and may share a parent).  ``parent`` -1 makes a dead slot and
        -2 the empty prefix; so does a dead parent make a dead child.  A symbol that no path spells there is no error:
        the child's masses are -inf.  A ``parent`` outside [-2, M) or a ``symbol`` outside the vocabulary raises
        ``NfstError`` (NFST_ERR_INDEX) after the launch."""
        from .ops import _raise_status

        parent = self._slots(parent, "parent")
        symbol = self._slots(symbol, "symbol", parent.shape[1])
        M_in = state.lengths.shape[1]
        cells, status = self._extend(state.cells, M_in, parent, symbol)
        _raise_status(status, "nfst_string_prefix_extend")
        return PrefixState(cells, self._lengths(state.lengths, parent))

    @staticmethod
    def _lengths(lengths: torch.Tensor, parent: torch.Tensor) -> torch.Tensor:
        of = lengths.gather(1, parent.clamp(min=0).to(torch.int64))
        grown = torch.where((parent >= 0) & (of >= 0), of + 1, torch.full_like(of, -1))
        return torch.where(parent == -2, torch.zeros_like(of), grown)

    def next(self, state: PrefixState) -> NextSymbols:
        """``string_next_log_probs`` of the state's prefixes (``nfst_string_prefix_state_next``), bit for bit; a dead
        slot gets -inf everywhere.  ``logz`` is the context's."""
        from .ops import _call

        B, M = state.lengths.shape
        dev, f64 = self.lat.device, torch.float64
        nxt = torch.empty((B, M, self.lat.vocab), dtype=f64, device=dev)
        eos, pre = torch.empty((B, M), dtype=f64, device=dev), torch.empty((B, M), dtype=f64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _call("nfst_string_prefix_state_next", self.lat, self._sc, self.keep_mask, self.marker, self.ws, self.ws.numel(), state.cells,
              state.cells.numel() * 8, M, nxt, eos, pre, status)
        return NextSymbols(nxt, eos, pre, self.logz)

    def state_of(self, prefixes: torch.Tensor, lengths: torch.Tensor) -> PrefixState:
        """The state of given prefixes (``prefixes`` [B, M, N], ``lengths`` [B, M], as ``string_next_log_probs`` takes
        them; a negative length makes a dead slot): ``extend`` position by position, slot m from slot m -- the entry for
        a search that starts from a prompt.  O(arcs * longest prefix); no kernel of its own."""
        B, dev = self.lat.n_lattices, self.lat.device
        if not isinstance(prefixes, torch.Tensor) or prefixes.dim() != 3 or prefixes.shape[0] != B or prefixes.is_floating_point():
            raise ValueError(f"prefixes must be an integer tensor [{B}, M, N]")
        M, N = prefixes.shape[1], prefixes.shape[2]
        lens = self._slots(lengths, "lengths", M)
        rows = prefixes.to(device=dev, dtype=torch.int32)
        if bool((lens > N).any()):
            raise ValueError(f"a length exceeds the row stride {N}")
        own = torch.arange(M, dtype=torch.int32, device=dev).expand(B, M).contiguous()
        none = torch.full_like(own, -1)
        cells, _ = self._extend(None, 0, torch.where(lens >= 0, torch.full_like(own, -2), none), torch.zeros_like(own))
        state = PrefixState(cells, torch.where(lens >= 0, torch.zeros_like(lens), none))
        for t in range(int(lens.max()) if B * M else 0):
            grows = lens > t
            nxt = self.extend(state, torch.where(grows, own, none), rows[:, :, t].contiguous())
            if not bool(grows.all()):  # a slot whose prefix is complete keeps its column
                nxt = PrefixState(self._carry(state.cells, nxt.cells, grows), torch.where(grows, nxt.lengths, state.lengths))
            state = nxt
        return state

    def _carry(self, old: torch.Tensor, new: torch.Tensor, grows: torch.Tensor) -> torch.Tensor:
        """``new`` in the slots that grew [B, M] and ``old`` in the others, for two states of M slots"""
        lat, M = self.lat, grows.shape[1]
        lat_of_row = np.searchsorted(lat.row_off.astype(np.int64), np.arange(lat.total_rows), side="right") - 1
        per_row = grows[torch.as_tensor(lat_of_row, device=new.device)]  # [total_rows, M]
        n = lat.total_rows * self.planes * M
        out = new.clone()
        out[:n] = torch.where(per_row[:, None, :], new[:n].view(-1, self.planes, M), old[:n].view(-1, self.planes, M)).reshape(-1)
        return out


def string_prefix_open(lat, theta, *, keep=None, marker: Optional[int] = None, arc_scores=None) -> PrefixContext:
    """Opens a ``PrefixContext`` on a batch (``nfst_string_prefix_open``): the level pass, the continuation weights of
    every state, the in-arc and label lists and ``logz`` (``string_log_prob``'s, bit for bit), everything that
    ``string_next_log_probs`` repeats per call although it depends on no prefix.  Tape and scores are
    ``string_log_prob``'s; the scores are copied, so later changes of ``theta`` or ``arc_scores`` do not reach the
    context.  No gradient."""
    from .ops import _call, _need_gpu, _raise_status, _scores

    _need_gpu(lat)
    keep_mask, mk, _ = _tape(keep, marker, lat.vocab, lat.device, need_one=True)
    if not isinstance(theta, torch.Tensor):
        theta = torch.as_tensor(theta, dtype=torch.float32)
    sc, alive = _scores(lat, theta.detach().clone(), None if arc_scores is None else arc_scores.detach().clone())
    n = int(_lib.lib.nfst_string_prefix_open_ws_bytes(C.byref(lat.c_struct()), int(mk >= 0)))
    if n < 0:
        _lib.check(n, "nfst_string_prefix_open_ws_bytes")
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device=lat.device)
    logz = torch.empty(lat.n_lattices, dtype=torch.float64, device=lat.device)
    status = torch.zeros(1, dtype=torch.int32, device=lat.device)
    _call("nfst_string_prefix_open", lat, sc, keep_mask, mk, ws, ws.numel(), logz, status)
    _raise_status(status, "nfst_string_prefix_open")
    return PrefixContext(lat, sc, alive, keep_mask, mk, ws, logz)

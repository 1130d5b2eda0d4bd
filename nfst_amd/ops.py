"""Operators of the lattice engine: thin wrappers that allocate outputs with torch
and launch the HIP kernels through the C ABI (include/nfst_hip.h) on torch's
current stream.  There is no CPU implementation: every function raises if the
batch is not on a HIP device.  Reference call sites replaced are cited per op.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import lib, check
from .lattice import IntersectResult, LatticeBatch


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(lat: LatticeBatch) -> None:
    if lat.device.type != "cuda":
        raise RuntimeError("nfst_amd: the lattice engine runs on the MI355X only (no CPU fallback); "
                           "move the batch with LatticeBatch.to('cuda')")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _det(t):
    """``t`` outside the autograd graph (None stays None; a tensor that is in none comes back as it is)."""
    return t if t is None or not t.requires_grad else t.detach()


# ----------------------------------------------------------------------------- marshalling
def _call(name: str, lat: Optional[LatticeBatch], *args) -> None:
    """``check(lib.<name>([batch,] *args, stream), name)`` on torch's current stream: a tensor goes as its
    ``data_ptr()``, None as a null pointer, a ctypes struct by reference (the declared argument types see to the last
    two), everything else as it is.  ``lat`` is None for the entry points that take no batch.  A wrapper is 10 to 30 us
    of host work and this helper adds about 0.3 us to it (``hasattr`` is the cheapest test that takes a Parameter too):
    ``viterbi``, ``k_best_terms`` and ``expectation_terms``, which showed it in the measurement, write their call out."""
    argv = [a.data_ptr() if hasattr(a, "data_ptr") else a for a in args]
    if lat is not None:
        argv.insert(0, C.byref(lat.c_struct()))
    rc = getattr(lib, name)(*argv, _stream())
    if rc:
        check(rc, name)


def _workspace(lat: LatticeBatch, query: str, *args) -> tuple:
    """(workspace on the batch's device, its size) as the library's ``query(lat, *args)`` sizes it"""
    ws_bytes = int(getattr(lib, query)(C.byref(lat.c_struct()), *args))
    if ws_bytes < 0:
        check(ws_bytes, query)
    return torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=lat.device), ws_bytes


MAX_K = 64  # (nfst_kbest: a back pointer keeps the rank in 6 bits)


def _check_k(k, bounded: bool = True) -> None:
    """``k`` paths or draws per lattice: an int >= 1 (a bool is not a count), for the k-best ops at most ``MAX_K``."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 1 or (bounded and k > MAX_K):
        raise ValueError(f"k must be an int in [1, {MAX_K}], not {k!r}" if bounded else f"k must be an int >= 1, not {k!r}")


def _max_len(lat: LatticeBatch, max_len: Optional[int]) -> int:
    """The length of a path list: the longest path of the batch + 1 (room for the pad) unless the caller gave one."""
    return int(lat.depth.max()) + 1 if max_len is None else max_len


def _path_outputs(lat: LatticeBatch, lead: tuple, L: int, best=False, arcs=True, n_paths=False, logq=False) -> tuple:
    """``(best, paths, arcs, lengths, n_paths, logq)`` of a path op, uninitialised on the batch's device: ``paths`` and
    ``arcs`` int32 ``[*lead, L]``, ``lengths`` int32 and ``best`` / ``logq`` float32 ``[*lead]`` with ``lead`` = (B,) or
    (B, k), ``n_paths`` int32 [B]; None for whatever is not wanted."""
    dev, i32, f32 = lat.device, torch.int32, torch.float32
    return (torch.empty(lead, dtype=f32, device=dev) if best else None,
            torch.empty((*lead, L), dtype=i32, device=dev),
            torch.empty((*lead, L), dtype=i32, device=dev) if arcs else None,
            torch.empty(lead, dtype=i32, device=dev),
            torch.empty(lead[0], dtype=i32, device=dev) if n_paths else None,
            torch.empty(lead, dtype=f32, device=dev) if logq else None)


def _raise_status(status: torch.Tensor, where: str) -> None:
    """Reads back the status word (an int32 zero on the device before the launch) that ``where`` wrote -- one
    synchronisation -- and raises what it reports."""
    st = int(status.item())
    if st != 0:
        raise _lib.NfstError(st, where)


def _scores(lat: LatticeBatch, theta: torch.Tensor, arc_scores: Optional[torch.Tensor]):
    """nfst_scores + the tensors that must stay alive during the launch."""
    if theta.dtype != torch.float32 or theta.device != lat.device:
        theta = theta.to(device=lat.device, dtype=torch.float32)
    theta = theta.contiguous()
    if theta.dim() == 1:
        if theta.shape[0] != lat.vocab:
            raise ValueError(f"theta must have {lat.vocab} entries")
        stride = 0
    elif theta.dim() == 2 and theta.shape == (lat.n_lattices, lat.vocab):
        stride = lat.vocab
    else:
        raise ValueError("theta must be [V] or [B, V]")
    if arc_scores is not None:
        arc_scores = arc_scores.to(device=lat.device, dtype=torch.float32).contiguous()
        if arc_scores.shape != (lat.total_arcs,):
            raise ValueError(f"arc_scores must be [{lat.total_arcs}] in canonical arc order")
        if arc_scores.data_ptr() % 16:
            # a slice or split of a larger score tensor is contiguous but starts anywhere; the kernels read
            # per-arc scores 16 bytes at a time (nfst_forward_backward refuses a misaligned base)
            arc_scores = arc_scores.clone()
    return _lib.Scores(theta.data_ptr(), stride, _ptr(arc_scores), None, 0), (theta, arc_scores)


class BackwardResult(NamedTuple):
    logbeta: Optional[torch.Tensor]  # [total_rows] float32
    logz: torch.Tensor  # [B] float32
    logz64: torch.Tensor  # [B] float64
    beta_me: Optional[torch.Tensor]  # [total_rows, 2] float32 (mantissa, exponent bits)


def backward(lat: LatticeBatch, theta, arc_scores=None, want_logbeta=True, want_me=False) -> BackwardResult:
    """beta sweep + log Z.  Replaces FSAGRUScorer.compute_beta
    (/root/reference/src/modules/scorers.py:858-875)."""
    _need_gpu(lat)
    sc, keep = _scores(lat, theta, arc_scores)
    dev, B = lat.device, lat.n_lattices
    logbeta = torch.empty(lat.total_rows, dtype=torch.float32, device=dev) if want_logbeta else None
    z64 = torch.empty(B, dtype=torch.float64, device=dev)
    z32 = torch.empty(B, dtype=torch.float32, device=dev)
    me = torch.empty((lat.total_rows, 2), dtype=torch.float32, device=dev) if want_me else None
    _call("nfst_backward", lat, sc, logbeta, z64, z32, me)
    return BackwardResult(logbeta, z32, z64, me)


class ForwardBackwardResult(NamedTuple):
    logz: torch.Tensor
    logz64: torch.Tensor
    logalpha: Optional[torch.Tensor]
    logbeta: Optional[torch.Tensor]
    posterior: Optional[torch.Tensor]  # [total_arcs] canonical order
    grad_theta: Optional[torch.Tensor]  # [B, V]
    beta_me: Optional[torch.Tensor]


def forward_backward(lat: LatticeBatch, theta, arc_scores=None, want_alpha_beta=True, want_posterior=True,
                     want_grad_theta=False, want_me=False,
                     out: Optional[ForwardBackwardResult] = None, total=None, total_slot: int = 0) -> ForwardBackwardResult:
    """alpha/beta sweeps, exact log Z and arc posteriors (the quantity the
    reference only estimates by IWAE, modules/estimatros.py:33-44).  ``out`` (a
    previous result of the same batch and flags) is overwritten in place instead of
    allocating new outputs -- the steady state of a training loop.  ``total`` (a float64 tensor
    of 3 zeros, owned by the caller) receives sum_b log Z[b] in ``total[total_slot]`` without a
    reduction kernel; pass ``total_slot = step % 3`` (the launch clears the next slot)."""
    _need_gpu(lat)
    sc, keep = _scores(lat, theta, arc_scores)
    dev = lat.device
    f32 = dict(dtype=torch.float32, device=dev)
    if out is not None:
        z32, z64, la, lb, post, gth, me = out
        if ((la is None) == want_alpha_beta or (post is None) == want_posterior or (gth is None) == want_grad_theta
                or (me is None) == want_me or z64.shape[0] != lat.n_lattices):
            raise ValueError("`out` was produced with different flags or for another batch")
    else:
        la = torch.empty(lat.total_rows, **f32) if want_alpha_beta else None
        lb = torch.empty(lat.total_rows, **f32) if want_alpha_beta else None
        z64 = torch.empty(lat.n_lattices, dtype=torch.float64, device=dev)
        z32 = torch.empty(lat.n_lattices, **f32)
        post = torch.empty(lat.total_arcs, **f32) if want_posterior else None
        gth = torch.empty((lat.n_lattices, lat.vocab), **f32) if want_grad_theta else None
        me = torch.empty((lat.total_rows, 2), **f32) if want_me else None
    if total is not None and (total.dtype != torch.float64 or total.numel() != 3 or total.device != z64.device):
        raise ValueError("`total` must be a float64 tensor of 3 elements on the batch's device")
    _call("nfst_forward_backward", lat, sc, la, lb, z64, z32, post, gth, me, total, int(total_slot))
    return ForwardBackwardResult(z32, z64, la, lb, post, gth, me)


class ForwardBackwardLaunch:
    """``forward_backward`` with everything a call computes on the host computed ONCE: the steady state of a training
    loop -- same batch, same score tensors (updated in place by the optimiser), outputs overwritten -- pays one ctypes call
    per step (~5 us) instead of the wrapper's argument checks and allocations (~40 us: longer than the 38 us the kernel takes
    on the BASELINE batch, so the GPU idled between launches).  ``launch = ForwardBackwardLaunch(lat, theta, ...)``;
    ``launch(total_slot)`` enqueues the step on torch's current stream and returns ``launch.out`` (a
    ``ForwardBackwardResult`` whose tensors are overwritten by every launch).  The tensors passed in are held; replacing
    them (instead of updating them in place) needs a new object."""

    def __init__(self, lat: LatticeBatch, theta, arc_scores=None, want_alpha_beta=True, want_posterior=True, want_grad_theta=False,
                 want_me=False, out: Optional[ForwardBackwardResult] = None, total=None):
        _need_gpu(lat)
        self.lat = lat
        self._sc, self._keep = _scores(lat, theta, arc_scores)
        self.out = forward_backward(lat, theta, arc_scores=arc_scores, want_alpha_beta=want_alpha_beta, want_posterior=want_posterior,
                                    want_grad_theta=want_grad_theta, want_me=want_me, out=out)  # (allocates / checks everything, once)
        if total is not None and (total.dtype != torch.float64 or total.numel() != 3 or total.device != lat.device):
            raise ValueError("`total` must be a float64 tensor of 3 elements on the batch's device")
        self.total = total
        z32, z64, la, lb, post, gth, me = self.out
        self._struct = lat.c_struct()
        vp = C.c_void_p
        self._args = (C.byref(self._struct), C.byref(self._sc), vp(_ptr(la)), vp(_ptr(lb)), vp(_ptr(z64)), vp(_ptr(z32)), vp(_ptr(post)),
                      vp(_ptr(gth)), vp(_ptr(me)), vp(_ptr(total)))
        self._fn = lib.nfst_forward_backward

    def __call__(self, total_slot: int = 0) -> "ForwardBackwardResult":
        rc = self._fn(*self._args, total_slot, torch.cuda.current_stream().cuda_stream)
        if rc:
            check(rc, "nfst_forward_backward")
        return self.out


# ----------------------------------------------------------------------------- gradient assembly
# Pure torch arithmetic on whatever device its arguments live on: no entry point of the library and no CUDA call, so
# the backward passes below are these functions and run on host tensors with a host-packed batch.
def _per_label(x: torch.Tensor, g: torch.Tensor, shared: bool) -> torch.Tensor:
    """[B, V] per-label sums times the incoming gradient [B]; summed over the batch for a shared [V] table."""
    y = x * g[:, None]
    return y.sum(dim=0) if shared else y


def _per_position(x: torch.Tensor, g: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """[B, T, V] per-position sums times the incoming gradient [B]; summed over the batch for a shared [T, V] tensor."""
    y = x * g[:, None, None]
    return (y.sum(dim=0) if like.dim() == 2 else y).to(like.dtype)


def _arc_grad(lat: LatticeBatch, g: torch.Tensor) -> torch.Tensor:
    """[total_arcs]: the incoming gradient [B] of every canonical arc's lattice (one small index upload: a backward
    that needs it for two gradients takes it once)."""
    return g[lat.arc_lattice()]


def _per_arc(lat: LatticeBatch, x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """[total_arcs] per-arc quantities times the incoming gradient [B] of the arc's lattice."""
    return x * _arc_grad(lat, g)


def _path_score_grads(lat: LatticeBatch, arcs: torch.Tensor, g: torch.Tensor, theta_like=None, arc_like=None,
                      pos_like=None) -> tuple:
    """``(d_theta, d_arc, d_pos)`` of path scores best[b, j] = the sum of the terms of path j of lattice b, given the
    paths as canonical arc ids ``arcs`` [B, K, T] (-1 padded; position t of a path is entry t) and the incoming gradient
    ``g`` [B, K]: every arc of a path gets g in ``d_arc`` [total_arcs], its label in ``d_theta`` ([V], or [B, V] per
    lattice) and its (position, label) in ``d_pos`` ([T, V], or [B, T, V]).  Each is computed only if its "like" tensor
    -- the input it is the gradient of -- is given, in float32, and returned in that tensor's shape, dtype and device.
    Entries of ``g`` that are not finite (the -inf scores of missing paths feed back -inf or NaN) count as 0."""
    B, K, T = arcs.shape
    V = lat.vocab
    a = arcs.to(torch.int64)
    on = a >= 0  # (-inf entries have no arcs)
    gg = torch.where(torch.isfinite(g), g, torch.zeros_like(g)).to(torch.float32)
    w = gg[:, :, None].expand(B, K, T)[on]
    idx = a[on]

    def scatter(n, index, like):
        return torch.zeros(n, dtype=torch.float32, device=arcs.device).index_add_(0, index, w).view(like.shape) \
            .to(dtype=like.dtype, device=like.device)

    def along(n, dim):  # (the index along ``dim`` of every path entry that holds an arc)
        shape = [1, 1, 1]
        shape[dim] = n
        return torch.arange(n, device=arcs.device).view(shape).expand(B, K, T)[on]

    d_theta = d_arc = d_pos = None
    if arc_like is not None:
        d_arc = scatter(lat.total_arcs, idx, arc_like)
    if theta_like is not None or pos_like is not None:
        lab = lat.arc_label.to(torch.int64)[idx]
    if theta_like is not None:
        d_theta = scatter(V, lab, theta_like) if theta_like.dim() == 1 else scatter(B * V, along(B, 0) * V + lab, theta_like)
    if pos_like is not None:
        t = along(T, 2)
        d_pos = scatter(T * V, t * V + lab, pos_like) if pos_like.dim() == 2 \
            else scatter(B * T * V, (along(B, 0) * T + t) * V + lab, pos_like)
    return d_theta, d_arc, d_pos


class _LogZ(torch.autograd.Function):
    """log Z with d log Z / d score = arc posterior."""

    @staticmethod
    def forward(ctx, lat, theta, arc_scores):
        need_t = theta.requires_grad
        need_a = arc_scores is not None and arc_scores.requires_grad
        r = forward_backward(lat, theta.detach(), _det(arc_scores), want_alpha_beta=False, want_posterior=need_a, want_grad_theta=need_t)
        ctx.lat = lat
        ctx.shared_theta = theta.dim() == 1
        ctx.inputs = (theta, arc_scores)  # (read only by a backward that builds a graph, create_graph=True)
        ctx.save_for_backward(r.posterior if need_a else None, r.grad_theta if need_t else None)
        return r.logz

    @staticmethod
    def backward(ctx, g):
        post, gth = ctx.saved_tensors
        if torch.is_grad_enabled():
            # create_graph=True: the posteriors depend on the scores; _LogZGrad carries that dependence (second order)
            theta, arc_scores = ctx.inputs
            g_theta, g_arc = _LogZGrad.apply(ctx.lat, ctx.shared_theta, theta, arc_scores, g, post, gth)
            return None, g_theta, g_arc
        return (None, None if gth is None else _per_label(gth, g, ctx.shared_theta),
                None if post is None else _per_arc(ctx.lat, post, g))


def log_z(lat: LatticeBatch, theta: torch.Tensor, arc_scores: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable exact log-marginal per lattice, float32 [B]."""
    return _LogZ.apply(lat, theta, arc_scores)


# ----------------------------------------------------------------------------- expectation semiring
class ExpectationResult(NamedTuple):
    logz64: torch.Tensor  # [B] float64
    ev64: torch.Tensor  # [B] float64 E[V]
    ev: torch.Tensor  # [B] float32 E[V]
    posterior: Optional[torch.Tensor]  # [total_arcs] p_a
    cov: Optional[torch.Tensor]  # [total_arcs] c_a = Cov(1_a, V)
    label_cov: Optional[torch.Tensor]  # [B, V] c_a summed per label
    label_post: Optional[torch.Tensor]  # [B, V] p_a summed per label


def _input(lat: LatticeBatch, t, name: str, per_lattice_ok: bool, per_arc: bool) -> Optional[torch.Tensor]:
    """Checks a score or value tensor of the expectation ops: on the batch's device, floating point, [V] / [B, V]
    (per-label) or [total_arcs] (per-arc).  Returns it as contiguous float32 (None stays None)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch.Tensor, not {type(t).__name__}")
    if t.device != lat.device:
        raise ValueError(f"{name} is on {t.device}, the lattice batch on {lat.device}")
    if not t.is_floating_point():
        raise ValueError(f"{name} must be a floating-point tensor, not {t.dtype}")
    if per_arc:
        if t.shape != (lat.total_arcs,):
            raise ValueError(f"{name} must be [{lat.total_arcs}] in canonical arc order, not {list(t.shape)}")
    elif not (t.shape == (lat.vocab,) or (per_lattice_ok and t.shape == (lat.n_lattices, lat.vocab))):
        raise ValueError(f"{name} must be [{lat.vocab}] or [{lat.n_lattices}, {lat.vocab}], not {list(t.shape)}")
    return t.to(torch.float32).contiguous()


def expectation_terms(lat: LatticeBatch, theta, arc_scores=None, label_values=None, arc_values=None, score_coef: float = 0.0,
                      want_posterior=False, want_cov=False, want_label_cov=False, want_label_post=False) -> ExpectationResult:
    """One launch of ``nfst_expectation`` (no autograd): for the per-arc values
    v_a = label_values[b, label_a] + arc_values[a] + score_coef * s_a (each term optional; s_a the arc's log weight),
    log Z, E[V] and, on request, the arc posteriors p_a, c_a = p_a (E[V | a] - E[V]) and both summed per label."""
    _need_gpu(lat)
    theta = _input(lat, theta, "theta", True, False)
    arc_scores = _input(lat, arc_scores, "arc_scores", False, True)
    label_values = _input(lat, label_values, "label_values", True, False)
    arc_values = _input(lat, arc_values, "arc_values", False, True)
    coef = float(score_coef)
    if coef != coef or coef in (float("inf"), float("-inf")):
        raise ValueError(f"score_coef must be finite, not {score_coef}")
    sc, keep = _scores(lat, theta, arc_scores)
    dev, f32, f64 = lat.device, torch.float32, torch.float64
    B, A = lat.n_lattices, lat.total_arcs
    ws, ws_bytes = _workspace(lat, "nfst_expectation_ws_bytes")
    z64 = torch.empty(B, dtype=f64, device=dev)
    ev64 = torch.empty(B, dtype=f64, device=dev)
    ev32 = torch.empty(B, dtype=f32, device=dev)
    post = torch.empty(A, dtype=f32, device=dev) if want_posterior else None
    cov = torch.empty(A, dtype=f32, device=dev) if want_cov else None
    lc = torch.empty((B, lat.vocab), dtype=f32, device=dev) if want_label_cov else None
    lp = torch.empty((B, lat.vocab), dtype=f32, device=dev) if want_label_post else None
    lv_stride = 0 if label_values is None or label_values.dim() == 1 else lat.vocab
    rc = lib.nfst_expectation(C.byref(lat.c_struct()), C.byref(sc), _ptr(label_values), lv_stride, _ptr(arc_values), coef,
                              ws.data_ptr(), ws_bytes, z64.data_ptr(), ev64.data_ptr(), ev32.data_ptr(), _ptr(post), _ptr(cov),
                              _ptr(lc), _ptr(lp), _stream())  # (written out: see _call)
    if rc:
        check(rc, "nfst_expectation")
    return ExpectationResult(z64, ev64, ev32, post, cov, lc, lp)


class _Expectation(torch.autograd.Function):
    """E[V] with dE/ds_a = c_a + coef p_a, dE/d(arc value) = p_a, dE/d(label value) = per-label sums of p_a."""

    @staticmethod
    def forward(ctx, lat, theta, arc_scores, label_values, arc_values, coef):
        nt, na, nlv, nav = ctx.needs_input_grad[1:5]
        r = expectation_terms(lat, theta.detach(), _det(arc_scores), _det(label_values), _det(arc_values), coef,
                              want_posterior=nav or (na and coef != 0.0), want_cov=na, want_label_cov=nt,
                              want_label_post=nlv or (nt and coef != 0.0))
        ctx.lat, ctx.coef = lat, coef
        ctx.shared = (theta.dim() == 1, label_values is not None and label_values.dim() == 1)
        ctx.save_for_backward(r.posterior, r.cov, r.label_cov, r.label_post)
        return r.ev

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        post, cov, lc, lp = ctx.saved_tensors
        nt, na, nlv, nav = ctx.needs_input_grad[1:5]
        k = ctx.coef
        ga = _arc_grad(ctx.lat, g) if (na or nav) else None
        d_theta = _per_label(lc if k == 0.0 else lc + k * lp, g, ctx.shared[0]) if nt else None
        d_arc = (cov if k == 0.0 else cov + k * post) * ga if na else None
        d_lv = _per_label(lp, g, ctx.shared[1]) if nlv else None
        d_av = post * ga if nav else None
        return None, d_theta, d_arc, d_lv, d_av, None


def expectation(lat: LatticeBatch, theta: torch.Tensor, arc_scores: Optional[torch.Tensor] = None,
                label_values: Optional[torch.Tensor] = None, arc_values: Optional[torch.Tensor] = None,
                score_coef: float = 0.0) -> torch.Tensor:
    """Exact E_p[sum over the path of v_a] per lattice, float32 [B], where p is the lattice distribution of the scores
    (``theta`` [V] or [B, V], ``arc_scores`` [total_arcs]) and v_a = label_values[(b,) label_a] + arc_values[a] +
    score_coef * s_a: expected path length (label_values = ones), expected label counts, expected cost.  Differentiable
    in theta, arc_scores, label_values and arc_values (one launch of the expectation semiring)."""
    return _Expectation.apply(lat, theta, arc_scores, label_values, arc_values, float(score_coef))


class _Entropy(torch.autograd.Function):
    """H(p) = log Z - E_p[S] from one launch with score_coef = 1; dH/ds_a = -c_a."""

    @staticmethod
    def forward(ctx, lat, theta, arc_scores):
        nt, na = ctx.needs_input_grad[1:3]
        r = expectation_terms(lat, theta.detach(), _det(arc_scores), score_coef=1.0, want_cov=na, want_label_cov=nt)
        ctx.lat, ctx.shared = lat, theta.dim() == 1
        ctx.save_for_backward(r.cov, r.label_cov)
        return (r.logz64 - r.ev64).to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        cov, lc = ctx.saved_tensors
        nt, na = ctx.needs_input_grad[1:3]
        d_theta = -_per_label(lc, g, ctx.shared) if nt else None
        d_arc = _per_arc(ctx.lat, -cov, g) if na else None
        return None, d_theta, d_arc


def entropy(lat: LatticeBatch, theta: torch.Tensor, arc_scores: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Exact path entropy H(p) = log Z - E_p[S] per lattice, float32 [B] (in nats; the difference is taken in float64).
    Differentiable in theta ([V] or [B, V]) and arc_scores: dH/ds_a = -Cov(1_a, S)."""
    return _Entropy.apply(lat, theta, arc_scores)


class _KL(torch.autograd.Function):
    """KL(p||q) = log Z_q - log Z_p + E_p[S_p - S_q] (arc_w cancels in S_p - S_q); dKL/ds_p = c(v = S_p - S_q),
    dKL/ds_q = p_q - p_p."""

    @staticmethod
    def forward(ctx, lat, theta_p, theta_q, arc_scores_p, arc_scores_q):
        ntp, ntq, nap, naq = ctx.needs_input_grad[1:5]
        tp, tq, asp, asq = theta_p.detach(), theta_q.detach(), _det(arc_scores_p), _det(arc_scores_q)
        for name, t in (("theta_p", tp), ("theta_q", tq)):
            _input(lat, t, name, True, False)
        for name, t in (("arc_scores_p", asp), ("arc_scores_q", asq)):
            _input(lat, t, name, False, True)
        lv = tp.to(torch.float32) - tq.to(torch.float32)  # ([V] - [B, V] broadcasts to [B, V])
        av = None
        if asp is not None or asq is not None:
            av = (asp.to(torch.float32) if asp is not None else 0.0) - (asq.to(torch.float32) if asq is not None else 0.0)
            if not isinstance(av, torch.Tensor):
                av = None
        rp = expectation_terms(lat, tp, asp, lv, av, 0.0, want_posterior=naq, want_cov=nap, want_label_cov=ntp,
                               want_label_post=ntq)
        rq = expectation_terms(lat, tq, asq, want_posterior=naq, want_label_post=ntq)
        ctx.lat, ctx.shared = lat, (theta_p.dim() == 1, theta_q.dim() == 1)
        ctx.save_for_backward(rp.cov, rp.label_cov, rp.posterior, rp.label_post, rq.posterior, rq.label_post)
        return (rq.logz64 - rp.logz64 + rp.ev64).to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        cov_p, lc_p, post_p, lp_p, post_q, lp_q = ctx.saved_tensors
        ntp, ntq, nap, naq = ctx.needs_input_grad[1:5]
        ga = _arc_grad(ctx.lat, g) if (nap or naq) else None
        return (None, _per_label(lc_p, g, ctx.shared[0]) if ntp else None,
                _per_label(lp_q - lp_p, g, ctx.shared[1]) if ntq else None,
                cov_p * ga if nap else None, (post_q - post_p) * ga if naq else None)


def kl_divergence(lat: LatticeBatch, theta_p: torch.Tensor, theta_q: torch.Tensor, arc_scores_p: Optional[torch.Tensor] = None,
                  arc_scores_q: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Exact KL(p || q) per lattice, float32 [B], of two weightings of the same batch (theta_p / theta_q [V] or [B, V],
    optional per-arc scores); the float64 parts are combined in float64.  Differentiable in all four score inputs:
    dKL/ds_p = Cov_p(1_a, S_p - S_q), dKL/ds_q = p_q - p_p.  The exact counterpart of the sampled KL terms of
    Estimators.estimate_offset_kl_q_p (/root/reference/src/modules/estimatros.py:236-285) for a WFST proposal."""
    return _KL.apply(lat, theta_p, theta_q, arc_scores_p, arc_scores_q)


class _LogZGrad(torch.autograd.Function):
    """The gradient of log Z as a differentiable function of the scores and of the incoming gradient g (the
    create_graph=True backward of log_z): G_theta[b, l] = g_b sum_{a: label l} p_a, G_arc[a] = g_b p_a.  Its own backward
    is one expectation launch with the incoming (u_theta, u_arc) as per-label and per-arc values:
    dG.u/ds_a = g_b c_a(v = u) (a Hessian-vector product of log Z) and dG.u/dg_b = E_b[V]."""

    @staticmethod
    def forward(ctx, lat, shared, theta, arc_scores, g, post, gth):
        ctx.lat, ctx.shared = lat, shared
        ctx.save_for_backward(theta, arc_scores, g)
        return None if gth is None else _per_label(gth, g, shared), None if post is None else _per_arc(lat, post, g)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, u_theta, u_arc):
        theta, arc_scores, g = ctx.saved_tensors
        nt, na, ng = ctx.needs_input_grad[2:5]
        lat = ctx.lat
        if u_theta is None and u_arc is None:
            return None, None, None, None, None, None, None
        f32 = dict(device=lat.device, dtype=torch.float32)  # (log_z takes scores anywhere and moves them; so does this)
        r = expectation_terms(lat, theta.detach().to(**f32), None if arc_scores is None else arc_scores.detach().to(**f32),
                              u_theta, u_arc, want_cov=na, want_label_cov=nt)
        d_theta = _per_label(r.label_cov, g, ctx.shared) if nt else None
        d_arc = _per_arc(lat, r.cov, g) if na else None
        d_g = r.ev.to(g.dtype) if ng else None
        return None, None, d_theta, d_arc, d_g, None, None


class ViterbiResult(NamedTuple):
    best: torch.Tensor  # [B] float32
    paths: torch.Tensor  # [B, max_len] int32, pad-terminated (bos .. eos)
    arcs: torch.Tensor  # [B, max_len] int32 canonical arc ids, -1 padded
    lengths: torch.Tensor  # [B] int32


def viterbi(lat: LatticeBatch, theta, arc_scores=None, max_len: Optional[int] = None, pad: int = 0) -> ViterbiResult:
    """Best path per lattice (best_sample of JointProb.forward, modules/lightning.py:474-479)."""
    _need_gpu(lat)
    sc, keep = _scores(lat, theta, arc_scores)
    max_len = _max_len(lat, max_len)
    best, paths, arcs, lens, _, _ = _path_outputs(lat, (lat.n_lattices,), max_len, best=True)
    check(lib.nfst_viterbi(C.byref(lat.c_struct()), C.byref(sc), best.data_ptr(), paths.data_ptr(), arcs.data_ptr(),
                           lens.data_ptr(), int(max_len), int(pad), _stream()), "nfst_viterbi")  # (written out: see _call)
    return ViterbiResult(best, paths, arcs, lens)


class KBestResult(NamedTuple):
    best: torch.Tensor  # [B, k] float32, non-increasing; -inf beyond n_paths
    paths: torch.Tensor  # [B, k, max_len] int32 labels (bos .. eos), pad-terminated
    arcs: torch.Tensor  # [B, k, max_len] int32 canonical arc ids, -1 padded
    lengths: torch.Tensor  # [B, k] int32 arcs per path (0 beyond n_paths)
    n_paths: torch.Tensor  # [B] int32 min(k, paths of score > -inf)


def k_best_terms(lat: LatticeBatch, theta, k: int, arc_scores=None, max_len: Optional[int] = None, pad: int = 0) -> KBestResult:
    """One launch of ``nfst_kbest`` (no autograd); see ``k_best``."""
    _need_gpu(lat)
    _check_k(k)
    sc, keep = _scores(lat, theta, arc_scores)
    # (length, outputs and call written out: the launch waits for what the host does here and the read-back below waits
    # for the launch, so this op shows every helper call; with _path_outputs and _call it took 0.9 us more than before)
    if max_len is None:
        max_len = int(lat.depth.max()) + 1
    ws, ws_bytes = _workspace(lat, "nfst_kbest_ws_bytes", k)
    dev, B = lat.device, lat.n_lattices
    best = torch.empty((B, k), dtype=torch.float32, device=dev)
    paths = torch.empty((B, k, max_len), dtype=torch.int32, device=dev)
    arcs = torch.empty((B, k, max_len), dtype=torch.int32, device=dev)
    lens = torch.empty((B, k), dtype=torch.int32, device=dev)
    n_paths = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = lib.nfst_kbest(C.byref(lat.c_struct()), C.byref(sc), k, ws.data_ptr(), ws_bytes, best.data_ptr(), paths.data_ptr(),
                        arcs.data_ptr(), lens.data_ptr(), n_paths.data_ptr(), int(max_len), int(pad), status.data_ptr(), _stream())
    if rc:
        check(rc, "nfst_kbest")
    _raise_status(status, "nfst_kbest")  # a path longer than max_len
    return KBestResult(best, paths, arcs, lens, n_paths)


class _KBest(torch.autograd.Function):
    """best[b, j] = the sum of the scores of path j's arcs: d/d arc_scores[a] = 1 on the path's arcs, d/d theta counts
    its labels (per lattice for a [B, V] theta); -inf entries (no path) get no gradient."""

    @staticmethod
    def forward(ctx, lat, theta, arc_scores, k, max_len, pad):
        r = k_best_terms(lat, theta.detach(), k, _det(arc_scores), max_len, pad)
        ctx.lat = lat
        ctx.like = (theta, arc_scores)
        ctx.save_for_backward(r.arcs)
        ctx.mark_non_differentiable(r.paths, r.arcs, r.lengths, r.n_paths)
        return r.best, r.paths, r.arcs, r.lengths, r.n_paths

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *_):
        (arcs,) = ctx.saved_tensors
        nt, na = ctx.needs_input_grad[1:3]
        theta, arc_scores = ctx.like
        d_theta, d_arc, _ = _path_score_grads(ctx.lat, arcs, g, theta if nt else None, arc_scores if na else None)
        return None, d_theta, d_arc, None, None, None


def k_best(lat: LatticeBatch, theta, k: int, arc_scores=None, max_len: Optional[int] = None, pad: int = 0) -> KBestResult:
    """The k best paths of every lattice, exact (``nfst_kbest``): the n-best list that
    evaluate/rerank.py reranks and the exact, deterministic form of JointProb.forward's "best of K samples"
    (modules/lightning.py:474-479).  ``theta`` [V] or [B, V], ``arc_scores`` [total_arcs] (optional); 1 <= k <= 64.
    Entry 0 is ``viterbi``'s path (bit for bit with its general kernel); ties on exactly equal scores go to the smaller
    first differing label.  Lattices with fewer than k paths of score > -inf fill the rest with score -inf, length 0,
    ``pad`` labels and arc -1 (``n_paths`` counts the real ones).  ``max_len`` defaults to the longest path + 1; a
    longer path raises ``NfstError`` (NFST_ERR_LENGTH).  ``best`` is differentiable in theta and arc_scores: the
    gradient of a path's score counts its labels / marks its arcs."""
    _check_k(k)
    if not isinstance(theta, torch.Tensor):
        theta = torch.as_tensor(theta, dtype=torch.float32)
    return KBestResult(*_KBest.apply(lat, theta, arc_scores, k, max_len, pad))


class ArcSlackResult(NamedTuple):
    best: torch.Tensor  # [B] float32: the best path's score (the bits of k_best(k=1).best)
    slack: torch.Tensor  # [total_arcs] float32 >= 0; +inf on arcs that lie on no path of finite score
    keep: Optional[torch.Tensor]  # [total_arcs] bool: slack <= beam (with a beam)
    n_kept: Optional[torch.Tensor]  # [B] int32 kept arcs per lattice (with a beam)
    vbeta: Optional[torch.Tensor]  # [total_rows] float32 best score from the row to the sink (want_rows)
    state_slack: Optional[torch.Tensor]  # [total_rows] float32 slack of the best path through the row (want_rows)


def _beam(lat: LatticeBatch, beam) -> torch.Tensor:
    """[B] float32 on the batch's device; every entry >= 0 (+inf allowed)."""
    if isinstance(beam, torch.Tensor):
        if beam.dim() == 0:
            beam = beam.reshape(1).expand(lat.n_lattices)
        if beam.shape != (lat.n_lattices,):
            raise ValueError(f"beam must be a number or a [{lat.n_lattices}] tensor, not {tuple(beam.shape)}")
        beam = beam.detach().to(device=lat.device, dtype=torch.float32).contiguous()
        if not bool((beam >= 0).all()):  # (NaN fails the comparison too)
            raise ValueError("every beam must be >= 0 (inf allowed), not negative or NaN")
        return beam
    if isinstance(beam, bool) or not isinstance(beam, (int, float)) or not beam >= 0:
        raise ValueError(f"beam must be a number >= 0 (inf allowed) or a [{lat.n_lattices}] tensor, not {beam!r}")
    return torch.full((lat.n_lattices,), float(beam), dtype=torch.float32, device=lat.device)


def arc_slack(lat: LatticeBatch, theta, arc_scores=None, beam=None, want_rows: bool = False) -> ArcSlackResult:
    """Exact arc slack (``nfst_arc_slack``, DESIGN.md sections 2 and 4.7): per canonical arc, how far the best path
    through the arc falls short of the best path of its lattice -- the max-plus counterpart of ``forward_backward``'s
    arc posteriors, next to ``viterbi`` and ``k_best``.  ``slack`` is >= 0, exactly 0 on the arcs of ``k_best``'s
    entry 0 and +inf on arcs that lie on no path of finite score; ``best - slack`` is the arc's max-marginal (one more
    rounding).  ``theta`` [V] or [B, V], ``arc_scores`` [total_arcs] (optional).  ``beam``: a number or a ``[B]`` tensor,
    every entry >= 0 (``inf`` allowed; a negative or NaN beam raises ``ValueError``): ``keep = slack <= beam`` and
    ``n_kept`` per lattice.  The kept arcs are trim -- every one lies on a path of kept arcs from state 0 to the sink
    -- so ``LatticeBatch.restrict(keep)`` packs them as they are.  ``want_rows``: ``vbeta`` and ``state_slack`` per
    row (-inf / +inf for rows on no path of finite score).  Results are bit-identical from call to call and for every
    packing of the same lattices.  Not differentiable: the outputs carry no gradient."""
    _need_gpu(lat)
    sc, alive = _scores(lat, theta.detach() if isinstance(theta, torch.Tensor) else torch.as_tensor(theta, dtype=torch.float32),
                        _det(arc_scores))
    dev = lat.device
    B, A, R = lat.n_lattices, lat.total_arcs, lat.total_rows
    bm = None if beam is None else _beam(lat, beam)
    ws, ws_bytes = _workspace(lat, "nfst_arc_slack_ws_bytes")
    best = torch.empty(B, dtype=torch.float32, device=dev)
    # (one element at least: a batch without any arc still hands the library pointers)
    slack = torch.empty(max(A, 1), dtype=torch.float32, device=dev)
    keep = torch.empty(max(A, 1), dtype=torch.uint8, device=dev) if bm is not None else None
    n_kept = torch.empty(B, dtype=torch.int32, device=dev) if bm is not None else None
    vbeta = torch.empty(R, dtype=torch.float32, device=dev) if want_rows else None
    sslack = torch.empty(R, dtype=torch.float32, device=dev) if want_rows else None
    _call("nfst_arc_slack", lat, sc, bm, ws, ws_bytes, best, vbeta, sslack, slack, keep, n_kept)
    if A == 0:
        slack, keep = slack[:0], None if keep is None else keep[:0]
    return ArcSlackResult(best, slack, None if keep is None else keep.view(torch.bool), n_kept, vbeta, sslack)


class PruneResult(NamedTuple):
    lat: LatticeBatch  # the kept arcs, packed: same rows, state ids and vocabulary
    arc_map: torch.Tensor  # int64 [A']: positions of the new canonical arcs among the old ones (increasing)
    n_kept: torch.Tensor  # [B] int32
    best: torch.Tensor  # [B] float32


def prune(lat: LatticeBatch, theta, beam, arc_scores=None, **pack_opts) -> PruneResult:
    """Beam pruning: the arcs whose best path is within ``beam`` of the lattice's best path (``arc_slack``), packed
    into a new batch (``LatticeBatch.restrict``; ``pack_opts`` go to the packer, ``chunks=`` / ``chunk_opts=``
    included).  ``arc_scores[arc_map]`` scores the new batch.  The best path always survives (beam 0 keeps exactly the
    arcs of the paths tied for best); a lattice without a path of finite score keeps nothing and raises ``ValueError``.
    One small read-back (``n_kept``)."""
    r = arc_slack(lat, theta, arc_scores=arc_scores, beam=beam)
    new, arc_map = lat.restrict(r.keep, n_kept=r.n_kept, **pack_opts)
    return PruneResult(new, arc_map, r.n_kept, r.best)


def intersect(lat: LatticeBatch, dfa, **pack_opts) -> IntersectResult:
    """The product of every lattice with a constraint automaton (``constraints.ConstraintDFA``, or the sparse
    ``constraints.WideDFA`` of up to 4096 states), packed into a new batch whose paths are exactly the accepted paths of
    ``lat``: ``LatticeBatch.intersect`` (``nfst_intersect_count`` / ``_write``, DESIGN.md sections 2 and 4.8; for a
    ``WideDFA`` ``nfst_intersect_wide_count`` / ``_write``, section 4.19).  ``(lattice, arc_map, arc_q, row_state,
    row_q)``; ``pack_opts`` go to the packer, ``chunks=`` / ``chunk_opts=`` included."""
    _need_gpu(lat)
    return lat.intersect(dfa, **pack_opts)


# ----------------------------------------------------------------------------- position-dependent scores
class PositionalResult(NamedTuple):
    logz: torch.Tensor  # [B] float32 log Z_T
    logz64: torch.Tensor  # [B] float64
    pos_posterior: Optional[torch.Tensor]  # [B, T, V] float32: P(the mark at position t is l) = d log Z_T / d pos_scores
    arc_posterior: Optional[torch.Tensor]  # [total_arcs] float32: sum over t of P(arc a is at position t)
    len_logz: Optional[torch.Tensor]  # [B, T + 1] float64: log weight of the paths of exactly L arcs (entry 0: -inf; 0 where state 0 is the sink)


class PositionalViterbiResult(NamedTuple):
    best: torch.Tensor  # [B] float32
    paths: torch.Tensor  # [B, T] int32 labels (bos .. eos), pad-terminated
    path_arcs: torch.Tensor  # [B, T] int32 canonical arc ids, -1 padded
    lengths: torch.Tensor  # [B] int32 (0 where best is -inf)


def _position_tensor(lat: LatticeBatch, t, name: str, T: Optional[int]):
    """(``t`` as contiguous float32, its stride) of a per-position tensor, checked: a floating-point tensor [T, V] (one
    table for the batch) or [B, T, V] on the batch's device, with the ``T`` of the call (None: any T >= 1)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch.Tensor, not {type(t).__name__}")
    if t.device != lat.device:
        raise ValueError(f"{name} is on {t.device}, the lattice batch on {lat.device}")
    if not t.is_floating_point():
        raise ValueError(f"{name} must be a floating-point tensor, not {t.dtype}")
    if t.dim() not in (2, 3) or t.shape[-1] != lat.vocab or (t.shape[-2] < 1 if T is None else t.shape[-2] != T) \
            or (t.dim() == 3 and t.shape[0] != lat.n_lattices):
        Ts, more = ("T", " with T >= 1") if T is None else (T, "")
        raise ValueError(f"{name} must be [{Ts}, {lat.vocab}] or [{lat.n_lattices}, {Ts}, {lat.vocab}]{more}, not {list(t.shape)}")
    return t.to(torch.float32).contiguous(), (0 if t.dim() == 2 else int(t.shape[-2]) * lat.vocab)


def _positions(lat: LatticeBatch, pos_scores, T):
    """(pos_scores as contiguous float32 or None, its stride, T) of the positional ops, checked by ``_position_tensor``;
    ``T`` defaults to the length of ``pos_scores``, and without ``pos_scores`` to the longest path of the batch."""
    if T is not None and (isinstance(T, bool) or not isinstance(T, int) or T < 1):
        raise ValueError(f"T must be an int >= 1, not {T!r}")
    if pos_scores is None:
        return None, 0, int(lat.depth.max()) if T is None else T
    pos, stride = _position_tensor(lat, pos_scores, "pos_scores", None)
    if T is not None and T != pos_scores.shape[-2]:
        raise ValueError(f"T = {T}, but pos_scores has {pos_scores.shape[-2]} positions")
    return pos, stride, int(pos_scores.shape[-2])


def _score_args(lat: LatticeBatch, theta, arc_scores, pos_scores=None, T: Optional[int] = None) -> tuple:
    """``(nfst_scores, the tensors it points into, pos, stride, T)`` of an op that checks its scores strictly: ``theta``
    and ``arc_scores`` by ``_input``, then ``pos_scores`` and ``T`` by ``_positions``, in that order; everything
    detached, since a launch reads values and records nothing."""
    theta = _input(lat, theta, "theta", True, False)
    arc_scores = _input(lat, arc_scores, "arc_scores", False, True)
    pos, stride, T = _positions(lat, pos_scores, T)
    sc, keep = _scores(lat, _det(theta), _det(arc_scores))
    return sc, keep, _det(pos), stride, T


def _positional_ws(lat: LatticeBatch, T: int, flags: int) -> tuple:
    return _workspace(lat, "nfst_positional_ws_bytes", T, flags)


def _positional_plan(lat: LatticeBatch, name: str, *args) -> tuple:
    lds, staged = C.c_int64(0), C.c_int32(0)
    check(getattr(lib, name)(C.byref(lat.c_struct()), *args, C.byref(lds), C.byref(staged)), name)
    return int(lds.value), bool(staged.value)


def positional_plan(lat: LatticeBatch, viterbi: bool = False) -> tuple:
    """(``lds_bytes``, ``staged``) of the launch ``positional_forward_backward`` (``viterbi=True``:
    ``positional_viterbi``) makes for this batch (``nfst_positional_plan``, the rule the launchers themselves call): the
    dynamic LDS of the kernel, and whether it keeps the arc records of the largest lattice there instead of reading the
    canonical arrays at every step.  Asked on the host: the batch may be host-packed, and no GPU is needed.  A batch
    beyond the op's LDS limit raises ``NfstError`` (-6), as the op would."""
    return _positional_plan(lat, "nfst_positional_plan", 1 if viterbi else 0)


def positional_forward_backward(lat: LatticeBatch, theta, pos_scores=None, T: Optional[int] = None, arc_scores=None,
                                want_pos_posterior: bool = True, want_arc_posterior: bool = False,
                                want_len: bool = False) -> PositionalResult:
    """One launch of ``nfst_positional`` (no autograd; DESIGN.md sections 2 and 4.10): exact sums over the paths of at
    most ``T`` arcs when the arc at position t of a path also scores ``pos_scores[(b,) t, label]`` -- per-position
    logits of a tagger or encoder -- on top of ``theta`` [V] or [B, V] and ``arc_scores`` [total_arcs].  Entries of
    ``pos_scores`` may be -inf (the mark is forbidden at that position); NaN or +inf are the caller's business (nothing
    scans for them); the pad column enters no result.  ``T`` defaults to ``pos_scores.shape[-2]``, without
    ``pos_scores`` to the longest path of the batch (then log Z and the arc posteriors are ``forward_backward``'s).
    Paths longer than ``T`` are not counted; a lattice without a path of finite score within ``T`` gets -inf and zero
    posteriors.  The workspace stores every beta row of every position: 12 (T + 1) total_rows bytes."""
    _need_gpu(lat)
    sc, keep, pos, stride, T = _score_args(lat, theta, arc_scores, pos_scores, T)
    dev = lat.device
    B = lat.n_lattices
    need = want_pos_posterior or want_arc_posterior or want_len
    ws, ws_bytes = _positional_ws(lat, T, 1 if need else 0)
    z64 = torch.empty(B, dtype=torch.float64, device=dev)
    z32 = torch.empty(B, dtype=torch.float32, device=dev)
    pp = torch.empty((B, T, lat.vocab), dtype=torch.float32, device=dev) if want_pos_posterior else None
    ap = torch.empty(lat.total_arcs, dtype=torch.float32, device=dev) if want_arc_posterior else None
    ll = torch.empty((B, T + 1), dtype=torch.float64, device=dev) if want_len else None
    _call("nfst_positional", lat, sc, pos, stride, T, ws, ws_bytes, z64, z32, ll, pp, ap)
    return PositionalResult(z32, z64, pp, ap, ll)


class _PositionalLogZ(torch.autograd.Function):
    """log Z_T with d/d pos_scores = the position posteriors, d/d theta = their sums over t, d/d arc_scores = the arc
    posteriors.  First order only: a double backward raises (once_differentiable)."""

    @staticmethod
    def forward(ctx, lat, theta, pos_scores, arc_scores):
        nt, npos, na = ctx.needs_input_grad[1:4]
        r = positional_forward_backward(lat, theta.detach(), pos_scores.detach(), None, _det(arc_scores),
                                        want_pos_posterior=nt or npos, want_arc_posterior=na)
        ctx.lat = lat
        ctx.shared = (theta.dim() == 1, pos_scores.dim() == 2)
        ctx.like = (theta, pos_scores, arc_scores)
        ctx.save_for_backward(r.pos_posterior, r.arc_posterior)
        return r.logz

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        pp, ap = ctx.saved_tensors
        nt, npos, na = ctx.needs_input_grad[1:4]
        theta, pos_scores, arc_scores = ctx.like
        g = g.to(torch.float32)
        d_theta = d_pos = d_arc = None
        if nt:
            d_theta = _per_label(pp.sum(dim=1), g, ctx.shared[0]).to(theta.dtype)
        if npos:
            d_pos = _per_position(pp, g, pos_scores)
        if na:
            d_arc = _per_arc(ctx.lat, ap, g).to(arc_scores.dtype)
        return None, d_theta, d_pos, d_arc


def positional_log_z(lat: LatticeBatch, theta: torch.Tensor, pos_scores: torch.Tensor,
                     arc_scores: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable exact log Z_T per lattice, float32 [B], under per-position scores ``pos_scores`` [T, V] or
    [B, T, V] (see ``positional_forward_backward``).  Gradients: ``pos_scores`` gets the position posteriors, ``theta``
    their sums over the positions, ``arc_scores`` the arc posteriors (each summed over the lattices for a shared
    tensor).  First derivatives only: a second backward raises.  The Hessian-vector product of log Z_T with
    (u_pos, u_theta, u_arc) is ``positional_expectation_terms(..., pos_values=u_pos, label_values=u_theta,
    arc_values=u_arc, want_pos_cov=True, want_arc_cov=True).pos_cov / .arc_cov``."""
    _need_gpu(lat)
    theta = _input(lat, theta, "theta", True, False)
    arc_scores = _input(lat, arc_scores, "arc_scores", False, True)
    if pos_scores is None:
        raise ValueError("positional_log_z needs pos_scores; without them use log_z")
    _positions(lat, pos_scores, None)
    return _PositionalLogZ.apply(lat, theta, pos_scores, arc_scores)


def length_distribution(lat: LatticeBatch, theta, T: Optional[int] = None, arc_scores=None):
    """(``log_p`` [B, T + 1] float64, ``logz64`` [B]): log P(the path has exactly L arcs) under truncation at ``T`` arcs
    (``T`` defaults to the longest path of the batch: no truncation), and the log Z over the paths that fit.  Entry 0 is
    -inf; a lattice without a path within ``T`` gets NaN-free -inf everywhere."""
    r = positional_forward_backward(lat, theta, None, T, arc_scores, want_pos_posterior=False, want_len=True)
    z = r.logz64[:, None]
    return torch.where(torch.isfinite(z), r.len_logz - z, torch.full_like(r.len_logz, float("-inf"))), r.logz64


# ----------------------------------------------------------------------------- expectations under positional scores
class PositionalExpectationResult(NamedTuple):
    logz64: torch.Tensor  # [B] float64 log Z_T
    logz: torch.Tensor  # [B] float32
    ev64: torch.Tensor  # [B] float64 E[V]
    ev: torch.Tensor  # [B] float32
    pos_posterior: Optional[torch.Tensor]  # [B, T, V] float32, the bits of positional_forward_backward
    arc_posterior: Optional[torch.Tensor]  # [total_arcs] float32, the bits of positional_forward_backward
    pos_cov: Optional[torch.Tensor]  # [B, T, V] float32: per label, the sum of c_{a,t} = P(a at t) (E[V | a at t] - E[V])
    arc_cov: Optional[torch.Tensor]  # [total_arcs] float32: the sum over t of c_{a,t}


def _position_values(lat: LatticeBatch, t, T: int, name: str):
    """(``t`` as contiguous float32 or None, its stride) of a per-position value tensor with the ``T`` of the call."""
    return (None, 0) if t is None else _position_tensor(lat, t, name, T)


def positional_expectation_plan(lat: LatticeBatch) -> tuple:
    """(``lds_bytes``, ``staged``) of the launch ``positional_expectation_terms`` makes for this batch
    (``nfst_positional_expectation_plan``, the rule the launcher itself calls), as ``positional_plan``: asked on the host,
    no GPU needed; a batch beyond the op's LDS limit raises ``NfstError`` (-6), as the op would."""
    return _positional_plan(lat, "nfst_positional_expectation_plan")


def positional_expectation_terms(lat: LatticeBatch, theta, pos_scores=None, T: Optional[int] = None, arc_scores=None,
                                 pos_values=None, label_values=None, arc_values=None, score_coef: float = 0.0,
                                 want_pos_posterior: bool = False, want_arc_posterior: bool = False, want_pos_cov: bool = False,
                                 want_arc_cov: bool = False) -> PositionalExpectationResult:
    """One launch of ``nfst_positional_expectation`` (no autograd; DESIGN.md sections 2 and 4.13): under the distribution
    p_T of ``positional_forward_backward`` (same ``theta``, ``pos_scores``, ``T``, ``arc_scores``), with the arc at
    position t of a path carrying  v_t(a) = pos_values[(b,) t, label] + label_values[(b,) label] + arc_values[a] +
    score_coef * (s_a + pos_scores[(b,) t, label])  (each term optional), log Z_T, E[V] and on request the posteriors (the
    bits of ``positional_forward_backward``), ``pos_cov`` and ``arc_cov``: the covariance of every (position, label) and
    of every arc with V.  For values that do not depend on the scores ``pos_cov`` / ``arc_cov`` are the Hessian of
    log Z_T times the values.  Value entries behind a score of -inf are never read.  The workspace stores every
    (beta, R) row of every position: 20 (T + 1) total_rows bytes."""
    _need_gpu(lat)
    theta = _input(lat, theta, "theta", True, False)
    arc_scores = _input(lat, arc_scores, "arc_scores", False, True)
    label_values = _input(lat, label_values, "label_values", True, False)
    arc_values = _input(lat, arc_values, "arc_values", False, True)
    pos, stride, T = _positions(lat, pos_scores, T)
    pv, pv_stride = _position_values(lat, pos_values, T, "pos_values")
    coef = float(score_coef)
    if coef != coef or coef in (float("inf"), float("-inf")):
        raise ValueError(f"score_coef must be finite, not {score_coef}")
    sc, keep = _scores(lat, theta, arc_scores)
    dev = lat.device
    B, A, V = lat.n_lattices, lat.total_arcs, lat.vocab
    ws, ws_bytes = _workspace(lat, "nfst_positional_expectation_ws_bytes", T)
    f32 = dict(dtype=torch.float32, device=dev)
    z64 = torch.empty(B, dtype=torch.float64, device=dev)
    ev64 = torch.empty(B, dtype=torch.float64, device=dev)
    z32, ev32 = torch.empty(B, **f32), torch.empty(B, **f32)
    pp = torch.empty((B, T, V), **f32) if want_pos_posterior else None
    ap = torch.empty(A, **f32) if want_arc_posterior else None
    pc = torch.empty((B, T, V), **f32) if want_pos_cov else None
    ac = torch.empty(A, **f32) if want_arc_cov else None
    lv_stride = 0 if label_values is None or label_values.dim() == 1 else V
    _call("nfst_positional_expectation", lat, sc, pos, stride, T, pv, pv_stride, label_values, lv_stride, arc_values, coef,
          ws, ws_bytes, z64, z32, ev64, ev32, pp, ap, pc, ac)
    return PositionalExpectationResult(z64, z32, ev64, ev32, pp, ap, pc, ac)


class _PositionalExpectation(torch.autograd.Function):
    """E[V] with d/d pos_scores = pos_cov + coef pos_post, d/d theta its sums over t, d/d arc_scores = arc_cov + coef
    arc_post, d/d pos_values = pos_post, d/d label_values its sums over t, d/d arc_values = arc_post."""

    @staticmethod
    def forward(ctx, lat, theta, pos_scores, arc_scores, pos_values, label_values, arc_values, coef, T):
        nt, npos, na, npv, nlv, nav = ctx.needs_input_grad[1:7]
        k = coef != 0.0
        r = positional_expectation_terms(lat, theta.detach(), _det(pos_scores), T, _det(arc_scores), _det(pos_values),
                                         _det(label_values), _det(arc_values), coef,
                                         want_pos_posterior=npv or nlv or (k and (nt or npos)), want_arc_posterior=nav or (k and na),
                                         want_pos_cov=nt or npos, want_arc_cov=na)
        ctx.lat, ctx.coef = lat, coef
        ctx.like = (theta, pos_scores, arc_scores, pos_values, label_values, arc_values)
        ctx.save_for_backward(r.pos_posterior, r.arc_posterior, r.pos_cov, r.arc_cov)
        return r.ev

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        pp, ap, pc, ac = ctx.saved_tensors
        nt, npos, na, npv, nlv, nav = ctx.needs_input_grad[1:7]
        theta, pos_scores, arc_scores, pos_values, label_values, arc_values = ctx.like
        k = ctx.coef
        g = g.to(torch.float32)
        ga = _arc_grad(ctx.lat, g) if (na or nav) else None
        d_theta = d_pos = d_arc = d_pv = d_lv = d_av = None
        if nt or npos:
            ds = pc if k == 0.0 else pc + k * pp
            if nt:
                d_theta = _per_label(ds.sum(dim=1), g, theta.dim() == 1).to(theta.dtype)
            if npos:
                d_pos = _per_position(ds, g, pos_scores)
        if na:
            d_arc = ((ac if k == 0.0 else ac + k * ap) * ga).to(arc_scores.dtype)
        if npv:
            d_pv = _per_position(pp, g, pos_values)
        if nlv:
            d_lv = _per_label(pp.sum(dim=1), g, label_values.dim() == 1).to(label_values.dtype)
        if nav:
            d_av = (ap * ga).to(arc_values.dtype)
        return None, d_theta, d_pos, d_arc, d_pv, d_lv, d_av, None, None


def positional_expectation(lat: LatticeBatch, theta: torch.Tensor, pos_scores: Optional[torch.Tensor] = None,
                           T: Optional[int] = None, arc_scores: Optional[torch.Tensor] = None,
                           pos_values: Optional[torch.Tensor] = None, label_values: Optional[torch.Tensor] = None,
                           arc_values: Optional[torch.Tensor] = None, score_coef: float = 0.0) -> torch.Tensor:
    """Exact E_{p_T}[V] per lattice, float32 [B], under per-position scores (see ``positional_expectation_terms``):
    expected cost of a tagger's output against a gold sequence (``pos_values = cost[b, t, label]``: minimum-risk
    training, expected Hamming loss), expected length (``label_values`` = ones), expected label counts.  Differentiable
    in ``theta``, ``pos_scores``, ``arc_scores``, ``pos_values``, ``label_values`` and ``arc_values`` (each gradient
    summed over the lattices for a shared tensor); one launch, first derivatives only."""
    _need_gpu(lat)
    _input(lat, theta, "theta", True, False)
    return _PositionalExpectation.apply(lat, theta, pos_scores, arc_scores, pos_values, label_values, arc_values,
                                        float(score_coef), T)


class _PositionalEntropy(torch.autograd.Function):
    """H(p_T) = log Z_T - E[S] from one launch with score_coef = 1; dH/d(score) = -c."""

    @staticmethod
    def forward(ctx, lat, theta, pos_scores, arc_scores, T):
        nt, npos, na = ctx.needs_input_grad[1:4]
        r = positional_expectation_terms(lat, theta.detach(), _det(pos_scores), T, _det(arc_scores), score_coef=1.0,
                                         want_pos_cov=nt or npos, want_arc_cov=na)
        ctx.lat = lat
        ctx.like = (theta, pos_scores, arc_scores)
        ctx.save_for_backward(r.pos_cov, r.arc_cov)
        return (r.logz64 - r.ev64).to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        pc, ac = ctx.saved_tensors
        nt, npos, na = ctx.needs_input_grad[1:4]
        theta, pos_scores, arc_scores = ctx.like
        g = -g.to(torch.float32)
        d_theta = _per_label(pc.sum(dim=1), g, theta.dim() == 1).to(theta.dtype) if nt else None
        d_pos = _per_position(pc, g, pos_scores) if npos else None
        d_arc = _per_arc(ctx.lat, ac, g).to(arc_scores.dtype) if na else None
        return None, d_theta, d_pos, d_arc, None


def positional_entropy(lat: LatticeBatch, theta: torch.Tensor, pos_scores: Optional[torch.Tensor] = None,
                       T: Optional[int] = None, arc_scores: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Exact entropy H(p_T) = log Z_T - E[S] per lattice, float32 [B] (nats; the difference is taken in float64), of the
    distribution over the paths of at most ``T`` arcs under per-position scores.  Differentiable in ``theta``,
    ``pos_scores`` and ``arc_scores``: dH/d(score) = -Cov(1[arc at t], S).  A lattice without a path within ``T`` gets
    NaN-free -inf."""
    _need_gpu(lat)
    _input(lat, theta, "theta", True, False)
    return _PositionalEntropy.apply(lat, theta, pos_scores, arc_scores, T)


def _diff(p, q):
    """p - q in float32 where either may be None (None when both are)."""
    if p is None and q is None:
        return None
    if q is None:
        return p.to(torch.float32)
    return (p.to(torch.float32) if p is not None else 0.0) - q.to(torch.float32)


class _PositionalKL(torch.autograd.Function):
    """KL(p_T || q_T) = log Z_q - log Z_p + E_p[S_p - S_q] (arc_w cancels); d/d(scores of p) = c(v = S_p - S_q),
    d/d(scores of q) = post_q - post_p."""

    @staticmethod
    def forward(ctx, lat, theta_p, pos_p, theta_q, pos_q, arc_scores_p, arc_scores_q, T):
        ntp, npp, ntq, npq, nap, naq = ctx.needs_input_grad[1:7]
        tp, tq, pp_, pq_ = theta_p.detach(), theta_q.detach(), _det(pos_p), _det(pos_q)
        asp, asq = _det(arc_scores_p), _det(arc_scores_q)
        for name, t in (("theta_p", tp), ("theta_q", tq)):
            _input(lat, t, name, True, False)
        for name, t in (("arc_scores_p", asp), ("arc_scores_q", asq)):
            _input(lat, t, name, False, True)
        _, _, T = _positions(lat, pp_ if pp_ is not None else pq_, T)
        _positions(lat, pq_, T)
        # (-inf - -inf is NaN and finite - -inf is +inf: behind a weight of zero under p neither is read; where p has mass
        # on something q forbids the result is +inf or NaN, the caller's business)
        rp = positional_expectation_terms(lat, tp, pp_, T, asp, _diff(pp_, pq_), _diff(tp, tq), _diff(asp, asq), 0.0,
                                          want_pos_posterior=ntq or npq, want_arc_posterior=naq, want_pos_cov=ntp or npp,
                                          want_arc_cov=nap)
        rq = positional_forward_backward(lat, tq, pq_, T, asq, want_pos_posterior=ntq or npq, want_arc_posterior=naq)
        ctx.lat = lat
        ctx.like = (theta_p, pos_p, theta_q, pos_q, arc_scores_p, arc_scores_q)
        ctx.save_for_backward(rp.pos_cov, rp.arc_cov, rp.pos_posterior, rp.arc_posterior, rq.pos_posterior, rq.arc_posterior)
        return (rq.logz64 - rp.logz64 + rp.ev64).to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        pc, ac, pp_p, ap_p, pp_q, ap_q = ctx.saved_tensors
        ntp, npp, ntq, npq, nap, naq = ctx.needs_input_grad[1:7]
        theta_p, pos_p, theta_q, pos_q, asp, asq = ctx.like
        g = g.to(torch.float32)
        ga = _arc_grad(ctx.lat, g) if (nap or naq) else None
        dq = pp_q - pp_p if (ntq or npq) else None
        return (None,
                _per_label(pc.sum(dim=1), g, theta_p.dim() == 1).to(theta_p.dtype) if ntp else None,
                _per_position(pc, g, pos_p) if npp else None,
                _per_label(dq.sum(dim=1), g, theta_q.dim() == 1).to(theta_q.dtype) if ntq else None,
                _per_position(dq, g, pos_q) if npq else None,
                (ac * ga).to(asp.dtype) if nap else None,
                ((ap_q - ap_p) * ga).to(asq.dtype) if naq else None, None)


def positional_kl_divergence(lat: LatticeBatch, theta_p: torch.Tensor, pos_p: Optional[torch.Tensor], theta_q: torch.Tensor,
                             pos_q: Optional[torch.Tensor], T: Optional[int] = None,
                             arc_scores_p: Optional[torch.Tensor] = None,
                             arc_scores_q: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Exact KL(p_T || q_T) per lattice, float32 [B], of two positional models over the paths of at most ``T`` arcs of
    the same batch (distillation): log Z_q - log Z_p + E_p[S_p - S_q], combined in float64.  One expectation launch under
    p (values ``pos_p - pos_q``, ``theta_p - theta_q`` and the arc-score difference) and one ``nfst_positional`` launch
    under q.  Differentiable in all six score inputs: d/d(scores of p) = Cov_p(1[arc at t], S_p - S_q), d/d(scores of q)
    = post_q - post_p -- exactly zero at q = p, the two launches write the same posterior bits.  Where p puts mass on
    something q forbids (-inf) the result is +inf or NaN: the caller's business, nothing scans for it."""
    _need_gpu(lat)
    return _PositionalKL.apply(lat, theta_p, pos_p, theta_q, pos_q, arc_scores_p, arc_scores_q, T)


def positional_viterbi(lat: LatticeBatch, theta, pos_scores=None, T: Optional[int] = None, arc_scores=None,
                       pad: int = 0) -> PositionalViterbiResult:
    """The best path of at most ``T`` arcs under per-position scores (``nfst_positional_viterbi``): plain float32
    max-plus from position T backwards, ties to the smaller canonical arc.  Without ``pos_scores`` and with ``T`` >= the
    longest path it is ``k_best(k=1)`` bit for bit.  A lattice without a path of finite score within ``T`` gets
    ``best`` -inf and length 0.  Not differentiable."""
    _need_gpu(lat)
    sc, keep, pos, stride, T = _score_args(lat, theta, arc_scores, pos_scores, T)
    ws, ws_bytes = _positional_ws(lat, T, 2)
    best, paths, arcs, lens, _, _ = _path_outputs(lat, (lat.n_lattices,), T, best=True)
    _call("nfst_positional_viterbi", lat, sc, pos, stride, T, ws, ws_bytes, best, paths, arcs, lens, int(pad))
    return PositionalViterbiResult(best, paths, arcs, lens)


class PositionalKBestResult(NamedTuple):
    best: torch.Tensor  # [B, k] float32, non-increasing; -inf beyond n_paths
    paths: torch.Tensor  # [B, k, T] int32 labels (bos .. eos), pad-terminated
    arcs: torch.Tensor  # [B, k, T] int32 canonical arc ids, -1 padded
    lengths: torch.Tensor  # [B, k] int32 arcs per path (0 beyond n_paths)
    n_paths: torch.Tensor  # [B] int32 min(k, paths of at most T arcs and score > -inf)


def positional_k_best_terms(lat: LatticeBatch, theta, k: int, pos_scores=None, T: Optional[int] = None, arc_scores=None,
                            pad: int = 0) -> PositionalKBestResult:
    """One launch of ``nfst_positional_kbest`` (no autograd); see ``positional_k_best``."""
    _need_gpu(lat)
    _check_k(k)
    sc, keep, pos, stride, T = _score_args(lat, theta, arc_scores, pos_scores, T)
    ws, ws_bytes = _workspace(lat, "nfst_positional_kbest_ws_bytes", T, k)
    best, paths, arcs, lens, n_paths, _ = _path_outputs(lat, (lat.n_lattices, k), T, best=True, n_paths=True)
    _call("nfst_positional_kbest", lat, sc, pos, stride, T, k, ws, ws_bytes, best, paths, arcs, lens, n_paths, int(pad))
    return PositionalKBestResult(best, paths, arcs, lens, n_paths)


class _PositionalKBest(torch.autograd.Function):
    """best[b, j] = the sum of the terms of path j: d/d arc_scores[a] = 1 on its arcs, d/d theta counts its labels,
    d/d pos_scores marks (t, label) of each of its positions (each summed over the lattices for a shared tensor);
    -inf entries (no path) get no gradient."""

    @staticmethod
    def forward(ctx, lat, theta, pos_scores, arc_scores, k, T, pad):
        r = positional_k_best_terms(lat, theta, k, pos_scores, T, arc_scores, pad)
        ctx.lat = lat
        ctx.like = (theta, pos_scores, arc_scores)
        ctx.save_for_backward(r.arcs)
        ctx.mark_non_differentiable(r.paths, r.arcs, r.lengths, r.n_paths)
        return r.best, r.paths, r.arcs, r.lengths, r.n_paths

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *_):
        (arcs,) = ctx.saved_tensors
        nt, npos, na = ctx.needs_input_grad[1:4]
        theta, pos_scores, arc_scores = ctx.like
        d_theta, d_arc, d_pos = _path_score_grads(ctx.lat, arcs, g, theta if nt else None, arc_scores if na else None,
                                                  pos_scores if npos else None)
        return None, d_theta, d_pos, d_arc, None, None, None


def positional_k_best(lat: LatticeBatch, theta, k: int, pos_scores=None, T: Optional[int] = None, arc_scores=None,
                      pad: int = 0) -> PositionalKBestResult:
    """The k best paths of at most ``T`` arcs under per-position scores, exact (``nfst_positional_kbest``, DESIGN.md
    sections 2 and 4.12): the n-best list a reranker consumes when the scores are a tagger's or encoder's logits
    ``pos_scores`` [T, V] or [B, T, V] on top of ``theta`` [V] or [B, V] and ``arc_scores`` [total_arcs]; 1 <= k <= 64.
    ``T`` defaults to ``pos_scores.shape[-2]``, without ``pos_scores`` to the longest path of the batch.  Entry 0 is
    ``positional_viterbi``'s path bit for bit; without ``pos_scores`` and with ``T`` >= the longest path every output is
    ``k_best``'s.  Ties on exactly equal scores go to the smaller canonical arc, then the smaller rank.  Lattices with
    fewer than k paths of score > -inf within ``T`` fill the rest with score -inf, length 0, ``pad`` labels and arc -1
    (``n_paths`` counts the real ones).  The workspace holds every list of every position: (8 k + 1) (T + 1) total_rows bytes.
    ``best`` is differentiable in theta, arc_scores and pos_scores (first derivatives only): the gradient of a path's
    score counts its labels, marks its arcs and marks (t, label) of each of its positions."""
    _need_gpu(lat)
    _check_k(k)
    theta = _input(lat, theta, "theta", True, False)
    arc_scores = _input(lat, arc_scores, "arc_scores", False, True)
    _positions(lat, pos_scores, T)
    return PositionalKBestResult(*_PositionalKBest.apply(lat, theta, pos_scores, arc_scores, k, T, pad))


class PositionalSampleResult(NamedTuple):
    paths: torch.Tensor  # [B, K, T] int32 labels, pad-terminated
    arcs: Optional[torch.Tensor]  # [B, K, T] int32 canonical arc ids, -1 padded (None with want_arcs=False)
    lengths: torch.Tensor  # [B, K] int32 (0 where logz is -inf)
    logq: torch.Tensor  # [B, K] float32 = S_T(path) - log Z_T (0 where logz is -inf)
    logz: torch.Tensor  # [B] float32 log Z_T
    logz64: torch.Tensor  # [B] float64: the bits of positional_forward_backward


def positional_sample_paths(lat: LatticeBatch, theta, k: int, pos_scores=None, T: Optional[int] = None, arc_scores=None,
                            uniforms: Optional[torch.Tensor] = None, seed: int = 0, pad: int = 0,
                            want_arcs: bool = True) -> PositionalSampleResult:
    """``k`` exact draws per lattice from p_T(path) = exp(S_T(path)) / Z_T over the paths of at most ``T`` arcs, under
    the scores of ``positional_forward_backward`` (``nfst_positional_sample``; DESIGN.md sections 2 and 4.10).  No draw
    overruns ``T`` and nothing is truncated: there is no "ran out of length budget".  ``logq`` is each draw's exact
    log-probability.  ``uniforms`` [B, k, T] float32 in [0, 1) decide the walks (walk (b, j) reads its own row only);
    without them Philox4x32-10 keyed by ``seed``, as ``sample_paths``.  A lattice without a path of finite score within
    ``T`` gets length 0, ``pad`` labels and ``logq`` 0.  One backward pass (every beta row stored: 12 (T + 1) total_rows
    bytes of workspace) and one wave per walk; the same bits at every launch and for every packing.  Not
    differentiable."""
    _need_gpu(lat)
    _check_k(k, bounded=False)
    sc, keep, pos, stride, T = _score_args(lat, theta, arc_scores, pos_scores, T)
    dev = lat.device
    B = lat.n_lattices
    if uniforms is not None:
        if not isinstance(uniforms, torch.Tensor) or tuple(uniforms.shape) != (B, k, T):
            raise ValueError(f"uniforms must be a tensor of shape [{B}, {k}, {T}]")
        uniforms = uniforms.detach().to(device=dev, dtype=torch.float32).contiguous()
    ws, ws_bytes = _positional_ws(lat, T, _lib.POS_WS_SAMPLE)
    z64 = torch.empty(B, dtype=torch.float64, device=dev)
    z32 = torch.empty(B, dtype=torch.float32, device=dev)
    _, paths, arcs, lens, _, logq = _path_outputs(lat, (B, k), T, arcs=want_arcs, logq=True)
    _call("nfst_positional_sample", lat, sc, pos, stride, T, k, uniforms, C.c_uint64(seed & (2 ** 64 - 1)), int(pad), ws, ws_bytes,
          z64, z32, paths, arcs, lens, logq)
    return PositionalSampleResult(paths, arcs, lens, logq, z32, z64)


def positional_score_paths(lat: LatticeBatch, theta, marks: torch.Tensor, pos_scores=None, T: Optional[int] = None,
                           arc_scores=None):
    """Forced walk of ``marks`` [B, K, T] (pad-terminated labels) under the scores of ``positional_forward_backward``
    (``nfst_positional_score_paths``): (``path_score`` [B, K] float32 -- -inf if a mark has no arc or an entry is -inf,
    ``end_state`` [B, K] -- 0 if the walk fell off the lattice, ``lengths`` [B, K] -- the marks before the first pad).
    ``T`` defaults to ``pos_scores.shape[-2]``, without ``pos_scores`` to ``marks.shape[-1]``.  The log p side of an
    importance weight whose log q is ``positional_sample_paths``'s.  Not differentiable."""
    _need_gpu(lat)
    theta = _input(lat, theta, "theta", True, False)
    arc_scores = _input(lat, arc_scores, "arc_scores", False, True)
    if not isinstance(marks, torch.Tensor) or marks.dim() != 3 or marks.shape[0] != lat.n_lattices or marks.shape[1] < 1 \
            or marks.is_floating_point():
        raise ValueError(f"marks must be an integer tensor [{lat.n_lattices}, K, T] with K >= 1")
    if pos_scores is None and T is None:
        T = int(marks.shape[2])
    pos, stride, T = _positions(lat, pos_scores, T)
    if marks.shape[2] != T:
        raise ValueError(f"marks has {marks.shape[2]} positions, T = {T}")
    sc, keep = _scores(lat, theta.detach(), _det(arc_scores))
    pos = _det(pos)
    marks = marks.to(device=lat.device, dtype=torch.int32).contiguous()
    B, K = int(marks.shape[0]), int(marks.shape[1])
    tot = torch.empty((B, K), dtype=torch.float32, device=lat.device)
    end = torch.empty((B, K), dtype=torch.int32, device=lat.device)
    lens = torch.empty((B, K), dtype=torch.int32, device=lat.device)
    _call("nfst_positional_score_paths", lat, sc, pos, stride, T, marks, K, tot, end, lens)
    return tot, end, lens


class SampleResult(NamedTuple):
    paths: torch.Tensor  # [B, K, max_len] int32 labels, pad-terminated
    arcs: torch.Tensor  # [B, K, max_len] int32 canonical arc ids
    lengths: torch.Tensor  # [B, K]
    logq: torch.Tensor  # [B, K] float32 = path score - log Z
    logz: torch.Tensor  # [B] float32


def sample_paths(lat: LatticeBatch, theta, k: int, arc_scores=None, max_len: Optional[int] = None,
                 uniforms: Optional[torch.Tensor] = None, seed: int = 0, pad: int = 0,
                 beta: Optional[BackwardResult] = None, want_arcs: bool = True) -> SampleResult:
    """K exact posterior samples per lattice (Sampler.sample, modules/samplers.py:137-335,
    with the exact posterior as proposal).  ``want_arcs=False`` leaves ``arcs`` None (the C entry
    point's path_arcs is optional; with it the kernel precomputes every arc's probability once per
    block, without it a walk computes the probabilities of the arcs it meets)."""
    _need_gpu(lat)
    sc, keep = _scores(lat, theta, arc_scores)
    max_len = _max_len(lat, max_len)
    if beta is None or beta.beta_me is None:
        beta = backward(lat, theta, arc_scores, want_logbeta=False, want_me=True)
    dev = lat.device
    B = lat.n_lattices
    if uniforms is not None:
        uniforms = uniforms.to(device=dev, dtype=torch.float32).contiguous()
        if uniforms.shape != (B, k, max_len):
            raise ValueError(f"uniforms must be [{B}, {k}, {max_len}]")
    _, paths, arcs, lens, _, logq = _path_outputs(lat, (B, k), max_len, arcs=want_arcs, logq=True)
    status = torch.zeros(1, dtype=torch.int32, device=lat.device)
    _call("nfst_sample_paths", lat, sc, beta.beta_me, beta.logz64, int(k), int(max_len), uniforms, C.c_uint64(seed & (2 ** 64 - 1)),
          int(pad), paths, arcs, lens, logq, status)
    _raise_status(status, "nfst_sample_paths")  # "ran out of length budget" (samplers.py:299-302)
    return SampleResult(paths, arcs, lens, logq, beta.logz)


def score_paths(lat: LatticeBatch, theta, marks: torch.Tensor, arc_scores=None):
    """Forced walk of marks [B, K, T] (samplers.py:208-218): (path_score [B,K], end_state [B,K])."""
    _need_gpu(lat)
    sc, keep = _scores(lat, theta, arc_scores)
    marks = marks.to(device=lat.device, dtype=torch.int32).contiguous()
    B, K, T = marks.shape
    if B != lat.n_lattices:
        raise ValueError("marks must be [B, K, T]")
    tot = torch.empty((B, K), dtype=torch.float32, device=lat.device)
    end = torch.empty((B, K), dtype=torch.int32, device=lat.device)
    _call("nfst_score_paths", lat, sc, marks, K, T, tot, end)
    return tot, end


def _walkers(lat: LatticeBatch, x: torch.Tensor, k: int, name: str) -> torch.Tensor:
    x = x.to(device=lat.device, dtype=torch.int64).contiguous()
    if x.shape != (lat.n_lattices * k,):
        raise ValueError(f"{name} must be [B*k] = [{lat.n_lattices * k}]")
    return x


def step(lat: LatticeBatch, state: torch.Tensor, label: torch.Tensor, k: int = 1) -> torch.Tensor:
    """state' = transition[state, label] (FSAGRUScorer.update_fsa_state, scorers.py:683-690)."""
    _need_gpu(lat)
    state, label = _walkers(lat, state, k, "state"), _walkers(lat, label, k, "label")
    out = torch.empty_like(state)
    _call("nfst_step", lat, state, label, out, int(k))
    return out


def emission_mask(lat: LatticeBatch, state: torch.Tensor, k: int = 1, inp: Optional[torch.Tensor] = None,
                  pad: int = 0, bos: int = 1, eos: int = 2, has_to_end: bool = False) -> torch.Tensor:
    """[B*k, V] mask of FSAGRUScorer.mask_out_invalid (scorers.py:1037-1054); with
    ``inp`` the bos/pad/eos legality masks (scorers.py:59-83) are fused in."""
    _need_gpu(lat)
    state = _walkers(lat, state, k, "state")
    if inp is not None:
        inp = _walkers(lat, inp, k, "inp")
    out = torch.empty((state.shape[0], lat.vocab), dtype=torch.float32, device=lat.device)
    _call("nfst_emission_mask", lat, state, inp, int(pad), int(bos), int(eos), int(bool(has_to_end)), out, int(k))
    return out


def beta_logits(lat: LatticeBatch, values: torch.Tensor, state: torch.Tensor, k: int = 1) -> torch.Tensor:
    """[B*k, V] = values[transition[state, :]] (GRUScorer beta-logit gather, scorers.py:581-593)."""
    _need_gpu(lat)
    state = _walkers(lat, state, k, "state")
    values = values.to(device=lat.device, dtype=torch.float32).contiguous().reshape(-1)
    if values.shape[0] != lat.total_rows:
        raise ValueError("values must be row-indexed [total_rows]")
    out = torch.empty((state.shape[0], lat.vocab), dtype=torch.float32, device=lat.device)
    _call("nfst_beta_logits", lat, values, state, out, int(k))
    return out


class ProposalStep(NamedTuple):
    symbol: torch.Tensor      # [N] int64
    logq: torch.Tensor        # [N] float32: log probability of the symbol
    logz: torch.Tensor        # [N] float32: logsumexp of the masked logits
    next_state: torch.Tensor  # [N] int64


class StepPenalties:
    """The per-walker counters and the constants of the insertion / length penalties of
    ``FSAGRUScorer.actual_left_to_right_score`` (scorers.py:654-677; defaults as its constructor, 930-933).
    ``accumulated`` [N] and ``vocab_use`` [N, V] are updated in place by every ``proposal_step``."""

    def __init__(self, n_walkers: int, vocab: int, device, insertion_mark: int, insert_threshold: int = 2,
                 insert_penalty: float = 1000.0, length_threshold: int = 0, length_penalty: float = 1000.0):
        self.accumulated = torch.zeros(n_walkers, dtype=torch.int64, device=device)
        self.vocab_use = torch.zeros(n_walkers, vocab, dtype=torch.float32, device=device)
        self.insertion_mark, self.insert_threshold, self.insert_penalty = int(insertion_mark), int(insert_threshold), float(insert_penalty)
        self.length_threshold, self.length_penalty = int(length_threshold), float(length_penalty)


class _ProposalStep(torch.autograd.Function):
    """(logq, logz) differentiable in ``scores`` (and ``values``): d logq / d scores = (onehot(symbol) -
    softmax(masked logits)) / T, as the reference's ``Categorical.log_prob`` (samplers.py:256-273)."""

    @staticmethod
    def forward(ctx, lat, scores, values, cfg):
        (state, inp, pad, bos, eos, has_to_end, temperature, uniforms, forced, extras, vstate, k, out) = cfg
        N, dev = state.shape[0], lat.device
        # (False under torch.no_grad(): a sampling loop with trainable proposal parameters then writes no [N, V] logits)
        need = ctx.needs_input_grad[1] or (values is not None and ctx.needs_input_grad[2])
        if out is not None:
            sym, logq, logz, nxt = out
        else:
            sym = torch.empty(N, dtype=torch.int64, device=dev)
            nxt = torch.empty(N, dtype=torch.int64, device=dev)
            logq = torch.empty(N, dtype=torch.float32, device=dev)
            logz = torch.empty(N, dtype=torch.float32, device=dev)
        logits = torch.empty(N, lat.vocab, dtype=torch.float32, device=dev) if need else None
        _call("nfst_proposal_step", lat, state, inp, scores, values, int(pad), int(bos), int(eos), int(bool(has_to_end)),
              float(temperature), uniforms, forced, extras, sym, logq, logz, nxt, logits, int(k))
        ctx.lat, ctx.k, ctx.pad, ctx.temperature = lat, k, pad, temperature
        ctx.need_values = values is not None and values.requires_grad
        ctx.n_values = 0 if values is None else values.shape[0]
        ctx.save_for_backward(logits, sym, logz, vstate)
        ctx.mark_non_differentiable(sym, nxt)
        return sym, logq, logz, nxt

    @staticmethod
    def backward(ctx, _gs, g_logq, g_logz, _gn):
        logits, sym, logz, vstate = ctx.saved_tensors
        lat = ctx.lat
        g_logq = None if g_logq is None else g_logq.to(torch.float32).contiguous()
        g_logz = None if g_logz is None else g_logz.to(torch.float32).contiguous()
        grad = torch.empty_like(logits)
        gv = torch.zeros(ctx.n_values, dtype=torch.float32, device=logits.device) if ctx.need_values else None
        _call("nfst_proposal_step_backward", lat, vstate, logits, sym, logz, g_logq, g_logz, int(ctx.pad), float(ctx.temperature),
              grad, gv, int(ctx.k))
        return None, grad, gv, None


def proposal_step(lat: LatticeBatch, state: torch.Tensor, scores: torch.Tensor, k: int = 1,
                  inp: Optional[torch.Tensor] = None, values: Optional[torch.Tensor] = None, pad: int = 0, bos: int = 1,
                  eos: int = 2, has_to_end: bool = False, temperature: float = 1.0,
                  uniforms: Optional[torch.Tensor] = None, forced: Optional[torch.Tensor] = None,
                  value_state: Optional[torch.Tensor] = None, penalties: Optional[StepPenalties] = None,
                  length: int = 1, out=None, not_pad: Optional[torch.Tensor] = None) -> ProposalStep:
    """One step of the reference's proposal sampler on the lattice side, fused
    (Sampler.stateful_sample, samplers.py:243-297: left_to_right_score + mask_out_invalid +
    Categorical sample / log_prob + update_fsa_state).  ``scores`` [N, V] are the proposal
    network's outputs for this step; ``values`` (row-indexed, e.g. beta) are added through the
    next-state gather of scorers.py:581-593 -- out of ``value_state`` if given (the reference reads the
    row of the state before the previous symbol was consumed), else out of ``state``; ``penalties``
    carries the insertion / length penalty counters (scorers.py:654-677) and ``length`` is the step's
    metadata["length"]; ``uniforms`` [N] drive the inverse-CDF draw, or ``forced`` [N] gives the symbols
    to evaluate.  ``logq`` and ``logz`` are differentiable in ``scores`` and ``values``.
    ``out`` = (symbol, logq, logz, next_state) tensors of a previous call or rows of buffers allocated once per
    sampling loop; ``not_pad``: an int32 device word (zeroed by the caller) that receives the number of walkers
    whose symbol is not ``pad`` (zero: every walker has ended)."""
    _need_gpu(lat)
    state = _walkers(lat, state, k, "state")
    N = state.shape[0]
    dev = lat.device
    scores = scores.to(device=dev, dtype=torch.float32).contiguous()
    if tuple(scores.shape) != (N, lat.vocab):
        raise ValueError("scores must be [n_lattices * k, vocab]")
    if inp is not None:
        inp = _walkers(lat, inp, k, "inp")
    if values is not None:
        values = values.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
        if values.shape[0] != lat.total_rows:
            raise ValueError("values must be row-indexed [total_rows]")
    if uniforms is None and forced is None:
        uniforms = torch.rand(N, device=dev)
    if uniforms is not None:
        uniforms = uniforms.to(device=dev, dtype=torch.float32).contiguous().reshape(N)
    if forced is not None:
        forced = forced.to(device=dev, dtype=torch.int64).contiguous().reshape(N)
    extras = None
    if not_pad is not None and (not_pad.dtype != torch.int32 or not_pad.numel() != 1 or not_pad.device != dev):
        raise ValueError("not_pad must be one int32 word on the batch's device")
    if out is not None:
        want = ((torch.int64, "symbol"), (torch.float32, "logq"), (torch.float32, "logz"), (torch.int64, "next_state"))
        if len(out) != 4 or any(o.dtype != d or o.shape != (N,) or o.device != dev or not o.is_contiguous() for o, (d, _) in zip(out, want)):
            raise ValueError("out must be (symbol int64, logq float32, logz float32, next_state int64), each [N] on the batch's device")
    if value_state is not None or penalties is not None or not_pad is not None:
        extras = _lib.StepExtras()
        if not_pad is not None:
            extras.not_pad = not_pad.data_ptr()
        if value_state is not None:
            value_state = _walkers(lat, value_state, k, "value_state")
            extras.value_state = value_state.data_ptr()
        if penalties is not None:
            if inp is None:
                raise ValueError("penalties need the previous symbols `inp`")
            if penalties.accumulated.shape != (N,) or penalties.vocab_use.shape != (N, lat.vocab):
                raise ValueError("penalty counters do not match the walkers")
            extras.accumulated, extras.vocab_use = penalties.accumulated.data_ptr(), penalties.vocab_use.data_ptr()
            extras.insertion_mark, extras.insert_threshold = penalties.insertion_mark, penalties.insert_threshold
            extras.insert_penalty, extras.length_threshold = penalties.insert_penalty, penalties.length_threshold
            extras.length_penalty, extras.length = penalties.length_penalty, int(length)
    vstate = value_state if value_state is not None else state
    cfg = (state, inp, pad, bos, eos, has_to_end, temperature, uniforms, forced, extras, vstate, k, out)
    return ProposalStep(*_ProposalStep.apply(lat, scores, values, cfg))


class BeamStep(NamedTuple):
    score: torch.Tensor         # [N] float32: the survivors' scores c (without the look-ahead), -inf on empty ranks
    parent: torch.Tensor        # [N] int32: the rank in the lattice's beam the survivor extends, -1 on empty ranks
    symbol: torch.Tensor        # [N] int64: its new mark (pad on empty ranks)
    next_state: torch.Tensor    # [N] int64: the state after the mark (0 on empty ranks)
    n_candidates: torch.Tensor  # [B] int32: candidates before the cut to k


def beam_lds_candidates() -> int:
    """The candidates of one lattice that ``nfst_beam_step`` keeps in LDS; beyond that (or beyond k * vocab, if smaller)
    every pass of its selection computes them again."""
    return int(lib.nfst_beam_lds_candidates())


def beam_step(lat: LatticeBatch, state: torch.Tensor, inp: torch.Tensor, beam_score: torch.Tensor, scores: torch.Tensor,
              k: int, lookahead: Optional[torch.Tensor] = None, pad: int = 0, bos: int = 1, eos: int = 2,
              has_to_end: bool = False, out=None, n_open: Optional[torch.Tensor] = None) -> BeamStep:
    """One step of lattice-constrained beam search (``nfst_beam_step``, DESIGN.md sections 2 and 4.9): the deterministic
    twin of ``proposal_step``.  N = B * k slots, slot n = rank n % k of lattice n // k.  ``state`` [N] is the state after
    ``inp`` [N], the previous mark, was consumed; ``beam_score`` [N] float32 (-inf: a dead slot); ``scores`` [N, V] the
    network's outputs for this step, normalised by the caller; ``lookahead`` [total_rows] (optional) is added to a
    candidate's score for ranking only.  Every live slot expands by the legal marks of its state (the bos/pad/eos rules
    of ``proposal_step``); a candidate scores ``c = beam_score + (scores[j, l] + arc_w)`` (pad scores 0) and the best k
    per lattice by (c + lookahead desc, slot asc, mark asc) survive.  ``out`` = (score, parent, symbol, next_state,
    n_candidates) tensors of a previous call or rows of buffers allocated once per search; ``n_open``: an int32 device
    word (zeroed by the caller) that receives the number of survivors whose mark is not ``pad`` (zero: every hypothesis
    has ended or died).  Not differentiable: re-score the paths with ``path_logprob``."""
    _need_gpu(lat)
    dev = lat.device
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError(f"k must be an int, not {k!r}")
    N, B = lat.n_lattices * max(k, 0), lat.n_lattices

    def arg(x, dtype, shape, name):
        if not isinstance(x, torch.Tensor) or x.dtype != dtype or tuple(x.shape) != shape:
            raise ValueError(f"{name} must be a {dtype} tensor of shape {list(shape)}")
        return x.to(device=dev).contiguous()

    state, inp = arg(state, torch.int64, (N,), "state"), arg(inp, torch.int64, (N,), "inp")
    beam_score = arg(beam_score, torch.float32, (N,), "beam_score")
    scores = arg(scores.detach(), torch.float32, (N, lat.vocab), "scores")
    if lookahead is not None:
        lookahead = arg(lookahead.detach(), torch.float32, (lat.total_rows,), "lookahead")
    if n_open is not None and (n_open.dtype != torch.int32 or n_open.numel() != 1 or n_open.device != dev):
        raise ValueError("n_open must be one int32 word on the batch's device")
    want = ((torch.float32, N), (torch.int32, N), (torch.int64, N), (torch.int64, N), (torch.int32, B))
    if out is not None:
        if len(out) != 5 or any(o.dtype != d or o.shape != (n,) or o.device != dev or not o.is_contiguous() for o, (d, n) in zip(out, want)):
            raise ValueError("out must be (score float32 [N], parent int32 [N], symbol int64 [N], next_state int64 [N], "
                             "n_candidates int32 [B]) on the batch's device")
    else:
        out = tuple(torch.empty(n, dtype=d, device=dev) for d, n in want)
    _call("nfst_beam_step", lat, state, inp, beam_score, scores, lookahead, int(pad), int(bos), int(eos), int(bool(has_to_end)),
          int(k), *out, n_open)
    return BeamStep(*out)


def beam_backtrack(parent: torch.Tensor, symbol: torch.Tensor, score: torch.Tensor, n_lattices: int, k: int,
                   n_steps: Optional[int] = None, max_len: Optional[int] = None, pad: int = 0):
    """``(paths [B, k, max_len] int32, lengths [B, k] int32)`` of a finished beam search (``nfst_beam_backtrack``):
    ``parent`` (int32) and ``symbol`` (int64) [T, B * k] as ``beam_step`` wrote them step by step, ``score`` [B * k] of
    the last step followed.  Every final slot follows its parents from step ``n_steps - 1`` (default T) back to step 0;
    its marks other than ``pad`` are written in order and the row is right-padded with ``pad`` (``max_len`` defaults to
    T).  A slot whose score is -inf gets length 0."""
    if parent.device.type != "cuda":
        raise RuntimeError("nfst_amd: beam_backtrack runs on the MI355X only (no CPU fallback)")
    dev = parent.device
    N = int(n_lattices) * int(k)
    if parent.dim() != 2 or parent.shape[1] != N or parent.dtype != torch.int32:
        raise ValueError("parent must be int32 [T, n_lattices * k]")
    T = parent.shape[0]
    if symbol.shape != parent.shape or symbol.dtype != torch.int64 or symbol.device != dev:
        raise ValueError("symbol must be int64 [T, n_lattices * k] on parent's device")
    if score.shape != (N,) or score.dtype != torch.float32 or score.device != dev:
        raise ValueError("score must be float32 [n_lattices * k] on parent's device")
    n_steps = T if n_steps is None else int(n_steps)
    max_len = max(T, 1) if max_len is None else int(max_len)
    if not 0 <= n_steps <= T:
        raise ValueError(f"n_steps must lie in [0, {T}]")
    parent, symbol, score = parent.contiguous(), symbol.contiguous(), score.contiguous()
    paths = torch.empty((n_lattices, k, max_len), dtype=torch.int32, device=dev)
    lengths = torch.empty((n_lattices, k), dtype=torch.int32, device=dev)
    _call("nfst_beam_backtrack", None, parent, symbol, score, n_steps, int(n_lattices), int(k), max_len, int(pad), paths, lengths)
    return paths, lengths


class NeuralBeta(NamedTuple):
    log_beta: torch.Tensor   # [total_rows] natural log of the reference's beta
    beta_hat: torch.Tensor   # [total_rows, H]


class _NeuralBeta(torch.autograd.Function):
    """nfst_backward_neural with nfst_backward_neural_grad behind it: differentiable in label_x
    ([V, H] = emb Wx^T + bias, made by torch ops, so Wx, bias and the embeddings get their gradients
    through it), Wh and w."""

    @staticmethod
    def forward(ctx, lat, label_x, wh, w):
        f32 = dict(device=lat.device, dtype=torch.float32)
        H = w.shape[0]
        ws = torch.empty(int(lib.nfst_neural_ws_floats(C.byref(lat.c_struct()), H)), **f32)
        log_beta = torch.empty(lat.total_rows, **f32)
        beta_hat = torch.empty(lat.total_rows, H, **f32)
        _call("nfst_backward_neural", lat, label_x, wh, w, H, log_beta, beta_hat, ws)
        ctx.lat = lat
        ctx.save_for_backward(label_x, wh, w, beta_hat, ws)
        return log_beta, beta_hat

    @staticmethod
    def backward(ctx, g_log_beta, g_beta_hat):
        lat = ctx.lat
        label_x, wh, w, beta_hat, ws_fwd = ctx.saved_tensors
        f32 = dict(device=lat.device, dtype=torch.float32)
        H = w.shape[0]
        g_lb = (torch.zeros(lat.total_rows, **f32) if g_log_beta is None else g_log_beta.to(**f32)).contiguous()
        # rows the sweep never reached carry -inf and no gradient
        g_lb = torch.where(torch.isfinite(g_lb), g_lb, torch.zeros_like(g_lb))
        g_bh = None if g_beta_hat is None else g_beta_hat.to(**f32).contiguous()
        gamma = torch.zeros(lat.total_rows, H, **f32)
        g_x = torch.zeros_like(label_x)
        g_w = torch.zeros(H, **f32)
        ws = torch.empty(int(lib.nfst_neural_grad_ws_floats(C.byref(lat.c_struct()), H)), **f32)
        wh_t = wh.t().contiguous()
        _call("nfst_backward_neural_grad", lat, label_x, wh_t, w, H, beta_hat, ws_fwd, g_lb, g_bh, gamma, g_x, g_w, ws)
        # dL/dWh[i, j] = sum over states of gamma(s)[i] beta_hat(s)[j]: a library GEMM
        return None, g_x, _gram(gamma, beta_hat), g_w


def _gram(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a^T b for tall, narrow a and b ([n, H], n ~ 5e5): as one GEMM with K = n the library takes 0.3 ms at
    H = 8 ... 1.25 ms at H = 256 on the BASELINE batch's rows; 256 row chunks as one batched GEMM and a sum take
    0.04 ... 0.54 ms (`profiles/tune/gemm_tall_skinny.py`) and add in a better order."""
    n, H = a.shape
    chunks = 256 if n >= 256 * 64 else 1
    m = (n // chunks) * chunks
    out = torch.bmm(a[:m].view(chunks, -1, H).transpose(1, 2), b[:m].view(chunks, -1, H)).sum(0)
    if m < n:
        out = out + a[m:].t() @ b[m:]
    return out


def backward_neural(lat: LatticeBatch, emb: torch.Tensor, Wx: torch.Tensor, Wh: torch.Tensor, W: torch.Tensor,
                    bias: torch.Tensor) -> NeuralBeta:
    """``FSAGRUScorer.compute_beta_per_sample`` / ``compute_beta_parallel`` with their Tree-LSTM-style
    messages (scorers.py:692-751, 753-856), parameters named as there: ``emb`` [V, H] mark embeddings,
    ``Wx``, ``Wh`` [H, H], ``W`` [1, H] or [H], ``bias`` [H].  The per-label part ``Wx e(l) + bias`` is
    one [V, H] x [H, H] product made here (a plain library GEMM); everything that depends on the
    lattice runs in the kernel.  Differentiable in all five parameters (the reference's
    ``tune_proposal`` trains them through ``compute_beta``, lightning.py:339-406): the gradient is
    ``nfst_backward_neural_grad`` plus two library GEMMs.  Both calls raise ``NfstError`` (NFST_ERR_LIMIT) before any
    launch when their rows do not fit the 160 KiB of LDS; the gradient's limit is the lower one (3388 against 5340 rows
    at H = 512, ``include/nfst_hip.h``), so a batch between the two runs forward and raises in ``backward()``."""
    _need_gpu(lat)
    f32 = dict(device=lat.device, dtype=torch.float32)
    emb, Wx, Wh, bias = emb.to(**f32), Wx.to(**f32), Wh.to(**f32), bias.to(**f32)
    w = W.to(**f32).reshape(-1).contiguous()
    H = w.shape[0]
    if emb.shape != (lat.vocab, H) or Wx.shape != (H, H) or Wh.shape != (H, H) or bias.shape != (H,):
        raise ValueError("emb must be [V, H], Wx and Wh [H, H], W [H] and bias [H]")
    label_x = torch.addmm(bias, emb, Wx.t()).contiguous()
    return NeuralBeta(*_NeuralBeta.apply(lat, label_x, Wh.contiguous(), w))


def gather_label_scores(lat: LatticeBatch, theta, arc_scores=None) -> torch.Tensor:
    """Per-arc log weights in canonical order (WFSTScorer, scorers.py:1671-1687)."""
    _need_gpu(lat)
    sc, keep = _scores(lat, theta, arc_scores)
    out = torch.empty(lat.total_arcs, dtype=torch.float32, device=lat.device)
    _call("nfst_gather_label_scores", lat, sc, out)
    return out


MASK_STATICRNN, MASK_GPT2 = 0, 1


def _plp_args(pad, bos, eos, max_length, temp, normalize, smoothing, mask_mode):
    return (int(pad), int(bos), int(eos), -1 if max_length is None else int(max_length), C.c_float(temp),
            int(bool(normalize)), C.c_float(smoothing), int(mask_mode))


class _PathLogprob(torch.autograd.Function):
    """out[n] = sum_t (log_softmax row gathered / label-smoothed), d out / d scores by
    nfst_path_logprob_backward (recomputes the rows; nothing but the inputs is saved)."""

    @staticmethod
    def forward(ctx, scores, marks, cfg):
        N, T, V = scores.shape
        out = torch.empty(N, dtype=torch.float32, device=scores.device)
        _call("nfst_path_logprob", None, scores, marks, N, T, V, *_plp_args(*cfg), out)
        ctx.cfg = cfg
        ctx.save_for_backward(scores, marks)
        return out

    @staticmethod
    def backward(ctx, g):
        scores, marks = ctx.saved_tensors
        N, T, V = scores.shape
        g = g.to(torch.float32).contiguous()
        grad = torch.empty_like(scores)
        _call("nfst_path_logprob_backward", None, scores, marks, g, N, T, V, *_plp_args(*ctx.cfg), grad)
        return grad, None, None


def path_logprob(scores: torch.Tensor, marks: torch.Tensor, pad: int = 0, bos: int = 1, eos: int = 2,
                 max_length: Optional[int] = None, temp: float = 1.0, normalize: bool = True,
                 smoothing: float = 0.0, mask_mode: int = MASK_STATICRNN) -> torch.Tensor:
    """Fused masks + log_softmax + gather + pad-masked sum over time
    (StaticRNNScorer.evaluate_seq_with_temp, scorers.py:1564-1611): scores [N,T,V], marks [N,T] -> [N].
    ``smoothing > 0`` selects the training branch (label-smoothed target, scorers.py:1584-1592).
    Differentiable with respect to ``scores`` -- the reference trains p~ through this op
    (lightning.py:511-516)."""
    if scores.device.type != "cuda":
        raise RuntimeError("nfst_amd: path_logprob runs on the MI355X only (no CPU fallback)")
    scores = scores.to(torch.float32).contiguous()
    marks = marks.to(device=scores.device, dtype=torch.int64).contiguous()
    N, T, V = scores.shape
    if marks.shape != (N, T):
        raise ValueError("marks must be [N, T]")
    return _PathLogprob.apply(scores, marks, (pad, bos, eos, max_length, temp, normalize, smoothing, mask_mode))


def gpt2_logprob(logits: torch.Tensor, x: torch.Tensor, pad: int = 0) -> torch.Tensor:
    """The arithmetic of ``GPT2Wrapper.forward`` after the language model (modules/transformer.py:45-52):
    ``logits`` [N, T+1, V] are the model's outputs for the bos-shifted input ``cat(bos, x)``, ``x`` [N, T] the
    marks; gold = ``cat(x, pad)``; the pad logit becomes -1e8, log_softmax, gather of gold, positions
    holding pad contribute 0, sum over time -> [N].  Differentiable with respect to ``logits``."""
    N, T = x.shape
    if tuple(logits.shape[:2]) != (N, T + 1):
        raise ValueError("logits must be [N, T + 1, V] for x [N, T]")
    gold = torch.cat((x, x.new_full((N, 1), pad)), dim=1)
    return path_logprob(logits, gold, pad=pad, normalize=True, mask_mode=MASK_GPT2)


def iwae(log_p: torch.Tensor, log_q: torch.Tensor):
    """(log_marginal [B], log_w [B,K]) of Estimators.iwae (modules/estimatros.py:11-44)."""
    if log_p.device.type != "cuda":
        raise RuntimeError("nfst_amd: iwae runs on the MI355X only (no CPU fallback)")
    log_p = log_p.to(torch.float32).contiguous()
    log_q = log_q.to(device=log_p.device, dtype=torch.float32).contiguous()
    B, K = log_p.shape
    log_w = torch.empty_like(log_p)
    lm = torch.empty(B, dtype=torch.float32, device=log_p.device)
    _call("nfst_iwae", None, log_p, log_q, B, K, log_w, lm)
    return lm, log_w


# ----------------------------------------------------------------------------- edit distance
# (at the end: edit.py takes the marshalling helpers above)
from .edit import EDIT_MAX_LEN, LatticeEditResult, edit_distance, lattice_edit_distance, pairwise_edit_distance  # noqa: E402,F401
from .constraints import constraint_log_prob  # noqa: E402,F401
from .strings import (MERGE_MAX_K, NextSymbols, PrefixScores, StringScores, StringSet, merge_paths, string_arc_posteriors,  # noqa: E402,F401
                      string_log_prob, string_next_log_probs, string_prefix_log_prob)
from .strings import STATE_MAX_M, PrefixContext, PrefixState, string_prefix_open  # noqa: E402,F401
from .strings import StringAlignment, StringSampleResult, string_alignment_log_prob, string_sample_paths, string_viterbi  # noqa: E402,F401

"""Lattice-constrained beam search for path-dependent scorers.

The exact decoders (``ops.viterbi``, ``ops.k_best``) need a score that decomposes over arcs.  A recurrent or
autoregressive scorer (the reference's ``StaticRNNScorer``, its GPT-2 wrapper, the learned proposal) gives weights that
depend on the whole prefix; for those ``BeamDecoder`` keeps k hypotheses per lattice and runs the loop of
``ProposalSampler.stateful_sample`` with the sampler's draw replaced by "the best k of all legal extensions": one
``score_fn`` call and one fused ``nfst_beam_step`` launch per mark (DESIGN.md sections 2 and 4.9).
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Union

import torch

from . import ops, swor
from .scorers import LatticeScorer


class BeamResult(NamedTuple):
    paths: torch.Tensor    # [B, k, T] int32: marks after the implicit bos up to eos, right-padded with pad
    lengths: torch.Tensor  # [B, k] int32 marks per path (0 on empty ranks)
    scores: torch.Tensor   # [B, k] float32: sum of the step scores along the path, best first; -inf on empty ranks
    n_steps: int           # steps that were kept (the last one is the first at which every hypothesis had ended or died)


def reorder_by_parent(hx, index: torch.Tensor):
    """``hx`` (a tensor with the slots along dim 0, or a tuple / list of such, or None) gathered by ``index`` [N]."""
    if hx is None:
        return None
    if isinstance(hx, (tuple, list)):
        return type(hx)(reorder_by_parent(h, index) for h in hx)
    return hx.index_select(0, index)


class BeamDecoder:
    """``score_fn(hx, inp) -> (new_hx, scores [N, V])`` is the network, as for ``ProposalSampler``: ``inp`` [N] int64 are
    the marks consumed last (bos first), ``scores`` what the step adds per next mark -- log probabilities if the scores
    are to be comparable across lengths; the decoder fuses no softmax.  N = B * k slots, slot n = rank n % k of lattice
    n // k.  After every step ``reorder_fn(new_hx, parent)`` moves the recurrent state to the survivors: ``parent`` [N]
    int64 is the global slot each survivor extends (an empty rank names itself); the default gathers along dim 0 and
    walks tuples.  ``sync_every``: steps between two looks at the device-side "every hypothesis has ended" counters."""

    def __init__(self, model: LatticeScorer, score_fn, reorder_fn=None, sync_every: int = 8):
        self.model = model
        self.score_fn = score_fn
        self.reorder_fn = reorder_by_parent if reorder_fn is None else reorder_fn
        self.sync_every = max(1, int(sync_every))

    def _lookahead(self, lookahead) -> Optional[torch.Tensor]:
        m = self.model
        lat = m._lat()
        if lookahead is None:
            return None
        if isinstance(lookahead, str):
            if lookahead == "viterbi":  # best score from the row to the sink under theta; -inf rows stay -inf
                return ops.arc_slack(lat, m.theta.detach(), want_rows=True).vbeta
            if lookahead == "log_beta":
                return m.compute_log_beta()[:: m.k].reshape(-1).contiguous()
            raise ValueError(f"lookahead must be None, 'viterbi', 'log_beta' or a [total_rows] tensor, not {lookahead!r}")
        return lookahead.detach().to(device=lat.device, dtype=torch.float32).reshape(-1)

    @torch.no_grad()
    def decode(self, k: int, lookahead: Union[None, str, torch.Tensor] = None, max_len: Optional[int] = None, hx=None) -> BeamResult:
        """Beam search with k hypotheses per lattice.  ``lookahead``: a row-indexed [total_rows] value added to a
        candidate's score for ranking only -- ``"viterbi"`` the exact best completion under the scorer's ``theta``
        (with a scorer that is ``theta`` itself, k = 1 then finds the best path), ``"log_beta"`` the scorer's
        ``compute_log_beta()``.  ``max_len`` replaces the scorer's ``max_length``: there are ``max_len + 1`` steps and
        on the last one only eos (or pad, for a hypothesis that has ended) is legal; a hypothesis that cannot end
        there dies.  ``hx`` is the recurrent state handed to the first ``score_fn`` call (slots along dim 0)."""
        m = self.model
        lat = m._lat()
        dev = lat.device
        B = lat.n_lattices
        N = B * k
        look = self._lookahead(lookahead)
        L = m.max_length if max_len is None else int(max_len)
        T = L + 1
        base = torch.arange(N, device=dev, dtype=torch.int64)
        base -= base % k  # first slot of the lattice
        own = torch.arange(N, device=dev, dtype=torch.int64)
        inp = torch.full((N,), m.__bos__, dtype=torch.int64, device=dev)
        # the implicit bos is consumed first, unscored, as the sampler does
        state = ops.step(lat, torch.zeros(N, dtype=torch.int64, device=dev), inp, k=k)
        score = torch.full((N,), float("-inf"), dtype=torch.float32, device=dev)
        score[::k] = 0.0
        # the outputs of all steps live in buffers allocated once; n_open[t] is read back every sync_every steps
        score_all = torch.empty((T, N), dtype=torch.float32, device=dev)
        parent_all = torch.empty((T, N), dtype=torch.int32, device=dev)
        sym_all = torch.empty((T, N), dtype=torch.int64, device=dev)
        nxt_all = torch.empty((T, N), dtype=torch.int64, device=dev)
        ncand_all = torch.empty((T, B), dtype=torch.int32, device=dev)
        n_open = torch.zeros(T, dtype=torch.int32, device=dev)
        CHECK = self.sync_every
        n_steps = 0
        for t in range(T):
            hx, scores = self.score_fn(hx, inp)
            r = ops.beam_step(lat, state, inp, score, scores, k, lookahead=look, pad=m.__pad__, bos=m.__bos__, eos=m.__eos__,
                              has_to_end=(t + 1) > L, out=(score_all[t], parent_all[t], sym_all[t], nxt_all[t], ncand_all[t]),
                              n_open=n_open[t:t + 1])
            p = r.parent.to(torch.int64)
            hx = self.reorder_fn(hx, torch.where(p >= 0, base + p, own))
            state, inp, score = r.next_state, r.symbol, r.score
            n_steps = t + 1
            if n_steps % CHECK == 0 or n_steps == T:
                first = n_steps - (CHECK if n_steps % CHECK == 0 else n_steps % CHECK)
                ended = (n_open[first:n_steps] == 0).nonzero()
                if ended.numel():
                    n_steps = first + int(ended[0]) + 1  # the first step after which nothing is open; later steps are dropped
                    break
        final = score_all[n_steps - 1]
        paths, lengths = ops.beam_backtrack(parent_all, sym_all, final, B, k, n_steps=n_steps, max_len=T, pad=m.__pad__)
        return BeamResult(paths, lengths, final.reshape(B, k).clone(), n_steps)


# ----------------------------------------------------------------------------- minimum-Bayes-risk selection
def mbr_select(distances: torch.Tensor, log_weights: torch.Tensor, n_paths: Optional[torch.Tensor] = None):
    """``(index [B] int64, risk [B, K] float64)``: the candidate of least expected distance to the weighted list it
    stands in.  ``distances`` [B, K, K] (``ops.pairwise_edit_distance``), ``log_weights`` [B, K] unnormalised;
    risk[b, i] = sum_j w[b, j] distances[b, i, j] with w the float64 softmax of ``log_weights`` over the valid entries.
    Entry j is valid when j < ``n_paths[b]``; without ``n_paths``, when its weight is finite.  An invalid candidate has
    risk +inf; ``index`` is the first valid candidate of least risk, -1 for a lattice with no valid entry (or whose
    valid entries all weigh -inf: there is no mass to take an expectation under).  Pure torch: works on CPU tensors too."""
    if distances.dim() != 3 or log_weights.dim() != 2 or distances.shape != (*log_weights.shape, log_weights.shape[1]):
        raise ValueError("distances must be [B, K, K] and log_weights [B, K]")
    lw = log_weights.detach().to(torch.float64)
    D = distances.to(device=lw.device, dtype=torch.float64)
    B, K = lw.shape
    inf = float("inf")
    if n_paths is None:
        valid = torch.isfinite(lw)
    else:
        valid = torch.arange(K, device=lw.device)[None, :] < n_paths.to(lw.device).reshape(B, 1)
    lw = torch.where(valid, lw, torch.full_like(lw, -inf))
    top = lw.max(dim=1, keepdim=True).values if K > 0 else lw.new_full((B, 1), -inf)
    some = (top > -inf) & (top < inf)
    w = torch.where(some, torch.exp(lw - torch.where(some, top, torch.zeros_like(top))), torch.zeros_like(lw))
    w = w / torch.where(some, w.sum(dim=1, keepdim=True), torch.ones_like(top))
    # (an invalid column weighs 0 whatever its distance: 0 * D is only taken of the finite D of valid columns)
    risk = (torch.where(valid[:, None, :], D, torch.zeros_like(D)) * w[:, None, :]).sum(dim=2)
    risk = torch.where(valid & some, risk, torch.full_like(risk, inf))
    if K == 0:
        return torch.full((B,), -1, dtype=torch.int64, device=lw.device), risk
    least = risk.min(dim=1, keepdim=True).values
    first = ((risk == least) & valid & some).to(torch.int8).argmax(dim=1)  # (argmax of a 0/1 row: its first 1)
    return torch.where(some[:, 0], first, torch.full_like(first, -1)), risk


def mbr_decode(result):
    """``(index [B] int64, risk [B, K] float64, distances [B, K, K] int32)`` of a drawn or enumerated path set under
    edit distance: the pairwise table of ``ops.pairwise_edit_distance`` on the set's paths, then ``mbr_select``.
    ``result`` is an ``ops.KBestResult`` or ``ops.PositionalKBestResult``, weighed by ``best`` (the path scores: log Z
    cancels in the softmax), or a ``swor.SworResult``, weighed by its Horvitz-Thompson weights (``swor.log_weights``),
    under which ``risk`` is the self-normalised estimate of every candidate's expected distance to a path of the
    posterior."""
    if isinstance(result, swor.SworResult):
        logw = swor.log_weights(result)
    elif isinstance(result, (ops.KBestResult, ops.PositionalKBestResult)):
        logw = result.best.detach()
    else:
        raise TypeError("mbr_decode takes a KBestResult, a PositionalKBestResult or a SworResult")
    D = ops.pairwise_edit_distance(result.paths, result.lengths)
    index, risk = mbr_select(D, logw, result.n_paths)
    return index, risk, D


# ----------------------------------------------------------------------------- output strings
class StringDecodeResult(NamedTuple):
    strings: torch.Tensor     # [B, k, L] int32: the distinct output strings of the path set, best first, pad-filled
    lengths: torch.Tensor     # [B, k] int32 (0 beyond n_strings)
    log_prob: torch.Tensor    # [B, k] float64: exact log p(y | x) (rescore=False: path_mass); -inf beyond n_strings
    n_strings: torch.Tensor   # [B] int32
    path_mass: torch.Tensor   # [B, k] float64: the merged weight of the string's paths in the set, less log Z
    first_path: torch.Tensor  # [B, k] int32: the row of the path set that represents the string (its heaviest alignment); -1 beyond n_strings


def path_scores64(lat, theta: torch.Tensor, r, arc_scores=None) -> torch.Tensor:
    """The scores [B, k] of the paths of a ``KBestResult`` summed again in float64 from their arcs (``best`` is the
    kernel's float32 sum): theta[label] + the table's weight + arc_scores per arc, as ``ops.string_log_prob`` takes them,
    so that a string's share of its paths compares with its exact weight at float64 round-off; -inf beyond ``n_paths``."""
    B, k, L = r.paths.shape
    dev = r.paths.device
    live = torch.arange(L, device=dev)[None, None, :] < r.lengths[:, :, None]
    labels, arcs = r.paths.to(torch.int64).clamp(min=0), r.arcs.to(torch.int64).clamp(min=0)
    th = theta.detach().to(device=dev, dtype=torch.float64)
    t = th[labels] if th.dim() == 1 else th.gather(1, labels.reshape(B, -1)).reshape(B, k, L)
    if lat.weighted:
        t = t + lat.arc_w.to(torch.float64)[arcs]
    if arc_scores is not None:
        t = t + arc_scores.detach().to(device=dev, dtype=torch.float64)[arcs]
    s = torch.where(live, t, torch.zeros_like(t)).sum(dim=2)
    return torch.where(torch.arange(k, device=dev)[None, :] < r.n_paths[:, None], s, torch.full_like(s, float("-inf")))


def decode_strings(lat, theta, k: int, *, keep=None, marker: Optional[int] = None, method: str = "k_best", rescore: bool = True,
                   arc_scores=None, seed: int = 0, pad: int = 0) -> StringDecodeResult:
    """The best output strings of every lattice with their exact probabilities.  The ``k`` best paths (``method="k_best"``,
    weighed by their scores ``best``, summed again in float64: ``path_scores64``) or ``k`` paths drawn without replacement (``"swor"``, weighed by ``swor.log_weights``) are
    merged by the string they spell on the tape ``keep`` or ``marker`` (``ops.merge_paths``): one alignment's score is
    not a string's, and the heaviest string need not own the best path.  ``rescore=True`` then computes log p(y | x) of
    every distinct string exactly (``ops.string_log_prob``) and ranks by it, ties keeping the merged order;
    ``path_mass`` keeps what the path set saw of each string, its merged weight minus log Z -- for ``k_best`` a lower
    bound of ``log_prob``.  ``rescore=False`` returns the merged order with ``log_prob`` = ``path_mass``."""
    if (keep is None) == (marker is None):
        raise ValueError("give keep (a set of labels) or marker (a label)")
    theta = torch.as_tensor(theta, dtype=torch.float32).detach()
    if method == "k_best":
        r = ops.k_best_terms(lat, theta, k, arc_scores, pad=pad)
        logw = path_scores64(lat, theta, r, arc_scores)  # (``best``, in float64)
    elif method == "swor":
        r = swor.sample(lat, theta, k, arc_scores, seed=seed, pad=pad)
        logw = swor.log_weights(r)  # (of probabilities: log Z is in them already)
    else:
        raise ValueError(f"method must be 'k_best' or 'swor', not {method!r}")
    s = ops.merge_paths(r.paths, r.lengths, logw, r.n_paths, keep=keep, marker=marker, vocab=lat.vocab, pad=pad)
    live = torch.arange(s.strings.shape[1], device=s.strings.device)[None, :] < s.n_strings[:, None]
    n_max = max(1, int(s.lengths.max())) if s.lengths.numel() else 1  # (the workspace grows with the candidates' row stride)
    cand = (s.strings[:, :, :n_max], s.lengths) if rescore else (s.strings[:, :0], s.lengths[:, :0])  # (no candidate: log Z alone)
    sc = ops.string_log_prob(lat, theta, *cand, keep=keep, marker=marker, arc_scores=ops._det(arc_scores))  # (the ranking carries no gradient)
    mass = torch.where(live, s.log_weights - sc.logz[:, None], s.log_weights) if method == "k_best" else s.log_weights
    if not rescore:
        return StringDecodeResult(s.strings, s.lengths, mass, s.n_strings, mass, s.first)
    logp = torch.where(live, sc.log_prob, torch.full_like(sc.log_prob, float("-inf")))
    # exact log p descending, ties and the dead entries in the merged order (a stable sort; NaN cannot occur)
    order = torch.sort(torch.where(live, -logp, torch.full_like(logp, float("inf"))), dim=1, stable=True).indices
    take = lambda x: x.gather(1, order)
    return StringDecodeResult(s.strings.gather(1, order[:, :, None].expand_as(s.strings)), take(s.lengths), take(logp), s.n_strings,
                              take(mass), take(s.first))


class PrefixSearchResult(NamedTuple):
    strings: torch.Tensor    # [B, k, L] int32: complete output strings, the most probable first, pad-filled
    lengths: torch.Tensor    # [B, k] int32 (0 beyond n_strings)
    log_prob: torch.Tensor   # [B, k] float64: exact log p(y | x); -inf beyond n_strings
    n_strings: torch.Tensor  # [B] int32
    bound: torch.Tensor      # [B] float64: log of the largest share of probability that the search set aside unexplored (-inf: none)
    exact: torch.Tensor      # [B] bool: the first entry is provably the most probable string of the lattice


def prefix_search(lat, theta, k: int = 8, max_len: Optional[int] = None, *, keep=None, marker: Optional[int] = None, arc_scores=None,
                  pad: int = 0, reserve: int = 64, refine_steps: int = 32, incremental: bool = False) -> PrefixSearchResult:
    """Prefix beam search for the most probable output strings with exact prefix probabilities
    (``ops.string_next_log_probs``), in two phases.  The first is length-synchronous: step t holds at most ``k`` open
    prefixes of length t per lattice and asks for their ``eos`` and ``next`` in one call (M = k, N = t).  Every ``eos`` is the
    exact weight of a complete string and enters the list of the k best complete strings.  The k V extensions are ranked
    by ``next``, the exact mass of all strings that start with them (ties go to the lower prefix slot, then to the lower
    label: a stable sort on the device), and the k heaviest stay open.  No string that starts with a pruned extension
    weighs more than the extension, so what is pruned bounds what was missed: the pruned extensions are set aside in a
    reserve of the ``reserve`` heaviest per lattice, and the heaviest one that the reserve drops raises ``bound[b]``.  A
    prefix of ``max_len`` symbols (default: the longest path of the batch) is not extended; its mass beyond its own ``eos``
    raises the bound.  A lattice leaves this phase when no open prefix outweighs its k-th complete string.  The second
    phase comes back to what was set aside: per step the k heaviest prefixes of the reserve, whatever their lengths, are
    scored in one call and all their extensions set aside, until the reserve holds nothing heavier than the lattice's
    first complete string or ``refine_steps`` steps have passed; what is then left in the reserve joins the bound.
    ``exact[b]`` is set when the first entry weighs at least ``bound[b]`` and at least every prefix that was open when the
    first phase stopped: it is then the most probable string of lattice b, which no list of paths can certify.
    ``reserve=0, refine_steps=0`` is the first phase alone, ``bound`` the heaviest mass ever pruned.  ``log_prob`` and
    ``bound`` are less log Z.  Every step sweeps the prefix table of the whole prefix again.  No gradient.
    ``incremental=True`` opens an ``ops.PrefixContext`` once and holds the open prefixes of the first phase as a
    ``PrefixState``, which every step extends by the symbols it picked: one column per step in place of the whole table,
    and the per-lattice indexes once per search.  Every field of the result is the same, bit for bit; k <= 1024.  The
    second phase is the same either way (its prefixes are scored once and never extended).  No gradient."""
    ops._check_k(k, bounded=False)
    if (keep is None) == (marker is None):
        raise ValueError("give keep (a set of labels) or marker (a label)")
    for name, x in (("reserve", reserve), ("refine_steps", refine_steps)):
        if isinstance(x, bool) or not isinstance(x, int) or x < 0:
            raise ValueError(f"{name} must be an int >= 0")
    ops._need_gpu(lat)
    theta = torch.as_tensor(theta, dtype=torch.float32).detach()
    arc_scores = ops._det(arc_scores)
    if max_len is None:
        max_len = min(int(lat.depth.max()), ops.EDIT_MAX_LEN)
    if isinstance(max_len, bool) or not isinstance(max_len, int) or not 0 <= max_len <= ops.EDIT_MAX_LEN:
        raise ValueError(f"max_len must be an int in [0, {ops.EDIT_MAX_LEN}]")
    B, V, dev, L, R = lat.n_lattices, lat.vocab, lat.device, max(max_len, 1), reserve
    f64, i32, ninf = torch.float64, torch.int32, float("-inf")
    new_rows = lambda n: torch.full((B, n, L), pad, dtype=i32, device=dev)
    new_mass = lambda n: torch.full((B, n), ninf, dtype=f64, device=dev)
    st = dict(comp_rows=new_rows(k), comp_len=torch.zeros((B, k), dtype=i32, device=dev), comp_w=new_mass(k), bound=new_mass(1)[:, 0],
              res_rows=new_rows(R), res_len=torch.zeros((B, R), dtype=i32, device=dev), res_mass=new_mass(R),
              logz=torch.zeros(B, dtype=f64, device=dev))

    def expand(rows, lens, live, N, state=None):
        """One call on the open prefixes (on their state where there is one): their eos into the complete lists, their
        extensions' masses [B, k V] (-inf for a dead slot and for a prefix of max_len symbols, whose mass beyond its eos
        raises the bound)"""
        if state is not None:
            ns = ctx.next(state)
        else:
            ns = ops.string_next_log_probs(lat, theta, rows[:, :, :max(N, 1)], lens, keep=keep, marker=marker, arc_scores=arc_scores)
        st["logz"] = ns.logz
        eos = torch.where(live, ns.eos, torch.full_like(ns.eos, ninf))
        nxt = torch.where(live[:, :, None], ns.next, torch.full_like(ns.next, ninf))
        # the complete strings: the k best of the list so far and this step's, the earlier entry first among equals
        w = torch.cat([st["comp_w"], eos], dim=1)
        order = torch.sort(-w, dim=1, stable=True).indices[:, :k]
        st["comp_w"] = w.gather(1, order)
        st["comp_len"] = torch.cat([st["comp_len"], torch.where(eos > ninf, lens, torch.zeros_like(lens))], dim=1).gather(1, order)
        st["comp_rows"] = torch.cat([st["comp_rows"], rows], dim=1).gather(1, order[:, :, None].expand(B, k, L))
        capped = (lens >= max_len)[:, :, None]
        rest = torch.logsumexp(torch.where(capped, nxt, torch.full_like(nxt, ninf)), dim=2).max(dim=1).values
        st["bound"] = torch.maximum(st["bound"], torch.where(rest.isnan(), torch.full_like(rest, ninf), rest))
        return torch.where(capped, torch.full_like(nxt, ninf), nxt).reshape(B, k * V)

    def extended(rows, lens, picked):
        """The prefixes of the extensions ``picked`` [B, n] (slot * V + label) of the open prefixes: (rows, lengths)"""
        slot, label = picked // V, picked % V
        at = lens.gather(1, slot).to(torch.int64)
        out = rows.gather(1, slot[:, :, None].expand(B, picked.shape[1], L)).clone()
        out.scatter_(2, at.clamp(max=L - 1)[:, :, None], label[:, :, None].to(i32))
        return out, (at + 1).to(i32)

    def set_aside(rows, lens, flat):
        """The extensions of mass ``flat`` [B, k V] into the reserve, which keeps its R heaviest entries in descending
        order (among equals its own entries first, then the lower slot and label); the heaviest dropped raises the bound"""
        both = torch.cat([st["res_mass"], flat], dim=1)
        order = torch.sort(-both, dim=1, stable=True).indices[:, :R + 1]
        if order.shape[1] > R:
            st["bound"] = torch.maximum(st["bound"], both.gather(1, order[:, R:]).squeeze(1))
        if R == 0:
            return
        order = order[:, :R]
        old = order < R
        e_rows, e_len = extended(rows, lens, (order - R).clamp(min=0))
        o = order.clamp(max=R - 1)
        mass = both.gather(1, order)
        st["res_rows"] = torch.where(old[:, :, None], st["res_rows"].gather(1, o[:, :, None].expand(B, R, L)), e_rows)
        st["res_len"] = torch.where(old, st["res_len"].gather(1, o), e_len)
        st["res_mass"] = mass

    # the length-synchronous phase
    open_rows, open_len, open_mass = new_rows(k), torch.zeros((B, k), dtype=i32, device=dev), new_mass(k)
    open_mass[:, 0] = 0.0  # the empty prefix in slot 0 (its mass is not needed)
    open_at_stop = new_mass(1)[:, 0]
    active = torch.ones(B, dtype=torch.bool, device=dev)
    n_open = min(k, k * V)
    ctx = ops.string_prefix_open(lat, theta, keep=keep, marker=marker, arc_scores=arc_scores) if incremental else None
    state, grown = None, None  # the open prefixes' state, and the (parent slot, symbol) [B, k] that make the next one
    for t in range(max_len + 1):
        if incremental:
            state = ctx.root(k) if grown is None else ops.PrefixState(ctx._extend(state.cells, k, *grown)[0], open_len)
        flat = expand(open_rows, open_len, active[:, None] & (open_mass > ninf), t, state)
        order = torch.sort(-flat, dim=1, stable=True).indices[:, :n_open]
        mass = flat.gather(1, order)
        rows, lens = extended(open_rows, open_len, order)
        set_aside(open_rows, open_len, flat.scatter(1, order, ninf))
        alive = mass > ninf
        open_rows, open_len, open_mass = new_rows(k), torch.zeros((B, k), dtype=i32, device=dev), new_mass(k)
        open_rows[:, :n_open] = torch.where(alive[:, :, None], rows, open_rows[:, :n_open])
        open_len[:, :n_open] = torch.where(alive, lens, open_len[:, :n_open])
        open_mass[:, :n_open] = mass
        if incremental:  # (a pick of no mass leaves its slot dead)
            grown = (torch.where(alive, order // V, torch.full_like(order, -1)).to(i32), (order % V).to(i32))
        go_on = active & (open_mass > st["comp_w"][:, k - 1, None]).any(dim=1)
        open_at_stop = torch.where(active & ~go_on, open_mass.max(dim=1).values, open_at_stop)
        active = go_on
        if not bool(active.any()):
            break
    # back to the reserve
    for _ in range(refine_steps if R else 0):
        active = st["res_mass"][:, 0] > st["comp_w"][:, 0]
        if not bool(active.any()):
            break
        n_pop = min(k, R)
        open_rows, open_len, open_mass = new_rows(k), torch.zeros((B, k), dtype=i32, device=dev), new_mass(k)
        taken = active[:, None] & (st["res_mass"][:, :n_pop] > ninf)
        open_rows[:, :n_pop] = torch.where(taken[:, :, None], st["res_rows"][:, :n_pop], open_rows[:, :n_pop])
        open_len[:, :n_pop] = torch.where(taken, st["res_len"][:, :n_pop], open_len[:, :n_pop])
        open_mass[:, :n_pop] = torch.where(taken, st["res_mass"][:, :n_pop], open_mass[:, :n_pop])
        st["res_mass"] = torch.cat([torch.where(taken, torch.full_like(open_mass[:, :n_pop], ninf), st["res_mass"][:, :n_pop]),
                                    st["res_mass"][:, n_pop:]], dim=1)
        set_aside(open_rows, open_len, expand(open_rows, open_len, open_mass > ninf, int(open_len.max())))
    comp_w, logz = st["comp_w"], st["logz"]
    bound = torch.maximum(st["bound"], st["res_mass"].max(dim=1).values) if R else st["bound"]
    found = comp_w > ninf
    first = comp_w[:, 0]
    exact = found[:, 0] & (first >= bound) & (first >= open_at_stop)
    log_prob = torch.where(found, comp_w - logz[:, None], comp_w)
    comp_rows = torch.where(found[:, :, None], st["comp_rows"], torch.full_like(st["comp_rows"], pad))
    return PrefixSearchResult(comp_rows, st["comp_len"], log_prob, found.sum(dim=1).to(i32), torch.where(bound > ninf, bound - logz, bound), exact)


def mbr_decode_strings(string_set):
    """``mbr_decode`` on output strings: ``(index [B] int64, risk [B, K] float64, distances [B, K, K] int32)`` of a
    ``ops.StringSet`` under edit distance between the strings, weighed by the merged weights."""
    D = ops.pairwise_edit_distance(string_set.strings, string_set.lengths)
    index, risk = mbr_select(D, string_set.log_weights.detach(), string_set.n_strings)
    return index, risk, D

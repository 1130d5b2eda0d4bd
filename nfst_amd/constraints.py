"""Constraint automata: small deterministic automata (DFAs) over the label vocabulary that
``LatticeBatch.intersect`` / ``ops.intersect`` multiply into every lattice of a batch (``nfst_intersect_count`` /
``_write``, DESIGN.md sections 2 and 4.8).

An automaton has Q states, 1 <= Q <= 64, and starts in state 0.  ``delta[q, l]`` in {-1, 0 .. Q-1} is the state after
reading label ``l`` in state ``q`` (-1: no transition), ``final[q]`` says whether a run may end in ``q``.  It reads the
label of every arc of a path, ``bos`` and ``eos`` included, never the sink's pad loop.  One automaton serves the whole
batch (``[Q, V]`` / ``[Q]``) or every lattice has its own (``[B, Q, V]`` / ``[B, Q]``).

``WideDFA`` is the second format, for up to 4096 states: sparse (per state a default target and a list of exceptions),
one automaton for the batch or one per lattice without padding, through the same calls (``nfst_intersect_wide_count`` /
``_write``).  It is what a gold string of more than 31 symbols, an exact-string acceptor or a
bigram model over the labels needs.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import numpy as np
import torch

MAX_STATES = 64


def _np(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


class ConstraintDFA:
    """``ConstraintDFA(delta, final, weight=None)``.  ``weight``: optional float log weight per transition, shaped as
    ``delta`` (a tensor; it may require grad): ``IntersectResult.scores`` adds ``weight[(b,) q, label]`` to every arc
    of the product.  Raises ``ValueError`` for Q outside 1 .. 64, entries outside -1 .. Q-1 or mismatched shapes."""

    def __init__(self, delta, final, weight=None):
        d, f = _np(delta), _np(final)
        if d.ndim not in (2, 3) or f.ndim != d.ndim - 1 or f.shape != d.shape[:-1]:
            raise ValueError(f"delta must be [Q, V] with final [Q], or [B, Q, V] with final [B, Q]; got {d.shape} and {f.shape}")
        if not (np.issubdtype(d.dtype, np.integer) or np.issubdtype(d.dtype, np.bool_)):
            raise ValueError("delta must hold integers")
        Q, V = d.shape[-2], d.shape[-1]
        if not 1 <= Q <= MAX_STATES:
            raise ValueError(f"an automaton has 1 .. {MAX_STATES} states, not {Q}")
        if V < 1:
            raise ValueError("delta has no label")
        if d.size and (d.min() < -1 or d.max() >= Q):
            raise ValueError(f"entries of delta must lie in -1 .. {Q - 1}")
        self.delta = np.ascontiguousarray(d, dtype=np.int8)
        self.final = np.ascontiguousarray(f != 0)
        if weight is not None:
            if not isinstance(weight, torch.Tensor):
                weight = torch.as_tensor(np.asarray(weight), dtype=torch.float32)
            if tuple(weight.shape) != self.delta.shape or not weight.dtype.is_floating_point:
                raise ValueError(f"weight must be a float tensor shaped as delta, {self.delta.shape}")
        self.weight = weight
        self._device = {}

    # ---------------------------------------------------------------- shape
    @property
    def n_states(self) -> int:
        return self.delta.shape[-2]

    @property
    def vocab(self) -> int:
        return self.delta.shape[-1]

    @property
    def n_lattices(self) -> Optional[int]:
        """B for per-lattice automata, None for one automaton shared by the batch."""
        return self.delta.shape[0] if self.delta.ndim == 3 else None

    def check(self, vocab: int, n_lattices: int) -> None:
        if self.vocab != vocab:
            raise ValueError(f"the automaton reads {self.vocab} labels, the batch has {vocab}")
        if self.n_lattices is not None and self.n_lattices != n_lattices:
            raise ValueError(f"{self.n_lattices} automata for a batch of {n_lattices} lattices")

    # ---------------------------------------------------------------- device layout
    def to(self, device):
        """``(delta_t, final_mask)`` on ``device``, built once per device: the table label-major, ``[(B,) V, 64]`` int8
        padded with -1 (the transitions one arc's label needs are one 64-byte line), and the final states as one
        64-bit mask per automaton (int64 bits)."""
        device = torch.device(device)
        hit = self._device.get(device)
        if hit is None:
            t = np.full(self.delta.shape[:-2] + (self.vocab, MAX_STATES), -1, dtype=np.int8)
            t[..., :self.n_states] = np.swapaxes(self.delta, -1, -2)
            bits = (self.final.astype(np.uint64) << np.arange(self.n_states, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)
            mask = np.atleast_1d(bits).astype(np.uint64).view(np.int64)
            hit = (torch.from_numpy(t).to(device), torch.from_numpy(mask.copy()).to(device))
            self._device[device] = hit
        return hit

    # ---------------------------------------------------------------- on the host
    def run(self, labels: Iterable[int], b: Optional[int] = None) -> int:
        """The state after reading ``labels`` from state 0 (-1: a step had no transition); ``b`` picks the automaton."""
        d = self.delta if self.delta.ndim == 2 else self.delta[0 if b is None else b]
        q = 0
        for l in labels:
            q = int(d[q, int(l)])
            if q < 0:
                return -1
        return q

    def accepts(self, labels: Iterable[int], b: Optional[int] = None) -> bool:
        q = self.run(labels, b)
        f = self.final if self.final.ndim == 1 else self.final[0 if b is None else b]
        return q >= 0 and bool(f[q])

    # ---------------------------------------------------------------- builders
    @staticmethod
    def stack(dfas: Sequence["ConstraintDFA"]) -> "ConstraintDFA":
        """Per-lattice automata from shared ones, padded to a common Q with states nothing leads to."""
        dfas = list(dfas)
        if not dfas or any(d.n_lattices is not None for d in dfas) or len({d.vocab for d in dfas}) != 1:
            raise ValueError("stack takes single automata over one vocabulary")
        weighted = [d.weight is not None for d in dfas]
        if any(weighted) and not all(weighted):
            raise ValueError("either every automaton carries weights or none does")
        Q, V = max(d.n_states for d in dfas), dfas[0].vocab
        delta = np.full((len(dfas), Q, V), -1, dtype=np.int8)
        final = np.zeros((len(dfas), Q), dtype=bool)
        for i, d in enumerate(dfas):
            delta[i, :d.n_states], final[i, :d.n_states] = d.delta, d.final
        weight = None
        if all(weighted):
            weight = torch.stack([torch.nn.functional.pad(d.weight, (0, 0, 0, Q - d.n_states)) for d in dfas])
        return ConstraintDFA(delta, final, weight)

    @staticmethod
    def accept_all(vocab: int) -> "ConstraintDFA":
        return ConstraintDFA(np.zeros((1, vocab), np.int8), np.ones(1, bool))

    @staticmethod
    def count_at_most(vocab: int, labels: Iterable[int], n: int) -> "ConstraintDFA":
        """At most ``n`` arcs with a label of ``labels`` (n + 1 states: the count so far)."""
        labels = _labels(vocab, labels)
        if not 0 <= n < MAX_STATES:
            raise ValueError(f"n must lie in 0 .. {MAX_STATES - 1}")
        delta = np.repeat(np.arange(n + 1, dtype=np.int64)[:, None], vocab, axis=1)
        delta[:, labels] += 1
        delta[delta > n] = -1
        return ConstraintDFA(delta, np.ones(n + 1, bool))

    @staticmethod
    def forbid_bigram(vocab: int, x: int, y: int) -> "ConstraintDFA":
        """Never label ``x`` directly followed by ``y`` (state 1: the last label was x)."""
        _labels(vocab, [x, y])
        delta = np.zeros((2, vocab), np.int64)
        delta[:, x] = 1
        delta[1, y] = -1
        return ConstraintDFA(delta, np.ones(2, bool))

    @staticmethod
    def parity(vocab: int, labels: Iterable[int]) -> "ConstraintDFA":
        """An even number of arcs with a label of ``labels``."""
        labels = _labels(vocab, labels)
        delta = np.repeat(np.arange(2, dtype=np.int64)[:, None], vocab, axis=1)
        delta[:, labels] ^= 1
        return ConstraintDFA(delta, np.array([True, False]))

    @staticmethod
    def contains(vocab: int, seq: Sequence[int]) -> "ConstraintDFA":
        """The label sequence contains ``seq`` as a contiguous sub-sequence (the Knuth-Morris-Pratt automaton,
        len(seq) + 1 states; the last one absorbs)."""
        seq = [int(x) for x in seq]
        _labels(vocab, seq)
        n = len(seq)
        if not 1 <= n < MAX_STATES:
            raise ValueError(f"seq must have 1 .. {MAX_STATES - 1} labels")
        delta = np.zeros((n + 1, vocab), np.int64)
        delta[0, seq[0]] = 1
        x = 0  # the state the longest proper border of seq[:q] leads to
        for q in range(1, n):
            delta[q] = delta[x]
            delta[q, seq[q]] = q + 1
            x = int(delta[x, seq[q]])
        delta[n] = n
        final = np.zeros(n + 1, bool)
        final[n] = True
        return ConstraintDFA(delta, final)

    @staticmethod
    def marked_sequence(vocab: int, marker: int, seq: Sequence[int]) -> "ConstraintDFA":
        """The labels that directly follow ``marker`` spell ``seq``: state 2 j = j of them read, state 2 j + 1 = the
        marker read after j of them (2 (len(seq) + 1) states; the last one has no transition).  With ``synth.edit_lattice``'s
        convention -- ``output_mark`` followed by the output symbol -- this is how the numerator lattice x o T o y sits
        inside the denominator lattice x o T."""
        seq = [int(x) for x in seq]
        _labels(vocab, seq + [marker])
        n = len(seq)
        if 2 * (n + 1) > MAX_STATES:
            raise ValueError(f"seq must have at most {MAX_STATES // 2 - 1} labels")
        delta = np.full((2 * (n + 1), vocab), -1, np.int64)
        for j in range(n + 1):
            delta[2 * j] = 2 * j
            delta[2 * j, marker] = 2 * j + 1
            if j < n:
                delta[2 * j + 1, seq[j]] = 2 * j + 2
        final = np.zeros(2 * (n + 1), bool)
        final[2 * n] = True
        return ConstraintDFA(delta, final)


MAX_WIDE_STATES = 4096


class WideDFA:
    """``WideDFA(dflt, exc_off, exc_label, exc_dst, final, q_off=None, weight_dflt=None, weight_exc=None, vocab=None)``:
    a deterministic automaton of 1 .. 4096 states, start state 0, stored sparsely (``nfst_intersect_wide_count`` /
    ``_write``, DESIGN.md sections 2 and 4.19): ``delta(q, l) = exc_dst[k]`` if some ``k`` in ``[exc_off[q], exc_off[q+1])``
    has ``exc_label[k] == l``, else ``dflt[q]``; -1 (in either place) means no transition.  The labels of a state's
    exceptions ascend strictly.  Reading rules are ``ConstraintDFA``'s.

    ``q_off = None``: one automaton for the batch.  ``q_off [n + 1]``: n automata, one per lattice, concatenated without
    padding (``dflt``, ``final`` ``[sum Q]``, ``exc_off [sum Q + 1]`` over all of them; targets relative to their own
    automaton).  ``weight_dflt [sum Q]`` / ``weight_exc [E]``: optional float log weights of the default and of every
    exception (tensors; they may require grad; give both or neither), added by ``IntersectResult.scores``.  ``vocab``:
    the number of labels, if known (the builders know it); ``check`` then refuses a batch over another vocabulary.
    Raises ``ValueError`` for Q outside 1 .. 4096, offsets that do not ascend or do not cover the arrays, targets
    outside -1 .. Q-1, negative labels, labels that do not ascend inside a state and mismatched weights."""

    def __init__(self, dflt, exc_off, exc_label, exc_dst, final, q_off=None, weight_dflt=None, weight_exc=None, vocab=None):
        ints = lambda a, name: self._ints(a, name)
        dflt, exc_off, exc_label, exc_dst = ints(dflt, "dflt"), ints(exc_off, "exc_off"), ints(exc_label, "exc_label"), ints(exc_dst, "exc_dst")
        fin = _np(final).reshape(-1)
        self.per_lattice = q_off is not None
        q_off = np.array([0, dflt.size], np.int64) if q_off is None else ints(q_off, "q_off")
        if q_off.size < 2 or q_off[0] != 0 or q_off[-1] != dflt.size:
            raise ValueError(f"q_off must run from 0 to the number of states, {dflt.size}")
        Q = np.diff(q_off)
        if (Q < 1).any() or (Q > MAX_WIDE_STATES).any():
            raise ValueError(f"an automaton has 1 .. {MAX_WIDE_STATES} states, not {int(Q.max() if (Q > MAX_WIDE_STATES).any() else Q.min())}")
        S, E = dflt.size, exc_label.size
        if fin.size != S:
            raise ValueError(f"final must have one entry per state, {S}")
        if exc_dst.size != E:
            raise ValueError("exc_label and exc_dst must have one entry per exception")
        if exc_off.size != S + 1 or exc_off[0] != 0 or exc_off[-1] != E or (np.diff(exc_off) < 0).any():
            raise ValueError(f"exc_off must have {S + 1} ascending entries from 0 to the number of exceptions, {E}")
        q_of = np.repeat(Q, Q)  # the states of every state's automaton
        if (dflt < -1).any() or (dflt >= q_of).any():
            raise ValueError("entries of dflt must lie in -1 .. Q-1 of their automaton")
        state_of = np.repeat(np.arange(S), np.diff(exc_off))  # the state of every exception
        if E and ((exc_dst < -1).any() or (exc_dst >= q_of[state_of]).any()):
            raise ValueError("entries of exc_dst must lie in -1 .. Q-1 of their automaton")
        if E and exc_label.min() < 0:
            raise ValueError("labels must not be negative")
        if vocab is not None and (vocab < 1 or (E and exc_label.max() >= vocab)):
            raise ValueError(f"labels must lie in 0 .. {vocab - 1}")
        if E > 1 and ((np.diff(exc_label) <= 0) & (np.diff(state_of) == 0)).any():
            raise ValueError("the labels of a state's exceptions must ascend strictly")
        if (weight_dflt is None) != (weight_exc is None):
            raise ValueError("give weight_dflt and weight_exc, or neither")
        if weight_dflt is not None:
            for t, n, name in ((weight_dflt, S, "weight_dflt"), (weight_exc, E, "weight_exc")):
                if not isinstance(t, torch.Tensor) or not t.dtype.is_floating_point or tuple(t.shape) != (n,):
                    raise ValueError(f"{name} must be a float tensor of {n} entries")
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        self.q_off, self.dflt, self.exc_off, self.exc_label, self.exc_dst = i32(q_off), i32(dflt), i32(exc_off), i32(exc_label), i32(exc_dst)
        self.final = np.ascontiguousarray(fin != 0)
        self.weight_dflt, self.weight_exc = weight_dflt, weight_exc
        self.vocab = None if vocab is None else int(vocab)
        self._state_of = state_of
        self._device = {}

    @staticmethod
    def _ints(a, name) -> np.ndarray:
        a = _np(a).reshape(-1)
        if a.size and not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.bool_)):
            raise ValueError(f"{name} must hold integers")
        return a.astype(np.int64)

    # ---------------------------------------------------------------- shape
    @property
    def n_states(self) -> int:
        """The largest Q."""
        return int(np.diff(self.q_off).max())

    @property
    def n_lattices(self) -> Optional[int]:
        """B for per-lattice automata, None for one automaton shared by the batch."""
        return self.q_off.size - 1 if self.per_lattice else None

    @property
    def weighted(self) -> bool:
        return self.weight_dflt is not None

    def check(self, vocab: int, n_lattices: int) -> None:
        if self.vocab is not None and self.vocab != vocab:
            raise ValueError(f"the automaton reads {self.vocab} labels, the batch has {vocab}")
        if self.exc_label.size and int(self.exc_label.max()) >= vocab:
            raise ValueError(f"the automaton names label {int(self.exc_label.max())}, the batch has {vocab} labels")
        if self.n_lattices is not None and self.n_lattices != n_lattices:
            raise ValueError(f"{self.n_lattices} automata for a batch of {n_lattices} lattices")

    # ---------------------------------------------------------------- device layout
    def to(self, device):
        """``(q_off, dflt, exc_off, exc_label, exc_dst, final)`` on ``device`` (int32, ``final`` uint8), built once per
        device; ``exc_label`` / ``exc_dst`` hold at least one entry so that their pointers are valid."""
        device = torch.device(device)
        hit = self._device.get(device)
        if hit is None:
            some = lambda a: a if a.size else np.full(1, -1, np.int32)
            hit = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in
                        (self.q_off, self.dflt, self.exc_off, some(self.exc_label), some(self.exc_dst), self.final.astype(np.uint8)))
            self._device[device] = hit
        return hit

    # ---------------------------------------------------------------- on the host
    def _delta(self, state: int, l: int) -> int:
        lo, hi = int(self.exc_off[state]), int(self.exc_off[state + 1])
        k = lo + int(np.searchsorted(self.exc_label[lo:hi], l))
        return int(self.exc_dst[k]) if k < hi and self.exc_label[k] == l else int(self.dflt[state])

    def run(self, labels: Iterable[int], b: Optional[int] = None) -> int:
        """The state after reading ``labels`` from state 0 (-1: a step had no transition); ``b`` picks the automaton."""
        base = int(self.q_off[0 if b is None else b])
        q = 0
        for l in labels:
            q = self._delta(base + q, int(l))
            if q < 0:
                return -1
        return q

    def accepts(self, labels: Iterable[int], b: Optional[int] = None) -> bool:
        q = self.run(labels, b)
        return q >= 0 and bool(self.final[int(self.q_off[0 if b is None else b]) + q])

    def to_dense(self, vocab: Optional[int] = None):
        """``(delta [Q, V] int64, final [Q] bool)``; for per-lattice automata a list of them, one per automaton."""
        V = vocab if vocab is not None else self.vocab
        if V is None:
            raise ValueError("to_dense needs the vocabulary size")
        if self.exc_label.size and int(self.exc_label.max()) >= V:
            raise ValueError(f"the automaton names label {int(self.exc_label.max())}, beyond {V} labels")
        delta = np.repeat(self.dflt.astype(np.int64)[:, None], V, axis=1)
        delta[self._state_of, self.exc_label] = self.exc_dst
        out = [(delta[a:b].copy(), self.final[a:b].copy()) for a, b in zip(self.q_off[:-1], self.q_off[1:])]
        return out if self.per_lattice else out[0]

    def _score_keys(self, device, vocab: int):
        """``(keys, offsets)`` on ``device``, built once per device and vocabulary: the sorted int64 keys
        ``state * vocab + label`` of the exceptions and the first state of every automaton."""
        hit = self._device.get((device, vocab))
        if hit is None:
            hit = (torch.from_numpy(self._state_of.astype(np.int64) * vocab + self.exc_label).to(device),
                   torch.from_numpy(self.q_off[:-1].astype(np.int64)).to(device))
            self._device[(device, vocab)] = hit
        return hit

    def arc_weights(self, arc_q: torch.Tensor, label: torch.Tensor, vocab: int, arc_lattice: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The float32 weight of reading ``label`` in state ``arc_q`` (of automaton ``arc_lattice``, for per-lattice
        automata), per entry, in torch on the tensors' device: the key (automaton offset + q) * vocab + label is looked
        up in the sorted keys of the exceptions (``torch.searchsorted``); a hit gathers ``weight_exc``, a miss
        ``weight_dflt`` of the state.  ``vocab`` is the vocabulary of the BATCH the labels come from (every label lies
        below it), not a property of the automaton: a smaller stride would let a label run into the next state's keys.
        Autograd flows to both weight tensors."""
        dev, vocab = label.device, int(vocab)
        if self.exc_label.size and int(self.exc_label.max()) >= vocab:
            raise ValueError(f"the automaton names label {int(self.exc_label.max())}, beyond {vocab} labels")
        keys, offsets = self._score_keys(dev, vocab)
        state = arc_q.to(torch.int64)
        if self.per_lattice:
            state = state + offsets[arc_lattice.to(torch.int64)]
        out = self.weight_dflt.to(device=dev, dtype=torch.float32)[state]
        if keys.numel():
            key = state * vocab + label.to(torch.int64)
            k = torch.searchsorted(keys, key).clamp_(max=keys.numel() - 1)
            out = torch.where(keys[k] == key, self.weight_exc.to(device=dev, dtype=torch.float32)[k], out)
        return out

    # ---------------------------------------------------------------- builders
    @staticmethod
    def from_dense(delta, final, weight=None) -> "WideDFA":
        """From a ``[Q, V]`` table.  Unweighted: the default of a state is its row's most frequent target (ties: the
        smallest), the other labels are its exceptions.  With ``weight [Q, V]`` (a float tensor) a default could carry
        only one weight for all its labels, so every label is an exception and ``weight_exc`` is ``weight`` flattened (a
        view: gradients reach ``weight``)."""
        d = _np(delta)
        if d.ndim != 2 or d.shape[1] < 1:
            raise ValueError(f"delta must be [Q, V]; got {d.shape}")
        d = WideDFA._ints(d, "delta").reshape(d.shape)
        Q, V = d.shape
        if d.min() < -1 or d.max() >= Q:
            raise ValueError(f"entries of delta must lie in -1 .. {Q - 1}")
        counts = np.zeros((Q, Q + 1), np.int64)
        np.add.at(counts, (np.repeat(np.arange(Q), V), (d + 1).reshape(-1)), 1)
        dflt = counts.argmax(axis=1) - 1  # (argmax takes the first of equal counts: the smallest target)
        if weight is not None:
            if not isinstance(weight, torch.Tensor):
                weight = torch.as_tensor(np.asarray(weight), dtype=torch.float32)
            if tuple(weight.shape) != (Q, V) or not weight.dtype.is_floating_point:
                raise ValueError(f"weight must be a float tensor shaped as delta, {(Q, V)}")
            exc = np.ones((Q, V), bool)
        else:
            exc = d != dflt[:, None]
        q_idx, l_idx = np.nonzero(exc)
        exc_off = np.zeros(Q + 1, np.int64)
        np.cumsum(exc.sum(axis=1), out=exc_off[1:])
        wd = None if weight is None else torch.zeros(Q, dtype=weight.dtype, device=weight.device)
        return WideDFA(dflt, exc_off, l_idx, d[q_idx, l_idx], final, weight_dflt=wd,
                       weight_exc=None if weight is None else weight.reshape(-1), vocab=V)

    @staticmethod
    def from_constraint(c: ConstraintDFA) -> "WideDFA":
        if c.n_lattices is None:
            return WideDFA.from_dense(c.delta, c.final, c.weight)
        return WideDFA.stack([WideDFA.from_dense(c.delta[b], c.final[b], None if c.weight is None else c.weight[b])
                              for b in range(c.n_lattices)])

    @staticmethod
    def stack(dfas: Sequence["WideDFA"]) -> "WideDFA":
        """Per-lattice automata from shared ones, ragged: concatenated as they are, no padding."""
        dfas = list(dfas)
        if not dfas or any(d.per_lattice for d in dfas) or len({d.vocab for d in dfas}) != 1:
            raise ValueError("stack takes single automata over one vocabulary")
        if len({d.weighted for d in dfas}) != 1:
            raise ValueError("either every automaton carries weights or none does")
        q_off = np.cumsum([0] + [d.dflt.size for d in dfas])
        e_off = np.cumsum([0] + [d.exc_label.size for d in dfas])
        exc_off = np.concatenate([d.exc_off[:-1].astype(np.int64) + e for d, e in zip(dfas, e_off)] + [e_off[-1:]])
        cat = lambda k: np.concatenate([getattr(d, k) for d in dfas])
        w = dfas[0].weighted
        return WideDFA(cat("dflt"), exc_off, cat("exc_label"), cat("exc_dst"), cat("final"), q_off=q_off,
                       weight_dflt=torch.cat([d.weight_dflt for d in dfas]) if w else None,
                       weight_exc=torch.cat([d.weight_exc for d in dfas]) if w else None, vocab=dfas[0].vocab)

    @staticmethod
    def accept_all(vocab: int) -> "WideDFA":
        return WideDFA([0], [0, 0], [], [], [True], vocab=vocab)

    @staticmethod
    def sequence(vocab: int, seq: Sequence[int]) -> "WideDFA":
        """The labels spell ``seq`` exactly (len(seq) + 1 states: the labels read so far); the caller includes bos and
        eos."""
        seq = _labels(vocab, seq)
        n = seq.size
        if not 1 <= n < MAX_WIDE_STATES:
            raise ValueError(f"seq must have 1 .. {MAX_WIDE_STATES - 1} labels")
        final = np.zeros(n + 1, bool)
        final[n] = True
        return WideDFA(np.full(n + 1, -1), np.minimum(np.arange(n + 2), n), seq, np.arange(1, n + 1), final, vocab=vocab)

    @staticmethod
    def marked_sequence(vocab: int, marker: int, seq: Sequence[int]) -> "WideDFA":
        """The labels that directly follow ``marker`` spell ``seq``: the automaton and the state numbering of
        ``ConstraintDFA.marked_sequence`` (state 2 j: j of them read, a loop on every label but the marker; state 2 j + 1:
        the marker read after j of them), for up to 2047 symbols."""
        seq = _labels(vocab, seq)
        _labels(vocab, [marker])
        n = seq.size
        if 2 * (n + 1) > MAX_WIDE_STATES:
            raise ValueError(f"seq must have at most {MAX_WIDE_STATES // 2 - 1} labels")
        Q = 2 * (n + 1)
        dflt = np.where(np.arange(Q) % 2 == 0, np.arange(Q), -1)
        # one exception per state but the last: the marker in an even state, the next symbol in an odd one
        exc_label = np.empty(Q - 1, np.int64)
        exc_label[0::2] = marker
        exc_label[1::2] = seq
        final = np.zeros(Q, bool)
        final[2 * n] = True
        return WideDFA(dflt, np.minimum(np.arange(Q + 1), Q - 1), exc_label, np.arange(1, Q), final, vocab=vocab)

    @staticmethod
    def projected_sequence(vocab: int, keep: Iterable[int], seq: Sequence[int]) -> "WideDFA":
        """The labels of the path that belong to ``keep`` spell ``seq``; every other label loops (len(seq) + 1 states:
        the kept labels read so far)."""
        keep = np.unique(_labels(vocab, keep))
        seq = _labels(vocab, seq)
        n, K = seq.size, keep.size
        if n + 1 > MAX_WIDE_STATES:
            raise ValueError(f"seq must have at most {MAX_WIDE_STATES - 1} labels")
        if not np.isin(seq, keep).all():
            raise ValueError("every label of seq must belong to keep")
        exc_dst = np.full((n + 1, K), -1, np.int64)
        if n:
            exc_dst[np.arange(n), np.searchsorted(keep, seq)] = np.arange(1, n + 1)
        final = np.zeros(n + 1, bool)
        final[n] = True
        return WideDFA(np.arange(n + 1), np.arange(n + 2) * K, np.tile(keep, n + 1), exc_dst.reshape(-1), final, vocab=vocab)

    @staticmethod
    def bigram(logp, start_logp=None) -> "WideDFA":
        """A bigram model over the labels as a weighted automaton: ``logp [V, V]`` float tensor, ``logp[prev, l]`` the log
        weight of label ``l`` after ``prev``; ``start_logp [V]`` that of the first label (zeros if absent).  V + 1 states:
        0 before any label, 1 + l after label ``l``; every state but 0 is final.  V <= 4095.  Every transition is an
        exception, so the weights are the caller's tensors, flattened: gradients reach them."""
        if not isinstance(logp, torch.Tensor):
            logp = torch.as_tensor(np.asarray(logp), dtype=torch.float32)
        if logp.dim() != 2 or logp.shape[0] != logp.shape[1] or not logp.dtype.is_floating_point:
            raise ValueError("logp must be a float [V, V] tensor")
        V = int(logp.shape[0])
        if not 1 <= V < MAX_WIDE_STATES:
            raise ValueError(f"a bigram automaton takes 1 .. {MAX_WIDE_STATES - 1} labels")
        if start_logp is None:
            start_logp = torch.zeros(V, dtype=logp.dtype, device=logp.device)
        elif not isinstance(start_logp, torch.Tensor):
            start_logp = torch.as_tensor(np.asarray(start_logp), dtype=logp.dtype)
        if tuple(start_logp.shape) != (V,):
            raise ValueError(f"start_logp must have {V} entries")
        final = np.ones(V + 1, bool)
        final[0] = False
        return WideDFA(np.full(V + 1, -1), np.arange(V + 2) * V, np.tile(np.arange(V), V + 1), np.tile(np.arange(1, V + 1), V + 1),
                       final, weight_dflt=torch.zeros(V + 1, dtype=logp.dtype, device=logp.device),
                       weight_exc=torch.cat([start_logp.to(logp.device), logp.reshape(-1)]), vocab=V)


def constraint_log_prob(lat, theta: torch.Tensor, dfa, arc_scores: Optional[torch.Tensor] = None, **pack_opts) -> torch.Tensor:
    """``ops.constraint_log_prob``: float32 ``[B]``, log Z of the product of ``lat`` with ``dfa`` (either automaton type), scored by
    ``IntersectResult.scores(arc_scores)`` -- the input's per-arc scores plus the automaton's weights --, minus log Z of
    ``lat``: the log of the (weighted) share of the accepted paths; for an unweighted automaton a log probability, <= 0.
    With ``WideDFA.marked_sequence`` on a denominator lattice x o T it is log p(y | x) from that lattice alone.
    Differentiable in ``theta``, ``arc_scores`` and the automaton's weights through ``log_z``.  Raises as ``intersect``
    does (an empty product: the probability is zero)."""
    from . import ops

    res = ops.intersect(lat, dfa, **pack_opts)
    return ops.log_z(res.lattice, theta, res.scores(arc_scores)) - ops.log_z(lat, theta, arc_scores)


def _labels(vocab: int, labels) -> np.ndarray:
    labels = np.asarray(list(labels), dtype=np.int64).reshape(-1)
    if vocab < 1 or (labels.size and (labels.min() < 0 or labels.max() >= vocab)):
        raise ValueError(f"labels must lie in 0 .. {vocab - 1}")
    return labels

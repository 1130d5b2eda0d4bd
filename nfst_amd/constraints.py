"""Constraint automata: small deterministic automata (DFAs) over the label vocabulary that
``LatticeBatch.intersect`` / ``ops.intersect`` multiply into every lattice of a batch (``nfst_intersect_count`` /
``_write``, DESIGN.md sections 2 and 4.8).

An automaton has Q states, 1 <= Q <= 64, and starts in state 0.  ``delta[q, l]`` in {-1, 0 .. Q-1} is the state after
reading label ``l`` in state ``q`` (-1: no transition), ``final[q]`` says whether a run may end in ``q``.  It reads the
label of every arc of a path, ``bos`` and ``eos`` included, never the sink's pad loop.  One automaton serves the whole
batch (``[Q, V]`` / ``[Q]``) or every lattice has its own (``[B, Q, V]`` / ``[B, Q]``).
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


def _labels(vocab: int, labels) -> np.ndarray:
    labels = np.asarray(list(labels), dtype=np.int64).reshape(-1)
    if vocab < 1 or (labels.size and (labels.min() < 0 or labels.max() >= vocab)):
        raise ValueError(f"labels must lie in 0 .. {vocab - 1}")
    return labels

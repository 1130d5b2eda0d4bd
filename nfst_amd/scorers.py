"""Host-side mirror of the reference's lattice scorer interface.

``LatticeScorer`` keeps the method names, argument meaning and error behaviour of
``FSAGRUScorer`` (/root/reference/src/modules/scorers.py:604-1054) for the lattice
part of that class -- ``set_masks``, ``set_k``, ``compute_beta``,
``update_fsa_state``, ``mask_out_invalid`` -- and of ``WFSTScorer`` (1663-1687) for
the arc weights ("an arc's weight is solely decided by the mark on it"): one
learnable score ``theta[mark]``.  Every method is a thin call into the HIP engine
(nfst_amd.ops); nothing is computed on the CPU.  The recurrent proposal network
of the reference (GRUCell, queries) is out of scope.
"""
from __future__ import annotations

from typing import Any, Dict, Optional

import torch

from . import ops, swor
from .lattice import LatticeBatch


class LatticeScorer(torch.nn.Module):
    def __init__(self, vocab_size: int, pad: int = 0, bos: int = 1, eos: int = 2, max_length: int = 400,
                 theta: Optional[torch.Tensor] = None, k: int = 1, chunks=False):
        """``chunks``: cut the chunked programs of the sweeps in ``set_masks`` (``LatticeBatch.from_dense``: False, True =
        when the cost model says they are faster, ``"force"``).  On tables that live on the GPU the cut runs on the device
        and adds a read-back to every ``set_masks``; worth it for deep, narrow machines (the SNIPS tagging shape) whose
        batch is swept more than once per ``set_masks``, or swept for long."""
        super().__init__()
        assert vocab_size > 3  # scorers.py:223
        self.vocab_size = vocab_size
        self.__pad__, self.__bos__, self.__eos__ = pad, bos, eos
        self.max_length = max_length
        self.k = k
        init = torch.zeros(vocab_size) if theta is None else torch.as_tensor(theta, dtype=torch.float32).clone()
        self.theta = torch.nn.Parameter(init)
        self.lattice: Optional[LatticeBatch] = None
        self.use_beta = True
        self.chunks = chunks

    # ------------------------------------------------------------ tables
    def set_masks(self, emission: torch.Tensor, transition: torch.Tensor):
        """scorers.py:877-885.  The dense tables are packed once (arcs + tile
        programs); K samples share them, nothing is expanded."""
        assert len(emission.shape) == 3
        assert len(transition.shape) == 3
        with torch.no_grad():
            self.lattice = LatticeBatch.from_dense(emission, transition, device=self.theta.device, chunks=self.chunks)
        return self

    def set_lattice(self, lattice: LatticeBatch):
        self.lattice = lattice.to(self.theta.device)
        return self

    def set_k(self, k: int):
        """scorers.py:887-918 materialises K copies of the tables; here K is only a
        launch parameter."""
        self.k = int(k)

    def _lat(self) -> LatticeBatch:
        assert self.lattice is not None, "set_masks() first"
        return self.lattice

    # ------------------------------------------------------------ beta sweep
    def compute_log_beta(self) -> torch.Tensor:
        """log beta ``[B*k, S+1]`` (rows unreachable from state 0 are -inf)."""
        lat = self._lat()
        r = ops.backward(lat, self.theta.detach())
        return lat.rows_view(r.logbeta).repeat_interleave(self.k, dim=0)

    def compute_beta(self) -> torch.Tensor:
        """``[B*k, S+1]`` in the probability domain like scorers.py:858-875 returns
        (float32: overflows to inf beyond log beta ~ 88, as the reference does)."""
        return torch.exp(self.compute_log_beta())

    def log_z(self) -> torch.Tensor:
        """Differentiable exact log Z per lattice ``[B]``; d/d theta = expected mark counts."""
        return ops.log_z(self._lat(), self.theta)

    def entropy(self) -> torch.Tensor:
        """Differentiable exact path entropy per lattice ``[B]`` (nats); d/d theta = -Cov(mark counts, path score)."""
        return ops.entropy(self._lat(), self.theta)

    def k_best(self, k: int, max_len: Optional[int] = None) -> "ops.KBestResult":
        """The k best paths of every lattice with their scores under ``theta`` (``ops.k_best``; ``best`` is
        differentiable in theta)."""
        return ops.k_best(self._lat(), self.theta, k, max_len=max_len, pad=self.__pad__)

    def sample_without_replacement(self, k: int, **kw) -> "swor.SworResult":
        """``k`` distinct paths per lattice drawn without replacement from the exact posterior under ``theta``, with
        their perturbed scores and the threshold of the Horvitz-Thompson weights (``swor.sample``; ``kw``: ``max_len``,
        ``uniforms``, ``seed``, ``beta``, ``want_arcs``)."""
        kw.setdefault("pad", self.__pad__)
        return swor.sample(self._lat(), self.theta.detach(), k, **kw)

    def positional_log_z(self, pos_scores: torch.Tensor) -> torch.Tensor:
        """Differentiable exact log Z per lattice ``[B]`` when the mark at position t also scores ``pos_scores[(b,) t,
        mark]`` (``ops.positional_log_z``): per-position logits of a tagger, marginalised over the lattice."""
        return ops.positional_log_z(self._lat(), self.theta, pos_scores)

    def positional_expectation(self, pos_scores: torch.Tensor, **values) -> torch.Tensor:
        """Differentiable exact E[V] per lattice ``[B]`` under ``theta`` plus per-position scores
        (``ops.positional_expectation``; ``values``: ``pos_values``, ``label_values``, ``arc_values``, ``score_coef``,
        ``T``)."""
        return ops.positional_expectation(self._lat(), self.theta, pos_scores, **values)

    def positional_entropy(self, pos_scores: torch.Tensor) -> torch.Tensor:
        """Differentiable exact entropy per lattice ``[B]`` (nats) of the paths of at most T arcs under ``theta`` plus
        per-position scores (``ops.positional_entropy``)."""
        return ops.positional_entropy(self._lat(), self.theta, pos_scores)

    def positional_risk(self, pos_scores: torch.Tensor, cost: torch.Tensor) -> torch.Tensor:
        """The minimum-risk objective: the exact expected cost per lattice ``[B]`` of the tagger's output against
        ``cost[(b,) t, mark]`` (expected Hamming loss for a 0/1 cost against a gold sequence), differentiable in ``theta``,
        ``pos_scores`` and ``cost``."""
        return ops.positional_expectation(self._lat(), self.theta, pos_scores, pos_values=cost)

    def length_distribution(self, T: Optional[int] = None):
        """``(log P(L = t) [B, T + 1], logz64 [B])`` over the paths of at most ``T`` arcs (``ops.length_distribution``)."""
        return ops.length_distribution(self._lat(), self.theta.detach(), T=T)

    def positional_viterbi(self, pos_scores: torch.Tensor) -> "ops.PositionalViterbiResult":
        """The best path under ``theta`` plus per-position scores (``ops.positional_viterbi``)."""
        return ops.positional_viterbi(self._lat(), self.theta.detach(), pos_scores, pad=self.__pad__)

    def positional_k_best(self, pos_scores: torch.Tensor, k: int) -> "ops.PositionalKBestResult":
        """The k best paths of every lattice under ``theta`` plus per-position scores (``ops.positional_k_best``;
        ``best`` is differentiable in theta and ``pos_scores``)."""
        return ops.positional_k_best(self._lat(), self.theta, k, pos_scores, pad=self.__pad__)

    def positional_nbest(self, pos_scores: torch.Tensor, k: int) -> list:
        """The reranker's list: per lattice ``[(log p, marks), ...]``, best first, of its (at most ``k``) best mark
        sequences under ``theta`` plus per-position scores, log p = best - log Z_T (float64, the log Z of
        ``ops.positional_forward_backward``): the exact probability of each entry among the paths of at most T arcs."""
        lat, theta = self._lat(), self.theta.detach()
        r = ops.positional_k_best_terms(lat, theta, k, pos_scores, pad=self.__pad__)
        z = ops.positional_forward_backward(lat, theta, pos_scores, want_pos_posterior=False).logz64
        logp = (r.best.double() - z[:, None]).cpu().numpy()
        paths, lens, n = r.paths.cpu().numpy(), r.lengths.cpu().numpy(), r.n_paths.cpu().numpy()
        return [[(float(logp[b, j]), paths[b, j, :lens[b, j]].tolist()) for j in range(int(n[b]))] for b in range(lat.n_lattices)]

    @staticmethod
    def _mbr_entries(r) -> list:
        from .decoders import mbr_decode

        index, risk, _ = mbr_decode(r)
        pick = index.clamp(min=0)
        rows = torch.arange(index.shape[0], device=index.device)
        marks, lens = r.paths[rows, pick].cpu().numpy(), r.lengths[rows, pick].cpu().numpy()
        index, risk = index.cpu().numpy(), risk[rows, pick].cpu().numpy()
        return [(float(risk[b]), marks[b, :lens[b]].tolist()) if index[b] >= 0 else (float("inf"), [])
                for b in range(len(index))]

    def mbr(self, k: int, draws: str = "k_best", **kw) -> list:
        """Minimum-Bayes-risk decoding under edit distance: per lattice ``(risk, marks)``, the mark sequence among ``k``
        candidates whose expected edit distance to the candidates, weighed by their probabilities, is least, and that
        expectation (``decoders.mbr_decode``).  ``draws="k_best"``: the k best paths under ``theta``, weighed by their
        scores; ``"swor"``: k paths drawn without replacement (``kw``: ``seed``, ``uniforms``, ...), weighed by their
        Horvitz-Thompson weights.  ``kw`` goes to the draw (``max_len`` for both).  A lattice without a path gives
        ``(inf, [])``."""
        if draws == "k_best":
            r = ops.k_best_terms(self._lat(), self.theta.detach(), k, pad=self.__pad__, **kw)
        elif draws == "swor":
            r = self.sample_without_replacement(k, **kw)
        else:
            raise ValueError(f"draws must be 'k_best' or 'swor', not {draws!r}")
        return self._mbr_entries(r)

    def decode_strings(self, k: int, **kw) -> list:
        """The best output strings of every lattice: per lattice ``[(log p, symbols), ...]``, best first, the distinct
        strings that the ``k`` best (``method="swor"``: drawn) paths spell on the tape ``keep`` or ``marker``, each with
        its exact log p(y | x) under ``theta`` (``decoders.decode_strings``; ``kw``: ``keep``, ``marker``, ``method``,
        ``rescore``, ``seed``)."""
        from .decoders import decode_strings

        r = decode_strings(self._lat(), self.theta.detach(), k, pad=self.__pad__, **kw)
        logp, rows, lens, n = (x.cpu().numpy() for x in (r.log_prob, r.strings, r.lengths, r.n_strings))
        return [[(float(logp[b, j]), rows[b, j, :lens[b, j]].tolist()) for j in range(int(n[b]))] for b in range(len(n))]

    def string_log_prob(self, strings: torch.Tensor, lengths: torch.Tensor, **kw) -> torch.Tensor:
        """The reranker's call: exact log p(y | x) float64 [B, M] of the candidate strings ``strings[b, m, :lengths[b,
        m]]`` under ``theta`` (``ops.string_log_prob``; ``kw``: ``keep`` or ``marker``); -inf for a string that no path
        spells.  Differentiable in ``theta``."""
        return ops.string_log_prob(self._lat(), self.theta, strings, lengths, **kw).log_prob

    def string_next_log_probs(self, prefixes: torch.Tensor, lengths: torch.Tensor, marker: Optional[int] = 4, **kw):
        """Incremental decoding: ``ops.NextSymbols`` of the prefixes ``prefixes[b, m, :lengths[b, m]]`` under ``theta``
        (``ops.string_next_log_probs``): the exact mass of every one-symbol extension, of the prefix as a complete
        string and of the prefix itself.  The tape is ``marker`` (default: the output mark 4) or ``keep=`` a set of
        labels.  No gradient."""
        tape = dict(keep=kw.pop("keep")) if kw.get("keep") is not None else dict(marker=marker)
        return ops.string_next_log_probs(self._lat(), self.theta.detach(), prefixes, lengths, **tape, **kw)

    def prefix_context(self, marker: Optional[int] = 4, **kw):
        """An ``ops.PrefixContext`` on the lattices under the ``theta`` of this moment (``ops.string_prefix_open``): prefix
        states that grow by one symbol per sweep, for incremental decoding at O(arcs) per symbol.  The tape is ``marker``
        (default: the output mark 4) or ``keep=`` a set of labels.  Open it again after ``theta`` changes.  No gradient."""
        tape = dict(keep=kw.pop("keep")) if kw.get("keep") is not None else dict(marker=marker)
        return ops.string_prefix_open(self._lat(), self.theta.detach(), **tape, **kw)

    def prefix_search(self, k: int = 8, marker: Optional[int] = 4, **kw):
        """The most probable output strings of every lattice by exact prefix beam search: ``decoders.PrefixSearchResult``
        (``decoders.prefix_search``; ``kw``: ``max_len``, ``incremental``, ``keep`` in place of ``marker``), whose ``exact`` flags say where
        the first string is provably the most probable one."""
        from .decoders import prefix_search

        tape = dict(keep=kw.pop("keep")) if kw.get("keep") is not None else dict(marker=marker)
        return prefix_search(self._lat(), self.theta.detach(), k, pad=self.__pad__, **tape, **kw)

    def align(self, strings: torch.Tensor, lengths: torch.Tensor, marker: Optional[int] = 4, **kw) -> list:
        """Forced alignment under ``theta``: per lattice a list with one ``(score, marks, align)`` per candidate string
        ``strings[b, m, :lengths[b, m]]`` -- the score of the best path that spells it, that path's marks and, per mark,
        the position of the string it emitted or -1 (``ops.string_viterbi``).  The tape is ``marker`` (default: the output
        mark 4) or ``keep=`` a set of labels; ``kw`` also takes ``max_len``.  A string that no path spells gives
        ``(-inf, [], [])``."""
        tape = dict(keep=kw.pop("keep")) if kw.get("keep") is not None else dict(marker=marker)
        kw.pop("keep", None)
        r = ops.string_viterbi(self._lat(), self.theta.detach(), strings, lengths, pad=self.__pad__, **tape, **kw)
        score, marks, al, lens = (x.cpu().numpy() for x in (r.score, r.paths, r.align, r.lengths))
        return [[(float(score[b, m]), marks[b, m, :lens[b, m]].tolist(), al[b, m, :lens[b, m]].tolist()) for m in range(score.shape[1])]
                for b in range(score.shape[0])]

    def sample_alignments(self, strings: torch.Tensor, lengths: torch.Tensor, k: int, marker: Optional[int] = 4, **kw):
        """``k`` exact draws per lattice and candidate string from p(path | x, y) under ``theta``, each with its exact
        log-probability: ``ops.StringSampleResult`` (``ops.string_sample_paths``; ``kw``: ``keep`` in place of ``marker``,
        ``uniforms``, ``seed``, ``max_len``).  No gradient."""
        tape = dict(keep=kw.pop("keep")) if kw.get("keep") is not None else dict(marker=marker)
        kw.pop("keep", None)
        kw.setdefault("pad", self.__pad__)
        return ops.string_sample_paths(self._lat(), self.theta.detach(), strings, lengths, k, **tape, **kw)

    def string_nll(self, strings: torch.Tensor, lengths: torch.Tensor, **kw) -> torch.Tensor:
        """The maximum-likelihood loss on strings: the mean over the batch of -log p(y | x), y = ``strings[b, 0,
        :lengths[b, 0]]`` the one reference string of lattice b (``strings`` [B, 1, N]; ``kw``: ``keep`` or ``marker``),
        float64 and differentiable in ``theta``.  ValueError if a lattice has no path that spells its string."""
        if strings.dim() != 3 or strings.shape[1] != 1:
            raise ValueError("strings must hold one reference string per lattice, [B, 1, N]")
        lp = self.string_log_prob(strings, lengths, **kw)
        if bool(torch.isneginf(lp).any()):
            raise ValueError("string_nll: a string has probability 0 (no path of its lattice spells it)")
        return -lp.mean()

    def _oracle(self, ref: torch.Tensor, ref_lengths: Optional[torch.Tensor]) -> tuple:
        """``(ops.LatticeEditResult, ref_lengths)`` of the oracle path under ``theta``; without ``ref_lengths`` the trailing
        entries of a row equal to the scorer's pad do not count."""
        ref = torch.as_tensor(ref)
        if ref_lengths is None:
            keep = ref != self.__pad__
            last = torch.arange(1, ref.shape[1] + 1, device=ref.device) * keep
            ref_lengths = last.max(dim=1).values if ref.shape[1] else torch.zeros(ref.shape[0], dtype=torch.int64, device=ref.device)
        ref_lengths = torch.as_tensor(ref_lengths)
        return ops.lattice_edit_distance(self._lat(), ref, ref_lengths, self.theta.detach(), pad=self.__pad__), ref_lengths

    def oracle(self, ref: torch.Tensor, ref_lengths: Optional[torch.Tensor] = None) -> list:
        """The oracle path of every lattice against the gold marks ``ref`` [B, R]: per lattice ``(distance, marks)``, the
        least edit distance of any path to ``ref[b, :ref_lengths[b]]`` and the mark sequence that attains it, the one of
        the greatest score under ``theta`` among equals (``ops.lattice_edit_distance``).  With ``ref_lengths=None``
        trailing entries equal to the scorer's pad do not count.  A lattice without a path gives ``(-1, [])``."""
        r, _ = self._oracle(ref, ref_lengths)
        dist, marks, lens = r.distance.cpu().numpy(), r.paths.cpu().numpy(), r.lengths.cpu().numpy()
        return [(int(dist[b]), marks[b, :lens[b]].tolist()) for b in range(len(dist))]

    def oracle_error_rate(self, ref: torch.Tensor, ref_lengths: Optional[torch.Tensor] = None) -> float:
        """The lattices' oracle error rate: the summed oracle distances over the summed reference lengths, over the
        lattices that have a path (NaN when no reference token is left to count)."""
        r, n = self._oracle(ref, ref_lengths)
        dist = r.distance.cpu().to(torch.int64)
        n = n.reshape(-1).cpu().to(torch.int64)
        has = dist >= 0
        total = int(n[has].sum())
        return float(dist[has].sum()) / total if total else float("nan")

    def positional_mbr(self, pos_scores: torch.Tensor, k: int, draws: str = "k_best", **kw) -> list:
        """``mbr`` under ``theta`` plus per-position scores and their length budget (``positional_k_best`` or
        ``positional_sample_without_replacement`` give the candidates)."""
        if draws == "k_best":
            r = ops.positional_k_best_terms(self._lat(), self.theta.detach(), k, pos_scores, pad=self.__pad__, **kw)
        elif draws == "swor":
            r = self.positional_sample_without_replacement(pos_scores, k, **kw)
        else:
            raise ValueError(f"draws must be 'k_best' or 'swor', not {draws!r}")
        return self._mbr_entries(r)

    def positional_sample(self, pos_scores: torch.Tensor, k: int, **kw) -> "ops.PositionalSampleResult":
        """``k`` exact draws per lattice under ``theta`` plus per-position scores, each with its log-probability
        (``ops.positional_sample_paths``; ``kw``: ``T``, ``uniforms``, ``seed``, ``want_arcs``)."""
        kw.setdefault("pad", self.__pad__)
        return ops.positional_sample_paths(self._lat(), self.theta.detach(), k, pos_scores, **kw)

    def positional_sample_without_replacement(self, pos_scores: torch.Tensor, k: int, **kw) -> "swor.SworResult":
        """``k`` distinct paths per lattice drawn without replacement under ``theta`` plus per-position scores, with
        their perturbed scores and the threshold of the Horvitz-Thompson weights (``swor.positional_sample``; ``kw``:
        ``T``, ``uniforms``, ``seed``, ``want_arcs``)."""
        kw.setdefault("pad", self.__pad__)
        return swor.positional_sample(self._lat(), self.theta.detach(), k, pos_scores, **kw)

    def positional_score(self, pos_scores: torch.Tensor, marks: torch.Tensor):
        """``(path_score, end_state, lengths)`` of the forced walk of ``marks`` [B, K, T] under the same scores
        (``ops.positional_score_paths``)."""
        return ops.positional_score_paths(self._lat(), self.theta.detach(), marks, pos_scores)

    def beam_decoder(self, score_fn, reorder_fn=None, sync_every: int = 8):
        """A ``decoders.BeamDecoder`` over the scorer's lattice for a path-dependent ``score_fn(hx, inp) -> (hx,
        scores [N, V])``: ``.decode(k, lookahead=...)`` keeps k hypotheses per lattice."""
        from .decoders import BeamDecoder

        return BeamDecoder(self, score_fn, reorder_fn=reorder_fn, sync_every=sync_every)

    def prune(self, beam, **pack_opts) -> "ops.PruneResult":
        """The scorer's lattice cut down to the arcs within ``beam`` of each lattice's best path under ``theta``
        (``ops.prune``): ``(lat, arc_map, n_kept, best)``.  The scorer keeps its own lattice; hand the result to
        ``set_lattice`` to go on with the pruned one."""
        return ops.prune(self._lat(), self.theta.detach(), beam, **pack_opts)

    def constrain(self, dfa, **pack_opts) -> "ops.IntersectResult":
        """The scorer's lattice under a constraint automaton (``ops.intersect``): ``(lattice, arc_map, arc_q, row_state,
        row_q)``.  The scorer keeps its own lattice; hand ``result.lattice`` to ``set_lattice`` to go on under the
        constraint."""
        return ops.intersect(self._lat(), dfa, **pack_opts)

    def constraint_log_prob(self, dfa, **pack_opts) -> torch.Tensor:
        """log Z of the scorer's lattice under ``dfa`` minus its log Z, per lattice, under ``theta``
        (``ops.constraint_log_prob``)."""
        return ops.constraint_log_prob(self._lat(), self.theta, dfa, **pack_opts)

    # ------------------------------------------------------------ per-step gathers
    def update_fsa_state(self, updated: torch.Tensor, prev_states: torch.Tensor) -> torch.Tensor:
        """scorers.py:683-690."""
        return ops.step(self._lat(), prev_states, updated, k=self.k)

    def mask_out_invalid(self, inp: torch.Tensor, metadata: Dict[str, Any]) -> torch.Tensor:
        """scorers.py:1037-1054 on top of 314-338 (bos/pad/eos legality)."""
        assert self.lattice is not None
        assert "length" in metadata
        return ops.emission_mask(self._lat(), metadata["state"], k=self.k, inp=inp, pad=self.__pad__, bos=self.__bos__,
                                 eos=self.__eos__, has_to_end=metadata["length"] > self.max_length)

    def beta_logits(self, beta: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
        """scorers.py:584-590: ``gather(beta, 1, transition_k[arange, state])``; beta ``[B*k, S+1]``
        with identical rows per lattice (as compute_beta returns) or ``[B, S+1]``."""
        lat = self._lat()
        rows = beta[:: self.k] if beta.shape[0] == lat.n_lattices * self.k and self.k > 1 else beta
        return ops.beta_logits(lat, rows.reshape(-1), state, k=self.k)

    # ------------------------------------------------------------ WFSTScorer
    def wfst_score(self, t: torch.Tensor) -> torch.Tensor:
        """scorers.py:1685-1687: sum over non-pad marks of theta[mark]."""
        assert len(t.shape) == 2
        sc = self.theta[t]
        return torch.where(t == self.__pad__, torch.zeros_like(sc), sc).sum(dim=1)

    def forward(self, sequence: torch.Tensor, **kwargs):
        return self.wfst_score(sequence)


class NeuralBetaScorer(LatticeScorer):
    """The ``use_beta=True`` part of ``FSAGRUScorer`` (scorers.py:954-970): parameters ``Wh``, ``Wx``
    [H, H], ``W`` [1, H], ``beta_bias`` [H] and the mark ``embeddings`` [V, H], initialised as
    there; ``compute_beta`` is the message-passing sweep of scorers.py:692-751 / 753-856 on the HIP
    engine (``ops.backward_neural``) and follows the per-sample semantics -- parallel arcs between
    a state pair count once each."""

    def __init__(self, hid_dim: int, vocab_size: int, **kw):
        super().__init__(vocab_size, **kw)
        self.hid_dim = hid_dim
        self.embeddings = torch.nn.Embedding(vocab_size, hid_dim)
        self.Wh = torch.nn.Parameter(torch.empty(hid_dim, hid_dim))
        self.Wx = torch.nn.Parameter(torch.empty(hid_dim, hid_dim))
        self.W = torch.nn.Parameter(torch.empty(1, hid_dim))
        for p in (self.Wh, self.Wx, self.W):
            torch.nn.init.xavier_uniform_(p)
        self.beta_bias = torch.nn.Parameter(torch.zeros(hid_dim))

    def compute_beta_hat(self):
        """``(log beta [B*k, S+1], beta_hat [B*k, S+1, H])``.  Differentiable in the five parameters
        (``tune_proposal`` trains them through it): under autograd the call keeps the forward workspace for the
        backward pass -- 2 B max_rows (H + 1) floats, 1.1 GB at H = 256 on the BASELINE batch.  A caller that only
        samples wraps the call in ``torch.no_grad()`` and nothing is kept."""
        lat = self._lat()
        r = ops.backward_neural(lat, self.embeddings.weight, self.Wx, self.Wh, self.W, self.beta_bias)
        return (lat.rows_view(r.log_beta).repeat_interleave(self.k, dim=0),
                lat.rows_view(r.beta_hat).repeat_interleave(self.k, dim=0))

    def compute_log_beta(self) -> torch.Tensor:
        return self.compute_beta_hat()[0]

"""Phonotactic language models for the CTC beam search: a bigram over a phoneme inventory as the dense table that
``amx_beam_ctc_lm_emissions`` fuses while it searches (``beam_ctc_decode(..., lm=...)``, ``Estimator.beam_decode``).

A ``PhonotacticLM`` over ``C`` classes holds a float32 ``[C + 1, C + 1]`` table of natural-log scores.  Row ``p`` is the
previous token of a prefix and row ``C`` begin (the empty prefix); column ``n`` is the next token and column ``C`` end.  The
blank's row and column are never read.  Entries are finite or ``-inf``; ``-inf`` forbids the transition at every weight.
The vocabulary is a language's inventory, so the table is small and can be estimated from any phonemised word list
(``from_sequences``) or read from an ARPA file of order 1 or 2 (``from_arpa``)."""
from __future__ import annotations

import math
import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

BEGIN, END = "<s>", "</s>"


class PhonotacticLM:
    """``table``: ``[C + 1, C + 1]`` natural-log scores (see the module docstring); ``blank``: the blank's class.  NaN and
    ``+inf`` entries are refused."""

    def __init__(self, table, blank: int = 0):
        table = torch.as_tensor(table)
        if table.dim() != 2 or table.shape[0] != table.shape[1]:
            raise ValueError(f"a language-model table is [C + 1, C + 1], got {tuple(table.shape)}")
        if table.shape[0] < 3:
            raise ValueError("a language model needs at least 2 classes")
        if not 0 <= int(blank) < table.shape[0] - 1:
            raise ValueError("blank out of range")
        table = table.detach().to(torch.float32).contiguous()
        if bool(torch.isnan(table).any()) or bool((table == math.inf).any()):
            raise ValueError("language-model scores are finite or -inf: the table holds NaN or +inf")
        self.table: Tensor = table
        self.blank = int(blank)

    @property
    def classes(self) -> int:
        return self.table.shape[0] - 1

    def __repr__(self) -> str:
        return f"PhonotacticLM(classes={self.classes}, blank={self.blank}, device={self.table.device})"

    @classmethod
    def from_counts(cls, bigram_counts, blank: int = 0, smoothing: float = 1.0) -> "PhonotacticLM":
        """Add-k estimate from ``bigram_counts`` ``[C + 1, C + 1]`` (row ``C``: begin, column ``C``: end): entry
        ``log((count + k) / (row total + k * V))`` with each row normalised over the ``V = C`` events "a non-blank class or
        end".  With ``smoothing=0`` an unseen bigram is ``-inf``, as is every entry of a row without counts."""
        counts = torch.as_tensor(bigram_counts).to(torch.float64)
        if counts.dim() != 2 or counts.shape[0] != counts.shape[1] or counts.shape[0] < 3:
            raise ValueError(f"bigram counts are [C + 1, C + 1] with C >= 2, got {tuple(counts.shape)}")
        if not bool(torch.isfinite(counts).all()) or bool((counts < 0).any()) or not math.isfinite(smoothing) or smoothing < 0:
            raise ValueError("counts and smoothing must be finite and non-negative")
        if not 0 <= int(blank) < counts.shape[0] - 1:
            raise ValueError("blank out of range")
        events = torch.ones(counts.shape[0], dtype=torch.bool)
        events[blank] = False
        smoothed = (counts + smoothing) * events
        total = smoothed.sum(1, keepdim=True)
        table = torch.where((smoothed > 0) & (total > 0), torch.log(smoothed / total.clamp_min(1e-300)),
                            torch.full_like(smoothed, -math.inf))
        table[blank, :] = 0.0  # never read
        table[:, blank] = 0.0
        return cls(table, blank)

    @classmethod
    def from_sequences(cls, sequences: Iterable[Sequence[int]], classes: int, blank: int = 0, smoothing: float = 1.0) -> "PhonotacticLM":
        """Add-k bigram of phoneme id sequences (e.g. a phonemised word list), begin and end included."""
        if classes < 2:
            raise ValueError("a language model needs at least 2 classes")
        counts = torch.zeros(classes + 1, classes + 1, dtype=torch.float64)
        for sequence in sequences:
            previous = classes
            for token in sequence:
                token = int(token)
                if not 0 <= token < classes or token == blank:
                    raise ValueError(f"token {token} is not a non-blank class of {classes}")
                counts[previous, token] += 1
                previous = token
            counts[previous, classes] += 1
        return cls.from_counts(counts, blank, smoothing)

    @classmethod
    def from_arpa(cls, text_or_path: str, symbols: Sequence[str], blank: int = 0) -> "PhonotacticLM":
        """An ARPA language model of order 1 or 2 over ``symbols`` (``symbols[c]``: the word of class ``c``; the blank's entry
        is ignored).  log10 becomes ln; a missing bigram is ``backoff(previous) + unigram(next)``; ``<s>`` and ``</s>`` become
        the begin row and the end column; a symbol the file does not list gets ``-inf`` (row and column).  Order 3 or higher
        raises ``ValueError``."""
        text = text_or_path
        if "\\data\\" not in text and "\n" not in text:
            with open(os.fspath(text_or_path), encoding="utf-8") as handle:
                text = handle.read()
        unigrams, bigrams = _parse_arpa(text)
        C = len(symbols)
        if C < 2:
            raise ValueError("a language model needs at least 2 classes")
        rows = list(symbols) + [BEGIN]
        columns = list(symbols) + [END]
        ln10 = math.log(10.0)
        table = torch.full((C + 1, C + 1), -math.inf, dtype=torch.float64)
        for p, previous in enumerate(rows):
            if p == blank or previous not in unigrams:
                continue
            backoff = unigrams[previous][1]
            for n, following in enumerate(columns):
                if n == blank or following not in unigrams:
                    continue
                score = bigrams.get((previous, following))
                table[p, n] = ln10 * (backoff + unigrams[following][0] if score is None else score)
        table[blank, :] = 0.0  # never read
        table[:, blank] = 0.0
        return cls(table, blank)

    def restrict(self, columns) -> "PhonotacticLM":
        """The table over a sub-inventory: ``columns`` are the kept classes in their new order, the blank among them (what
        ``LanguageInventories.columns`` gives).  Scores are taken as they are, not renormalised."""
        columns = [int(c) for c in (columns.tolist() if isinstance(columns, Tensor) else columns)]
        if len(set(columns)) != len(columns) or any(not 0 <= c < self.classes for c in columns):
            raise ValueError("columns must be distinct classes of the language model")
        if self.blank not in columns:
            raise ValueError("columns must keep the blank")
        index = torch.tensor(columns + [self.classes], dtype=torch.int64, device=self.table.device)
        return PhonotacticLM(self.table.index_select(0, index).index_select(1, index), columns.index(self.blank))

    def to(self, device) -> "PhonotacticLM":
        moved = PhonotacticLM.__new__(PhonotacticLM)
        moved.table = self.table.to(device)
        moved.blank = self.blank
        return moved

    @staticmethod
    def stack(lms: Sequence["PhonotacticLM"]) -> Tensor:
        """``[n_lm, C + 1, C + 1]``, the stack a decode call takes; the models must agree in classes and blank."""
        lms = list(lms)
        if not lms:
            raise ValueError("at least one language model is needed")
        if any(lm.classes != lms[0].classes or lm.blank != lms[0].blank for lm in lms):
            raise ValueError("language models of one call must have the same classes and blank")
        return torch.stack([lm.table for lm in lms]).contiguous()


def _parse_arpa(text: str) -> Tuple[Dict[str, Tuple[float, float]], Dict[Tuple[str, str], float]]:
    """word -> (log10 probability, log10 backoff) and (previous, next) -> log10 probability."""
    unigrams: Dict[str, Tuple[float, float]] = {}
    bigrams: Dict[Tuple[str, str], float] = {}
    order = 0
    seen_data = False
    for raw in text.splitlines():
        line = raw.strip()
        if not line:
            continue
        if line == "\\data\\":
            seen_data = True
        elif line == "\\end\\":
            break
        elif line.startswith("ngram "):
            if int(line[6:].split("=")[0]) > 2:
                raise ValueError("ARPA language models of order 1 or 2 only")
        elif line.startswith("\\") and line.endswith("-grams:"):
            order = int(line[1:-7])
            if order > 2:
                raise ValueError("ARPA language models of order 1 or 2 only")
        elif order:
            fields = line.split()
            if len(fields) < order + 1:
                raise ValueError(f"malformed ARPA line: {raw!r}")
            score = float(fields[0])
            if order == 1:
                unigrams[fields[1]] = (score, float(fields[2]) if len(fields) > 2 else 0.0)
            else:
                bigrams[(fields[1], fields[2])] = score
    if not seen_data or not unigrams:
        raise ValueError("not an ARPA language model: no \\data\\ section with 1-grams")
    return unigrams, bigrams


LMs = Union[PhonotacticLM, Sequence[PhonotacticLM]]


def lm_call(lm: LMs, lm_ids, utterances: int) -> Tuple[List[PhonotacticLM], Tensor]:
    """The models of a decode call as a list, and the int32 host ``lm_ids`` ``[utterances]`` (-1: the row runs without a
    model); left as ``None`` every row runs under the only model."""
    lms = [lm] if isinstance(lm, PhonotacticLM) else list(lm)
    if not lms or not all(isinstance(m, PhonotacticLM) for m in lms):
        raise ValueError("lm must be a PhonotacticLM or a sequence of them")
    if lm_ids is None:
        if len(lms) != 1:
            raise ValueError("several language models need lm_ids, one index per utterance")
        ids = torch.zeros(utterances, dtype=torch.int32)
    else:
        ids = torch.as_tensor(lm_ids).detach().to("cpu", torch.int32).reshape(-1)
        if ids.numel() != utterances:
            raise ValueError(f"{ids.numel()} lm_ids for {utterances} utterances")
        if ids.numel() and (int(ids.min()) < -1 or int(ids.max()) >= len(lms)):
            raise ValueError(f"lm_ids must be -1 or index the {len(lms)} language models")
    return lms, ids


def check_scalars(lm_weight: float, token_score: float) -> None:
    if not math.isfinite(lm_weight) or not math.isfinite(token_score):
        raise ValueError("lm_weight and token_score must be finite")

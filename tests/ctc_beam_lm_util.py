"""Executable form of the CTC beam-search contract with a token-level language model: flashlight's
``LexiconFreeDecoder`` with a bigram instead of ZeroLM, restated in plain float64 NumPy: the frame loop is
``ctc_beam_util.search``, which both restatements share and which states the tie rule.  It enumerates every (state, token)
candidate of every frame.  The HIP kernel (amx_ctc_beam_lm.hip) is held to it in test_gpu_beam_lm.py and, on tied inputs,
in test_gpu_beam_ties.py; it is held to brute force over all alignments in test_ctc_beam_lm_contract.py.

``table`` is ``[C + 1, C + 1]``: row = previous token of the prefix (row C: begin), column = next token (column C: end).  A
pair (state, token n) that emits a new token after the prefix P scores ``(s + e[t, n]) + (weight * table[last(P), n] +
token_score)``; an -inf entry forbids the transition at every weight.  The frame threshold is taken against the best
generated candidate.  At the end every state adds ``weight * table[last(P), C]``, and an -inf entry drops the state.
``table=None`` is the decoder without a language model."""
from typing import List, Optional, Tuple

import numpy as np

from ctc_beam_util import THRESHOLD, Hypothesis, brute_force, search


def beam_search_lm(em, length: int, beam_width: int, n_best: int, table, weight: float = 1.0, token_score: float = 0.0,
                   blank: int = 0, exp: bool = True, threshold: float = THRESHOLD, reverse_ties: bool = False,
                   report: Optional[dict] = None) -> List[Hypothesis]:
    """Decodes one utterance: ``em`` fp32 [T, C]; frames at or beyond min(length, T) are ignored.  Ties resolve by the rule
    stated at ``ctc_beam_util.search``, which holds the one frame loop of both restatements; ``reverse_ties`` and ``report``
    are for tests and described there."""
    return search(em, length, beam_width, n_best, table, weight, token_score, blank=blank, exp=exp, threshold=threshold,
                  reverse_ties=reverse_ties, report=report)


def lm_score(labelling, table, weight: float, token_score: float) -> float:
    """What the language model adds to a whole labelling: every token's term and the end term (-inf if forbidden)."""
    lm = np.asarray(table, dtype=np.float32).astype(np.float64)
    C = lm.shape[0] - 1
    total, previous = 0.0, C
    for token in labelling:
        if not np.isfinite(lm[previous, token]):
            return -np.inf
        total += weight * lm[previous, token] + token_score
        previous = token
    if not np.isfinite(lm[previous, C]):
        return -np.inf
    return total + weight * lm[previous, C]


def brute_force_lm(em, length: int, table, weight: float = 1.0, token_score: float = 0.0, blank: int = 0, exp: bool = True
                   ) -> List[Tuple[Tuple[int, ...], float]]:
    """``brute_force``'s exact labelling scores plus each labelling's language-model, bonus and end terms; forbidden
    labellings are left out.  Sorted by descending score."""
    fused = []
    for labelling, score in brute_force(em, length, blank=blank, exp=exp):
        extra = lm_score(labelling, table, weight, token_score)
        if np.isfinite(extra):
            fused.append((labelling, score + extra))
    return sorted(fused, key=lambda kv: -kv[1])

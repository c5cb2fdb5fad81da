"""Executable form of the CTC beam-search contract with a token-level language model: flashlight's
``LexiconFreeDecoder`` with a bigram instead of ZeroLM, restated in plain float64 NumPy over the helpers of
``ctc_beam_util``.  It enumerates every (state, token) candidate of every frame.  The HIP kernel (amx_ctc_beam_lm.hip) is
held to it in test_gpu_beam_lm.py, and it is held to brute force over all alignments in test_ctc_beam_lm_contract.py.

``table`` is ``[C + 1, C + 1]``: row = previous token of the prefix (row C: begin), column = next token (column C: end).  A
pair (state, token n) that emits a new token after the prefix P scores ``(s + e[t, n]) + (weight * table[last(P), n] +
token_score)``; an -inf entry forbids the transition at every weight.  The frame threshold is taken against the best
generated candidate.  At the end every state adds ``weight * table[last(P), C]``, and an -inf entry drops the state.
``table=None`` is the decoder without a language model."""
from typing import List, Optional, Tuple

import numpy as np

from ctc_beam_util import THRESHOLD, Hypothesis, _fold, _Trie, brute_force, emissions_as_added


def beam_search_lm(em, length: int, beam_width: int, n_best: int, table, weight: float = 1.0, token_score: float = 0.0,
                   blank: int = 0, exp: bool = True, threshold: float = THRESHOLD) -> List[Hypothesis]:
    """Decodes one utterance: ``em`` fp32 [T, C]; frames at or beyond min(length, T) are ignored."""
    em = np.asarray(em)
    T, C = em.shape
    L = max(0, min(int(length), T))
    e = emissions_as_added(em[:L], exp)
    lm = None if table is None else np.asarray(table, dtype=np.float32).astype(np.float64)
    if lm is not None:
        assert lm.shape == (C + 1, C + 1)
    weight, token_score = float(weight), float(token_score)
    trie = _Trie()
    pid = np.array([0], dtype=np.int64)
    k = np.array([blank], dtype=np.int64)
    b = np.array([False])
    s = np.array([0.0])
    back: List[Tuple[np.ndarray, np.ndarray]] = []
    n_all = np.arange(C, dtype=np.int64)

    def last_of(ids):
        last = np.array(trie.last)[ids]
        return np.where(last < 0, C, last)

    for t in range(L):
        S = len(s)
        x = (s[:, None] + e[t][None, :]).ravel()
        slot = np.repeat(np.arange(S), C)
        n = np.tile(n_all, S)
        ks, bs, ps = k[slot], b[slot], pid[slot]
        parent = np.array(trie.parent)[ps]
        last = np.array(trie.last)[ps]
        emit = (n != blank) & ((n != ks) | bs)
        is_blank = n == blank
        generated = np.ones(len(x), dtype=bool)
        if lm is not None:
            entry = lm[last_of(ps), n]
            allowed = np.isfinite(entry)
            a = weight * np.where(allowed, entry, 0.0) + token_score
            x = np.where(emit, x + a, x)
            generated = ~emit | allowed
        key = np.empty((len(x), 4), dtype=np.int64)
        key[:, 0] = np.where(emit, ps, parent)
        key[:, 1] = np.where(emit, n, last)
        key[:, 2] = np.where(is_blank, blank, n)
        key[:, 3] = np.where(is_blank, 1, 0)
        best = np.max(x[generated])
        keep = generated & ~(x < best - threshold)
        key, x, slot, n = key[keep], x[keep], slot[keep], n[keep]
        gkeys, acc, head = _fold(key, x)
        top = np.argsort(-acc, kind="stable")[:beam_width]
        gkeys, acc, head = gkeys[top], acc[top], head[top]
        pid = np.array([0 if pk[1] < 0 else trie.get(int(pk[0]), int(pk[1])) for pk in gkeys], dtype=np.int64)
        k = gkeys[:, 2].copy()
        b = gkeys[:, 3].astype(bool)
        s = acc
        back.append((slot[head], n[head]))
    # end: every state becomes (P, blank, false, s + weight * table[last(P), end]), merged by prefix
    alive = np.ones(len(s), dtype=bool)
    if lm is not None:
        entry = lm[last_of(pid), C]
        alive = np.isfinite(entry)
        s = s + weight * np.where(alive, entry, 0.0)
    if not alive.any():
        return []
    keep = alive & ~(s < np.max(s[alive]) - threshold)
    gkeys, acc, head = _fold(pid[keep][:, None], s[keep])
    slots = np.flatnonzero(keep)[head]
    top = np.argsort(-acc, kind="stable")[:beam_width][:n_best]
    hyps = []
    for g in top:
        slot = int(slots[g])
        frames = [0] * L
        for t in range(L - 1, -1, -1):
            parents, tokens = back[t]
            frames[t] = int(tokens[slot])
            slot = int(parents[slot])
        out, ts, prev = [], [], blank
        for t, v in enumerate(frames):
            if v != blank and v != prev:
                out.append(v)
                ts.append(t + 1)
            prev = v
        hyps.append(Hypothesis(out, float(acc[g]), ts))
    return hyps


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

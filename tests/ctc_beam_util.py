"""Executable form of the CTC beam-search contract: the reference's ``BeamCTCDecoder`` is torchaudio's flashlight
``ctc_decoder`` built lexicon-free with no LM (ZeroLM), blank = silence, ``log_add=True``, ``beam_threshold=50`` and every
token considered per frame.  This module restates that decoder in plain float64 NumPy; it enumerates every (state, token)
candidate of every frame.  The HIP kernel (amx_ctc_beam.hip) is held to it in test_gpu_beam.py, and it is held to brute
force over all alignments in test_ctc_beam_oracle.py.

A state is (prefix P, last frame token k, prevBlank b).  A prefix is identified globally (ZeroLM keeps a trie): here by its
trie id, and inside one frame by the pair (id of P without its last token, last token)."""
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

THRESHOLD = 50.0


class Hypothesis(NamedTuple):
    tokens: List[int]
    score: float
    timesteps: List[int]


def emissions_as_added(em, exp: bool) -> np.ndarray:
    """The values flashlight adds: fp32 emissions, or (EXP) their fp32 exponentials, as float64.  The exponential is
    computed in float64 and rounded once to float32 (the correctly rounded expf), which is what the kernel computes."""
    em = np.asarray(em, dtype=np.float32)
    if exp:
        em = np.exp(em.astype(np.float64)).astype(np.float32)
    return em.astype(np.float64)


def logadd(a, c):
    hi, lo = np.maximum(a, c), np.minimum(a, c)
    return hi + np.log1p(np.exp(lo - hi))


class _Trie:
    def __init__(self):
        self.parent = [-1]   # prefix id -> id of the prefix without its last token
        self.last = [-1]     # prefix id -> last token
        self.child = {}

    def get(self, parent: int, token: int) -> int:
        key = (parent, token)
        node = self.child.get(key)
        if node is None:
            node = len(self.parent)
            self.child[key] = node
            self.parent.append(parent)
            self.last.append(token)
        return node


def _fold(keys: np.ndarray, x: np.ndarray):
    """Merges candidates with equal rows of ``keys``: members folded in descending order of x with log-add.  Returns the
    group keys, merged scores and the index of each group's highest member."""
    order = np.lexsort((-x,) + tuple(keys[:, c] for c in reversed(range(keys.shape[1]))))
    ks, xs = keys[order], x[order]
    start = np.ones(len(order), dtype=bool)
    start[1:] = np.any(ks[1:] != ks[:-1], axis=1)
    heads = np.flatnonzero(start)
    bounds = np.append(heads, len(order))
    acc = xs[heads].copy()
    for r in range(1, int(np.max(np.diff(bounds))) if len(heads) else 1):
        has = heads + r < bounds[1:]
        acc[has] = logadd(acc[has], xs[heads[has] + r])
    return ks[heads], acc, order[heads]


def beam_search(em, length: int, beam_width: int, n_best: int, blank: int = 0, exp: bool = True,
                threshold: float = THRESHOLD, end_threshold: Optional[float] = None) -> List[Hypothesis]:
    """Decodes one utterance: ``em`` fp32 [T, C]; frames at or beyond min(length, T) are ignored.  ``end_threshold``
    (default: ``threshold``) is the end step's, separate only so that tests can show which of the two cuts decides."""
    if end_threshold is None:
        end_threshold = threshold
    em = np.asarray(em)
    T, C = em.shape
    L = max(0, min(int(length), T))
    e = emissions_as_added(em[:L], exp)
    trie = _Trie()
    # beam: prefix id, last token, prevBlank, score; backpointers per frame: (parent slot, frame token)
    pid = np.array([0], dtype=np.int64)
    k = np.array([blank], dtype=np.int64)
    b = np.array([False])
    s = np.array([0.0])
    back: List[Tuple[np.ndarray, np.ndarray]] = []
    n_all = np.arange(C, dtype=np.int64)
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
        # resulting state as (parent prefix, last token of the prefix, k, b)
        key = np.empty((len(x), 4), dtype=np.int64)
        key[:, 0] = np.where(emit, ps, parent)
        key[:, 1] = np.where(emit, n, last)
        key[:, 2] = np.where(is_blank, blank, n)
        key[:, 3] = np.where(is_blank, 1, 0)
        best = np.max(x)
        keep = ~(x < best - threshold)
        key, x, slot, n = key[keep], x[keep], slot[keep], n[keep]
        gkeys, acc, head = _fold(key, x)
        top = np.argsort(-acc, kind="stable")[:beam_width]
        gkeys, acc, head = gkeys[top], acc[top], head[top]
        pid = np.array([0 if pk[1] < 0 else trie.get(int(pk[0]), int(pk[1])) for pk in gkeys], dtype=np.int64)
        k = gkeys[:, 2].copy()
        b = gkeys[:, 3].astype(bool)
        s = acc
        back.append((slot[head], n[head]))
    # end: every state becomes (P, blank, false, s), merged by prefix
    keep = ~(s < np.max(s) - end_threshold)
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


def brute_force(em, length: int, blank: int = 0, exp: bool = True) -> List[Tuple[Tuple[int, ...], float]]:
    """Exact prefix scores: for every labelling, the log-sum-exp over all C^T alignments that collapse to it of the summed
    emissions, sorted by descending score."""
    em = np.asarray(em)
    L = max(0, min(int(length), em.shape[0]))
    e = emissions_as_added(em[:L], exp)
    C = em.shape[1]
    scores = {}
    for a in np.ndindex(*([C] * L)):
        v = float(sum(e[t, a[t]] for t in range(L)))
        lab, prev = [], blank
        for n in a:
            if n != blank and n != prev:
                lab.append(n)
            prev = n
        lab = tuple(lab)
        scores[lab] = v if lab not in scores else float(logadd(scores[lab], v))
    return sorted(scores.items(), key=lambda kv: -kv[1])

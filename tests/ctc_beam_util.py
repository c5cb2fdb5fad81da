"""Executable form of the CTC beam-search contract: the reference's ``BeamCTCDecoder`` is torchaudio's flashlight
``ctc_decoder`` built lexicon-free with no LM (ZeroLM), blank = silence, ``log_add=True``, ``beam_threshold=50`` and every
token considered per frame.  This module restates that decoder in plain float64 NumPy; it enumerates every (state, token)
candidate of every frame.  The HIP kernel (amx_ctc_beam.hip) is held to it in test_gpu_beam.py, and it is held to brute
force over all alignments in test_ctc_beam_oracle.py.

A state is (prefix P, last frame token k, prevBlank b).  A prefix is identified globally (ZeroLM keeps a trie): here by its
trie id.  Equal scores resolve by the tie rule stated at ``search``, the one frame loop of this restatement and of the one
with a language model (tests/ctc_beam_lm_util.py); flashlight's own order among equal scores is not known here."""
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


def _fold(keys: np.ndarray, x: np.ndarray, rank: Optional[np.ndarray] = None):
    """Merges candidates with equal rows of ``keys``: members folded in descending order of x with log-add.  Returns the
    group keys in ascending row order, merged scores, the index of each group's highest member (of equal ones the one with
    the lowest ``rank``), and per group the smallest relative difference between that member and an unequal one."""
    if rank is None:
        rank = np.zeros(len(x), dtype=np.int64)
    order = np.lexsort((rank, -x) + tuple(keys[:, c] for c in reversed(range(keys.shape[1]))))
    ks, xs = keys[order], x[order]
    start = np.ones(len(order), dtype=bool)
    start[1:] = np.any(ks[1:] != ks[:-1], axis=1)
    heads = np.flatnonzero(start)
    bounds = np.append(heads, len(order))
    acc = xs[heads].copy()
    gap = np.full(len(heads), np.inf)
    for r in range(1, int(np.max(np.diff(bounds))) if len(heads) else 1):
        has = heads + r < bounds[1:]
        hi, lo = xs[heads[has]], xs[heads[has] + r]
        gap[has] = np.minimum(gap[has], np.where(hi != lo, _relative(hi, lo), np.inf))
        acc[has] = logadd(acc[has], lo)
    return ks[heads], acc, order[heads], gap


def _relative(a, c):
    """|a - c| relative to max(1, |a|, |c|): the measure of the 1e-9 score tolerance of the device tests."""
    return np.abs(a - c) / np.maximum(1.0, np.maximum(np.abs(a), np.abs(c)))


def _cut_gap(acc: np.ndarray, kept: np.ndarray) -> float:
    """The smallest relative difference between a kept and a dropped score that are not equal (inf if there is none)."""
    inside, outside = acc[kept], np.delete(acc, kept)
    outside = outside[np.isfinite(outside)]
    if not len(inside) or not len(outside):
        return np.inf
    gap = np.inf
    low, high = np.min(inside), np.max(outside)
    below, above = outside[outside < low], inside[inside > high]
    if len(below):
        gap = min(gap, float(_relative(low, np.max(below))))
    if len(above):
        gap = min(gap, float(_relative(np.min(above), high)))
    return gap


def _threshold_gap(x: np.ndarray, cut: float) -> float:
    x = x[np.isfinite(x) & (x != cut)]
    return float(np.min(_relative(x, cut))) if len(x) and np.isfinite(cut) else np.inf


def search(em, length: int, beam_width: int, n_best: int, table=None, weight: float = 1.0, token_score: float = 0.0,
           blank: int = 0, exp: bool = True, threshold: float = THRESHOLD, end_threshold: Optional[float] = None,
           reverse_ties: bool = False, report: Optional[dict] = None, restrict=None) -> List[Hypothesis]:
    """The decoder of ``beam_search`` and of ``ctc_beam_lm_util.beam_search_lm`` (``table``: see there; None: no language
    model), with the tie rule of DESIGN 9.

    Beam states are kept in slot order, the initial state in slot 0.  The merged candidates of a frame are ordered by
    (kind, slot, token): kind 0 is the successor (P, k, false) of a non-blank state in the beam, under that state's slot
    (the extensions of P[:-1] by k land here); kind 1 an extension to a state (P+n, n, false) that is not in the beam, under
    the lowest slot holding P and the token n; kind 2 the blank successor (P, blank, true), under the lowest slot holding
    P.  The survivors are the beam_width first by (score descending, then that order) and take the new slots in that
    order.  A merged candidate keeps the path of its highest member; of equal members the lower slot first, for kind 0 the
    state itself before the states of P[:-1].  The end step ranks by (merged score descending, then lowest slot of the
    prefix), equal members by lower slot.

    Arguments for tests only.  ``reverse_ties``: the same rule with the higher class index, slot and kind first.
    ``report``: a dict that receives ``gap``, the smallest relative difference between two unequal scores whose comparison
    decided something (a frame's survivors against the candidates it dropped, a member against the threshold, the highest
    member of a surviving group against the others, neighbours in the end ranking; the order among a frame's survivors
    decides nothing, since slots follow candidate order), and ``dropped``, the number of candidates that a threshold or
    the beam width dropped (the end step's n_best cut is not counted).  ``restrict``: a function called once per frame as
    ``restrict(e_t, a, permitted, lead)`` -- the C emissions as added, the [S, C] table terms, the [S, C] pairs that the
    table permits, and per slot the lowest slot of its prefix -- which returns an [S, C] mask: a kind 1 candidate is
    enumerated only where the mask is set, and the frame's best is taken over what remains.  It lets a test compare a
    reduced enumeration with this full one (``ctc_beam_ties_util.reduced_search``)."""
    if end_threshold is None:
        end_threshold = threshold
    sign = -1 if reverse_ties else 1
    em = np.asarray(em)
    T, C = em.shape
    L = max(0, min(int(length), T))
    e = emissions_as_added(em[:L], exp)
    lm = None if table is None else np.asarray(table, dtype=np.float32).astype(np.float64)
    if lm is not None:
        assert lm.shape == (C + 1, C + 1)
    weight, token_score = float(weight), float(token_score)
    trie = _Trie()
    # beam: prefix id, last token, prevBlank, score; backpointers per frame: (parent slot, frame token)
    pid = np.array([0], dtype=np.int64)
    k = np.array([blank], dtype=np.int64)
    b = np.array([False])
    s = np.array([0.0])
    back: List[Tuple[np.ndarray, np.ndarray]] = []
    n_all = np.arange(C, dtype=np.int64)
    gap, dropped = np.inf, 0

    def leaders(ids):
        first = {}
        return np.array([first.setdefault(int(p), j) for j, p in enumerate(ids)], dtype=np.int64)

    def row_of(ids):
        last = np.array(trie.last)[ids]
        return np.where(last < 0, C, last)

    for t in range(L):
        S = len(s)
        lead = leaders(pid)
        x = s[:, None] + e[t][None, :]
        slot = np.repeat(np.arange(S), C).reshape(S, C)
        n = np.tile(n_all, S).reshape(S, C)
        emit = (n != blank) & ((n != k[:, None]) | b[:, None])
        is_blank = n == blank
        generated = np.ones((S, C), dtype=bool)
        a = np.zeros((S, C))
        if lm is not None:
            entry = lm[row_of(pid)]
            allowed = np.isfinite(entry[:, :C])
            a = weight * np.where(allowed, entry[:, :C], 0.0) + token_score
            x = np.where(emit, x + a, x)
            generated = ~emit | allowed
        # the candidate each pair belongs to, as (kind, slot, token), and the pair's place among equal members
        kind = np.where(is_blank, 2, np.where(emit, 1, 0))
        cslot = np.where(kind == 0, slot, lead[slot])
        ctok = np.where(kind == 1, n, 0)
        rank = np.where(kind == 0, -1, slot)
        parent = np.array(trie.parent)[pid]
        for j in range(S):
            if k[j] != blank and not b[j]:
                for i in np.flatnonzero(pid == parent[j]):
                    if emit[i, k[j]]:
                        kind[i, k[j]], cslot[i, k[j]], ctok[i, k[j]] = 0, j, 0
        seen = generated
        if restrict is not None:
            listed = restrict(e[t], a, generated, lead)
            seen = generated & (listed | ~emit)
            generated = generated & (listed | (kind != 1))
        best = np.max(x[seen])
        keep = generated & ~(x < best - threshold)
        gap = min(gap, _threshold_gap(x[generated], best - threshold))
        dropped += int(np.sum(generated & ~keep))
        keys = sign * np.stack([kind[keep], cslot[keep], ctok[keep]], axis=1)
        x, slot, n = x[keep], slot[keep], n[keep]
        gkeys, acc, head, member_gap = _fold(keys, x, sign * rank[keep])
        top = np.sort(np.argsort(-acc, kind="stable")[:beam_width])
        gap = min(gap, _cut_gap(acc, top), float(np.min(member_gap[top])))
        dropped += len(acc) - len(top)
        gkeys, acc, head = sign * gkeys[top], acc[top], head[top]
        old_pid, old_k = pid, k
        pid = np.array([trie.get(int(old_pid[j]), int(tok)) if kd == 1 else old_pid[j] for kd, j, tok in gkeys], dtype=np.int64)
        k = np.array([tok if kd == 1 else (blank if kd == 2 else old_k[j]) for kd, j, tok in gkeys], dtype=np.int64)
        b = gkeys[:, 0] == 2
        s = acc
        back.append((slot[head], n[head]))
    # end: every state becomes (P, blank, false, s + weight * table[last(P), end]), merged by prefix
    alive = np.ones(len(s), dtype=bool)
    if lm is not None:
        entry = lm[row_of(pid), C]
        alive = np.isfinite(entry)
        s = s + weight * np.where(alive, entry, 0.0)
    if not alive.any():
        if report is not None:
            report.update(gap=gap, dropped=dropped)
        return []
    cut = np.max(s[alive]) - end_threshold
    keep = alive & ~(s < cut)
    gap = min(gap, _threshold_gap(s[alive], cut))
    dropped += int(np.sum(alive & ~keep))
    kept = np.flatnonzero(keep)
    gkeys, acc, head, member_gap = _fold(sign * leaders(pid)[kept][:, None], s[kept], sign * kept)
    slots = kept[head]
    top = np.argsort(-acc, kind="stable")[:beam_width][:n_best]
    ranked = acc[np.argsort(-acc, kind="stable")[:len(top) + 1]]
    steps = _relative(ranked[:-1], ranked[1:])[ranked[:-1] != ranked[1:]]
    gap = min([gap, float(np.min(member_gap[top]))] + ([float(np.min(steps))] if len(steps) else []))
    if report is not None:
        report.update(gap=gap, dropped=dropped)
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


def beam_search(em, length: int, beam_width: int, n_best: int, blank: int = 0, exp: bool = True,
                threshold: float = THRESHOLD, end_threshold: Optional[float] = None, reverse_ties: bool = False,
                report: Optional[dict] = None) -> List[Hypothesis]:
    """Decodes one utterance: ``em`` fp32 [T, C]; frames at or beyond min(length, T) are ignored.  ``end_threshold``
    (default: ``threshold``) is the end step's, separate only so that tests can show which of the two cuts decides.
    ``reverse_ties`` and ``report`` are for tests: see ``search``."""
    return search(em, length, beam_width, n_best, None, blank=blank, exp=exp, threshold=threshold, end_threshold=end_threshold,
                  reverse_ties=reverse_ties, report=report)


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

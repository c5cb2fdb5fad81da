"""The CTC search contract (include/allophant_amx_search.h) as executable code: a literal numpy fp32 restatement of the
recurrence, the tie rules and the outputs, the same a whole frame at a time (for the long rows of the GPU tests), and a
float64 brute force over every span and every class path for tiny rows."""
import itertools
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

NEG_INF = np.float32(-np.inf)


class Row(NamedTuple):
    status: int
    best_score: Optional[np.float32]
    best_span: Optional[Tuple[int, int]]
    end_scores: Optional[np.ndarray]  # float32 [T]; None for a malformed row
    end_starts: Optional[np.ndarray]  # int32 [T]


def _refused() -> Row:
    return Row(-2, None, None, None, None)


def frame_costs(lp: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """m[t] and the costs lp[t][c] - m[t] of every class (-inf where lp is -inf, also in a frame that is -inf throughout)."""
    T, C = lp.shape
    m = lp.max(axis=1) if T else np.zeros(0, np.float32)
    with np.errstate(invalid="ignore"):
        e = np.where(lp == NEG_INF, NEG_INF, lp - m[:, None]).astype(np.float32)
    return m, e


def _sweep_literal(lp: np.ndarray, y: List[int], blank: int):
    """The recurrence cell by cell, as the contract writes it."""
    T, S = lp.shape[0], 2 * len(y) - 1
    label = [y[i // 2] if i % 2 == 0 else blank for i in range(S)]
    d = np.full(S, NEG_INF, np.float32)
    b = np.full(S, -1, np.int32)
    end_scores, end_starts = np.zeros(T, np.float32), np.zeros(T, np.int32)
    for t in range(T):
        m = np.float32(max(lp[t]))
        nd, nb = np.empty(S, np.float32), np.empty(S, np.int32)
        for i in range(S):
            r, s = d[i], b[i]
            if i >= 1 and d[i - 1] > r:
                r, s = d[i - 1], b[i - 1]
            if i % 2 == 0 and i >= 2 and y[i // 2] != y[i // 2 - 1] and d[i - 2] > r:
                r, s = d[i - 2], b[i - 2]
            if i == 0 and 0 > r:
                r, s = np.float32(0), t
            x = lp[t, label[i]]
            e = NEG_INF if x == NEG_INF else np.float32(x - m)  # one fp32 subtraction
            nd[i], nb[i] = np.float32(r + e), s                 # one fp32 addition
        d, b = nd, nb
        end_scores[t] = d[S - 1]
        end_starts[t] = b[S - 1] if d[S - 1] > NEG_INF else -1
    return end_scores, end_starts


def _sweep_fast(lp: np.ndarray, y: List[int], blank: int):
    """The same comparisons, the same subtraction and the same single addition per cell, a whole frame at a time
    (tests/test_ctc_search_contract.py holds it equal to the literal sweep bit for bit)."""
    T, S = lp.shape[0], 2 * len(y) - 1
    states = np.arange(S)
    ids = np.asarray(y, np.int64)
    label = np.where(states % 2 == 0, ids[states // 2], blank)
    skip = np.zeros(S, bool)
    even = states[(states % 2 == 0) & (states >= 2)]
    skip[even] = ids[even // 2] != ids[even // 2 - 1]
    m, costs = frame_costs(lp)
    e = costs[:, label]  # [T, S]
    d = np.full(S, NEG_INF, np.float32)
    b = np.full(S, -1, np.int32)
    end_scores, end_starts = np.zeros(T, np.float32), np.zeros(T, np.int32)
    for t in range(T):
        x1 = np.concatenate((np.full(1, NEG_INF, np.float32), d[:-1]))
        s1 = np.concatenate((np.full(1, -1, np.int32), b[:-1]))
        x2 = np.where(skip, np.concatenate((np.full(2, NEG_INF, np.float32), d[:-2]))[:S], NEG_INF)
        s2 = np.concatenate((np.full(2, -1, np.int32), b[:-2]))[:S]
        r, s = d, b
        step = x1 > r
        r, s = np.where(step, x1, r), np.where(step, s1, s)
        jump = x2 > r
        r, s = np.where(jump, x2, r), np.where(jump, s2, s)
        if 0 > r[0]:
            r[0], s[0] = 0, t
        d, b = r + e[t], s.astype(np.int32)
        assert d.dtype == np.float32
        end_scores[t] = d[S - 1]
        end_starts[t] = b[S - 1] if d[S - 1] > NEG_INF else -1
    return end_scores, end_starts


def search_row(lp: np.ndarray, query: Sequence[int], blank: int = 0, fast: bool = False) -> Row:
    """One row: ``lp`` fp32 ``[T, C]`` (T = the utterance's frame length), ``query`` ``y[0..L)``."""
    lp = np.asarray(lp, dtype=np.float32)
    T, C = lp.shape
    y = [int(v) for v in query]
    if not y or any(v < 0 or v >= C or v == blank for v in y):
        return _refused()
    end_scores, end_starts = (_sweep_fast if fast else _sweep_literal)(lp, y, blank)
    best, span = NEG_INF, None
    for t in range(T):
        if end_scores[t] > NEG_INF and end_scores[t] >= best:
            best, span = end_scores[t], (int(end_starts[t]), t + 1)
    if span is None:
        return Row(-1, None, None, end_scores, end_starts)
    return Row(0, np.float32(best), span, end_scores, end_starts)


def search_batch(emissions: np.ndarray, lengths: Sequence[int], offsets: Sequence[int], ids: Sequence[int], max_query: int,
                 blank: int = 0, fast: bool = False) -> List[Row]:
    """The batch form as the C ABI takes it: ``emissions`` ``[N, T, C]``, frame lengths, CSR queries; rows ``n * Q + q``.  A
    row is refused (-2) for a frame length outside ``[0, T]``, offsets not ascending within ``[0, offsets[Q]]``, ``L == 0`` or
    ``L > max_query``."""
    N, T, _ = emissions.shape
    Q = len(offsets) - 1
    rows = []
    for n in range(N):
        length = int(lengths[n])
        for q in range(Q):
            lo, hi = int(offsets[q]), int(offsets[q + 1])
            if length < 0 or length > T or lo < 0 or hi <= lo or hi > int(offsets[Q]) or hi - lo > max_query:
                rows.append(_refused())
                continue
            rows.append(search_row(emissions[n, :length], list(ids[lo:hi]), blank, fast))
    return rows


def expected_buffers(emissions: np.ndarray, lengths, offsets, ids, max_query: int, blank: int, sentinel_i: int, sentinel_f: float):
    """What the device buffers hold after a call on buffers pre-filled with the sentinels: every entry the contract leaves
    untouched keeps its sentinel.  (best_scores, best_spans, status, end_scores, end_starts)."""
    N, T, _ = emissions.shape
    R = N * (len(offsets) - 1)
    best_scores = np.full(R, sentinel_f, np.float32)
    best_spans = np.full((R, 2), sentinel_i, np.int32)
    status = np.zeros(R, np.int32)
    end_scores = np.full((R, T), sentinel_f, np.float32)
    end_starts = np.full((R, T), sentinel_i, np.int32)
    for r, row in enumerate(search_batch(emissions, lengths, offsets, ids, max_query, blank, fast=True)):
        status[r] = row.status
        if row.status == -2:
            continue
        k = len(row.end_scores)
        end_scores[r, :k], end_starts[r, :k] = row.end_scores, row.end_starts
        if row.status == 0:
            best_scores[r], best_spans[r] = row.best_score, row.best_span
    return best_scores, best_spans, status, end_scores, end_starts


def pack_queries(queries: Sequence[Sequence[int]]) -> Tuple[List[int], List[int]]:
    offsets = np.concatenate(([0], np.cumsum([len(q) for q in queries]))).astype(int).tolist()
    return offsets, [int(v) for q in queries for v in q]


def minimum_frames(query: Sequence[int]) -> int:
    """Symbols plus one blank per adjacent repeat."""
    return len(query) + sum(1 for i in range(1, len(query)) if query[i] == query[i - 1])


def collapse(path: Sequence[int], blank: int) -> List[int]:
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def bruteforce(lp: np.ndarray, query: Sequence[int], blank: int = 0):
    """Float64, for tiny rows only: for every end frame t the best score over every span ``[s, t + 1)`` and every class path
    over it that collapses to ``query`` and starts and ends on its first and last symbol, with the set of starts that reach
    it.  Returns ``(best[t], starts[t])`` (``-inf`` and the empty set where no path has a finite score)."""
    lp64 = np.asarray(lp, dtype=np.float64)
    T, C = lp64.shape
    y = [int(v) for v in query]
    with np.errstate(invalid="ignore"):
        cost = np.where(lp64 == -np.inf, -np.inf, lp64 - lp64.max(axis=1, keepdims=True)) if T else lp64
    best = [-np.inf] * T
    starts: List[set] = [set() for _ in range(T)]
    for s in range(T):
        for t in range(s, T):
            top = -np.inf
            for path in itertools.product(range(C), repeat=t + 1 - s):
                if path[0] != y[0] or path[-1] != y[-1] or collapse(path, blank) != y:
                    continue
                total = 0.0
                for k, c in enumerate(path):
                    total += cost[s + k, c]
                top = max(top, total)
            if top == -np.inf:
                continue
            if top > best[t]:
                best[t], starts[t] = top, {s}
            elif top == best[t]:
                starts[t].add(s)
    return best, starts


def plant(T: int, C: int, blank: int, occurrences: Sequence[Tuple[int, Sequence[int]]], filler: int, low: float = -30.0
          ) -> np.ndarray:
    """Sharp emissions: 0 at one class per frame and ``low`` elsewhere.  ``occurrences`` are (start frame, class per frame);
    every other frame's class is ``filler``."""
    lp = np.full((T, C), low, np.float32)
    top = np.full(T, filler)
    for start, classes in occurrences:
        top[start:start + len(classes)] = classes
    lp[np.arange(T), top] = 0.0
    return lp

"""The CTC forced-alignment contract (include/allophant_amx_align.h) as executable code: a literal numpy fp32 restatement
of the recurrence, the tie rule and the outputs, and a float64 brute-force enumeration of every CTC path for tiny rows.

The tie rule (the smaller move wins) is this project's.  The Viterbi aligner of the audio library upstream depends on was
read, not run (it is not a dependency here): at ``x1 == x2 > x0`` it takes ``x0``."""
import itertools
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

NEG_INF = np.float32(-np.inf)


class Row(NamedTuple):
    status: int
    paths: Optional[np.ndarray]         # int32 [T]
    frame_scores: Optional[np.ndarray]  # float32 [T]
    spans: Optional[np.ndarray]         # int32 [L, 2]
    span_scores: Optional[np.ndarray]   # float32 [L]
    total: Optional[np.float32]
    states: Optional[np.ndarray]        # int32 [T]: the walked states (not an output of the kernel)


def _refused(status: int) -> Row:
    return Row(status, None, None, None, None, None, None)


def _sweep_literal(lp: np.ndarray, y: List[int], blank: int):
    """The recurrence cell by cell, as the contract writes it."""
    T, S = lp.shape[0], 2 * len(y) + 1
    label = [blank if i % 2 == 0 else y[i // 2] for i in range(S)]
    a = np.full(S, NEG_INF, np.float32)
    a[0] = lp[0, blank]
    if S > 1:
        a[1] = lp[0, y[0]]
    move = np.zeros((T, S), np.int8)
    for t in range(1, T):
        b = np.empty(S, np.float32)
        for i in range(S):
            x0 = a[i]
            x1 = a[i - 1] if i >= 1 else NEG_INF
            x2 = a[i - 2] if (i % 2 == 1 and i >= 3 and y[i // 2] != y[i // 2 - 1]) else NEG_INF
            r, m = x0, 0
            if x1 > r:
                r, m = x1, 1
            if x2 > r:
                r, m = x2, 2
            b[i] = np.float32(r) + lp[t, label[i]]  # one fp32 addition
            move[t, i] = m
        a = b
    return a, move


def _sweep_fast(lp: np.ndarray, y: List[int], blank: int):
    """The same comparisons and the same single fp32 addition per cell, a whole frame at a time (for the long rows of the GPU
    tests; tests/test_ctc_align_contract.py holds it equal to the literal sweep bit for bit)."""
    T, S = lp.shape[0], 2 * len(y) + 1
    states = np.arange(S)
    targets = np.asarray(y + [blank], np.int64)  # (the extra entry keeps the even states' lookup in range)
    label = np.where(states % 2 == 0, blank, targets[states // 2])
    skip = np.zeros(S, bool)
    odd = states[(states % 2 == 1) & (states >= 3)]
    skip[odd] = targets[odd // 2] != targets[odd // 2 - 1]
    a = np.full(S, NEG_INF, np.float32)
    a[0] = lp[0, blank]
    if S > 1:
        a[1] = lp[0, y[0]]
    move = np.zeros((T, S), np.int8)
    for t in range(1, T):
        x1 = np.concatenate((np.full(1, NEG_INF, np.float32), a[:-1]))
        x2 = np.where(skip, np.concatenate((np.full(2, NEG_INF, np.float32), a[:-2]))[:S], NEG_INF)
        r = a
        m = move[t]
        step = x1 > r
        r = np.where(step, x1, r)
        m[step] = 1
        jump = x2 > r
        r = np.where(jump, x2, r)
        m[jump] = 2
        a = r + lp[t, label]
        assert a.dtype == np.float32
    return a, move


def align_row(lp: np.ndarray, targets: Sequence[int], blank: int = 0, fast: bool = False) -> Row:
    """One row: ``lp`` fp32 ``[T, C]`` (T = the row's frame length), ``targets`` ``y[0..L)``."""
    lp = np.asarray(lp, dtype=np.float32)
    T, C = lp.shape
    y = [int(v) for v in targets]
    L = len(y)
    if any(v < 0 or v >= C or v == blank for v in y):
        return _refused(-2)
    if T == 0:
        if L:
            return _refused(-1)
        empty_i, empty_f = np.zeros(0, np.int32), np.zeros(0, np.float32)
        return Row(0, empty_i, empty_f, np.zeros((0, 2), np.int32), empty_f, np.float32(0), empty_i)
    S = 2 * L + 1
    label = [blank if i % 2 == 0 else y[i // 2] for i in range(S)]
    a, move = (_sweep_fast if fast else _sweep_literal)(lp, y, blank)
    e = S - 1 if (S == 1 or a[S - 1] > a[S - 2]) else S - 2
    total = np.float32(a[e])
    if total == NEG_INF:
        return _refused(-1)
    states = np.zeros(T, np.int32)
    for t in range(T - 1, -1, -1):
        states[t] = e
        e -= int(move[t, e])
    paths = np.array([label[s] for s in states], np.int32)
    frame_scores = lp[np.arange(T), paths].astype(np.float32)
    spans = np.zeros((L, 2), np.int32)
    span_scores = np.zeros(L, np.float32)
    for l in range(L):
        frames = np.nonzero(states == 2 * l + 1)[0]
        spans[l] = (frames[0], frames[-1] + 1)
        acc = np.float32(0)
        for t in frames:
            acc = np.float32(acc + frame_scores[t])
        span_scores[l] = acc
    return Row(0, paths, frame_scores, spans, span_scores, total, states)


def align_batch(emissions: np.ndarray, lengths: Sequence[int], offsets: Sequence[int], ids: Sequence[int], max_target: int,
                blank: int = 0, fast: bool = False) -> List[Row]:
    """The batch form as the C ABI takes it: ``emissions`` ``[N, T, C]``, frame lengths, CSR targets.  A row is refused (-2)
    for a frame length outside ``[0, T]``, offsets not ascending within ``[0, offsets[N]]`` or ``L > max_target``."""
    N, T, _ = emissions.shape
    rows = []
    for n in range(N):
        lo, hi, length = int(offsets[n]), int(offsets[n + 1]), int(lengths[n])
        if length < 0 or length > T or lo < 0 or hi < lo or hi > int(offsets[N]) or hi - lo > max_target:
            rows.append(_refused(-2))
            continue
        rows.append(align_row(emissions[n, :length], list(ids[lo:hi]), blank, fast))
    return rows


def expected_buffers(emissions: np.ndarray, lengths, offsets, ids, max_target: int, blank: int, sentinel_i: int, sentinel_f: float):
    """What the device buffers hold after a call on buffers pre-filled with the sentinels: every entry the contract leaves
    untouched keeps its sentinel."""
    N, T, _ = emissions.shape
    paths = np.full((N, T), sentinel_i, np.int32)
    frame_scores = np.full((N, T), sentinel_f, np.float32)
    spans = np.full((N, max_target, 2), sentinel_i, np.int32)
    span_scores = np.full((N, max_target), sentinel_f, np.float32)
    totals = np.full(N, sentinel_f, np.float32)
    status = np.zeros(N, np.int32)
    for n, row in enumerate(align_batch(emissions, lengths, offsets, ids, max_target, blank, fast=True)):
        status[n] = row.status
        if row.status < 0:
            continue
        k, L = len(row.paths), len(row.span_scores)
        paths[n, :k], paths[n, k:] = row.paths, -1
        frame_scores[n, :k] = row.frame_scores
        spans[n, :L], span_scores[n, :L] = row.spans, row.span_scores
        totals[n] = row.total
    return paths, frame_scores, spans, span_scores, totals, status


def minimum_frames(targets: Sequence[int]) -> int:
    """Targets plus one blank per adjacent repeat."""
    return len(targets) + sum(1 for i in range(1, len(targets)) if targets[i] == targets[i - 1])


def collapse(path: Sequence[int], blank: int) -> List[int]:
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def best_paths_bruteforce(lp: np.ndarray, targets: Sequence[int], blank: int = 0) -> Tuple[float, List[Tuple[int, ...]]]:
    """Every length-T class sequence that collapses to ``targets``, scored in float64: the best total (``-inf`` and no paths
    when none is finite) and all paths within 1e-9 of it.  For tiny rows only (C ** T sequences)."""
    lp64 = np.asarray(lp, dtype=np.float64)
    T, C = lp64.shape
    y = [int(v) for v in targets]
    best, paths = -np.inf, []
    if T == 0:
        return (0.0, [()]) if not y else (best, paths)
    scored = []
    for path in itertools.product(range(C), repeat=T):
        if collapse(path, blank) != y:
            continue
        total = 0.0
        for t, c in enumerate(path):
            total += lp64[t, c]
        if total > -np.inf:
            scored.append((total, path))
            best = max(best, total)
    paths = [p for s, p in scored if s >= best - 1e-9]
    return best, paths

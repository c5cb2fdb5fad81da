"""The contract of the CTC forced alignment over label graphs (include/allophant_amx_align_graph.h) as executable code: a
literal numpy fp32 restatement, cell by cell and candidate by candidate; the same comparisons a whole frame at a time (for the
GPU tests' larger rows; tests/test_ctc_align_graph_contract.py holds the two equal bit for bit); the batch form with the
malformed-row rules; and the enumeration of the label sequences a graph accepts."""
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

NEG_INF = np.float32(-np.inf)
MAX_IN = 6
MAX_NODES = 4095


class Graph(NamedTuple):
    classes: List[int]
    flags: List[int]        # bit 0 initial, bit 1 final
    preds: List[List[int]]  # ordered, every entry below the node's own index


class Row(NamedTuple):
    status: int
    paths: Optional[np.ndarray]         # int32 [T]
    frame_scores: Optional[np.ndarray]  # float32 [T]
    spans: Optional[np.ndarray]         # int32 [L, 2], (-1, -1) for an unvisited node
    span_scores: Optional[np.ndarray]   # float32 [L], 0 for an unvisited node
    total: Optional[np.float32]
    states: Optional[np.ndarray]        # int32 [T]: the walked states (not an output of the kernel)


def _refused(status: int) -> Row:
    return Row(status, None, None, None, None, None, None)


def chain(ids: Sequence[int]) -> Graph:
    L = len(ids)
    return Graph([int(v) for v in ids], [(1 if j == 0 else 0) | (2 if j == L - 1 else 0) for j in range(L)],
                 [[j - 1] if j else [] for j in range(L)])


def of_target_graph(g) -> Graph:
    """An allophant_amd.graph_alignment.TargetGraph in this module's form."""
    return Graph(list(g.classes), [int(bool(i)) + 2 * int(bool(f)) for i, f in zip(g.initial, g.final)], [list(p) for p in g.preds])


def finals_of(g: Graph) -> List[int]:
    return [j for j, f in enumerate(g.flags) if f & 2]


def candidates(g: Graph, i: int) -> List[Tuple[int, int]]:
    """The (move, source state) pairs of state i in the contract's order; an absent candidate is left out."""
    L, y = len(g.classes), g.classes
    if i == 2 * L:
        return [(0, i)] + [(2 + k, 2 * f + 1) for k, f in enumerate(finals_of(g))]
    j = i // 2
    if i % 2:
        return [(0, i), (1, i - 1)] + [(2 + k, 2 * p + 1) for k, p in enumerate(g.preds[j]) if y[p] != y[j]]
    return [(0, i)] + [(2 + k, 2 * p + 1) for k, p in enumerate(g.preds[j])]


def _labels(g: Graph, blank: int) -> List[int]:
    return [blank if i % 2 == 0 else g.classes[i // 2] for i in range(2 * len(g.classes) + 1)]


def _start(lp: np.ndarray, g: Graph, blank: int) -> np.ndarray:
    L = len(g.classes)
    a = np.full(2 * L + 1, NEG_INF, np.float32)
    for j in range(L):
        if g.flags[j] & 1:
            a[2 * j] = lp[0, blank]
            a[2 * j + 1] = lp[0, g.classes[j]]
    if L == 0:
        a[0] = lp[0, blank]
    return a


def _sweep_literal(lp: np.ndarray, g: Graph, blank: int):
    T, S = lp.shape[0], 2 * len(g.classes) + 1
    label = _labels(g, blank)
    cands = [candidates(g, i) for i in range(S)]
    a = _start(lp, g, blank)
    move = np.zeros((T, S), np.int8)
    for t in range(1, T):
        b = np.empty(S, np.float32)
        for i in range(S):
            r, m = a[i], 0
            for index, source in cands[i][1:]:
                if a[source] > r:
                    r, m = a[source], index
            b[i] = np.float32(r) + lp[t, label[i]]  # one fp32 addition
            move[t, i] = m
        a = b
    return a, move


def _sweep_fast(lp: np.ndarray, g: Graph, blank: int):
    """The same comparisons in the same order and the same single fp32 addition per cell, a whole frame at a time: per move a
    source column, an absent candidate reading a slot that holds -inf."""
    T, S = lp.shape[0], 2 * len(g.classes) + 1
    label = np.asarray(_labels(g, blank), np.int64)
    source = np.full((2 + MAX_IN, S), S, np.int64)  # S: the -inf slot
    for i in range(S):
        for index, state in candidates(g, i):
            source[index, i] = state
    a = _start(lp, g, blank)
    move = np.zeros((T, S), np.int8)
    for t in range(1, T):
        padded = np.concatenate((a, np.full(1, NEG_INF, np.float32)))
        r = a
        m = move[t]
        for index in range(1, 2 + MAX_IN):
            x = padded[source[index]]
            better = x > r
            r = np.where(better, x, r)
            m[better] = index
        a = r + lp[t, label]
        assert a.dtype == np.float32
    return a, move


def malformed(g: Graph, C: int, blank: int) -> bool:
    L = len(g.classes)
    if any(v < 0 or v >= C or v == blank for v in g.classes):
        return True
    for j, p in enumerate(g.preds):
        if len(p) > MAX_IN or any(v < 0 or v >= j for v in p):
            return True
    if L and (not any(f & 1 for f in g.flags) or not 1 <= len(finals_of(g)) <= MAX_IN):
        return True
    return False


def align_row(lp: np.ndarray, g: Graph, blank: int = 0, fast: bool = False) -> Row:
    """One row: ``lp`` fp32 ``[T, C]`` (T = the row's frame length)."""
    lp = np.asarray(lp, dtype=np.float32)
    T, C = lp.shape
    L = len(g.classes)
    if malformed(g, C, blank):
        return _refused(-2)
    if T == 0:
        if L:
            return _refused(-1)
        empty_i, empty_f = np.zeros(0, np.int32), np.zeros(0, np.float32)
        return Row(0, empty_i, empty_f, np.zeros((0, 2), np.int32), empty_f, np.float32(0), empty_i)
    label = _labels(g, blank)
    a, move = (_sweep_fast if fast else _sweep_literal)(lp, g, blank)
    ends = [2 * f + 1 for f in finals_of(g)] + [2 * L]
    e = ends[0]
    for i in ends[1:]:
        if a[i] > a[e]:
            e = i
    total = np.float32(a[e])
    if total == NEG_INF:
        return _refused(-1)
    states = np.zeros(T, np.int32)
    for t in range(T - 1, -1, -1):
        states[t] = e
        e = dict(candidates(g, e))[int(move[t, e])]
    paths = np.array([label[s] for s in states], np.int32)
    frame_scores = lp[np.arange(T), paths].astype(np.float32)
    spans = np.full((L, 2), -1, np.int32)
    span_scores = np.zeros(L, np.float32)
    for l in range(L):
        frames = np.nonzero(states == 2 * l + 1)[0]
        if len(frames) == 0:
            continue
        assert frames[-1] - frames[0] + 1 == len(frames)  # a node's frames are one run
        spans[l] = (frames[0], frames[-1] + 1)
        acc = np.float32(0)
        for t in frames:
            acc = np.float32(acc + frame_scores[t])
        span_scores[l] = acc
    return Row(0, paths, frame_scores, spans, span_scores, total, states)


class Packed(NamedTuple):
    """Graphs as the C ABI takes them."""
    node_offsets: List[int]
    node_classes: List[int]
    node_flags: List[int]
    arc_offsets: List[int]
    arc_preds: List[int]


def pack(graphs: Sequence[Graph]) -> Packed:
    node_offsets, classes, flags, arc_offsets, arcs = [0], [], [], [0], []
    for g in graphs:
        classes += g.classes
        flags += g.flags
        for p in g.preds:
            arcs += p
            arc_offsets.append(len(arcs))
        node_offsets.append(len(classes))
    return Packed(node_offsets, classes, flags, arc_offsets, arcs)


def align_batch(emissions: np.ndarray, lengths: Sequence[int], packed: Packed, max_nodes: int, blank: int = 0,
                fast: bool = False) -> List[Row]:
    """The batch form: a row is refused (-2) for a frame length outside ``[0, T]``, node offsets not ascending within
    ``[0, node_offsets[N]]``, ``L > max_nodes``, arc offsets that do not ascend or leave ``[0, arc_offsets[last]]``, and for
    everything ``malformed`` names.  Nothing out of range is read for such a row."""
    N, T, _ = emissions.shape
    node_count = int(packed.node_offsets[N])
    rows = []
    for n in range(N):
        lo, hi, length = int(packed.node_offsets[n]), int(packed.node_offsets[n + 1]), int(lengths[n])
        if length < 0 or length > T or lo < 0 or hi < lo or hi > node_count or hi - lo > max_nodes:
            rows.append(_refused(-2))
            continue
        arc_count = int(packed.arc_offsets[node_count])
        preds, bad = [], False
        for j in range(lo, hi):
            ab, ae = int(packed.arc_offsets[j]), int(packed.arc_offsets[j + 1])
            if ab < 0 or ae < ab or ae > arc_count or ae - ab > MAX_IN:
                bad = True
                break
            preds.append([int(v) for v in packed.arc_preds[ab:ae]])
        if bad:
            rows.append(_refused(-2))
            continue
        g = Graph([int(v) for v in packed.node_classes[lo:hi]], [int(v) for v in packed.node_flags[lo:hi]], preds)
        rows.append(align_row(emissions[n, :length], g, blank, fast))
    return rows


def expected_buffers(emissions: np.ndarray, lengths, packed: Packed, max_nodes: int, blank: int, sentinel_i: int, sentinel_f: float):
    """What the device buffers hold after a call on buffers pre-filled with the sentinels: every entry the contract leaves
    untouched keeps its sentinel."""
    N, T, _ = emissions.shape
    paths = np.full((N, T), sentinel_i, np.int32)
    frame_scores = np.full((N, T), sentinel_f, np.float32)
    spans = np.full((N, max_nodes, 2), sentinel_i, np.int32)
    span_scores = np.full((N, max_nodes), sentinel_f, np.float32)
    totals = np.full(N, sentinel_f, np.float32)
    status = np.zeros(N, np.int32)
    for n, row in enumerate(align_batch(emissions, lengths, packed, max_nodes, blank, fast=True)):
        status[n] = row.status
        if row.status < 0:
            continue
        k, L = len(row.paths), len(row.span_scores)
        paths[n, :k], paths[n, k:] = row.paths, -1
        frame_scores[n, :k] = row.frame_scores
        spans[n, :L], span_scores[n, :L] = row.spans, row.span_scores
        totals[n] = row.total
    return paths, frame_scores, spans, span_scores, totals, status


def accepted_sequences(g: Graph) -> List[Tuple[int, ...]]:
    """Every label sequence the graph accepts: the classes along each node path from an initial to a final node (sorted,
    without duplicates).  The graph of no nodes accepts the empty sequence."""
    L = len(g.classes)
    if L == 0:
        return [()]
    successors: List[List[int]] = [[] for _ in range(L)]
    for j, p in enumerate(g.preds):
        for v in p:
            successors[v].append(j)
    found = set()

    def extend(j: int, prefix: Tuple[int, ...]) -> None:
        prefix = prefix + (g.classes[j],)
        if g.flags[j] & 2:
            found.add(prefix)
        for k in successors[j]:
            extend(k, prefix)

    for j in range(L):
        if g.flags[j] & 1:
            extend(j, ())
    return sorted(found)


def random_dag(rng, L: int, C: int, blank: int, max_in: int = MAX_IN, same_class: float = 0.2) -> Graph:
    """L nodes with in-degrees 0 .. max_in (predecessors drawn without order among the earlier nodes, nearby ones
    preferred), one to three initial nodes, one to MAX_IN final nodes; a predecessor shares its successor's class with
    probability about ``same_class`` (always, when there is one non-blank class)."""
    classes_of = [c for c in range(C) if c != blank]
    classes, flags, preds = [], [], []
    for j in range(L):
        d = int(min(j, rng.integers(0, max_in + 1)))
        if j and d == 0 and rng.random() < 0.7:
            d = 1
        pool = list(range(max(0, j - 12), j))
        p = [int(v) for v in rng.permutation(pool)[:d]]
        c = int(rng.choice(classes_of))
        if p and rng.random() < same_class:
            c = classes[p[0]]
        classes.append(c)
        preds.append(p)
        flags.append(1 if (j == 0 or not p or rng.random() < 0.05) else 0)
    if L:
        for j in set([L - 1] + [int(v) for v in rng.integers(max(0, L - 8), L, int(rng.integers(0, MAX_IN)))]):
            flags[j] |= 2
    return Graph(classes, flags, preds)

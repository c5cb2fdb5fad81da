"""CTC forced alignment over pronunciation graphs on the device (``include/allophant_amx_align_graph.h``): which of several
alternative label sequences was spoken, and where in the frames each of its symbols lies.

  * ``TargetGraph``  a row's label graph: ``chain`` (one fixed sequence), ``from_slots`` (a transcript whose positions have
    alternatives, some of them optional), ``from_lexicon`` (one slot per word, its pronunciations as alternatives)
  * ``ctc_graph_align``  one ``[N, T, C]`` emission tensor, like ``alignment.ctc_forced_align``
  * ``Estimator.align_graph_device`` / ``Estimator.align_graph``  every output of a ``Predictions`` (``GraphAligned`` stays in HBM)
  * ``slot_targets``  slots of symbol strings -> slots of class indices (``alignment.output_targets`` per alternative)

The path is the Viterbi path of the graph's CTC trellis with ties going to the earlier candidate (a state itself, its
leading blank, then its predecessors in list order); a chain gives ``ctc_forced_align``'s result bit for bit.  There is no CPU
path."""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import alignment as _alignment, ctc as _ctc, lib as _lib
from .ctc import frame_stride

ALIGN_GRAPH_MAX_NODES = _lib.ALIGN_GRAPH_MAX_NODES
ALIGN_GRAPH_MAX_IN = _lib.ALIGN_GRAPH_MAX_IN

Slots = Sequence[Sequence[Sequence[int]]]


class TargetGraph(NamedTuple):
    """The label graph of one row.  Node ``j`` has the class ``classes[j]``, the ordered predecessors ``preds[j]`` (node
    indices below ``j``), and may be ``initial[j]`` and ``final[j]``; ``where[j]`` is its (slot, alternative, position).
    ``skips[s]`` is the index of slot ``s``'s empty alternative, or ``None`` when the slot cannot be skipped."""
    classes: List[int]
    preds: List[List[int]]
    initial: List[bool]
    final: List[bool]
    where: List[Tuple[int, int, int]]
    skips: List[Optional[int]]

    @classmethod
    def chain(cls, ids: Sequence[int]) -> "TargetGraph":
        """One fixed label sequence, every symbol a slot of its own: what ``ctc_forced_align`` aligns."""
        ids = [int(v) for v in ids]
        L = len(ids)
        return cls(ids, [[j - 1] if j else [] for j in range(L)], [j == 0 for j in range(L)], [j == L - 1 for j in range(L)],
                   [(j, 0, 0) for j in range(L)], [None] * L)

    @classmethod
    def from_slots(cls, slots: Slots) -> "TargetGraph":
        """A transcript as a sequence of slots, each a list of alternative class sequences; an empty alternative makes its
        slot optional.  The graph accepts exactly the concatenations of one alternative per slot.  Nodes are emitted slot by
        slot and alternative by alternative; the first node of an alternative is preceded by the exits so far (the last nodes
        of the previous slot's non-empty alternatives, and the exits before it when that slot can be skipped), ascending, and
        is initial while every earlier slot can be skipped; the exits after the last slot are final.  ``ValueError`` names
        the slot at which an in-degree or the final count would pass ``ALIGN_GRAPH_MAX_IN``, and is raised when every slot can
        be skipped (the empty transcript is not a graph row)."""
        classes: List[int] = []
        preds: List[List[int]] = []
        initial: List[bool] = []
        where: List[Tuple[int, int, int]] = []
        skips: List[Optional[int]] = []
        exits: List[int] = []
        open_start = True  # every earlier slot can be skipped
        for s, slot in enumerate(slots):
            if len(slot) == 0:
                raise ValueError(f"slot {s} has no alternative")
            leaving: List[int] = []
            skip: Optional[int] = None
            for k, alternative in enumerate(slot):
                if len(alternative) == 0:
                    skip = k if skip is None else skip
                    continue
                if len(exits) > ALIGN_GRAPH_MAX_IN:
                    raise ValueError(f"slot {s}: its alternatives would have {len(exits)} predecessors, at most "
                                     f"{ALIGN_GRAPH_MAX_IN} are aligned on the device")
                for position, value in enumerate(alternative):
                    node = len(classes)
                    classes.append(int(value))
                    preds.append([node - 1] if position else list(exits))
                    initial.append(open_start and position == 0)
                    where.append((s, k, position))
                leaving.append(len(classes) - 1)
            exits = sorted(leaving + (exits if skip is not None else []))
            open_start = open_start and skip is not None
            skips.append(skip)
        if open_start:
            raise ValueError("every slot can be skipped: the empty transcript is not a graph row")
        if len(exits) > ALIGN_GRAPH_MAX_IN:
            raise ValueError(f"slot {len(skips) - 1}: the graph would end in {len(exits)} final nodes, at most "
                             f"{ALIGN_GRAPH_MAX_IN} are aligned on the device")
        if len(classes) > ALIGN_GRAPH_MAX_NODES:
            raise ValueError(f"at most {ALIGN_GRAPH_MAX_NODES} nodes per row on the device, got {len(classes)}")
        last = set(exits)
        return cls(classes, preds, initial, [j in last for j in range(len(classes))], where, skips)

    @classmethod
    def from_lexicon(cls, words: Sequence[Any], lexicon: Dict[Any, Sequence[Sequence[int]]]) -> "TargetGraph":
        """One slot per word of ``words``, with that word's pronunciations in ``lexicon`` (class sequences) as alternatives."""
        missing = [w for w in words if w not in lexicon]
        if missing:
            raise ValueError(f"word {missing[0]!r} is not in the lexicon")
        return cls.from_slots([lexicon[w] for w in words])

    def sequence(self, choices: Sequence[int]) -> List[int]:
        """The class sequence of one alternative per slot (``choices[s]`` indexes slot ``s``'s alternatives)."""
        taken = {(s, int(k)) for s, k in enumerate(choices)}
        return [c for c, (s, k, _) in zip(self.classes, self.where) if (s, k) in taken]


def slot_targets(maps_or_evaluator, output, slots_of_symbols: Sequence[Sequence[Sequence[str]]]) -> List[List[List[int]]]:
    """Slots of symbol strings as slots of class indices on ``output`` (its name or index among the maps' outputs): every
    alternative goes through ``alignment.output_targets``, so a symbol may expand to several classes or to none."""
    maps = getattr(maps_or_evaluator, "maps", maps_or_evaluator)
    o = maps.names.index(output) if isinstance(output, str) else int(output)
    return [_alignment.output_targets(maps, o, [list(a) for a in slot], row_name=f"slot {s}, alternative")
            for s, slot in enumerate(slots_of_symbols)]


class GraphAlignment(NamedTuple):
    """One aligned row on the host: ``tokens`` int32 ``[T]`` / ``scores`` fp32 ``[T]`` as in ``Alignment``; ``nodes`` the K
    visited nodes in ascending order (the chosen pronunciation), ``labels`` their classes, ``spans`` int32 ``[K, 2]`` and
    ``span_scores`` fp32 ``[K]`` per visited node, ``total`` the path's log-probability, ``graph`` the row's graph."""
    tokens: Tensor
    scores: Tensor
    nodes: List[int]
    labels: List[int]
    spans: Tensor
    span_scores: Tensor
    total: float
    graph: TargetGraph

    def choices(self) -> List[int]:
        """Per slot the index of the alternative the path took; a skipped slot reports its empty alternative's index."""
        taken: List[Optional[int]] = list(self.graph.skips)
        for j in self.nodes:
            s, k, _ = self.graph.where[j]
            taken[s] = k
        return [int(k) for k in taken]  # (every slot is either visited or skippable)

    def seconds(self, spec: Dict[str, Any], sample_rate: int = 16000) -> Tensor:
        """``spans`` in seconds (float64 ``[K, 2]``): frame index x the spec's frame stride / sample rate."""
        return self.spans.to(torch.float64) * (frame_stride(spec) / float(sample_rate))


def pack_graphs(graphs: Sequence[TargetGraph]) -> Tuple[Tensor, List[int], List[int]]:
    """The rows' graphs as the C ABI takes them, in one host int32 tensor: node offsets ``[R + 1]``, classes, flags, arc
    offsets ``[nodes + 1]`` and predecessors (one spare element closes it, so no array is empty).  Returns the tensor, the
    element offsets of the five arrays in it and the rows' node counts."""
    counts = [len(g.classes) for g in graphs]
    if counts and max(counts) > ALIGN_GRAPH_MAX_NODES:
        raise ValueError(f"at most {ALIGN_GRAPH_MAX_NODES} nodes per row on the device, got {max(counts)}")
    node_offsets, classes, flags, arc_offsets, arcs = [0], [], [], [0], []
    for g in graphs:
        if not (len(g.preds) == len(g.initial) == len(g.final) == len(g.classes)):
            raise ValueError("a TargetGraph's classes, preds, initial and final must have one entry per node")
        classes += [int(c) for c in g.classes]
        flags += [int(bool(i)) + 2 * int(bool(f)) for i, f in zip(g.initial, g.final)]
        for p in g.preds:
            arcs += [int(v) for v in p]
            arc_offsets.append(len(arcs))
        node_offsets.append(len(classes))
    parts = [node_offsets, classes, flags, arc_offsets, arcs + [0]]
    starts = [0]
    for part in parts[:-1]:
        starts.append(starts[-1] + len(part))
    return torch.tensor([v for part in parts for v in part], dtype=torch.int32), starts, counts


def graph_pointers(meta: Tensor, starts: Sequence[int]):
    """The five device pointers of a packed graph tensor (``pack_graphs``, copied to the device)."""
    return tuple(C.c_void_p(meta.data_ptr() + 4 * s) for s in starts)


def allocate(lib, rows: int, T: int, max_nodes: int, device) -> "_alignment._Buffers":
    """The workspace and outputs of ``rows`` rows of ``T`` frames and up to ``max_nodes`` nodes."""
    size = C.c_size_t()
    _lib.check(lib, None, lib.amx_ctc_align_graph_workspace(rows, T, max_nodes, C.byref(size)))
    empty = lambda *shape, dtype: _ctc.empty(*shape, dtype=dtype, device=device)  # noqa: E731
    return _alignment._Buffers(torch.empty(max(1, size.value), dtype=torch.uint8, device=device), size.value,
                               empty(rows, T, dtype=torch.int32), empty(rows, T, dtype=torch.float32),
                               empty(rows, max_nodes, 2, dtype=torch.int32), empty(rows, max_nodes, dtype=torch.float32),
                               empty(rows, dtype=torch.float32), empty(rows, dtype=torch.int32))


def _rows(paths: Tensor, frame_scores: Tensor, spans: Tensor, span_scores: Tensor, totals: Tensor, status: Tensor,
          lengths: Sequence[int], graphs: Sequence[TargetGraph], label: str = "row") -> List[Optional[GraphAlignment]]:
    """Host form of ``R`` aligned rows: ``None`` where no path exists, ``ValueError`` for a row the kernel flagged."""
    status_h = status.cpu().tolist()
    bad = [r for r, s in enumerate(status_h) if s == -2]
    if bad:
        raise ValueError(f"{label} {bad[0]}: malformed graph row (a class equal to the blank or outside the classes, a "
                         f"predecessor that is not an earlier node, more than {ALIGN_GRAPH_MAX_IN} predecessors or final nodes, "
                         "no initial or no final node, or a frame length outside the tensor)")
    paths_h, scores_h, spans_h, span_scores_h, totals_h = (t.cpu() for t in (paths, frame_scores, spans, span_scores, totals))
    out: List[Optional[GraphAlignment]] = []
    for r, s in enumerate(status_h):
        if s != 0:
            out.append(None)
            continue
        k, graph = int(lengths[r]), graphs[r]
        L = len(graph.classes)
        nodes = torch.nonzero(spans_h[r, :L, 0] >= 0).flatten()
        out.append(GraphAlignment(paths_h[r, :k].clone(), scores_h[r, :k].clone(), nodes.tolist(),
                                  [graph.classes[j] for j in nodes.tolist()], spans_h[r, :L][nodes].clone(),
                                  span_scores_h[r, :L][nodes].clone(), float(totals_h[r]), graph))
    return out


class GraphAligned(NamedTuple):
    """Graph alignments of a batch, one row per output, on the device: the buffers of ``alignment.Aligned`` with ``max_nodes``
    for ``max_target`` (``spans`` / ``span_scores`` are indexed by node); ``graphs[o][n]`` is the graph of each row."""
    names: List[str]
    present: List[str]
    paths: Tensor
    frame_scores: Tensor
    spans: Tensor
    span_scores: Tensor
    totals: Tensor
    status: Tensor
    lengths: List[int]
    graphs: List[List[TargetGraph]]

    def alignments(self) -> Dict[str, List[Optional[GraphAlignment]]]:
        """Fetched to the host: per present output and utterance a ``GraphAlignment``, or ``None`` where no path exists."""
        result = {}
        for o, name in enumerate(self.names):
            if name in self.present:
                result[name] = _rows(self.paths[o], self.frame_scores[o], self.spans[o], self.span_scores[o], self.totals[o],
                                     self.status[o], self.lengths, self.graphs[o], label=f"output {name!r}, utterance")
        return result


def ctc_graph_align(log_emissions: Tensor, lengths: Optional[Tensor], graphs: Sequence[TargetGraph],
                    blank_index: int = 0) -> List[Optional[GraphAlignment]]:
    """The best CTC path through each row's graph over ``log_emissions`` (an fp32 ``[N, T, C]`` cuda tensor of any strides
    with a unit class stride, read in place) via ``amx_ctc_align_graph_emissions``.  Per row a ``GraphAlignment``, or ``None``
    where no path exists (too few frames, or ``-inf`` emissions on every path); ``ValueError`` names a malformed row."""
    log_emissions, N, T, Cn = _ctc.emissions(log_emissions, "aligns")
    lib = _lib.load()
    device = log_emissions.device
    if len(graphs) != N:
        raise ValueError(f"{len(graphs)} graphs for {N} emission rows")
    _ctc.check_classes(Cn, blank_index, "alignment")
    if N == 0:
        return []
    packed, starts, counts = pack_graphs(graphs)
    max_nodes = max(counts)
    with torch.cuda.device(device):
        frame_lengths, index, stream = _ctc.frame(log_emissions, lengths)
        meta = packed.to(device)
        b = allocate(lib, N, T, max_nodes, device)
        code = lib.amx_ctc_align_graph_emissions(
            index, C.c_void_p(log_emissions.data_ptr()), log_emissions.stride(0), log_emissions.stride(1),
            C.c_void_p(frame_lengths.data_ptr()), N, T, Cn, blank_index, *graph_pointers(meta, starts), max_nodes, *b.pointers(),
            C.c_void_p(stream))
        _lib.check(lib, None, code)
        return _rows(b.paths, b.frame_scores, b.spans, b.span_scores, b.totals, b.status, frame_lengths.cpu().tolist(), graphs)

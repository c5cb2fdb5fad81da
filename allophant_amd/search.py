"""CTC search on the device (``include/allophant_amx_search.h``): where in each utterance a short label sequence occurs,
start and end free.

  * ``ctc_search``  one ``[N, T, C]`` emission tensor, every utterance against every query (``Found`` stays in HBM)
  * ``Estimator.search_device`` / ``Estimator.search``  one output of a ``Predictions``
  * ``query_targets``  symbol strings -> class indices of one output (the expansion of ``alignment.label_targets``)
  * ``pick_hits``  the host selection of non-overlapping occurrences from a row's curves

The score of a span is the log-likelihood ratio of the query's best path through it against the frame-wise best path over
the same frames: at most 0, and 0 exactly when the argmax path over the span reads the query.  There is no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import ctc as _ctc, lib as _lib
from .alignment import output_targets
from .ctc import frame_stride

SEARCH_MAX_QUERY = _lib.SEARCH_MAX_QUERY


class Hit(NamedTuple):
    """One occurrence: frames ``[start, end)`` and its score (<= 0)."""
    start: int
    end: int
    score: float

    def seconds(self, spec: Dict[str, Any], sample_rate: int = 16000):
        """``(start, end)`` in seconds: frame index x the spec's frame stride / sample rate."""
        scale = frame_stride(spec) / float(sample_rate)
        return self.start * scale, self.end * scale


def pick_hits(end_scores, end_starts, length: int, threshold: float, max_hits: Optional[int] = None) -> List[Hit]:
    """Every non-overlapping occurrence of one row scoring at least ``threshold``, from its curves (numpy arrays or CPU
    tensors; the first ``length`` frames count).  The candidates are the frames with ``end_scores[t] >= threshold`` and
    ``> -inf``, taken by score descending, then by end descending; one is accepted when its ``[start, end)`` overlaps no
    accepted span, until ``max_hits`` are held.  The hits are returned sorted by start."""
    scores = np.asarray(end_scores, dtype=np.float32)[:length]
    starts = np.asarray(end_starts)[:length]
    frames = np.nonzero((scores >= threshold) & (scores > -np.inf))[0]
    order = sorted(frames.tolist(), key=lambda t: (-float(scores[t]), -t))
    hits: List[Hit] = []
    for t in order:
        if max_hits is not None and len(hits) >= max_hits:
            break
        start, end = int(starts[t]), t + 1
        if all(end <= h.start or start >= h.end for h in hits):
            hits.append(Hit(start, end, float(scores[t])))
    return sorted(hits)


class Found(NamedTuple):
    """The search of ``N`` utterances for ``Q`` queries: ``scores`` fp32 ``[N, Q]``, ``spans`` int32 ``[N, Q, 2]`` and ``status``
    int32 ``[N, Q]`` on the device (status codes as in ``include/allophant_amx_search.h``: only the entries of status 0 hold a
    score and a span); with ``curves`` also ``end_scores`` fp32 / ``end_starts`` int32 ``[N, Q, T]``, defined below each
    utterance's frame length.  ``lengths`` are the frame lengths on the host."""
    scores: Tensor
    spans: Tensor
    status: Tensor
    end_scores: Optional[Tensor]
    end_starts: Optional[Tensor]
    lengths: List[int]

    def _status(self) -> List[List[int]]:
        status = self.status.cpu().tolist()
        for n, row in enumerate(status):
            for q, s in enumerate(row):
                if s == -2:
                    raise ValueError(f"utterance {n}, query {q}: malformed search row (an empty query, an id equal to the blank or "
                                     "outside the classes, or a frame length outside the tensor)")
        return status

    def best(self) -> List[List[Optional[Hit]]]:
        """Fetched to the host: per utterance and query the best occurrence, or ``None`` where there is none."""
        status = self._status()
        scores, spans = self.scores.cpu().tolist(), self.spans.cpu().tolist()
        return [[Hit(spans[n][q][0], spans[n][q][1], scores[n][q]) if s == 0 else None for q, s in enumerate(row)]
                for n, row in enumerate(status)]

    def hits(self, threshold: float, max_hits: Optional[int] = None) -> List[List[List[Hit]]]:
        """Per utterance and query every non-overlapping occurrence scoring at least ``threshold`` (``pick_hits`` on the
        curves, which are fetched to the host)."""
        if self.end_scores is None or self.end_starts is None:
            raise ValueError("hits() needs the curves: search with curves=True")
        status = self._status()
        end_scores, end_starts = self.end_scores.cpu().numpy(), self.end_starts.cpu().numpy()
        return [[pick_hits(end_scores[n, q], end_starts[n, q], self.lengths[n], threshold, max_hits) for q in range(len(row))]
                for n, row in enumerate(status)]

    def seconds(self, spec: Dict[str, Any], sample_rate: int = 16000) -> Tensor:
        """``spans`` in seconds (float64 ``[N, Q, 2]`` on the device): frame index x the spec's frame stride / sample rate."""
        return self.spans.to(torch.float64) * (frame_stride(spec) / float(sample_rate))


def pack_queries(queries: Sequence[Sequence[int]], classes: int, blank_index: int):
    """Queries as the C ABI takes them: int32 offsets ``[Q + 1]`` and int32 ids (host tensors).  ``ValueError`` names a
    malformed query."""
    for q, query in enumerate(queries):
        if not 1 <= len(query) <= SEARCH_MAX_QUERY:
            raise ValueError(f"query {q}: 1 to {SEARCH_MAX_QUERY} symbols per query on the device, got {len(query)}")
        for v in query:
            if not 0 <= int(v) < classes or int(v) == blank_index:
                raise ValueError(f"query {q}: id {int(v)} is the blank or outside the {classes} classes")
    return _ctc.pack_targets(queries)[:2]


def ctc_search(log_emissions: Tensor, lengths: Optional[Tensor], queries: Sequence[Sequence[int]], blank_index: int = 0,
               curves: bool = False) -> Found:
    """Searches every utterance of ``log_emissions`` (an fp32 ``[N, T, C]`` cuda tensor of any strides with a unit class
    stride, read in place) for every query (a sequence of class indices) via ``amx_ctc_search_emissions``.  With ``curves``
    the result also holds, per frame, the best score of an occurrence ending there and its start (``Found.hits``).
    ``ValueError`` names a malformed query."""
    log_emissions, N, T, Cn = _ctc.emissions(log_emissions, "searches")
    lib = _lib.load()
    device = log_emissions.device
    _ctc.check_classes(Cn, blank_index, "the search")
    offsets, ids = pack_queries(queries, Cn, blank_index)
    Q = len(queries)
    if N * Q * T >= 2 ** 31:
        raise ValueError(f"utterances x queries x frames must be below 2^31, got {N} x {Q} x {T}")
    with torch.cuda.device(device):
        frame_lengths, index, stream = _ctc.frame(log_emissions, lengths)
        if frame_lengths.shape != (N,):
            raise ValueError(f"{frame_lengths.numel()} lengths for {N} emission rows")
        empty = lambda *shape, dtype: _ctc.empty(*shape, dtype=dtype, device=device)  # noqa: E731
        scores, spans, status = empty(N, Q, dtype=torch.float32), empty(N, Q, 2, dtype=torch.int32), empty(N, Q, dtype=torch.int32)
        end_scores = empty(N, Q, T, dtype=torch.float32) if curves else None
        end_starts = empty(N, Q, T, dtype=torch.int32) if curves else None
        host_lengths = frame_lengths.cpu().tolist()
        bad = [n for n, k in enumerate(host_lengths) if not 0 <= k <= T]
        if bad:
            raise ValueError(f"utterance {bad[0]}: frame length {host_lengths[bad[0]]} outside [0, {T}]")
        if N == 0 or Q == 0:
            return Found(scores, spans, status, end_scores, end_starts, host_lengths)
        max_query = max(len(query) for query in queries)
        size = C.c_size_t()
        _lib.check(lib, None, lib.amx_ctc_search_workspace(N, Q, T, max_query, C.byref(size)))
        workspace = torch.empty(max(1, size.value), dtype=torch.uint8, device=device)
        meta = torch.cat([offsets, ids]).to(device)
        pointer = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        code = lib.amx_ctc_search_emissions(
            index, pointer(log_emissions), log_emissions.stride(0), log_emissions.stride(1), pointer(frame_lengths), N, T, Cn,
            blank_index, pointer(meta), C.c_void_p(meta.data_ptr() + 4 * (Q + 1)), Q, max_query, pointer(workspace), size.value,
            pointer(scores), pointer(spans), pointer(status), pointer(end_scores), pointer(end_starts), C.c_void_p(stream))
        _lib.check(lib, None, code)
        return Found(scores, spans, status, end_scores, end_starts, host_lengths)


def query_targets(maps_or_evaluator, queries: Sequence[Sequence[str]], output: str) -> List[List[int]]:
    """The class indices of each query's symbols on one output of an ``Evaluator`` (or its ``EvaluationMaps``): the expansion
    and class lookup of ``alignment.label_targets`` for that output.  ``ValueError`` names a symbol with no class."""
    maps = getattr(maps_or_evaluator, "maps", maps_or_evaluator)
    if output not in maps.names:
        raise ValueError(f"unknown output {output!r}, the maps hold {list(maps.names)}")
    return output_targets(maps, list(maps.names).index(output), queries, row_name="query")

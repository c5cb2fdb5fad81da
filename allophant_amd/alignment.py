"""CTC forced alignment on the device (``include/allophant_amx_align.h``): where in the frames each symbol of a known label
sequence lies.

  * ``ctc_forced_align``  one ``[N, T, C]`` emission tensor, like ``beam_ctc_decode``
  * ``Estimator.align_device`` / ``Estimator.align``  every output of a ``Predictions`` (``Aligned`` stays in HBM)
  * ``segments``  utterance bounds and scores from an ``Alignment`` and target boundaries (what a long alignment is for)
  * ``label_targets``  expected strings per output (``EvaluationMaps.expand_label``) -> class indices, the inverse of
    ``phonetic.hypothesis_symbols``

The path is the Viterbi path of the CTC trellis with ties going to the smaller move; there is no CPU path.  Rows of up to
``ALIGN_MAX_TARGET`` targets run one workgroup each (``amx_ctc_align.hip``); a call whose largest row has more, up to
``ALIGN_LONG_MAX_TARGET`` -- a whole transcript against the output of ``Estimator.predict_long`` -- runs the same recurrence
spread over the device (``amx_ctc_align_long.hip``), with the same outputs bit for bit."""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import ctc as _ctc, lib as _lib
from .ctc import frame_stride, pack_targets  # noqa: F401  (part of this module's interface)
from .phonetic import BLANK_OFFSET, IPA_LAYERS

ALIGN_MAX_TARGET = _lib.ALIGN_MAX_TARGET
ALIGN_LONG_MAX_TARGET = _lib.ALIGN_LONG_MAX_TARGET


def use_long(max_target: int, long: Optional[bool]) -> bool:
    """Whether a call whose largest row has ``max_target`` targets takes the long form: with ``long=None`` exactly when the
    row is past ``ALIGN_MAX_TARGET``; ``True`` forces it, ``False`` keeps the refusal of such rows."""
    return max_target > ALIGN_MAX_TARGET if long is None else bool(long)


class Alignment(NamedTuple):
    """One aligned row on the host: ``tokens`` int32 ``[T]`` the class of every frame (blank between symbols), ``scores``
    fp32 ``[T]`` its log-probability, ``spans`` int32 ``[L, 2]`` (first frame, last frame + 1) per target, ``span_scores``
    fp32 ``[L]`` the sum of the span's frame scores, ``total`` the path's log-probability."""
    tokens: Tensor
    scores: Tensor
    spans: Tensor
    span_scores: Tensor
    total: float

    def seconds(self, spec: Dict[str, Any], sample_rate: int = 16000) -> Tensor:
        """``spans`` in seconds (float64 ``[L, 2]``): frame index x the spec's frame stride / sample rate."""
        return self.spans.to(torch.float64) * (frame_stride(spec) / float(sample_rate))


def _rows(paths: Tensor, frame_scores: Tensor, spans: Tensor, span_scores: Tensor, totals: Tensor, status: Tensor,
          lengths: Sequence[int], target_counts: Sequence[int], label: str = "row") -> List[Optional[Alignment]]:
    """Host form of ``R`` aligned rows (``lengths`` / ``target_counts`` per row): ``None`` where no alignment exists,
    ``ValueError`` for a row the kernel flagged as malformed."""
    status_h = status.cpu().tolist()
    bad = [r for r, s in enumerate(status_h) if s == -2]
    if bad:
        raise ValueError(f"{label} {bad[0]}: malformed alignment row (a target equal to the blank or outside the classes, a "
                         "frame length outside the tensor, more targets than max_target, or offsets that do not ascend)")
    paths_h, scores_h, spans_h, span_scores_h, totals_h = (t.cpu() for t in (paths, frame_scores, spans, span_scores, totals))
    out: List[Optional[Alignment]] = []
    for r, s in enumerate(status_h):
        if s != 0:
            out.append(None)
            continue
        k, L = int(lengths[r]), int(target_counts[r])
        out.append(Alignment(paths_h[r, :k].clone(), scores_h[r, :k].clone(), spans_h[r, :L].clone(),
                             span_scores_h[r, :L].clone(), float(totals_h[r])))
    return out


class Aligned(NamedTuple):
    """Forced alignments of a batch, one row per output: ``paths`` int32 / ``frame_scores`` fp32 ``[O, N, T]``, ``spans`` int32
    ``[O, N, max_target, 2]``, ``span_scores`` fp32 ``[O, N, max_target]``, ``totals`` fp32 / ``status`` int32 ``[O, N]`` on the
    device (layout and status codes as in ``include/allophant_amx_align.h``); ``lengths`` / ``target_counts`` on the host.
    ``names`` are the outputs, ``present`` those that were given targets."""
    names: List[str]
    present: List[str]
    paths: Tensor
    frame_scores: Tensor
    spans: Tensor
    span_scores: Tensor
    totals: Tensor
    status: Tensor
    lengths: List[int]
    target_counts: List[List[int]]

    def alignments(self) -> Dict[str, List[Optional[Alignment]]]:
        """Fetched to the host: per present output and utterance an ``Alignment``, or ``None`` where none exists."""
        result = {}
        for o, name in enumerate(self.names):
            if name in self.present:
                result[name] = _rows(self.paths[o], self.frame_scores[o], self.spans[o], self.span_scores[o], self.totals[o],
                                     self.status[o], self.lengths, self.target_counts[o], label=f"output {name!r}, utterance")
        return result


class _Buffers(NamedTuple):
    workspace: Tensor
    size: int
    paths: Tensor
    frame_scores: Tensor
    spans: Tensor
    span_scores: Tensor
    totals: Tensor
    status: Tensor

    def pointers(self):
        return (C.c_void_p(self.workspace.data_ptr()), self.size, C.c_void_p(self.paths.data_ptr()),
                C.c_void_p(self.frame_scores.data_ptr()), C.c_void_p(self.spans.data_ptr()),
                C.c_void_p(self.span_scores.data_ptr()), C.c_void_p(self.totals.data_ptr()), C.c_void_p(self.status.data_ptr()))


def allocate(lib, rows: int, T: int, max_target: int, device, long: bool = False) -> _Buffers:
    """The workspace and outputs of ``rows`` rows of ``T`` frames (at least one element each, so every pointer is valid);
    with ``long`` the workspace of the long form.  A workspace that cannot be allocated raises ``RuntimeError`` naming its
    bytes (an hour against 40 000 targets records about 3.6 GB of moves)."""
    size = C.c_size_t()
    sizer = lib.amx_ctc_align_long_workspace if long else lib.amx_ctc_align_workspace
    _lib.check(lib, None, sizer(rows, T, max_target, C.byref(size)))
    empty = lambda *shape, dtype: _ctc.empty(*shape, dtype=dtype, device=device)  # noqa: E731
    try:
        workspace = torch.empty(max(1, size.value), dtype=torch.uint8, device=device)
    except torch.cuda.OutOfMemoryError as error:
        raise RuntimeError(f"the alignment workspace of {size.value} bytes ({rows} rows x {T} frames x {max_target} targets) "
                           f"cannot be allocated on {device}") from error
    return _Buffers(workspace, size.value,
                    empty(rows, T, dtype=torch.int32), empty(rows, T, dtype=torch.float32),
                    empty(rows, max_target, 2, dtype=torch.int32), empty(rows, max_target, dtype=torch.float32),
                    empty(rows, dtype=torch.float32), empty(rows, dtype=torch.int32))


def ctc_forced_align(log_emissions: Tensor, lengths: Optional[Tensor],
                     targets: Union[Sequence[Sequence[int]], Tuple[Tensor, Tensor]], blank_index: int = 0,
                     long: Optional[bool] = None) -> List[Optional[Alignment]]:
    """The best CTC path of each row's ``targets`` through ``log_emissions`` (an fp32 ``[N, T, C]`` cuda tensor of any strides
    with a unit class stride, read in place) via ``amx_ctc_align_emissions``.  ``targets``: one int sequence per row, or a
    padded ``[N, max_len]`` tensor with its lengths ``(padded, target_lengths)``.  Per row an ``Alignment``, or ``None`` where
    no alignment exists (too few frames, or ``-inf`` emissions on every path); ``ValueError`` names a malformed row.

    ``long=None`` sends the call to ``amx_ctc_align_long_emissions`` exactly when its largest row has more than
    ``ALIGN_MAX_TARGET`` targets (up to ``ALIGN_LONG_MAX_TARGET``); ``True`` forces that path, which gives the same bits, and
    ``False`` refuses such rows."""
    log_emissions, N, T, Cn = _ctc.emissions(log_emissions, "aligns")
    lib = _lib.load()
    device = log_emissions.device
    if isinstance(targets, tuple) and len(targets) == 2 and isinstance(targets[0], Tensor):
        padded, target_lengths = targets[0].cpu().tolist(), [int(v) for v in targets[1].cpu().tolist()]
        targets = [row[:k] for row, k in zip(padded, target_lengths)]
    if len(targets) != N:
        raise ValueError(f"{len(targets)} target rows for {N} emission rows")
    _ctc.check_classes(Cn, blank_index, "alignment")
    if N == 0:
        return []
    offsets, ids, counts = pack_targets(targets, limit=ALIGN_MAX_TARGET if long is False else ALIGN_LONG_MAX_TARGET)
    max_target = max(counts)
    long = use_long(max_target, long)
    entry = lib.amx_ctc_align_long_emissions if long else lib.amx_ctc_align_emissions
    with torch.cuda.device(device):
        frame_lengths, index, stream = _ctc.frame(log_emissions, lengths)
        meta = torch.cat([offsets, ids, torch.zeros(1, dtype=torch.int32)]).to(device)  # (never an empty tensor)
        b = allocate(lib, N, T, max_target, device, long)
        code = entry(
            index, C.c_void_p(log_emissions.data_ptr()), log_emissions.stride(0), log_emissions.stride(1),
            C.c_void_p(frame_lengths.data_ptr()), N, T, Cn, blank_index, C.c_void_p(meta.data_ptr()),
            C.c_void_p(meta.data_ptr() + 4 * (N + 1)), max_target, *b.pointers(), C.c_void_p(stream))
        _lib.check(lib, None, code)
        host_lengths = frame_lengths.cpu().tolist()
        return _rows(b.paths, b.frame_scores, b.spans, b.span_scores, b.totals, b.status, host_lengths, counts)


def segments(alignment: Alignment, boundaries: Sequence[int], spec: Optional[Dict[str, Any]] = None,
             sample_rate: int = 16000) -> Tuple[Tensor, Tensor]:
    """Cuts an aligned row into segments (utterances of a transcript, say): ``boundaries`` are ascending target indices
    ``b_0 = 0 < b_1 < ... < b_K = L``, and segment ``j`` covers the targets ``[b_j, b_{j+1})``, from ``spans[b_j, 0]`` to
    ``spans[b_{j+1} - 1, 1]``.  Returns the bounds -- int32 ``[K, 2]`` in frames, or float64 seconds when a ``spec`` is given
    (as ``Alignment.seconds``) -- and float64 ``[K]`` scores: the float64 mean of ``scores`` over the segment's frames, the
    blanks between its targets included."""
    bounds = [int(b) for b in boundaries]
    L = int(alignment.spans.shape[0])
    if len(bounds) < 2 or bounds[0] != 0 or bounds[-1] != L:
        raise ValueError(f"boundaries must run from 0 to the row's {L} targets, got {bounds[:1]} .. {bounds[-1:]}")
    if any(b <= a for a, b in zip(bounds, bounds[1:])):
        raise ValueError("boundaries must ascend strictly (every segment holds a target)")
    lower = torch.tensor(bounds[:-1], dtype=torch.int64)
    upper = torch.tensor(bounds[1:], dtype=torch.int64) - 1
    frames = torch.stack([alignment.spans[lower, 0], alignment.spans[upper, 1]], dim=1).to(torch.int32)
    sums = torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(alignment.scores.to(torch.float64), 0)])
    first, past = frames[:, 0].to(torch.int64), frames[:, 1].to(torch.int64)
    scores = (sums[past] - sums[first]) / (past - first).to(torch.float64)
    if spec is not None:
        return frames.to(torch.float64) * (frame_stride(spec) / float(sample_rate)), scores
    return frames, scores


def label_targets(maps_or_evaluator, labels: Sequence[Sequence[str]], languages: Optional[Sequence[str]] = None
                  ) -> Dict[str, List[List[int]]]:
    """Per output of an ``Evaluator`` (or its ``EvaluationMaps``) and utterance, the class indices of the expected symbols:
    the label expanded exactly as ``EvaluationMaps.expand_label`` does (contours, split segments, replacements), then
    ``inventory.index(p) + BLANK_OFFSET`` on the ``phone`` / ``phoneme`` outputs and
    ``feature_categories(name).index(v) + BLANK_OFFSET`` on attribute outputs -- the inverse of
    ``phonetic.hypothesis_symbols``.  ``languages`` (one per utterance, optional) are checked against the maps' languages.
    A symbol with no class (e.g. a phoneme outside the inventory) raises ``ValueError`` naming the output and the symbol."""
    maps = getattr(maps_or_evaluator, "maps", maps_or_evaluator)
    if languages is not None:
        if len(languages) != len(labels):
            raise ValueError(f"{len(languages)} languages for {len(labels)} labels")
        unknown = sorted(set(languages) - set(maps.languages))
        if unknown:
            raise ValueError(f"languages {unknown} are not among {maps.languages}")
    return {name: output_targets(maps, o, labels) for o, name in enumerate(maps.names)}


def output_targets(maps, o: int, labels: Sequence[Sequence[str]], row_name: str = "utterance") -> List[List[int]]:
    """``label_targets`` for output ``o`` of ``maps`` alone; ``row_name`` is what an error calls a row of ``labels``."""
    name = maps.names[o]
    categories = list(maps.inventory) if name in IPA_LAYERS else maps.table.feature_categories(name)
    classes = {}
    for k, symbol in enumerate(categories):
        classes.setdefault(symbol, k + BLANK_OFFSET)
    rows = []
    for n, label in enumerate(labels):
        unknown = [s for s in label if s not in maps.label_ids]
        if unknown:
            raise ValueError(f"output {name!r}, {row_name} {n}: label symbol {unknown[0]!r} is not in the attribute table")
        row = []
        for symbol in maps.expand_label(o, label):
            if symbol not in classes:
                raise ValueError(f"output {name!r}, {row_name} {n}: symbol {symbol!r} has no class under this inventory")
            row.append(classes[symbol])
        rows.append(row)
    return rows

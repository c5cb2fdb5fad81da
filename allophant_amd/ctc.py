"""The call frame that the CTC entry points share: ``greedy_ctc_decode`` / ``beam_ctc_decode`` (``estimator``),
``ctc_forced_align`` (``alignment``), ``ctc_score`` (``scoring``) and ``ctc_search`` (``search``) all take one ``[N, T, C]``
emission tensor, pack integer rows as offsets and ids, and allocate outputs that may have no element."""
from __future__ import annotations

import math
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import lib as _lib

MAX_TARGET = _lib.ALIGN_MAX_TARGET  # (the scoring limit is the same, and the search's is smaller)
assert MAX_TARGET == _lib.SCORE_MAX_TARGET >= _lib.SEARCH_MAX_QUERY


def frame_stride(spec: Dict[str, Any]) -> int:
    """Samples per output frame: the product of the spec's convolution strides."""
    return math.prod(int(s) for s in spec["conv_stride"])


def emissions(log_emissions: Tensor, verb: str) -> Tuple[Tensor, int, int, int]:
    """``log_emissions`` as the C ABI reads it (fp32, unit class stride, otherwise in place) and its ``N, T, C``.  ``verb``
    says what the caller does on the MI355X ("decodes", "aligns", ...)."""
    if log_emissions.dim() != 3:
        raise ValueError("log_emissions must be [N, T, C]")
    if log_emissions.device.type != "cuda":
        raise RuntimeError(f"allophant_amd {verb} on an MI355X only (log_emissions must be a cuda tensor); there is no CPU fallback")
    if log_emissions.dtype != torch.float32:
        log_emissions = log_emissions.float()
    if log_emissions.stride(2) != 1:
        log_emissions = log_emissions.contiguous()
    return (log_emissions, *log_emissions.shape)


def check_classes(classes: int, blank_index: int, what: Optional[str] = None) -> None:
    """``blank_index`` lies in the classes, of which ``what`` (when given: "alignment", "scoring", ...) needs two."""
    if what is not None and classes < 2:
        raise ValueError(f"{what} needs at least 2 classes")
    if not 0 <= blank_index < classes:
        raise ValueError("blank_index out of range")


class Frame(NamedTuple):
    """Where a call over an emission tensor runs: the int32 ``frame_lengths`` on the device, its index and the stream."""
    frame_lengths: Tensor
    index: int
    stream: int


def frame(log_emissions: Tensor, lengths: Optional[Tensor]) -> Frame:
    """The ``Frame`` of a call over ``log_emissions``; without ``lengths`` every utterance has all ``T`` frames."""
    device = log_emissions.device
    if lengths is None:
        frame_lengths = torch.full(log_emissions.shape[:1], log_emissions.shape[1], dtype=torch.int32, device=device)
    else:
        frame_lengths = lengths.detach().to(device=device, dtype=torch.int32).contiguous()
    return Frame(frame_lengths, device.index if device.index is not None else torch.cuda.current_device(),
                 torch.cuda.current_stream(device).cuda_stream)


def pack_targets(rows: Sequence[Sequence[int]], utterances: Optional[int] = None, candidates: int = 1,
                 limit: int = MAX_TARGET) -> Tuple[Tensor, Tensor, List[int]]:
    """Target rows as the C ABI takes them: int32 offsets ``[R + 1]``, int32 ids, and the rows' lengths (host tensors).  With
    ``utterances`` the row count must be ``utterances * candidates`` (row ``n * candidates + g``).  ``limit`` is the most
    targets a row may have (``lib.ALIGN_LONG_MAX_TARGET`` for the long form of the alignment)."""
    if candidates < 1:
        raise ValueError("candidates must be at least 1")
    if utterances is not None and len(rows) != utterances * candidates:
        raise ValueError(f"{len(rows)} target rows for {utterances} emission rows x {candidates} candidates")
    counts = [len(row) for row in rows]
    if counts and max(counts) > limit:
        raise ValueError(f"at most {limit} targets per row on the device, got {max(counts)}")
    offsets = torch.zeros(len(rows) + 1, dtype=torch.int32)
    if rows:
        offsets[1:] = torch.cumsum(torch.tensor(counts, dtype=torch.int64), 0).to(torch.int32)
    ids = torch.tensor([int(v) for row in rows for v in row], dtype=torch.int32)
    return offsets, ids, counts


def empty(*shape: int, dtype: torch.dtype, device) -> Tensor:
    """``torch.empty`` of ``shape`` over at least one element, so that its pointer is valid when the shape holds none."""
    count = math.prod(shape)
    return torch.empty(max(1, count), dtype=dtype, device=device)[:count].view(*shape)

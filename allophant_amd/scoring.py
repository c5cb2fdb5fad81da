"""CTC forward-backward scoring on the device (``include/allophant_amx_score.h``): how probable a known label sequence is
given the emissions (the sum over every alignment, where ``alignment`` finds the best one), and the posterior occupancy,
position and log-probability of each of its symbols.

  * ``ctc_score``  one ``[N, T, C]`` emission tensor, ``candidates`` target rows per utterance
  * ``Estimator.score_device`` / ``Estimator.score``  every output of a ``Predictions`` (``Scored`` stays in HBM)
  * ``Estimator.rescore_device``  the exact log-likelihood of every hypothesis of a ``BeamDecoded`` and the softmax over
    each n-best list

There is no CPU path."""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import ctc as _ctc, lib as _lib
from .ctc import frame_stride, pack_targets  # noqa: F401  (part of this module's interface)

SCORE_MAX_TARGET = _lib.SCORE_MAX_TARGET


class Score(NamedTuple):
    """One scored row on the host: ``log_likelihood`` = log P(targets | emissions); per target, fp32 ``[L]``, ``occupancy``
    the expected number of frames it holds, ``positions`` its expected frame (``position_sums / occupancy``) and ``scores``
    its expected log-probability (``score_sums / occupancy``); ``posteriors`` fp32 ``[len, 2L + 1]`` the probability of each
    trellis state (blank, y0, blank, ...) in each frame, or ``None`` when they were not asked for."""
    log_likelihood: float
    occupancy: Tensor
    positions: Tensor
    scores: Tensor
    posteriors: Optional[Tensor]

    def seconds(self, spec: Dict[str, Any], sample_rate: int = 16000) -> Tensor:
        """``positions`` in seconds (float64 ``[L]``): frame index x the spec's frame stride / sample rate."""
        return self.positions.to(torch.float64) * (frame_stride(spec) / float(sample_rate))


class Scored(NamedTuple):
    """Forward-backward scores of a batch on the device (layout and status codes as in ``include/allophant_amx_score.h``).
    With ``names`` (the outputs of a ``Predictions``; ``present`` those that were given targets) the leading shape is
    ``[O, N, G]``, for one emission tensor (``names`` is ``None``) ``[N, G]``, ``G`` the candidates per utterance:
    ``log_likelihood`` fp32 / ``status`` int32 ``[..., G]``, ``occupancy`` / ``position_sums`` / ``score_sums`` fp32
    ``[..., G, max_target]``, ``posteriors`` fp32 ``[..., G, T, 2 max_target + 1]`` or ``None``.  ``lengths`` (per utterance)
    and ``target_counts`` (per row, flat) are on the host."""
    names: Optional[List[str]]
    present: List[str]
    log_likelihood: Tensor
    occupancy: Tensor
    position_sums: Tensor
    score_sums: Tensor
    posteriors: Optional[Tensor]
    status: Tensor
    lengths: List[int]
    target_counts: List[int]

    def _rows(self, first: int, label: str) -> List[List[Optional[Score]]]:
        """Host form of the ``N x G`` rows that start at flat row ``first``."""
        N, G = self.status.shape[-2:]
        flat = lambda t: t.reshape(-1, *t.shape[self.status.dim():])[first:first + N * G].cpu()  # noqa: E731
        status = flat(self.status).tolist()
        bad = [r for r, s in enumerate(status) if s == -2]
        if bad:
            raise ValueError(f"{label} {bad[0] // G}, candidate {bad[0] % G}: malformed scoring row (a target equal to the blank "
                             "or outside the classes, a frame length outside the tensor, more targets than max_target, or "
                             "offsets that do not ascend)")
        ll, occupancy, position_sums, score_sums = (flat(t) for t in (self.log_likelihood, self.occupancy, self.position_sums,
                                                                      self.score_sums))
        posteriors = None if self.posteriors is None else flat(self.posteriors)
        out: List[List[Optional[Score]]] = []
        for n in range(N):
            out.append([])
            for g in range(G):
                r = n * G + g
                if status[r] != 0:
                    out[-1].append(None)
                    continue
                L, k = int(self.target_counts[first + r]), int(self.lengths[n])
                occ = occupancy[r, :L].clone()
                out[-1].append(Score(float(ll[r]), occ, position_sums[r, :L] / occ, score_sums[r, :L] / occ,
                                     None if posteriors is None else posteriors[r, :k, :2 * L + 1].clone()))
        return out

    def scores(self) -> Union[List[List[Optional[Score]]], Dict[str, List[List[Optional[Score]]]]]:
        """Fetched to the host: per utterance and candidate a ``Score``, or ``None`` where no path exists (per present output
        first, when the rows are the outputs of a ``Predictions``); ``ValueError`` names a malformed row."""
        if self.names is None:
            return self._rows(0, "row")
        N, G = self.status.shape[-2:]
        return {name: self._rows(o * N * G, f"output {name!r}, utterance") for o, name in enumerate(self.names)
                if name in self.present}

    def ctc_loss(self, zero_infinity: bool = True) -> Tensor:
        """The negated sum of the rows' ``log_likelihood`` (of the present outputs) as a float64 device scalar: upstream's
        ``CTCWrapper`` value, ``nn.CTCLoss(reduction="sum", zero_infinity=True)``.  Rows without a path (status -1) count as
        0, or as ``+inf`` with ``zero_infinity=False``; a malformed row (status -2) makes the result NaN."""
        ll, status = self.log_likelihood, self.status
        if self.names is not None:
            keep = [o for o, name in enumerate(self.names) if name in self.present]
            ll, status = ll[keep], status[keep]
        loss = -ll.to(torch.float64)
        loss = torch.where(status == -1, torch.full_like(loss, 0.0 if zero_infinity else math.inf), loss)
        loss = torch.where(status == -2, torch.full_like(loss, math.nan), loss)
        return loss.sum()


class Rescored(NamedTuple):
    """Exact scores of an n-best list: ``log_likelihood`` fp32 ``[O, N, n_best]`` = log P(hypothesis | emissions), ``-inf`` at
    and past ``hyp_counts``; ``nbest_posteriors`` the softmax over each list's present hypotheses (0 for the absent ones, and
    for a list none of whose hypotheses has a path); ``status`` int32 ``[O, N, n_best]``."""
    names: List[str]
    log_likelihood: Tensor
    nbest_posteriors: Tensor
    status: Tensor


class _Buffers(NamedTuple):
    workspace: Tensor
    size: int
    log_likelihood: Tensor
    occupancy: Tensor
    position_sums: Tensor
    score_sums: Tensor
    posteriors: Optional[Tensor]
    status: Tensor

    def pointers(self):
        p = lambda t: C.c_void_p(None if t is None else t.data_ptr())  # noqa: E731
        return (p(self.workspace), self.size, p(self.log_likelihood), p(self.occupancy), p(self.position_sums), p(self.score_sums),
                p(self.posteriors), p(self.status))


def allocate(lib, rows: int, T: int, max_target: int, device, posteriors: bool = False) -> _Buffers:
    """The workspace and outputs of ``rows`` rows of ``T`` frames (at least one element each, so every pointer is valid)."""
    size = C.c_size_t()
    _lib.check(lib, None, lib.amx_ctc_score_workspace(rows, T, max_target, C.byref(size)))
    empty = lambda *shape: _ctc.empty(*shape, dtype=torch.float32, device=device)  # noqa: E731
    return _Buffers(torch.empty(max(1, size.value), dtype=torch.uint8, device=device), size.value, empty(rows),
                    empty(rows, max_target), empty(rows, max_target), empty(rows, max_target),
                    empty(rows, T, 2 * max_target + 1) if posteriors else None,
                    _ctc.empty(rows, dtype=torch.int32, device=device))


def scored(b: _Buffers, leading: Tuple[int, ...], T: int, max_target: int, names, present, lengths, counts) -> Scored:
    """``Scored`` over the buffers of one call, the rows viewed as ``leading``."""
    return Scored(names, present, b.log_likelihood.view(*leading), b.occupancy.view(*leading, max_target),
                  b.position_sums.view(*leading, max_target), b.score_sums.view(*leading, max_target),
                  None if b.posteriors is None else b.posteriors.view(*leading, T, 2 * max_target + 1),
                  b.status.view(*leading), lengths, counts)


def ctc_score(log_emissions: Tensor, lengths: Optional[Tensor], targets: Union[Sequence[Sequence[int]], Tuple[Tensor, Tensor]],
              blank_index: int = 0, candidates: int = 1, posteriors: bool = False) -> Scored:
    """Forward-backward scores of each row's ``targets`` under ``log_emissions`` (an fp32 ``[N, T, C]`` cuda tensor of any
    strides with a unit class stride, read in place) via ``amx_ctc_score_emissions``.  ``targets``: one int sequence per row
    ``n * candidates + g``, or a padded ``[N * candidates, max_len]`` tensor with its lengths ``(padded, target_lengths)``.
    Returns the device form (leading shape ``[N, candidates]``); ``Scored.scores()`` fetches it."""
    log_emissions, N, T, Cn = _ctc.emissions(log_emissions, "scores")
    lib = _lib.load()
    device = log_emissions.device
    if isinstance(targets, tuple) and len(targets) == 2 and isinstance(targets[0], Tensor):
        padded, target_lengths = targets[0].cpu().tolist(), [int(v) for v in targets[1].cpu().tolist()]
        targets = [row[:k] for row, k in zip(padded, target_lengths)]
    _ctc.check_classes(Cn, blank_index, "scoring")
    offsets, ids, counts = pack_targets(targets, N, candidates)
    max_target = max(counts, default=0)
    with torch.cuda.device(device):
        frame_lengths, index, stream = _ctc.frame(log_emissions, lengths)
        b = allocate(lib, N * candidates, T, max_target, device, posteriors)
        if N:
            meta = torch.cat([offsets, ids, torch.zeros(1, dtype=torch.int32)]).to(device)  # (never an empty tensor)
            code = lib.amx_ctc_score_emissions(
                index, C.c_void_p(log_emissions.data_ptr()), log_emissions.stride(0), log_emissions.stride(1),
                C.c_void_p(frame_lengths.data_ptr()), N, T, Cn, blank_index, candidates, C.c_void_p(meta.data_ptr()),
                C.c_void_p(meta.data_ptr() + 4 * (N * candidates + 1)), max_target, *b.pointers(), C.c_void_p(stream))
            _lib.check(lib, None, code)
        return scored(b, (N, candidates), T, max_target, None, [], frame_lengths.cpu().tolist(), counts)

"""CTC scoring of every one-edit variant of a transcript on the device (``include/allophant_amx_variants.h``): where the
model disagrees with a known label sequence, and with what alternative -- pronunciation assessment and transcript
verification.

  * ``ctc_variants``  one ``[N, T, C]`` emission tensor and one transcript per utterance (``Variants`` stays in HBM)
  * ``Estimator.variants_device`` / ``Estimator.variants``  one output of a ``Predictions``

For every position ``l`` of a transcript the log-likelihood of the transcript with ``y[l]`` replaced by each class (the blank
column: with ``y[l]`` deleted), and for every gap ``p`` with each class inserted there (the blank column: nothing inserted,
the transcript's own log-likelihood).  There is no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import ctc as _ctc, lib as _lib
from .evaluation import Action

VARIANTS_MAX_TARGET = _lib.VARIANTS_MAX_TARGET
VARIANTS_MAX_CLASSES = _lib.VARIANTS_MAX_CLASSES

Finding = Tuple[Action, int, int, float]  # (kind, position or gap, class, log-likelihood ratio against the transcript)


class Alternatives(NamedTuple):
    """The ``k`` most probable classes per position and per gap with their log-posteriors, best first:
    ``substitution_*`` ``[N, max_target, k]``, ``insertion_*`` ``[N, max_target + 1, k]``.  The blank stands for "nothing"
    (the symbol deleted, or nothing inserted)."""
    substitution_classes: Tensor
    substitution_log_posteriors: Tensor
    insertion_classes: Tensor
    insertion_log_posteriors: Tensor


class Variants(NamedTuple):
    """One-edit variants of ``N`` transcripts (layout and status codes as in ``include/allophant_amx_variants.h``):
    ``log_likelihood`` fp32 / ``status`` int32 ``[N]``, ``substitutions`` fp32 ``[N, max_target, C]``, ``insertions`` fp32
    ``[N, max_target + 1, C]``, ``targets`` int64 ``[N, max_target]`` (padded with the blank) and ``target_counts`` int64
    ``[N]``, all on the device; ``lengths`` are the frame lengths on the host.  Only rows of status 0 hold variants, and only
    their first ``target_counts`` positions (one more gap); the methods give NaN elsewhere."""
    log_likelihood: Tensor
    substitutions: Tensor
    insertions: Tensor
    status: Tensor
    targets: Tensor
    target_counts: Tensor
    blank: int
    lengths: List[int]

    def _valid(self, gaps: bool) -> Tensor:
        """Which positions (or gaps) of which rows hold variants: bool ``[N, max_target (+ 1)]``."""
        width = self.targets.shape[1] + (1 if gaps else 0)
        at = torch.arange(width, device=self.status.device).view(1, width)
        return (at < self.target_counts.view(-1, 1) + (1 if gaps else 0)) & (self.status == 0).view(-1, 1)

    def _masked(self, values: Tensor, gaps: bool) -> Tensor:
        valid = self._valid(gaps)
        return torch.where(valid.view(*valid.shape, *([1] * (values.dim() - 2))), values, torch.full_like(values, float("nan")))

    def goodness(self) -> Tensor:
        """``sub[l][y[l]] - logsumexp_c sub[l][c]``, fp32 ``[N, max_target]``: the log-posterior of the transcript's own symbol
        at each position given the rest of the transcript (goodness of pronunciation).  NaN where no variant of the position
        has a path."""
        own = self.substitutions.gather(2, self.targets.unsqueeze(2)).squeeze(2)
        return self._masked(own - torch.logsumexp(self.substitutions, 2), False)

    def insertion_free(self) -> Tensor:
        """``ins[p][blank] - logsumexp_c ins[p][c]``, fp32 ``[N, max_target + 1]``: the log-posterior that nothing stands in
        each gap."""
        return self._masked(self.insertions[:, :, self.blank] - torch.logsumexp(self.insertions, 2), True)

    def alternatives(self, k: int) -> Alternatives:
        """The top ``k`` classes of every position and gap with their log-posteriors."""
        sub = torch.topk(self.substitutions - torch.logsumexp(self.substitutions, 2, keepdim=True), k, dim=2)
        ins = torch.topk(self.insertions - torch.logsumexp(self.insertions, 2, keepdim=True), k, dim=2)
        return Alternatives(sub.indices, self._masked(sub.values, False), ins.indices, self._masked(ins.values, True))

    def diagnose(self, threshold: float = 0.0) -> List[Optional[List[Finding]]]:
        """Fetched to the host: per utterance (``None`` for status -1) every single edit whose log-likelihood exceeds the
        transcript's by more than ``threshold`` nats, as ``(kind, position, class, log_ratio)`` ordered by position: a
        ``SUBSTITUTION`` of ``y[position]`` by ``class``, a ``DELETION`` of ``y[position]`` (``class`` is the deleted symbol) or
        an ``INSERTION`` of ``class`` into the gap before ``y[position]``.  ``ValueError`` names a malformed row."""
        status = self.status.cpu().tolist()
        bad = [n for n, s in enumerate(status) if s == -2]
        if bad:
            raise ValueError(f"row {bad[0]}: malformed variants row (a target equal to the blank or outside the classes, a frame "
                             "length outside the tensor, more targets than max_target, or offsets that do not ascend)")
        ll = self.log_likelihood.view(-1, 1, 1)
        with_sub = (self.substitutions - ll > threshold) & self._valid(False).unsqueeze(2)
        own = torch.zeros_like(with_sub).scatter_(2, self.targets.unsqueeze(2), True)
        with_sub &= ~own
        with_ins = (self.insertions - ll > threshold) & self._valid(True).unsqueeze(2)
        with_ins[:, :, self.blank] = False
        sub_ratio, ins_ratio = (self.substitutions - ll).cpu(), (self.insertions - ll).cpu()
        targets = self.targets.cpu()
        found: List[Optional[List[Finding]]] = [None if s != 0 else [] for s in status]
        for n, l, c in with_sub.nonzero().cpu().tolist():
            deleted = c == self.blank
            found[n].append((Action.DELETION if deleted else Action.SUBSTITUTION, l, int(targets[n, l]) if deleted else c,
                             float(sub_ratio[n, l, c])))
        for n, p, c in with_ins.nonzero().cpu().tolist():
            found[n].append((Action.INSERTION, p, c, float(ins_ratio[n, p, c])))
        for row in found:
            if row:
                row.sort(key=lambda f: (f[1], f[0] != Action.INSERTION, f[2]))  # a gap comes before the position it precedes
        return found


def check_targets(targets: Sequence[Sequence[int]], classes: int, blank_index: int) -> None:
    """``ValueError`` names a transcript symbol that is the blank or outside the classes."""
    for n, row in enumerate(targets):
        for v in row:
            if int(v) == blank_index:
                raise ValueError(f"row {n}: the blank ({blank_index}) among the targets")
            if not 0 <= int(v) < classes:
                raise ValueError(f"row {n}: target {int(v)} outside the {classes} classes")


def ctc_variants(log_emissions: Tensor, lengths: Optional[Tensor], targets: Sequence[Sequence[int]], blank: int = 0) -> Variants:
    """The one-edit variants of each row's ``targets`` (one int sequence per utterance) under ``log_emissions`` (an fp32
    ``[N, T, C]`` cuda tensor of any strides with a unit class stride, read in place) via ``amx_ctc_variants_emissions``.
    Returns the device form; ``Variants.diagnose()`` fetches the edits that beat the transcript."""
    if log_emissions.dim() != 3:
        raise ValueError("log_emissions must be [N, T, C]")
    classes = log_emissions.shape[2]
    _ctc.check_classes(classes, blank, "variant scoring")
    if classes > VARIANTS_MAX_CLASSES:
        raise ValueError(f"at most {VARIANTS_MAX_CLASSES} classes on the device, got {classes}")
    targets = [[int(v) for v in row] for row in targets]
    check_targets(targets, classes, blank)
    offsets, ids, counts = _ctc.pack_targets(targets, log_emissions.shape[0], limit=VARIANTS_MAX_TARGET)
    log_emissions, N, T, Cn = _ctc.emissions(log_emissions, "scores variants")
    lib = _lib.load()
    device = log_emissions.device
    max_target = max(counts, default=0)
    with torch.cuda.device(device):
        frame_lengths, index, stream = _ctc.frame(log_emissions, lengths)
        if frame_lengths.shape != (N,):
            raise ValueError(f"{frame_lengths.numel()} lengths for {N} emission rows")
        size = C.c_size_t()
        _lib.check(lib, None, lib.amx_ctc_variants_workspace(N, T, max_target, C.byref(size)))
        workspace = torch.empty(max(1, size.value), dtype=torch.uint8, device=device)
        empty = lambda *shape, dtype=torch.float32: _ctc.empty(*shape, dtype=dtype, device=device)  # noqa: E731
        ll, sub, ins = empty(N), empty(N, max_target, Cn), empty(N, max_target + 1, Cn)
        status = empty(N, dtype=torch.int32)
        padded = torch.full((N, max_target), blank, dtype=torch.int64)
        for n, row in enumerate(targets):
            padded[n, :len(row)] = torch.tensor(row, dtype=torch.int64)
        if N:
            meta = torch.cat([offsets, ids, torch.zeros(1, dtype=torch.int32)]).to(device)  # (never an empty tensor)
            p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
            code = lib.amx_ctc_variants_emissions(
                index, p(log_emissions), log_emissions.stride(0), log_emissions.stride(1), p(frame_lengths), N, T, Cn, blank,
                p(meta), C.c_void_p(meta.data_ptr() + 4 * (N + 1)), max_target, p(workspace), size.value, p(ll), p(sub), p(ins),
                p(status), C.c_void_p(stream))
            _lib.check(lib, None, code)
        return Variants(ll, sub, ins, status, padded.to(device), torch.tensor(counts, dtype=torch.int64).to(device), blank,
                        frame_lengths.cpu().tolist())

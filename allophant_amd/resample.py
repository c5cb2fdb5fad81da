"""Sinc resampling on the device: what upstream runs before every ``Estimator.predict``.

Upstream resamples each utterance with torchaudio, on the host: the README's inference recipe calls
``torchaudio.functional.resample(audio, sample_rate, model.sample_rate)``, and the corpus loader of ``run.py predict`` applies
``torchaudio.transforms.Resample(source_rate, 16000)`` with default parameters (datasets/speech_corpus.py).  Here
``amx_resample`` (include/allophant_amx_resample.h) computes the same ``sinc_interp_hann`` resampling for a whole padded
batch in one launch, one source rate per row:

  * ``resample`` / ``Resample``   ``torchaudio.functional.resample`` / ``torchaudio.transforms.Resample`` for fp32 cuda tensors
  * ``resample_batch``            a ``Batch`` at mixed source rates -> a ``Batch`` at ``new_freq`` (``Estimator.resample``)

The filter bank is built on the host (``amx_resample_bank``: float64, rounded to fp32 once) and kept on the device.  There is
no CPU path: CPU tensors and other dtypes raise.
"""
from __future__ import annotations

import ctypes as C
import math
import threading
from typing import Dict, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import lib as _lib

_METHOD = "sinc_interp_hann"


def _check_method(resampling_method: str) -> None:
    if resampling_method != _METHOD:
        raise ValueError(f"only resampling_method={_METHOD!r} is supported on the device (upstream uses no other), "
                         f"got {resampling_method!r}")


def _reduced(orig_freq: int, new_freq: int) -> Tuple[int, int]:
    g = math.gcd(orig_freq, new_freq)
    return orig_freq // g, new_freq // g


def _rate(value, name: str) -> int:
    if isinstance(value, float) and not value.is_integer():
        raise ValueError(f"{name} must be an integer number of Hz, got {value}")
    rate = int(value)
    if rate <= 0:
        raise ValueError(f"{name} must be positive, got {value}")
    return rate


def output_length(n: int, orig_freq: int, new_freq: int) -> int:
    """``ceil(new * n / orig)`` in exact integer arithmetic (upstream's utterance-length rule, speech_corpus.py)."""
    o, m = _reduced(orig_freq, new_freq)
    return -(-m * n // o)


def host_bank(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """``amx_resample_bank`` (pure host code): ``(geometry, bank fp32 [K, m] tap-major, phases int32 [2, m])`` where
    ``phases[0]`` holds each phase's first kept tap and ``phases[1]`` its count; raises ``ValueError`` outside the limits."""
    lib = _lib.load()
    geometry = _lib.AmxResampleGeometry()
    _lib.check(lib, None, lib.amx_resample_bank(orig_freq, new_freq, lowpass_filter_width, float(rolloff), C.byref(geometry),
                                                None, None))
    bank = torch.zeros(geometry.taps, geometry.m, dtype=torch.float32)
    phases = torch.zeros(2, geometry.m if geometry.taps else 0, dtype=torch.int32)
    _lib.check(lib, None, lib.amx_resample_bank(orig_freq, new_freq, lowpass_filter_width, float(rolloff), C.byref(geometry),
                                                C.c_void_p(bank.data_ptr()), C.c_void_p(phases.data_ptr())))
    return geometry, bank, phases


class _DeviceBank:
    """One geometry's bank and phase table on one device."""

    def __init__(self, orig_freq: int, new_freq: int, lowpass_filter_width: int, rolloff: float, device: torch.device):
        self.geometry, bank, phases = host_bank(orig_freq, new_freq, lowpass_filter_width, rolloff)
        self.bank = bank.reshape(-1).to(device)
        self.phases = phases.reshape(-1).to(device)
        self.row_dev = torch.tensor(self.row(), dtype=torch.int64).to(device)

    def row(self, bank_offset: int = 0, phase_offset: int = 0):
        return _row(self.geometry, bank_offset, phase_offset)


def _row(geometry, bank_offset: int = 0, phase_offset: int = 0):
    """An amx_resample_row (fields in lib.RESAMPLE_ROW_FIELDS order)."""
    return [geometry.o, geometry.m, geometry.width, geometry.taps, bank_offset, phase_offset]


_banks: Dict[tuple, _DeviceBank] = {}
_banks_lock = threading.Lock()


def _device_bank(orig_freq: int, new_freq: int, lowpass_filter_width: int, rolloff: float, device: torch.device) -> _DeviceBank:
    """The bank of ``(o, m, lowpass_filter_width, rolloff)`` on ``device``, built once per process."""
    o, m = _reduced(orig_freq, new_freq)
    key = (o, m, int(lowpass_filter_width), float(rolloff), device)
    with _banks_lock:
        entry = _banks.get(key)
        if entry is None:
            entry = _banks[key] = _DeviceBank(o, m, lowpass_filter_width, rolloff, device)
    return entry


def _device_index(device: torch.device) -> int:
    return device.index if device.index is not None else torch.cuda.current_device()


def _launch(x: Tensor, lengths: Tensor, rows: Tensor, bank: Tensor, phases: Tensor, window: int, L_out: int) -> Tensor:
    """``amx_resample`` on the current stream of ``x``'s device: x fp32 [N, L_in] with unit time stride, lengths int64 [N] and
    rows int64 [N, 6] on that device.  Returns y fp32 [N, L_out], written completely by the kernel."""
    lib = _lib.load()
    N, L_in = x.shape
    device = x.device
    y = torch.empty(N, L_out, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        code = lib.amx_resample(_device_index(device), C.c_void_p(x.data_ptr()), x.stride(0) if N > 1 else L_in, L_in,
                                C.c_void_p(lengths.data_ptr()), C.c_void_p(rows.data_ptr()), C.c_void_p(bank.data_ptr()),
                                C.c_void_p(phases.data_ptr()), window, N, L_out, C.c_void_p(y.data_ptr()), C.c_void_p(stream))
        _lib.check(lib, None, code)
    return y


def _check_waveform(waveform: Tensor) -> None:
    if not isinstance(waveform, Tensor):
        raise TypeError("waveform must be a torch.Tensor")
    if waveform.device.type != "cuda":
        raise RuntimeError("allophant_amd resamples on an MI355X only (the waveform must be a cuda tensor); there is no CPU "
                           "fallback")
    if waveform.dtype != torch.float32:
        raise TypeError(f"the device resampler takes float32 waveforms, got {waveform.dtype}")
    if waveform.dim() < 1:
        raise ValueError("waveform must have a time dimension (the last one)")


def _rows_2d(waveform: Tensor) -> Tensor:
    """[..., L] -> [N, L] with unit time stride (a view whenever the layout allows one: any row stride is read in place)."""
    x = waveform.reshape(-1, waveform.shape[-1])
    if x.shape[1] > 1 and x.stride(1) != 1:
        x = x.contiguous()
    return x


def _resample_with(waveform: Tensor, geometry, bank: Tensor, phases: Tensor, row: Tensor) -> Tensor:
    """Every row of ``waveform`` [..., L] at one geometry; ``row`` is its int64 [6] descriptor on the device.  Only device
    work is enqueued (a fill, a copy, the kernel)."""
    x = _rows_2d(waveform)
    N, L = x.shape
    L_out = output_length(L, geometry.o, geometry.m)
    if N == 0 or L_out == 0:
        return torch.zeros(*waveform.shape[:-1], L_out, dtype=torch.float32, device=waveform.device)
    lengths = torch.full((N,), L, dtype=torch.int64, device=x.device)
    rows = row.expand(N, len(_lib.RESAMPLE_ROW_FIELDS)).contiguous()
    y = _launch(x, lengths, rows, bank, phases, geometry.window, L_out)
    return y.view(*waveform.shape[:-1], L_out)


def resample(waveform: Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
             resampling_method: str = _METHOD) -> Tensor:
    """``torchaudio.functional.resample`` for fp32 cuda tensors of shape ``[..., time]``: band-limited sinc interpolation
    with a Hann window.  ``orig_freq == new_freq`` returns ``waveform`` itself, like torchaudio.  Any row stride is read in
    place; a time stride other than 1 is copied first.  Asynchronous on the current stream (no host synchronisation)."""
    _check_method(resampling_method)
    orig_freq, new_freq = _rate(orig_freq, "orig_freq"), _rate(new_freq, "new_freq")
    _check_waveform(waveform)
    if orig_freq == new_freq:
        return waveform
    entry = _device_bank(orig_freq, new_freq, lowpass_filter_width, rolloff, waveform.device)
    return _resample_with(waveform, entry.geometry, entry.bank, entry.phases, entry.row_dev)


class Resample(torch.nn.Module):
    """``torchaudio.transforms.Resample(orig_freq, new_freq, resampling_method, lowpass_filter_width, rolloff)`` on the device.
    The bank is built once, at construction, and held as (non-persistent) buffers: move the module with ``.to(device)`` /
    ``.cuda()``, as upstream's.  A call launches only device work (a fill, a copy and the kernel), so it can be captured in
    a ``torch.cuda.graph``."""

    def __init__(self, orig_freq: int = 16000, new_freq: int = 16000, resampling_method: str = _METHOD,
                 lowpass_filter_width: int = 6, rolloff: float = 0.99) -> None:
        super().__init__()
        _check_method(resampling_method)
        self.orig_freq, self.new_freq = _rate(orig_freq, "orig_freq"), _rate(new_freq, "new_freq")
        self.resampling_method = resampling_method
        self.lowpass_filter_width = int(lowpass_filter_width)
        self.rolloff = float(rolloff)
        geometry, bank, phases = host_bank(self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff)
        self._geometry = geometry
        self.register_buffer("bank", bank.reshape(-1), persistent=False)
        self.register_buffer("phases", phases.reshape(-1), persistent=False)
        self.register_buffer("row", torch.tensor(_row(geometry), dtype=torch.int64), persistent=False)

    def forward(self, waveform: Tensor) -> Tensor:
        _check_waveform(waveform)
        if self.orig_freq == self.new_freq:
            return waveform
        if self.bank.device != waveform.device:
            raise RuntimeError(f"the Resample module is on {self.bank.device}, the waveform on {waveform.device}: move the "
                               "module with .to(device)")
        return _resample_with(waveform, self._geometry, self.bank, self.phases, self.row)


def resample_batch(batch, sample_rates: Union[int, Sequence[int], Tensor], new_freq: int = 16000,
                   lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """A padded ``Batch`` whose utterance n was recorded at ``sample_rates[n]`` (an int applies to every row; rates may be
    mixed freely) -> a new ``Batch`` at ``new_freq``, in one launch: ``lengths = ceil(m * len / o)`` per row,
    ``L == max(lengths)``, zero padding, the same ``language_ids``.  Samples at or past each input length are never read.

    The output geometry depends on the lengths, so lengths held on the device cost one host synchronisation (their copy
    to the host); lengths on the host cost none.  The audio must be an fp32 cuda tensor [N, L]."""
    from .estimator import Batch

    audio = batch.audio_features
    _check_waveform(audio)
    if audio.dim() != 2:
        raise ValueError("audio_features must be [N, L]")
    new_freq = _rate(new_freq, "new_freq")
    N, L = audio.shape
    lengths = batch.lengths.detach().to("cpu", torch.int64)  # (the one synchronisation when the lengths are on the device)
    if lengths.dim() != 1 or lengths.numel() != N:
        raise ValueError("lengths must have one entry per utterance")
    if N and (int(lengths.min()) < 0 or int(lengths.max()) > L):
        raise ValueError(f"lengths must lie in [0, {L}] (the padded length of the batch)")
    if isinstance(sample_rates, Tensor):
        rates = [int(r) for r in sample_rates.detach().cpu().reshape(-1).tolist()]
    elif isinstance(sample_rates, (int, float)):
        rates = [sample_rates] * N
    else:
        rates = list(sample_rates)
    if len(rates) != N:
        raise ValueError(f"sample_rates has {len(rates)} entries for {N} utterances")
    rates = [_rate(r, "sample rate") for r in rates]
    device = audio.device

    # one bank per distinct geometry, concatenated in order of first appearance
    entries: Dict[Tuple[int, int], Tuple[_DeviceBank, int, int]] = {}
    bank_parts, phase_parts, rows, out_lengths = [], [], [], []
    bank_off = phase_off = 0
    for rate, n_in in zip(rates, lengths.tolist()):
        key = _reduced(rate, new_freq)
        if key not in entries:
            entry = _device_bank(rate, new_freq, lowpass_filter_width, rolloff, device)
            entries[key] = (entry, bank_off, phase_off)
            bank_parts.append(entry.bank)
            phase_parts.append(entry.phases)
            bank_off += entry.bank.numel()
            phase_off += entry.phases.numel()
        entry, b, p = entries[key]
        rows.append(entry.row(b, p))
        out_lengths.append(output_length(n_in, rate, new_freq))
    new_lengths = torch.tensor(out_lengths, dtype=torch.int64)
    L_out = max(out_lengths, default=0)
    if N == 0 or L_out == 0:
        out = torch.zeros(N, L_out, dtype=torch.float32, device=device)
    else:
        window = max(e.geometry.window for e, _, _ in entries.values())
        bank = bank_parts[0] if len(bank_parts) == 1 else torch.cat(bank_parts)
        phases = phase_parts[0] if len(phase_parts) == 1 else torch.cat(phase_parts)
        x = audio if audio.stride(1) == 1 or L <= 1 else audio.contiguous()
        out = _launch(x, lengths.to(device), torch.tensor(rows, dtype=torch.int64).to(device), bank, phases, window, L_out)
    return Batch(out, new_lengths.to(batch.lengths.device), batch.language_ids)

"""The sinc resampling contract as float64 code: torchaudio's ``functional.resample(..., resampling_method="sinc_interp_hann")``
restated from its definition (include/allophant_amx_resample.h), with the full, untruncated filter bank.

    g = gcd(orig, new), o = orig / g, m = new / g, f_c = min(o, m) * rolloff, W = ceil(lpw * o / f_c)
    tau = clamp(((i - W) / o - j / m) * f_c, -lpw, lpw)            phase j in [0, m), tap i in [0, 2W + o)
    h_j[i] = f_c / o * cos^2(pi tau / (2 lpw)) * sinc(pi tau)       sinc(0) = 1
    y[f * m + j] = sum_i h_j[i] * x[f * o + i - W]                  x = 0 outside [0, len), len' = ceil(m * len / o)
"""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np


def reduced(orig: int, new: int) -> Tuple[int, int]:
    g = math.gcd(orig, new)
    return orig // g, new // g


def output_length(n: int, orig: int, new: int) -> int:
    o, m = reduced(orig, new)
    return -(-m * n // o)


def bank(orig: int, new: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(o, m, W, h float64 [m, 2W + o], tau float64 [m, 2W + o] before the clamp); None for o == m."""
    o, m = reduced(orig, new)
    if o == m:
        return None
    lpw = lowpass_filter_width
    f_c = min(o, m) * rolloff
    W = math.ceil(lpw * o / f_c)
    i = np.arange(2 * W + o, dtype=np.float64)
    j = np.arange(m, dtype=np.float64)
    raw = ((i[None, :] - W) / o - j[:, None] / m) * f_c
    tau = np.clip(raw, -lpw, lpw)
    window = np.cos(np.pi * tau / (2 * lpw)) ** 2
    safe = np.where(tau == 0, 1.0, np.pi * tau)
    sinc = np.where(tau == 0, 1.0, np.sin(safe) / safe)
    return o, m, W, (f_c / o) * window * sinc, raw


def tap_ranges(raw: np.ndarray, lowpass_filter_width: int = 6):
    """Per phase, (first, count) of the taps with |unclamped tau| < lpw: the contiguous run the device keeps."""
    keep = np.abs(raw) < lowpass_filter_width
    first = keep.argmax(axis=1)
    count = keep.sum(axis=1)
    return first, count


def resample_row(x: np.ndarray, orig: int, new: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> np.ndarray:
    """One utterance (1-D, every sample valid) in float64."""
    x = np.asarray(x, dtype=np.float64)
    spec = bank(orig, new, lowpass_filter_width, rolloff)
    if spec is None:
        return x.copy()
    o, m, W, h, _ = spec
    n_out = output_length(len(x), orig, new)
    frames = -(-n_out // m)
    taps = 2 * W + o
    padded = np.zeros(frames * o + taps, dtype=np.float64)
    padded[W: W + len(x)] = x
    windows = np.lib.stride_tricks.sliding_window_view(padded, taps)[:: o][:frames]
    return (windows @ h.T).reshape(-1)[:n_out]


def resample_batch(audio: np.ndarray, lengths, rates, new: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """A padded batch, one source rate per row: (float64 [N, max len'] zero padded, int64 [N] len')."""
    rows = [resample_row(np.asarray(audio[n, : int(lengths[n])]), int(rates[n]), new, lowpass_filter_width, rolloff)
            for n in range(len(lengths))]
    out_len = np.array([len(r) for r in rows], dtype=np.int64)
    out = np.zeros((len(rows), int(out_len.max()) if len(rows) else 0), dtype=np.float64)
    for n, r in enumerate(rows):
        out[n, : len(r)] = r
    return out, out_len

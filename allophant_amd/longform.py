"""Long recordings as windows of utterance size (include/allophant_amx_long.h; ``Estimator.predict_long`` is the user).

One forward pass takes utterance-sized rows: attention is O(T^2) over the whole row, the 32-bit plane offsets run out for rows
of a few minutes, and a wav2vec 2.0 encoder fine-tuned on utterances is not meant to see 40 minutes at once.  A long recording
is therefore predicted as overlapping windows, each an ordinary row of a batch, and the middle frames of every window are
stitched into the output of the recording (HF's CTC pipeline: ``chunk_length_s`` / ``stride_length_s``):

  * ``plan_windows``    the windows of a batch of recordings (``amx_long_plan``, host): ``LongPlan``
  * ``gather_windows``  the windows' audio as one padded batch (``amx_long_gather``, one launch)
  * ``stitch_windows``  the windows' kept output frames into the recordings' outputs (``amx_long_stitch``, one launch)

Frame ``g`` of a recording covers the samples ``[g * hop, g * hop + receptive_field)``, so a window that starts at sample
``a * hop`` produces the recording's frames ``a, a + 1, ...`` as its own ``0, 1, ...``.  There is no CPU path for the two
launches: CPU tensors raise.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Any, Dict, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import lib as _lib

RECORDING, INDEX, START, KEEP_LO, KEEP_HI, SAMPLES = range(6)  # columns of LongPlan.windows (lib.LONG_WINDOW_FIELDS)


@dataclass
class LongPlan:
    """``windows`` int32 ``[W, 6]`` (``recording, index, start, keep_lo, keep_hi, samples``; start / keep_* in frames of the
    recording), rows ordered by recording, then by index; ``frames`` int64 ``[R]`` output frames per recording; ``window``
    samples per window, ``context`` frames dropped on each inner side of a window, ``hop`` samples between two frames."""

    windows: np.ndarray
    frames: np.ndarray
    window: int
    context: int
    hop: int

    def __len__(self) -> int:
        return int(self.windows.shape[0])


def plan_windows(lengths: Sequence[int], spec: Dict[str, Any], window: int, context: int) -> LongPlan:
    """``amx_long_plan`` for recordings of ``lengths`` samples under the conv stack of ``spec``; raises ``ValueError`` where the
    library refuses the arguments (a window below the receptive field, no frame left between the contexts, ...)."""
    lib = _lib.load()
    if not hasattr(lib, "amx_long_plan"):
        raise RuntimeError(f"{_lib.LIB_PATH} predates long recordings (amx_long_plan): rebuild it")
    values = np.ascontiguousarray(np.asarray([int(v) for v in lengths], dtype=np.int64))
    R = int(values.shape[0])
    kernels, strides = list(spec["conv_kernel"]), list(spec["conv_stride"])
    if len(kernels) != len(strides):
        raise ValueError("conv_kernel and conv_stride differ in length")
    conv_kernel, conv_stride = (C.c_int32 * len(kernels))(*kernels), (C.c_int32 * len(strides))(*strides)
    pointer = values.ctypes.data_as(C.POINTER(C.c_int64))
    frames = np.zeros(R, dtype=np.int64)
    count = C.c_int64(0)
    args = (pointer, R, int(window), int(context), conv_kernel, conv_stride, len(kernels))
    _lib.check(lib, None, lib.amx_long_plan(*args, None, 0, C.byref(count), frames.ctypes.data_as(C.POINTER(C.c_int64))))
    windows = np.zeros((count.value, 6), dtype=np.int32)
    _lib.check(lib, None, lib.amx_long_plan(*args, C.c_void_p(windows.ctypes.data), count.value, C.byref(count), None))
    return LongPlan(windows, frames, int(window), int(context), math.prod(int(s) for s in strides))


def _launch_frame(*tensors: Tensor) -> Tuple[int, int]:
    device = tensors[0].device
    for t in tensors:
        if t.device.type != "cuda":
            raise RuntimeError("allophant_amd gathers and stitches windows on an MI355X only (cuda tensors); there is no CPU fallback")
        if t.device != device:
            raise ValueError("the tensors of one call must be on one device")
    index = device.index if device.index is not None else torch.cuda.current_device()
    return index, torch.cuda.current_stream(device).cuda_stream


def _rows(windows: Tensor) -> int:
    if windows.dtype != torch.int32 or windows.dim() != 2 or windows.shape[1] != 6 or not windows.is_contiguous():
        raise ValueError("windows must be a contiguous int32 [n, 6] tensor (LongPlan.windows)")
    return int(windows.shape[0])


def gather_windows(audio: Tensor, lengths: Tensor, windows: Tensor, hop: int, out: Tensor, status: Tensor) -> None:
    """``amx_long_gather`` on the current stream: ``audio`` fp32 ``[R, L]`` with a unit sample stride, ``lengths`` int64
    ``[R]``, ``windows`` int32 ``[n, 6]``, ``out`` fp32 ``[n, L_out]`` contiguous, ``status`` int32 ``[n]``, all on the device.
    ``out[w, s] = audio[recording, start * hop + s]`` for ``s < samples`` and 0 beyond; ``status[w]`` is 0, or -2 for a
    malformed row (written as zeros)."""
    n = _rows(windows)
    if audio.dtype != torch.float32 or audio.dim() != 2 or (audio.shape[1] > 1 and audio.stride(1) != 1):
        raise ValueError("audio must be fp32 [R, L] with a unit sample stride")
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != n or not out.is_contiguous():
        raise ValueError("out must be a contiguous fp32 [n, L_out] tensor")
    R = int(audio.shape[0])
    if lengths.dtype != torch.int64 or lengths.numel() != R or not lengths.is_contiguous():
        raise ValueError("lengths must be a contiguous int64 [R] tensor")
    if status.dtype != torch.int32 or status.numel() < n or not status.is_contiguous():
        raise ValueError("status must be a contiguous int32 tensor of at least n entries")
    index, stream = _launch_frame(audio, lengths, windows, out, status)
    lib = _lib.load()
    code = lib.amx_long_gather(index, C.c_void_p(audio.data_ptr()), audio.stride(0) if R > 1 else audio.shape[1],
                               C.c_void_p(lengths.data_ptr()), R, C.c_void_p(windows.data_ptr()), n, int(hop), int(out.shape[1]),
                               C.c_void_p(out.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(stream))
    _lib.check(lib, None, code)


def stitch_windows(src: Tensor, src_T: int, windows: Tensor, blocks: Sequence[Tuple[int, int, int]], dst: Tensor, R: int,
                   dst_T: int, status: Tensor) -> None:
    """``amx_long_stitch`` on the current stream: ``src`` / ``dst`` flat fp32 device buffers, ``blocks`` host triples
    ``(src_offset, dst_offset, classes)``: block b is ``[src_T, n, classes]`` at ``src[src_offset:]`` and ``[dst_T, R, classes]``
    at ``dst[dst_offset:]``.  ``dst_b[g, recording] = src_b[g - start, w]`` for ``g`` in ``[keep_lo, keep_hi)`` of every row
    ``w``; nothing else in ``dst`` is touched.  ``status[w]`` is 0, or -2 for a malformed row (which writes nothing).  More than
    ``lib.LONG_MAX_BLOCKS`` blocks go out as several launches."""
    n = _rows(windows)
    for t, name in ((src, "src"), (dst, "dst")):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous fp32 buffer")
    if status.dtype != torch.int32 or status.numel() < n or not status.is_contiguous():
        raise ValueError("status must be a contiguous int32 tensor of at least n entries")
    for src_offset, dst_offset, classes in blocks:
        if src_offset < 0 or dst_offset < 0 or classes < 1 or src_offset + src_T * n * classes > src.numel() or \
                dst_offset + dst_T * R * classes > dst.numel():
            raise ValueError(f"block ({src_offset}, {dst_offset}, {classes}) does not lie inside src and dst")
    index, stream = _launch_frame(src, windows, dst, status)
    lib = _lib.load()
    blocks = list(blocks)
    for lo in range(0, len(blocks), _lib.LONG_MAX_BLOCKS):
        part = blocks[lo: lo + _lib.LONG_MAX_BLOCKS]
        array = (_lib.AmxLongBlock * len(part))(*[_lib.AmxLongBlock(*b) for b in part])
        code = lib.amx_long_stitch(index, C.c_void_p(src.data_ptr()), int(src_T), n, C.c_void_p(windows.data_ptr()), array,
                                   len(part), C.c_void_p(dst.data_ptr()), int(R), int(dst_T), C.c_void_p(status.data_ptr()),
                                   C.c_void_p(stream))
        _lib.check(lib, None, code)

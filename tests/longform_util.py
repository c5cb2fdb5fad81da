"""The contract of the long-recording entry points (include/allophant_amx_long.h) restated in NumPy as plain loops: the plan,
the gather of the windows' audio and the stitch of their kept frames.  What the library and the kernels are compared with."""
import numpy as np

RECORDING, INDEX, START, KEEP_LO, KEEP_HI, SAMPLES = range(6)
MALFORMED = -2


def constants(kernels, strides):
    """(S, RF): the hop and the receptive field of a conv stack."""
    S, RF = 1, 1
    for k, s in zip(kernels, strides):
        RF += (k - 1) * S
        S *= s
    return S, RF


def frames(L, kernels, strides):
    S, RF = constants(kernels, strides)
    return 0 if L < RF else (L - RF) // S + 1


def nested_frames(L, kernels, strides):
    """The per-layer formula of the forward pass (csrc conv_lengths), which the closed form must equal."""
    for k, s in zip(kernels, strides):
        L = 0 if L < k else (L - k) // s + 1
    return L


def length_for(T, kernels, strides, extra=0):
    """The shortest recording of T >= 1 frames, plus `extra` samples (< S keeps T)."""
    S, RF = constants(kernels, strides)
    return RF + (T - 1) * S + extra


def plan(lengths, window, context, kernels, strides):
    """(windows int32 [W, 6], frames int64 [R]); ValueError where amx_long_plan returns AMX_EINVAL."""
    S, RF = constants(kernels, strides)
    if window < RF or context < 0 or any(length < 0 for length in lengths):
        raise ValueError("refused")
    Wf = frames(window, kernels, strides)
    K = Wf - 2 * context
    if K < 1:
        raise ValueError("refused")
    rows, counts = [], []
    for r, length in enumerate(lengths):
        T = frames(length, kernels, strides)
        counts.append(T)
        n = 0 if T == 0 else 1 if T <= Wf else -(-(T - Wf) // K) + 1
        for i in range(n):
            a = min(i * K, max(0, T - Wf))
            rows.append((r, i, a, 0 if i == 0 else i * K + context, T if i == n - 1 else (i + 1) * K + context,
                         min(window, length - a * S)))
    return np.array(rows, dtype=np.int32).reshape(-1, 6), np.array(counts, dtype=np.int64)


def gather(audio, lengths, windows, hop, L_out):
    """audio [R, stride] -> (batch fp32 [n, L_out], status int32 [n]); reads nothing at or past lengths[r]."""
    n = len(windows)
    batch, status = np.zeros((n, L_out), dtype=np.float32), np.zeros(n, dtype=np.int32)
    for w, row in enumerate(windows):
        r, a, samples = int(row[RECORDING]), int(row[START]), int(row[SAMPLES])
        if not 0 <= r < len(lengths) or a < 0 or samples < 0 or samples > L_out or a * hop + samples > lengths[r]:
            status[w] = MALFORMED
            continue
        batch[w, :samples] = audio[r, a * hop: a * hop + samples]
    return batch, status


def stitch(src_blocks, windows, dst_blocks):
    """src_blocks: list of [src_T, n, C_b]; dst_blocks: list of [dst_T, R, C_b], changed in place.  Returns status [n]."""
    status = np.zeros(len(windows), dtype=np.int32)
    for w, row in enumerate(windows):
        r, a, lo, hi = int(row[RECORDING]), int(row[START]), int(row[KEEP_LO]), int(row[KEEP_HI])
        src_T, (dst_T, R) = src_blocks[0].shape[0], dst_blocks[0].shape[:2]
        if lo > hi or lo < a or lo < 0 or hi > a + src_T or hi > dst_T or not 0 <= r < R:
            status[w] = MALFORMED
            continue
        for src, dst in zip(src_blocks, dst_blocks):
            dst[lo:hi, r] = src[lo - a: hi - a, w]
    return status

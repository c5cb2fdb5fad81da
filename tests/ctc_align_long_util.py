"""The cut of the long forced alignment (allophant_amd/csrc/amx_ctc_align_long.hip) as a numpy emulation: the trellis swept in
blocks of F frames by tiles that own `owned` states and recompute a left halo of H states from the previous block's last state
row, with the comparisons and the single fp32 addition per cell of ``ctc_align_util._sweep_fast``.  A halo cell at the tile's
left edge lacks its predecessors; with H = 2F that error stops short of the owned states, with a smaller halo it does not."""
from typing import List, Optional, Tuple

import numpy as np

from ctc_align_util import NEG_INF


def sweep_tiled(lp: np.ndarray, y: List[int], blank: int, owned: int, F: int, H: int) -> Tuple[np.ndarray, np.ndarray]:
    """The last state row and the moves ``[T, S]``, as ``_sweep_fast`` returns them."""
    T, S = lp.shape[0], 2 * len(y) + 1
    states = np.arange(S)
    targets = np.asarray(y + [blank], np.int64)
    label = np.where(states % 2 == 0, blank, targets[states // 2])
    skip = np.zeros(S, bool)
    odd = states[(states % 2 == 1) & (states >= 3)]
    skip[odd] = targets[odd // 2] != targets[odd // 2 - 1]
    a = np.full(S, NEG_INF, np.float32)
    a[0] = lp[0, blank]
    if S > 1:
        a[1] = lp[0, y[0]]
    move = np.zeros((T, S), np.int8)
    minus = np.full(2, NEG_INF, np.float32)
    for t_block in range(0, T, F):
        t_first, t_last = max(1, t_block), min(T - 1, t_block + F - 1)
        new = a.copy()  # the other state row: tiles read `a`, owners write `new`
        for own0 in range(0, S, owned):
            base, end = max(own0 - H, 0), min(own0 + owned, S)
            local = np.arange(end - base)
            x = a[base:end].copy()
            tile_label = label[base:end]
            tile_skip = skip[base:end] & (local >= 2)  # (the tile's first two cells cannot see two to the left)
            for t in range(t_first, t_last + 1):
                x1 = np.concatenate((minus[:1], x[:-1]))
                x2 = np.where(tile_skip, np.concatenate((minus, x[:-2]))[:len(x)], NEG_INF)
                r = x
                m = np.zeros(len(x), np.int8)
                step = x1 > r
                r = np.where(step, x1, r)
                m[step] = 1
                jump = x2 > r
                r = np.where(jump, x2, r)
                m[jump] = 2
                x = r + lp[t, tile_label]
                assert x.dtype == np.float32
                move[t, own0:end] = m[own0 - base:]
            new[own0:end] = x[own0 - base:]
        a = new
    return a, move


def walk(a: np.ndarray, move: np.ndarray, y: List[int], blank: int) -> Tuple[int, Optional[np.ndarray]]:
    """The end-state rule and the walk of the contract on a sweep's result: (status, paths).  States are clamped at 0, as the
    kernels clamp them, so that a wrong sweep still yields a path to compare."""
    T, S = move.shape
    e = S - 1 if (S == 1 or a[S - 1] > a[S - 2]) else S - 2
    if a[e] == NEG_INF:
        return -1, None
    paths = np.zeros(T, np.int32)
    for t in range(T - 1, -1, -1):
        paths[t] = blank if e % 2 == 0 else y[e // 2]
        e = max(e - int(move[t, e]), 0)
    return 0, paths

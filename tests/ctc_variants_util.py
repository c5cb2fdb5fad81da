"""The one-edit-variant contract (include/allophant_amx_variants.h) as executable code, in float64 on the CPU: the lattice
with its two virtual frames and the bridging recursions, a class vector at a time (`variants_row`); and the brute force it
replaces, the forward-backward truth of tests/ctc_score_util.py on every explicitly edited sequence (`variants_brute`)."""
from typing import Iterable, NamedTuple, Optional, Sequence

import numpy as np

import ctc_score_util as U

NEG_INF = -np.inf


class VariantRow(NamedTuple):
    status: int
    ll: float                    # -inf with status -1
    sub: Optional[np.ndarray]    # float64 [L, C]; NaN rows where `slots` left them out
    ins: Optional[np.ndarray]    # float64 [L + 1, C]


def lattice(lp: np.ndarray, y: Sequence[int], blank: int):
    """a and b with their virtual frames: A[t + 1][i] = a[t][i] for t in [-1, T), B[t][i] = b[t][i] for t in [0, T]."""
    T, L = lp.shape[0], len(y)
    S = 2 * L + 1
    states = np.arange(S)
    labels = np.where(states % 2 == 0, blank, np.asarray(list(y) + [blank], np.int64)[states // 2])
    skip_from = np.zeros(S, bool)  # state i may be entered from i - 2
    skip_from[3:] = (states[3:] % 2 == 1) & (labels[3:] != labels[1:-2])
    A = np.full((T + 1, S), NEG_INF)
    A[0, 0] = 0.0
    B = np.full((T + 1, S), NEG_INF)
    B[T, S - 1] = 0.0
    x1, x2 = np.full(S, NEG_INF), np.full(S, NEG_INF)
    for t in range(T):
        prev = A[t]
        x1[1:] = prev[:-1]
        x2[2:] = np.where(skip_from[2:], prev[:-2], NEG_INF)
        A[t + 1] = np.logaddexp(np.logaddexp(prev, x1), x2) + lp[t, labels]
    x1[:], x2[:] = NEG_INF, NEG_INF
    for t in range(T - 1, -1, -1):
        nxt = B[t + 1]
        x1[:-1] = nxt[1:]
        x2[:-2] = np.where(skip_from[2:], nxt[2:], NEG_INF)
        B[t] = np.logaddexp(np.logaddexp(nxt, x1), x2) + lp[t, labels]
    return A, B


def _lse(*xs):
    out = xs[0]
    for x in xs[1:]:
        out = np.logaddexp(out, x)
    return out


def _substitution(lp, y, blank, A, B, l):
    T, C = lp.shape
    L = len(y)
    c = np.arange(C)
    a = lambda t, i: A[t + 1][i] if i >= 0 else NEG_INF            # noqa: E731
    b = lambda t, i: B[t][i] if i < 2 * L + 1 else NEG_INF         # noqa: E731
    from_left = (c != y[l - 1]) if l >= 1 else np.zeros(C, bool)
    to_right = (c != y[l + 1]) if l + 1 < L else np.zeros(C, bool)
    v, out = np.full(C, NEG_INF), np.full(C, NEG_INF)
    for t in range(T):
        v = _lse(v, a(t - 1, 2 * l), np.where(from_left, a(t - 1, 2 * l - 1), NEG_INF)) + lp[t]
        out = np.logaddexp(out, v + np.logaddexp(b(t + 1, 2 * l + 2), np.where(to_right, b(t + 1, 2 * l + 3), NEG_INF)))
    deleted = NEG_INF
    with_left = l >= 1 and (l + 1 == L or y[l - 1] != y[l + 1])
    for t in range(-1, T):
        x = b(t + 1, 2 * l + 3) if l + 1 < L else (0.0 if t + 1 == T else NEG_INF)
        deleted = np.logaddexp(deleted, np.logaddexp(a(t, 2 * l), a(t, 2 * l - 1) if with_left else NEG_INF) + x)
    out[blank] = deleted
    return out


def _insertion(lp, y, blank, A, B, p, ll):
    T, C = lp.shape
    L = len(y)
    c = np.arange(C)
    a = lambda t, i: A[t + 1][i] if i >= 0 else NEG_INF            # noqa: E731
    from_left = (c != y[p - 1]) if p >= 1 else np.zeros(C, bool)
    u, w, out = np.full(C, NEG_INF), np.full(C, NEG_INF), np.full(C, NEG_INF)
    for t in range(T):
        w = np.logaddexp(w, u) + lp[t, blank]  # (u is still u[t-1])
        u = _lse(u, a(t - 1, 2 * p), np.where(from_left, a(t - 1, 2 * p - 1), NEG_INF)) + lp[t]
        if p < L:
            out = np.logaddexp(out, np.logaddexp(w, np.where(c != y[p], u, NEG_INF)) + B[t + 1][2 * p + 1])
    if p == L and T > 0:
        out = np.logaddexp(u, w)
    out[blank] = ll
    return out


def variants_row(lp: np.ndarray, targets: Sequence[int], blank: int = 0, slots: Optional[Iterable[int]] = None) -> VariantRow:
    """One row: ``lp`` [T, C] (any float type, taken to float64), its targets and the blank.  ``slots`` limits the work to
    some slots (2l + 1: substitution row l, 2p: insertion row p); the other rows are NaN."""
    lp = np.asarray(lp, dtype=np.float64)
    T, C = lp.shape
    y = [int(v) for v in targets]
    if any(v < 0 or v >= C or v == blank for v in y):
        return VariantRow(-2, NEG_INF, None, None)
    L = len(y)
    if T == 0 and L > 0:
        return VariantRow(-1, NEG_INF, None, None)
    A, B = lattice(lp, y, blank)
    S = 2 * L + 1
    ll = float(np.logaddexp(A[T][S - 1], A[T][S - 2] if S > 1 else NEG_INF))
    sub, ins = np.full((L, C), np.nan), np.full((L + 1, C), np.nan)
    with np.errstate(invalid="ignore"):
        for slot in (range(S) if slots is None else slots):
            if slot & 1:
                sub[slot >> 1] = _substitution(lp, y, blank, A, B, slot >> 1)
            else:
                ins[slot >> 1] = _insertion(lp, y, blank, A, B, slot >> 1, ll)
    return VariantRow(0, ll, sub, ins)


def _ll(lp, y, blank):
    return U.score_row(lp, y, blank, posteriors=False).ll


def variants_brute(lp: np.ndarray, targets: Sequence[int], blank: int = 0) -> VariantRow:
    """The same cells by brute force: the float64 forward-backward truth of every explicitly edited sequence."""
    lp = np.asarray(lp, dtype=np.float64)
    T, C = lp.shape
    y = [int(v) for v in targets]
    L = len(y)
    ll = _ll(lp, y, blank)
    sub, ins = np.full((L, C), NEG_INF), np.full((L + 1, C), NEG_INF)
    for l in range(L):
        for c in range(C):
            sub[l, c] = _ll(lp, y[:l] + y[l + 1:], blank) if c == blank else _ll(lp, y[:l] + [c] + y[l + 1:], blank)
    for p in range(L + 1):
        for c in range(C):
            ins[p, c] = ll if c == blank else _ll(lp, y[:p] + [c] + y[p:], blank)
    return VariantRow(0, ll, sub, ins)

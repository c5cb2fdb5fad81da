"""The CTC forward-backward contract (include/allophant_amx_score.h) as executable code, in float64 on the CPU: a, b, ll, g
and the three per-target sums, a frame at a time over all states; the pool of rows and the fp32 torch yardsticks the device
is held to; and the bounds."""
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

NEG_INF = -np.inf


class Row(NamedTuple):
    status: int
    ll: float                              # -inf with status -1
    occupancy: Optional[np.ndarray]        # float64 [L]
    position_sums: Optional[np.ndarray]    # float64 [L]
    score_sums: Optional[np.ndarray]       # float64 [L]
    g: Optional[np.ndarray]                # float64 [T, S], when asked for
    labels: Optional[np.ndarray]           # int64 [S]


def _refused(status: int) -> Row:
    return Row(status, NEG_INF, None, None, None, None, None)


def _lse3(x0, x1, x2):
    """-inf where all three are -inf (np.logaddexp(-inf, -inf) is -inf, without a warning or a NaN)."""
    return np.logaddexp(np.logaddexp(x0, x1), x2)


def score_row(lp: np.ndarray, targets: Sequence[int], blank: int = 0, posteriors: bool = True) -> Row:
    """One row: ``lp`` [T, C] (any float type, taken to float64), its targets and the blank."""
    lp = np.asarray(lp, dtype=np.float64)
    T, C = lp.shape
    y = [int(v) for v in targets]
    if any(v < 0 or v >= C or v == blank for v in y):
        return _refused(-2)
    L = len(y)
    S = 2 * L + 1
    if T == 0:
        return Row(0, 0.0, np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 1)) if posteriors else None, np.array([blank])) \
            if L == 0 else _refused(-1)
    states = np.arange(S)
    padded = np.asarray(y + [blank], np.int64)  # (the extra entry keeps the even states' lookup in range)
    labels = np.where(states % 2 == 0, blank, padded[states // 2])
    odd = states % 2 == 1
    skip_from = np.zeros(S, bool)  # state i may be entered from i - 2
    skip_from[3:] = odd[3:] & (labels[3:] != labels[1:-2])
    skip_to = np.zeros(S, bool)    # state i may step to i + 2
    skip_to[:-2] = skip_from[2:]

    a = np.full((T, S), NEG_INF)
    a[0, 0] = lp[0, blank]
    if S > 1:
        a[0, 1] = lp[0, y[0]]
    x1, x2 = np.full(S, NEG_INF), np.full(S, NEG_INF)
    for t in range(1, T):
        prev = a[t - 1]
        x1[1:] = prev[:-1]
        x2[2:] = np.where(skip_from[2:], prev[:-2], NEG_INF)
        a[t] = _lse3(prev, x1, x2) + lp[t, labels]
    ll = float(np.logaddexp(a[T - 1, S - 1], a[T - 1, S - 2] if S > 1 else NEG_INF))
    if ll == NEG_INF:
        return _refused(-1)

    g_all = np.zeros((T, S)) if posteriors else None
    occupancy, position_sums, score_sums = np.zeros(S), np.zeros(S), np.zeros(S)
    e = lp[T - 1, labels]
    b = np.full(S, NEG_INF)
    b[S - 1] = e[S - 1]
    if S > 1:
        b[S - 2] = e[S - 2]
    x1[:], x2[:] = NEG_INF, NEG_INF
    for t in range(T - 1, -1, -1):
        if t < T - 1:
            e = lp[t, labels]
            x1[:-1] = b[1:]
            x2[:-2] = np.where(skip_to[:-2], b[2:], NEG_INF)
            b = _lse3(b, x1, x2) + e
        reachable = (a[t] > NEG_INF) & (b > NEG_INF)
        with np.errstate(invalid="ignore"):
            g = np.where(reachable, np.exp(a[t] + b - e - ll), 0.0)
            weighted = np.where(g != 0.0, g * e, 0.0)
        occupancy += g
        position_sums += t * g
        score_sums += weighted
        if posteriors:
            g_all[t] = g
    return Row(0, ll, occupancy[1::2].copy(), position_sums[1::2].copy(), score_sums[1::2].copy(), g_all, labels)


def class_occupancy(row: Row, C: int) -> np.ndarray:
    """g summed over the states of each class: float64 [T, C]."""
    out = np.zeros((row.g.shape[0], C))
    for c in np.unique(row.labels):
        out[:, c] = row.g[:, row.labels == c].sum(axis=1)
    return out


def score_batch(emissions: np.ndarray, lengths: Sequence[int], offsets: Sequence[int], ids: Sequence[int], max_target: int,
                blank: int = 0, candidates: int = 1, posteriors: bool = True) -> List[Row]:
    """The batch form of the C ABI: row r scores utterance r // candidates; malformed rows are refused with -2."""
    N, T, _ = emissions.shape
    rows = []
    for r in range(N * candidates):
        n = r // candidates
        lb, le, k = int(offsets[r]), int(offsets[r + 1]), int(lengths[n])
        if k < 0 or k > T or lb < 0 or le < lb or le > int(offsets[N * candidates]) or le - lb > max_target:
            rows.append(_refused(-2))
        else:
            rows.append(score_row(emissions[n, :k], list(ids[lb:le]), blank, posteriors))
    return rows


def minimum_frames(targets: Sequence[int]) -> int:
    """Targets plus one blank per adjacent repeat."""
    return len(targets) + sum(1 for i in range(1, len(targets)) if targets[i] == targets[i - 1])


# ---------------------------------------------------------------------------------------------------------------------------
# the pool and the yardsticks
# ---------------------------------------------------------------------------------------------------------------------------
class PoolRow(NamedTuple):
    lp: torch.Tensor        # fp32 [T, C]
    targets: List[int]
    truth: Row


def _targets(rng, L: int, C: int, repeat: float) -> List[int]:
    out: List[int] = []
    for _ in range(L):
        if out and (C == 2 or rng.random() < repeat):
            out.append(out[-1])
        else:
            out.append(int(rng.choice([c for c in range(1, C) if not out or c != out[-1]])))
    return out


def _peaky(rng, T: int, C: int) -> torch.Tensor:
    """Peaky rows: a sticky walk over the classes (like the one of oracle/gen_golden.py's G4c), its class 6 to 9 nats up."""
    logits = rng.standard_normal((T, C))
    c = int(rng.integers(0, C))
    for t in range(T):
        if rng.random() < 0.3:
            c = int(rng.integers(0, C))
        logits[t, c] += rng.uniform(6.0, 9.0)
    return torch.log_softmax(torch.from_numpy(logits).float(), -1)


def make_pool(count: int = 208, seed: int = 20260) -> List[PoolRow]:
    """Fixed-seed rows: T from 1 to 500, L from 0 to 100, C in {2, 5, 37, 201}, repeated neighbours, flat and peaky
    emissions; feasible and infeasible rows alike, each with its float64 truth."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    pool = []
    for k in range(count):
        C = (2, 5, 37, 201)[k % 4]
        if k < 8:  # the corners
            T, L = ((1, 0), (1, 1), (500, 100), (500, 0), (2, 1), (3, 2), (500, 1), (201, 100))[k]
        else:
            T = int(rng.integers(1, 501))
            L = int(rng.integers(0, min(100, T) + 1))
        y = _targets(rng, L, C, repeat=0.25 if k % 3 else 0.0)
        if (k // 4) % 2:
            lp = _peaky(rng, T, C)
        else:
            lp = torch.log_softmax(torch.randn(T, C, generator=g) * (1.0 + (k % 5)), -1)
        pool.append(PoolRow(lp, y, score_row(lp.numpy(), y)))
    return pool


def torch_loss_and_grad(lp: torch.Tensor, targets: Sequence[int], dtype=torch.float32):
    """torch's CPU ``ctc_loss`` (reduction none, blank 0) of one row and its gradient with respect to the log-probabilities,
    which equals exp(lp) minus the per-class occupancy."""
    x = lp.to(dtype).unsqueeze(1).clone().requires_grad_(True)  # [T, 1, C]
    loss = F.ctc_loss(x, torch.tensor([list(targets)], dtype=torch.long), torch.tensor([lp.shape[0]]), torch.tensor([len(targets)]),
                      blank=0, reduction="none", zero_infinity=False)
    grad, = torch.autograd.grad(loss.sum(), x)
    return float(loss.detach()[0]), grad[:, 0]


class Yardsticks(NamedTuple):
    E_ll: float
    E_post: float


def scale(ll: float) -> float:
    return max(1.0, abs(ll))


def yardsticks(pool: Sequence[PoolRow]) -> Yardsticks:
    """The error of torch's own fp32 CPU kernel against the float64 truth on the pool's feasible rows, relative to
    max(1, |ll|): of the log-likelihood, and of the class occupancy exp(lp) - grad, the maximum over frames and classes."""
    E_ll = E_post = 0.0
    for row in pool:
        if row.truth.status != 0:
            continue
        loss, grad = torch_loss_and_grad(row.lp, row.targets)
        E_ll = max(E_ll, abs(-loss - row.truth.ll) / scale(row.truth.ll))
        occupancy = (row.lp.double().exp() - grad.double()).numpy()
        E_post = max(E_post, float(np.abs(occupancy - class_occupancy(row.truth, row.lp.shape[1])).max()) / scale(row.truth.ll))
    return Yardsticks(E_ll, E_post)


MARGIN = 4.0  # the device runs the same recursion at the same depth in the same precision; it may group the 3-way sum and round
#               exp / log differently, each a small factor per step


def ll_bound(y: Yardsticks, ll: float) -> float:
    return MARGIN * y.E_ll * scale(ll)


def g_bound(y: Yardsticks, ll: float) -> float:
    return MARGIN * y.E_post * scale(ll)


def sum_bound(y: Yardsticks, ll: float, frames: int, value: np.ndarray) -> np.ndarray:
    """Per-target sums: the posterior bound plus the sequential fp32 summation bound of `frames` terms, relative to
    max(1, |x|)."""
    return (g_bound(y, ll) + (frames - 1) * 2.0 ** -24) * np.maximum(1.0, np.abs(value))

"""The six row entries of the edit family on a workspace of exactly the size that amx_edit_workspace /
amx_edit_operations_workspace report, with guard bytes on both sides inside one allocation: a launcher whose offsets disagree
with the reported size changes a guard byte (or an output).  The lengths are those at which the padding to 16 and the number
of 64-symbol strips of path codes change.  Outputs against the restatements of tests/edit_util.py, edit_ops_util.py,
edit_weighted_util.py and confusion_util.py; everything is an exact integer or compared as bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import confusion_util as CU
import edit_ops_util as U
import edit_util as E
import edit_weighted_util as W

pytestmark = pytest.mark.gpu

CASES = [(0, 1), (1, 0), (15, 16), (16, 17), (64, 15), (65, 1), (17, 65)]  # (max_expected, max_actual)
ALPHABET = 4
GUARD, FILL = 256, 0xA5
COSTS = (0.3, 0.7)
TABLE = {0: [0, 1, 0], 1: [1, 1, 0], 2: [0, 1, 0], 3: [1, 0, 1]}  # 0 and 2: different symbols, equal rows
BEST = [1, 0, 1]  # the candidates that the confusion calls walk


@pytest.fixture(scope="module")
def ev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import evaluation, lib

    assert lib.load() is not None
    return evaluation


def _sequences(rng, max_expected, max_actual):
    """Three rows of two candidates: both limits are reached, by candidate 0 (the operations calls take it alone) and by
    candidate 1."""
    lengths = [(max_expected, (max_actual // 2, max_actual)), (max_expected // 2, (max_actual, max(max_actual - 1, 0))),
               (min(max_expected, 1), (min(max_actual, 2), 0))]
    draw = lambda n: rng.integers(0, ALPHABET, n).tolist()  # noqa: E731
    return [draw(m) for m, _ in lengths], [[draw(n) for n in ns] for _, ns in lengths]


def _rows(ev, expected, candidates, max_expected, max_actual):
    """The pairs as one output in one group with the identity as both maps, symbols as their own ids."""
    device = torch.device("cuda", 0)
    N, K, T = len(expected), len(candidates[0]), max(1, max_actual)
    offsets = np.zeros(N + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(e) for e in expected])
    block = np.concatenate([offsets, np.zeros(N, dtype=np.int32), np.asarray([s for e in expected for s in e], dtype=np.int32)])
    tokens = np.zeros((1, N, K, T), dtype=np.int64)
    for n, row in enumerate(candidates):
        for k, actual in enumerate(row):
            tokens[0, n, k, :len(actual)] = actual
    counts = np.asarray([[len(actual) for actual in row] for row in candidates], dtype=np.int32).reshape(1, N, K)
    identity = np.concatenate([np.arange(ALPHABET + 1, dtype=np.int32), np.arange(ALPHABET, dtype=np.int32)])
    descriptor = torch.tensor([0, ALPHABET], dtype=torch.int32, device=device)
    up = lambda array: torch.from_numpy(array).to(device)  # noqa: E731
    return ev._EditRows(up(tokens), up(counts), None, up(block), N, 1, up(identity), ALPHABET + 1, descriptor, descriptor, 1,
                        max_expected, max_actual)


class _Guarded:
    """A workspace of exactly the reported size between two guard regions of one allocation."""

    def __init__(self, ev, codes, rows, max_expected, max_actual):
        handle, size = ev._library(), C.c_size_t()
        report = handle.amx_edit_operations_workspace if codes else handle.amx_edit_workspace
        assert report(rows, max_expected, max_actual, C.byref(size)) == 0 and size.value > 0
        self.buffer = torch.full((GUARD + size.value + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.workspace = self.buffer[GUARD:GUARD + size.value]

    def check(self, used, what):
        torch.cuda.synchronize()
        assert used.data_ptr() == self.workspace.data_ptr() and used.numel() == self.workspace.numel(), what
        assert bool((self.buffer[:GUARD] == FILL).all()), f"{what}: bytes before the workspace changed"
        assert bool((self.buffer[GUARD + self.workspace.numel():] == FILL).all()), f"{what}: bytes after the workspace changed"


def _bits(x) -> bytes:
    return np.asarray(x, dtype=np.float32).tobytes()


def _chosen(statistics):
    """run.py:447-464 on a row's statistics: the first candidate whose rate is strictly below the best so far, or -1."""
    lowest, best = np.inf, -1
    for k, stats in enumerate(statistics):
        rate = E.word_error_rate(stats)
        if rate < lowest:
            lowest, best = rate, k
    return best


def _table_of(found):
    out = {}
    for g, o, e, a, c in found.entries():
        out[(g, o, CU.EPSILON if e < 0 else found.symbols[o][e], CU.EPSILON if a < 0 else found.symbols[o][a])] = c
    return out


@pytest.mark.parametrize("max_expected,max_actual", CASES)
def test_exact_workspaces(ev, max_expected, max_actual):
    from allophant_amd.confusion import ConfusionCounts

    rng = np.random.default_rng(1000 * max_expected + max_actual)
    expected, candidates = _sequences(rng, max_expected, max_actual)
    assert max(map(len, expected)) == max_expected and max(len(a) for row in candidates for a in row) == max_actual
    assert max(len(row[0]) for row in candidates) == max_actual
    rows = _rows(ev, expected, candidates, max_expected, max_actual)
    device = rows.tokens.device
    N, K = len(expected), 2
    weighting = ev.PropertyWeighting(*COSTS, TABLE)
    weights = ev._Weights(weighting.insertion_cost, weighting.deletion_cost, torch.tensor([[0, ALPHABET]], dtype=torch.int64, device=device),
                          weighting.cost_table(list(range(ALPHABET)), device))
    uniform = [[(U.levensthein_operations_fast(e, a), E.levensthein_statistics_fast(e, a)) for a in row]
               for e, row in zip(expected, candidates)]
    weighted = [[W.operations_fast(e, a, *COSTS, TABLE) for a in row] for e, row in zip(expected, candidates)]

    # statistics, K = 2
    for what, w in (("amx_edit_statistics", None), ("amx_edit_weighted_statistics", weights)):
        guarded = _Guarded(ev, False, N * K, max_expected, max_actual)
        totals = torch.zeros(1, 1, 4, dtype=torch.int64, device=device)
        statistics, best, used, costs = ev._run(rows, guarded.workspace, totals, w)  # (raises unless the call returned AMX_OK)
        guarded.check(used, what)
        if w is None:
            want = [[stats for _, stats in row] for row in uniform]
        else:
            want = [[stats for _, _, stats in row] for row in weighted]
            assert [[_bits(c) for c in row] for row in costs[0].cpu().tolist()] == [[_bits(cost) for _, cost, _ in row] for row in weighted]
        assert [[tuple(s) for s in row] for row in statistics[0].cpu().tolist()] == want, what
        chosen = [_chosen(row) for row in want]
        assert best[0].cpu().tolist() == chosen, what
        total = np.sum([row[k] for row, k in zip(want, chosen) if k >= 0], axis=0, dtype=np.int64)
        assert totals.reshape(4).cpu().tolist() == (total.tolist() if np.ndim(total) else [0, 0, 0, 0]), what

    # operations, candidate 0
    for what, w in (("amx_edit_operations", None), ("amx_edit_weighted_operations", weights)):
        guarded = _Guarded(ev, True, N, max_expected, max_actual)
        operations, counts, used, costs = ev._run_operations(rows.first(), guarded.workspace, w)
        guarded.check(used, what)
        records, lengths = operations[0].cpu().numpy(), counts[0].cpu().tolist()
        for n in range(N):
            if w is None:
                want_operations, want_cost = uniform[n][0][0]
                assert lengths[n] == want_cost, (what, n)
            else:
                want_operations, want_cost, _ = weighted[n][0]
                assert lengths[n] == len(want_operations) and _bits(costs[0, n].item()) == _bits(want_cost), (what, n)
            assert [tuple(r) for r in records[n, :lengths[n], :3].tolist()] == [tuple(int(v) for v in op) for op in want_operations], (what, n)

    # confusions, K = 2, the candidates of BEST
    best = torch.tensor([BEST], dtype=torch.int32, device=device)
    for what, w in (("amx_edit_confusions", None), ("amx_edit_weighted_confusions", weights)):
        guarded = _Guarded(ev, True, N, max_expected, max_actual)
        accumulator = ConfusionCounts(device, 4096, ["total"], ["pairs"], [list(range(ALPHABET))])
        accumulator._workspace = guarded.workspace
        row_events = accumulator.add_rows(rows, best, w)
        guarded.check(accumulator._workspace, what)
        if w is None:
            want = [CU.events(e, row[k], fast=True) for e, row, k in zip(expected, candidates, BEST)]
        else:
            want = [CU.weighted_events(e, row[k], *COSTS, TABLE, fast=True) for e, row, k in zip(expected, candidates, BEST)]
        assert row_events[0].cpu().tolist() == [CU.event_count(f) for f in want], what
        assert accumulator.events() == (sum(CU.event_count(f) for f in want), 0), what
        assert _table_of(accumulator.fetch()) == CU.table_of((0, 0, f) for f in want), what

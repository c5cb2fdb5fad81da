"""Python restatement of the confusion-table contract (test infrastructure), from upstream's own outputs: the events of a
row are what ``levensthein_operations`` records (tests/edit_ops_util.py; tests/edit_weighted_util.py for the weighted costs)
plus its matches, which no record names -- the expected and actual positions left over, paired in order.  An event is
``(expected symbol, actual symbol)`` with ``EPSILON`` for the missing side of a deletion or insertion.

Also the form the kernels compute (``walk_confusions`` of amx_edit_dp.inc): the walk over the sweep's path codes with every
move an event, ended after S + D + I operations, then the all-match tail (A[q], B[q]), q < i."""
from collections import Counter
from typing import Dict, Hashable, Iterable, Sequence, Tuple

import edit_ops_util as U
import edit_weighted_util as W

EPSILON = None
Event = Tuple[Hashable, Hashable]


def events_of(a: Sequence, b: Sequence, operations: Iterable[Tuple[int, int, int]]) -> Counter:
    """The multiset of events of one row from upstream's records (action, i, j)."""
    operations = list(operations)
    out: Counter = Counter()
    named_a, named_b = set(), set()
    for action, i, j in operations:
        if action == U.DELETION:
            out[(a[i], EPSILON)] += 1
            named_a.add(i)
        elif action == U.INSERTION:
            out[(EPSILON, b[j])] += 1
            named_b.add(j)
        else:
            assert action == U.SUBSTITUTION
            out[(a[i], b[j])] += 1
            named_a.add(i)
            named_b.add(j)
    left_a = [i for i in range(len(a)) if i not in named_a]
    left_b = [j for j in range(len(b)) if j not in named_b]
    assert len(left_a) == len(left_b)
    for i, j in zip(left_a, left_b):  # the matches: a monotone path pairs them in order
        out[(a[i], b[j])] += 1
    return out


def events(a: Sequence, b: Sequence, fast: bool = False) -> Counter:
    """Uniform costs."""
    operations, _ = (U.levensthein_operations_fast if fast else U.levensthein_operations)(a, b)
    return events_of(a, b, operations)


def weighted_events(a: Sequence, b: Sequence, insertion_cost, deletion_cost, table, fast: bool = False) -> Counter:
    if fast:
        operations = W.operations_fast(a, b, insertion_cost, deletion_cost, table)[0]
    else:
        operations = W.levensthein_operations(a, b, insertion_cost, deletion_cost, table)[0]
    return events_of(a, b, operations)


def statistics(found: Counter, zero_cost=None) -> Tuple[int, int, int, int]:
    """(I, D, S, C) implied by a row's events; ``zero_cost(e, a)`` says which pairs are matches (default: equal symbols)."""
    zero_cost = zero_cost or (lambda e, a: e == a)
    ins = dels = subs = correct = 0
    for (e, a), count in found.items():
        if e is EPSILON:
            ins += count
        elif a is EPSILON:
            dels += count
        elif zero_cost(e, a):
            correct += count
        else:
            subs += count
    return ins, dels, subs, correct


def event_count(found: Counter) -> int:
    return sum(found.values())


def kernel_form(a: Sequence, b: Sequence, insertion_cost=1.0, deletion_cost=1.0, table=None) -> Tuple[Counter, int]:
    """What the confusion kernels compute: (events, their number).  A row with an empty side is pure deletions or
    insertions; otherwise the walk follows the sweep's (diagonal, second) codes from (m, n), every move an event, until
    count = S + D + I operations are seen, and the rest is the tail (a[q], b[q]), q < i."""
    m, n = len(a), len(b)
    out: Counter = Counter()
    if m == 0 or n == 0:
        for x in a:
            out[(x, EPSILON)] += 1
        for y in b:
            out[(EPSILON, y)] += 1
        return out, m + n
    _, S, D, diagonal, second = W.sweep(a, b, insertion_cost, deletion_cost, table)
    s, d = int(S[m, n]), int(D[m, n])
    count = n - m + 2 * d + s
    i, j, k, moves = m, n, 0, 0
    while k < count and (i > 0 or j > 0):
        if i == 0:
            act, j = U.INSERTION, j - 1
        elif j == 0:
            act, i = U.DELETION, i - 1
        elif diagonal[i, j]:
            act = U.SUBSTITUTION if second[i, j] else 0
            i, j = i - 1, j - 1
        elif second[i, j]:
            act, i = U.DELETION, i - 1
        else:
            act, j = U.INSERTION, j - 1
        out[(a[i] if act != U.INSERTION else EPSILON, b[j] if act != U.DELETION else EPSILON)] += 1
        moves += 1
        k += act != 0
    assert i == j
    for q in range(i):
        out[(a[q], b[q])] += 1
    return out, moves + i


def table_of(rows: Iterable[Tuple[int, int, Counter]]) -> Dict[Tuple[int, int, Hashable, Hashable], int]:
    """(group, output, row events) of the contributing rows -> {(group, output, expected, actual): count}."""
    out: Counter = Counter()
    for g, o, found in rows:
        for (e, a), count in found.items():
            out[(g, o, e, a)] += count
    return dict(out)

"""Literal Python restatement of upstream's ``PropertyWeighting`` (test infrastructure): ``levensthein_matrix_general`` /
``levensthein_operations_general`` / ``levensthein_statistics_general`` under ``PropertyWeighting.cost_function``
(edit_distance.rs:116-260, 372-481, 498-599) in ``np.float32``, and the module-level ``levensthein_matrix`` (unit costs,
``a != b``).  Read from the source, not run against it.

Also the forms the kernels compute (amx_edit_weighted.hip): the matrix filled by anti-diagonals (each cell the same additions
and minima, so the same bits), the forward-carried statistics, and the path codes with a walk that stops after S + D + I
records and writes record k at index count - 1 - k.

``table`` is anything with ``__getitem__`` from a symbol to a 1-D row; ``None`` stands for no table (``a != b``)."""
from typing import List, Optional, Sequence, Tuple

import numpy as np

INSERTION, DELETION, SUBSTITUTION = 1, 2, 3
Operation = Tuple[int, int, int]
Stats = Tuple[int, int, int, int]  # insertions, deletions, substitutions, correct
F32 = np.float32


def substitution_cost(table, x, y) -> np.float32:
    """``table[x].ne(table[y]).sum()`` as f32; without a table ``x != y``."""
    if table is None:
        return F32(1.0 if x != y else 0.0)
    return F32(int(np.sum(np.asarray(table[x]) != np.asarray(table[y]))))


def levensthein_matrix_weighted(a: Sequence, b: Sequence, insertion_cost, deletion_cost, table) -> np.ndarray:
    """levensthein_matrix_general with PropertyWeighting.cost_function, cell by cell."""
    insertion_cost, deletion_cost = F32(insertion_cost), F32(deletion_cost)
    m, n = len(a), len(b)
    matrix = [[F32(j) for j in range(n + 1)]]
    for i in range(m):
        previous_row = matrix[i]
        current_row = list(previous_row)
        current_row[0] = F32(current_row[0] + deletion_cost)
        for j in range(n):
            insertion = F32(current_row[j] + insertion_cost)
            deletion = F32(previous_row[j + 1] + deletion_cost)
            substitution = F32(previous_row[j] + substitution_cost(table, a[i], b[j]))
            current_row[j + 1] = min(min(insertion, deletion), substitution)
        matrix.append(current_row)
    return np.asarray(matrix, dtype=np.float32).reshape(m + 1, n + 1)


def levensthein_matrix(a: Sequence, b: Sequence) -> np.ndarray:
    """Upstream's module-level levensthein_matrix: deletion_cost 1 and uniform_costs."""
    return levensthein_matrix_weighted(a, b, 1.0, 1.0, None)


def walk(matrix, m: int, n: int) -> Tuple[List[Operation], np.float32, Stats]:
    """The back-trace shared by levensthein_operations_general and levensthein_statistics_general: the reversed operations,
    the final cost and the statistics of the same path."""
    best_path = []
    final_cost = matrix[m][n]
    current_cost = final_cost
    i, j = m, n
    ins = dels = subs = correct = 0
    while current_cost != 0.0:
        if i == 0:
            if j == 0:
                break
            operation, cost = INSERTION, matrix[i][j - 1]
        elif j == 0:
            operation, cost = DELETION, matrix[i - 1][j]
        else:
            deletion, insertion, substitution = matrix[i - 1][j], matrix[i][j - 1], matrix[i - 1][j - 1]
            operation, cost = (DELETION, deletion) if deletion < insertion else (INSERTION, insertion)
            if substitution <= cost:
                operation = None if substitution == current_cost else SUBSTITUTION
                cost = substitution
        current_cost = cost
        if operation is None:
            i, j, correct = i - 1, j - 1, correct + 1
        elif operation == SUBSTITUTION:
            i, j, subs = i - 1, j - 1, subs + 1
        elif operation == DELETION:
            i, dels = i - 1, dels + 1
        else:
            j, ins = j - 1, ins + 1
        if operation is not None:
            best_path.append((operation, i, j))
    correct += i
    best_path.reverse()
    return best_path, F32(final_cost), (ins, dels, subs, correct)


def levensthein_operations(a, b, insertion_cost, deletion_cost, table) -> Tuple[List[Operation], np.float32]:
    return walk(levensthein_matrix_weighted(a, b, insertion_cost, deletion_cost, table), len(a), len(b))[:2]


def levensthein_statistics(a, b, insertion_cost, deletion_cost, table) -> Stats:
    return walk(levensthein_matrix_weighted(a, b, insertion_cost, deletion_cost, table), len(a), len(b))[2]


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels' forms

def pair_costs(a: Sequence, b: Sequence, table) -> np.ndarray:
    """d(a_i, b_j) for every cell, float32 [m, n]."""
    m, n = len(a), len(b)
    if m == 0 or n == 0:
        return np.zeros((m, n), dtype=np.float32)
    if table is None:
        symbols = {s: k for k, s in enumerate(dict.fromkeys(list(a) + list(b)))}
        ia = np.asarray([symbols[s] for s in a])
        ib = np.asarray([symbols[s] for s in b])
        return (ia[:, None] != ib[None, :]).astype(np.float32)
    symbols = list(dict.fromkeys(list(a) + list(b)))
    index = {s: k for k, s in enumerate(symbols)}
    rows = np.stack([np.asarray(table[s]).reshape(-1) for s in symbols])
    pairwise = (rows[:, None, :] != rows[None, :, :]).sum(axis=2).astype(np.float32)
    return pairwise[np.asarray([index[s] for s in a])][:, np.asarray([index[s] for s in b])]


def sweep(a: Sequence, b: Sequence, insertion_cost, deletion_cost, table):
    """The wavefront sweep, one anti-diagonal at a time.  Returns (matrix f32 [m + 1, n + 1], S, D int [m + 1, n + 1] of the
    walk that starts at each cell, and the path codes diagonal / second bool [m + 1, n + 1])."""
    insertion_cost, deletion_cost = F32(insertion_cost), F32(deletion_cost)
    m, n = len(a), len(b)
    d = pair_costs(a, b, table)
    M = np.zeros((m + 1, n + 1), dtype=np.float32)
    S = np.zeros((m + 1, n + 1), dtype=np.int64)
    D = np.zeros((m + 1, n + 1), dtype=np.int64)
    diagonal = np.zeros((m + 1, n + 1), dtype=bool)
    second = np.zeros((m + 1, n + 1), dtype=bool)
    M[0] = np.arange(n + 1, dtype=np.float32)
    column = F32(0.0)
    for i in range(1, m + 1):  # repeated addition, rounded each time
        column = F32(column + deletion_cost)
        M[i, 0] = column
        D[i, 0] = i
    for t in range(2, m + n + 1):
        i = np.arange(max(1, t - n), min(m, t - 1) + 1)
        j = t - i
        up, left, dg = M[i - 1, j], M[i, j - 1], M[i - 1, j - 1]
        chosen = np.minimum(up, left)  # deletion if strictly cheaper, else insertion
        cost = np.minimum(np.minimum(left + insertion_cost, up + deletion_cost), dg + d[i - 1, j - 1])
        assert cost.dtype == np.float32
        deletion = up < left
        s = np.where(deletion, S[i - 1, j], S[i, j - 1])
        dd = np.where(deletion, D[i - 1, j] + 1, D[i, j - 1])
        is_diagonal = dg <= chosen
        s = np.where(is_diagonal, S[i - 1, j - 1] + (dg != cost), s)
        dd = np.where(is_diagonal, D[i - 1, j - 1], dd)
        stop = cost == 0  # the walk stops here: everything above is correct
        M[i, j] = cost
        S[i, j] = np.where(stop, 0, s)
        D[i, j] = np.where(stop, 0, dd)
        diagonal[i, j] = is_diagonal
        second[i, j] = np.where(is_diagonal, dg != cost, deletion)
    return M, S, D, diagonal, second


def matrix_fast(a, b, insertion_cost, deletion_cost, table) -> np.ndarray:
    """The sweep's matrix alone (the same additions and minima per cell): for the long pairs of the GPU tests."""
    insertion_cost, deletion_cost = F32(insertion_cost), F32(deletion_cost)
    m, n = len(a), len(b)
    d = pair_costs(a, b, table)
    M = np.zeros((m + 1, n + 1), dtype=np.float32)
    M[0] = np.arange(n + 1, dtype=np.float32)
    column = F32(0.0)
    for i in range(1, m + 1):
        column = F32(column + deletion_cost)
        M[i, 0] = column
    for t in range(2, m + n + 1):
        i = np.arange(max(1, t - n), min(m, t - 1) + 1)
        j = t - i
        M[i, j] = np.minimum(np.minimum(M[i, j - 1] + insertion_cost, M[i - 1, j] + deletion_cost), M[i - 1, j - 1] + d[i - 1, j - 1])
    return M


def carried_statistics(a, b, insertion_cost, deletion_cost, table) -> Tuple[Stats, np.float32]:
    """The statistics kernel's form: (S, D) of cell (m, n), then C = m - S - D and I = n - C - S; and the cost."""
    m, n = len(a), len(b)
    M, S, D, _, _ = sweep(a, b, insertion_cost, deletion_cost, table)
    s, d = int(S[m, n]), int(D[m, n])
    c = m - s - d
    return (n - c - s, d, s, c), F32(M[m, n])


def kernel_form(a, b, insertion_cost, deletion_cost, table) -> Tuple[List[Optional[Operation]], np.float32, Stats]:
    """The operations kernel's form: the sweep records (diagonal, second) per cell, the walk from (m, n) follows the codes
    (i == 0 inserts, j == 0 deletes), stops after count = S + D + I records and writes record k at index count - 1 - k."""
    m, n = len(a), len(b)
    M, S, D, diagonal, second = sweep(a, b, insertion_cost, deletion_cost, table)
    s, d = int(S[m, n]), int(D[m, n])
    c = m - s - d
    ins = n - c - s
    count = s + d + ins
    operations: List[Optional[Operation]] = [None] * count
    i, j, k = m, n, 0
    while k < count and (i > 0 or j > 0):
        if i == 0:
            act, j = INSERTION, j - 1
        elif j == 0:
            act, i = DELETION, i - 1
        elif diagonal[i, j]:
            act = SUBSTITUTION if second[i, j] else 0
            i, j = i - 1, j - 1
        elif second[i, j]:
            act, i = DELETION, i - 1
        else:
            act, j = INSERTION, j - 1
        if act:
            operations[count - 1 - k] = (act, i, j)
            k += 1
    return operations, F32(M[m, n]), (ins, d, s, c)


def operations_fast(a, b, insertion_cost, deletion_cost, table) -> Tuple[List[Operation], np.float32, Stats]:
    """The literal walk on the anti-diagonal matrix: for the long pairs of the GPU tests."""
    return walk(matrix_fast(a, b, insertion_cost, deletion_cost, table), len(a), len(b))


def canonical_codes(rows: np.ndarray) -> np.ndarray:
    """Per column, the values numbered in order of first appearance: what the binding hands to the kernels."""
    rows = np.asarray(rows)
    codes = np.zeros(rows.shape, dtype=np.uint8)
    for f in range(rows.shape[1]):
        seen = {}
        for v, value in enumerate(rows[:, f].tolist()):
            codes[v, f] = seen.setdefault(value, len(seen))
    return codes

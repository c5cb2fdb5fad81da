"""Literal Python restatement of upstream's ``edits`` (test infrastructure): ``levensthein_operations_general`` with uniform
costs (edit_distance.rs:122-202: the full matrix, then the first best path walked back from (m, n) and reversed),
``to_substitutions`` (:105-119), ``predictions.levensthein_substitutions`` and run.py's ``_compute_edits`` (:502-521) on
strings, with ``UtteranceEdits`` in mashumaro's dict shape.  Also the form the kernel computes (amx_edit_ops.hip): per
(strip, step) two 64-bit masks of move codes, and a walk through 64-word windows that stops after ``cost`` operations and
writes operation k at index cost - 1 - k."""
import json
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import edit_util as E

INSERTION, DELETION, SUBSTITUTION = 1, 2, 3
Operation = Tuple[int, int, int]


def _walk(matrix, m: int, n: int) -> Tuple[List[Operation], float]:
    """The back-trace of levensthein_operations_general, on any matrix indexable as matrix[i][j]."""
    best_path = []
    final_cost = float(matrix[m][n])
    current_cost = final_cost
    i, j = m, n
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
        current_cost = float(cost)
        if operation is None or operation == SUBSTITUTION:
            i, j = i - 1, j - 1
        elif operation == DELETION:
            i -= 1
        else:
            j -= 1
        if operation is not None:
            best_path.append((operation, i, j))
    best_path.reverse()
    return best_path, final_cost


def levensthein_operations(a: Sequence, b: Sequence) -> Tuple[List[Operation], float]:
    """``string_a`` = expected, ``string_b`` = actual; the matrix of levensthein_operations_general with uniform_costs."""
    m, n = len(a), len(b)
    matrix = [[float(j) for j in range(n + 1)]]
    for i in range(m):
        previous_row = matrix[i]
        current_row = list(previous_row)
        current_row[0] += 1.0
        for j in range(n):
            deletion = previous_row[j + 1] + 1.0  # uniform_costs: (above + 1, left + 1, upper left + (a != b))
            insertion = current_row[j] + 1.0
            substitution = previous_row[j] + (0.0 if a[i] == b[j] else 1.0)
            current_row[j + 1] = min(insertion, deletion, substitution)
        matrix.append(current_row)
    return _walk(matrix, m, n)


def _matrix(a: Sequence, b: Sequence) -> np.ndarray:
    """The same matrix filled by numpy (a row's left-to-right dependency as a running minimum)."""
    m, n = len(a), len(b)
    a_ids, b_ids = np.asarray(list(a)), np.asarray(list(b))
    matrix = np.empty((m + 1, n + 1), dtype=np.int64)
    matrix[0] = np.arange(n + 1)
    ramp = np.arange(n + 1)
    for i in range(1, m + 1):
        prev = matrix[i - 1]
        row = np.empty(n + 1, dtype=np.int64)
        row[0] = i
        if n:
            row[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (a_ids[i - 1] != b_ids))
        matrix[i] = np.minimum.accumulate(row - ramp) + ramp
    return matrix


def levensthein_operations_fast(a: Sequence, b: Sequence) -> Tuple[List[Operation], float]:
    """``levensthein_operations`` with the matrix filled by numpy and the same walk: for the long pairs of the GPU tests."""
    return _walk(_matrix(a, b), len(a), len(b))


def to_substitutions(a: Sequence[str], b: Sequence[str], operations: Sequence[Operation]) -> List[Tuple[int, str, str]]:
    out = []
    for operation, i, j in operations:
        if operation == DELETION:
            out.append((operation, a[i], ""))
        elif operation == INSERTION:
            out.append((operation, "", b[j]))
        else:
            out.append((operation, a[i], b[j]))
    return out


def levensthein_substitutions(expected: Sequence[str], actual: Sequence[str]) -> List[Tuple[int, str, str]]:
    return to_substitutions(expected, actual, levensthein_operations(expected, actual)[0])


def kernel_form(a: Sequence, b: Sequence) -> Tuple[List[Operation], float, int, int]:
    """What amx_edit_ops.hip computes.  The sweep: lane l of strip s owns row i = 64 s + l + 1 and meets cell (i, j) at step
    t = j + l, where it sets bit l of the step's (diagonal, second) masks from the three predecessors alone.  The walk from
    (m, n): i == 0 inserts, j == 0 deletes, else the cell's code: diagonal (a substitution when `second`, else a match),
    deletion (`second`) or insertion.  It loads the 64 words [max(0, t - 63), ...] of a strip when t leaves the loaded
    window, stops after `cost` operations and writes operation k at index cost - 1 - k.  Returns (operations, cost, moves,
    window loads)."""
    m, n = len(a), len(b)
    matrix = _matrix(a, b)
    strips = (m + 63) // 64
    diag_masks = np.zeros((strips, n + 64), dtype=np.uint64)
    second_masks = np.zeros((strips, n + 64), dtype=np.uint64)
    if m and n:
        up, left, dg = matrix[:-1, 1:], matrix[1:, :-1], matrix[:-1, :-1]
        chosen = np.minimum(up, left)  # deletion if strictly cheaper, else insertion
        diag = dg <= chosen
        second = np.where(diag, np.asarray(list(a))[:, None] != np.asarray(list(b))[None, :], up < left)
        rows = np.arange(m)
        s, l = rows // 64, (rows % 64).astype(np.uint64)
        t = np.arange(1, n + 1)[None, :] + (rows % 64)[:, None]
        strip = np.broadcast_to(s[:, None], t.shape)
        np.bitwise_or.at(diag_masks, (strip, t), diag.astype(np.uint64) << l[:, None])
        np.bitwise_or.at(second_masks, (strip, t), second.astype(np.uint64) << l[:, None])
    cost = int(matrix[m, n])
    operations: List[Optional[Operation]] = [None] * cost
    i, j, k, moves, loads = m, n, 0, 0, 0
    window = None
    while k < cost:
        moves += 1
        if i == 0:
            act, j = INSERTION, j - 1
        elif j == 0:
            act, i = DELETION, i - 1
        else:
            s, l = divmod(i - 1, 64)
            t = j + l
            if window is None or window[0] != s or t < window[1]:
                window, loads = (s, max(0, t - 63)), loads + 1
            assert window[1] <= t < window[1] + 64
            is_diag = int(diag_masks[s, t]) >> l & 1
            is_second = int(second_masks[s, t]) >> l & 1
            if is_diag:
                i, j, act = i - 1, j - 1, SUBSTITUTION if is_second else 0
            elif is_second:
                act, i = DELETION, i - 1
            else:
                act, j = INSERTION, j - 1
        if act:
            operations[cost - 1 - k] = (act, i, j)
            k += 1
    return operations, float(cost), moves, loads


def replay(a: Sequence, b: Sequence, operations: Sequence[Operation]) -> List:
    """Applies the operations (in order) to ``a``: equals ``b`` when they are an edit script of a into b."""
    out, i = [], 0
    for act, oi, oj in operations:
        if act == INSERTION:
            out.extend(a[i:oi])
            i = oi
            out.append(b[oj])
        else:
            out.extend(a[i:oi])
            i = oi + 1
            if act == SUBSTITUTION:
                out.append(b[oj])
    out.extend(a[i:])
    return out


def compute_edits(language: str, utterance_id: str, names: Sequence[str], label: Sequence[str],
                  candidates: Dict[str, Sequence[Sequence[str]]], contours, split, split_complex: bool,
                  replacements: Optional[Dict[str, str]] = None, source_map: Optional[Dict[str, str]] = None) -> Dict:
    """run.py _compute_edits for one utterance: per output the expected symbols (as evaluate compares them) and the
    substitutions of the FIRST candidate (processed as evaluate processes candidates); the UtteranceEdits dict mashumaro's
    to_dict gives (Action as its int, tuples as lists)."""
    expected_sequences, edits = {}, {}
    for name in names:
        expected = E.expected_symbols(name, label, contours, split, split_complex, replacements)
        actual = E.actual_symbols(name, candidates[name][0], split, split_complex, source_map)
        edits[name] = [list(t) for t in levensthein_substitutions(expected, actual)]
        expected_sequences[name] = expected
    return {"language": language, "utterance_id": utterance_id, "expected": expected_sequences, "edit_operations": edits}


def to_json(edits: Dict) -> str:
    """mashumaro's DataClassJSONMixin.to_json: json.dumps of to_dict with the defaults."""
    return json.dumps(edits)

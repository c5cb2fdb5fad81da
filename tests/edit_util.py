"""Literal Python restatement of upstream's evaluation (test infrastructure): ``levensthein_statistics_general`` with uniform
costs (edit_distance.rs:372-481: the full matrix, then the first best path walked back from (m, n)), ``word_error_rate`` in
fp32 (:311-317), and ``run.py``'s ``_process_prediction`` / ``_process_candidates`` / ``_compute_edit_statistics`` /
``evaluate`` aggregation (:392-499) on strings.  Also the forward-carried form the kernel computes, and a plain two-row
Levenshtein distance as an independent check."""
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

Stats = Tuple[int, int, int, int]  # insertions, deletions, substitutions, correct


def levensthein_statistics(a: Sequence, b: Sequence) -> Stats:
    """``string_a`` = expected, ``string_b`` = actual."""
    m, n = len(a), len(b)
    matrix = [[float(j) for j in range(n + 1)]]
    for i in range(m):
        previous = matrix[i]
        current = list(previous)
        current[0] += 1.0
        for j in range(n):
            insertion = previous[j + 1] + 1.0  # uniform_costs: (above + 1, left + 1, upper left + (a != b))
            deletion = current[j] + 1.0
            substitution = previous[j] + (0.0 if a[i] == b[j] else 1.0)
            current[j + 1] = min(insertion, deletion, substitution)
        matrix.append(current)
    cost = matrix[m][n]
    i, j = m, n
    ins = dels = subs = correct = 0
    while cost != 0.0:
        if i == 0:
            if j == 0:
                break
            op, cost = "I", matrix[i][j - 1]
        elif j == 0:
            op, cost = "D", matrix[i - 1][j]
        else:
            deletion, insertion, substitution = matrix[i - 1][j], matrix[i][j - 1], matrix[i - 1][j - 1]
            op, c = ("D", deletion) if deletion < insertion else ("I", insertion)
            if substitution <= c:
                op = "C" if substitution == cost else "S"
                c = substitution
            cost = c
        if op == "C":
            i, j, correct = i - 1, j - 1, correct + 1
        elif op == "D":
            i, dels = i - 1, dels + 1
        elif op == "I":
            j, ins = j - 1, ins + 1
        else:
            i, j, subs = i - 1, j - 1, subs + 1
    correct += i
    return ins, dels, subs, correct


def carried_statistics(a: Sequence, b: Sequence) -> Stats:
    """The kernel's form: per cell (cost, S, D) of the walk that starts there, carried forward row by row; no matrix and no
    back-trace.  C = m - S - D, I = n - C - S."""
    m, n = len(a), len(b)
    prev = [(j, 0, 0) for j in range(n + 1)]
    for i in range(1, m + 1):
        cur = [(i, 0, i)]
        for j in range(1, n + 1):
            up, left, diag = prev[j], cur[j - 1], prev[j - 1]
            chosen = min(up[0], left[0])
            cost = min(chosen + 1, diag[0] + (0 if a[i - 1] == b[j - 1] else 1))
            s, d = (up[1], up[2] + 1) if up[0] < left[0] else (left[1], left[2])
            if diag[0] <= chosen:
                s, d = diag[1] + (diag[0] != cost), diag[2]
            cur.append((cost, 0, 0) if cost == 0 else (cost, s, d))
        prev = cur
    _, s, d = prev[n]
    c = m - s - d
    return n - c - s, d, s, c


def levenshtein(a: Sequence, b: Sequence) -> int:
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def word_error_rate(stats: Stats) -> np.float32:
    ins, dels, subs, correct = stats
    sd = np.float32(subs + dels)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (sd + np.float32(ins)) / (sd + np.float32(correct))


def best_candidate(expected: Sequence, candidates: Sequence[Sequence]) -> Tuple[int, Optional[Stats]]:
    """run.py:447-464: the first candidate whose rate is strictly below the best so far; (-1, None) if none is below inf."""
    lowest, best, best_stats = math.inf, -1, None
    for k, actual in enumerate(candidates):
        stats = levensthein_statistics(expected, actual)
        rate = word_error_rate(stats)
        if rate < lowest:
            lowest, best, best_stats = rate, k, stats
    return best, best_stats


def expected_symbols(name: str, label: Sequence[str], contours: Dict[str, Dict[str, List[str]]], split, split_complex: bool,
                     replacements: Optional[Dict[str, str]] = None) -> List[str]:
    """_process_prediction: an IPA output compares the label itself (split under --split-complex); an attribute output the
    categories of ``get_named`` (contours concatenated) of the label after the --fix-unicode replacements.
    ``contours``: phoneme -> feature -> category strings."""
    if name in ("phone", "phoneme"):
        return [p for s in label for p in split(s)] if split_complex else list(label)
    replacements = replacements or {}
    return [c for p in label for c in contours[replacements.get(p, p)][name]]


def actual_symbols(name: str, candidate: Sequence[str], split, split_complex: bool,
                   source_map: Optional[Dict[str, str]] = None) -> List[str]:
    """_process_candidates: IPA outputs are remapped, then split; attribute outputs compare as they are."""
    if name not in ("phone", "phoneme"):
        return list(candidate)
    actual = list(candidate) if source_map is None else [source_map[p] for p in candidate]
    return [p for s in actual for p in split(s)] if split_complex else actual


def evaluate(names: Sequence[str], languages: Sequence[str], utterances) -> Dict[str, Dict[str, Stats]]:
    """_compute_edit_statistics + evaluate: ``utterances`` yields (language, {name: (expected, candidates)}); returns
    language -> name -> summed statistics, with ``"total"`` the sum over languages."""
    out = {language: {name: (0, 0, 0, 0) for name in names} for language in languages}
    for language, per_output in utterances:
        for name, (expected, candidates) in per_output.items():
            _, stats = best_candidate(expected, candidates)
            if stats is None:
                continue
            out[language][name] = tuple(x + y for x, y in zip(out[language][name], stats))
    total = {name: (0, 0, 0, 0) for name in names}
    for language in languages:
        for name in names:
            total[name] = tuple(x + y for x, y in zip(total[name], out[language][name]))
    out["total"] = total
    return out


# A small Allophoible-format table: contour cells ("-,+"), complex segments ("ts", "t͡ʃ"), a precomposed "é" that a
# decomposed label form maps to under --fix-unicode, and three categories per feature column.
TABLE_HEADER = ("InventoryID,Glottocode,ISO6393,LanguageName,SpecificDialect,GlyphID,Phoneme,Allophones,Marginal,SegmentClass,"
                "Source,tone,syllabic,long,nasal")
TABLE_ROWS = [
    ("a", "0", "+", "-", "-"),
    ("e", "0", "+", "-", "-"),
    ("é", "0", "+", "-", "0"),
    ("aː", "0", "+", "-,+", "-"),
    ("t", "0", "-", "-", "-"),
    ("s", "0", "-", "-", "-"),
    ("ts", "0", "-,-", "-", "-,0"),
    ("t͡ʃ", "0", "-", "-", "0,-"),
    ("ʃ", "0", "-", "-", "-"),
    ("m", "0", "-", "-", "+"),
    ("i", "0", "0", "0", "-"),
]


def synthetic_table_text() -> str:
    lines = [TABLE_HEADER]
    for k, (phoneme, tone, syllabic, long_, nasal) in enumerate(TABLE_ROWS):
        lines.append(f'1,glot,xxx,Language,,G{k},{phoneme},{phoneme},FALSE,segment,src,{tone},"{syllabic}","{long_}","{nasal}"')
    return "\n".join(lines) + "\n"


def levensthein_statistics_fast(a: Sequence, b: Sequence) -> Stats:
    """``levensthein_statistics`` with the matrix filled by numpy (a row's left-to-right dependency as a running minimum)
    and the same back-trace: for the long pairs of the GPU tests."""
    m, n = len(a), len(b)
    a_ids, b_ids = np.asarray(a), np.asarray(b)
    matrix = np.empty((m + 1, n + 1), dtype=np.int64)
    matrix[0] = np.arange(n + 1)
    ramp = np.arange(n + 1)
    for i in range(1, m + 1):
        prev = matrix[i - 1]
        row = np.empty(n + 1, dtype=np.int64)
        row[0] = i
        if n:
            row[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (a_ids[i - 1] != b_ids))
        matrix[i] = np.minimum.accumulate(row - ramp) + ramp  # current[j] = min_k (t[k] + j - k)
    cost = matrix[m, n]
    i, j = m, n
    ins = dels = subs = correct = 0
    while cost != 0:
        if i == 0:
            j, ins, cost = j - 1, ins + 1, matrix[0, j - 1]
            continue
        if j == 0:
            i, dels, cost = i - 1, dels + 1, matrix[i - 1, 0]
            continue
        deletion, insertion, substitution = matrix[i - 1, j], matrix[i, j - 1], matrix[i - 1, j - 1]
        chosen = deletion if deletion < insertion else insertion
        if substitution <= chosen:
            if substitution == cost:
                correct += 1
            else:
                subs += 1
            i, j, cost = i - 1, j - 1, substitution
        elif deletion < insertion:
            i, dels, cost = i - 1, dels + 1, deletion
        else:
            j, ins, cost = j - 1, ins + 1, insertion
    return ins, dels, subs, correct + i

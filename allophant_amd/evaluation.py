"""Phoneme and attribute error rates of decoded batches: upstream's ``run.py evaluate`` (run.py:392-499) on the device.

``Evaluator.add`` scores the hypotheses that ``Estimator.greedy_decode_device`` / ``beam_decode_device`` left in HBM against
the batch's labels with the ``amx_edit_statistics`` kernel (include/allophant_amx_edit.h): upstream's
``levensthein_statistics`` per (output, utterance, candidate), the candidate of the lowest fp32 error rate, and per-language
totals, all without a host synchronisation.  ``Evaluator.results`` fetches the totals once and returns upstream's
``MultilingualEvaluationResults`` (evaluation.py:33-73), JSON keys included.

The kernel compares ids.  Every output gets an id space built from the strings upstream compares, and two CSR maps into it:
the label map (a label phoneme -> its attribute contour, after the ``--fix-unicode`` replacements, or the phoneme itself,
split under ``--split-complex``) and the hypothesis map (a token -> ``inventory[token - 1]``, remapped per language and split,
or the category ``feature_values(name, token - 1)``; the blank expands to nothing).

``Evaluator.operations`` / ``Evaluator.edits`` are upstream's ``run.py edits`` (run.py:502-528) on the same ids: the
``amx_edit_operations`` kernel walks ``levensthein_operations``'s path for the first candidate of every (output, utterance), and
``edits`` turns the records into ``UtteranceEdits`` (predictions.py:58-83) with one host synchronisation.

``PropertyWeighting`` is upstream's class of that name (edit_distance.rs:498-599): fp32 insertion and deletion costs and, as the
substitution cost, the number of features in which two phonemes' rows of a property table differ, through the
``amx_edit_weighted_*`` / ``amx_edit_matrix`` kernels.  ``Evaluator(weighting=...)`` scores the IPA outputs under it.

``Evaluator(confusions=True)`` also keeps confusion tables (confusion.py): every ``add`` hands the candidates it has just
chosen to the ``amx_edit_confusions`` kernel, and ``Evaluator.confusions`` fetches the accumulated ``ConfusionTable``.
"""
from __future__ import annotations

import ctypes as C
import json
import unicodedata
from dataclasses import dataclass, field
from enum import IntEnum
from typing import Dict, Hashable, IO, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import lib as _lib
from .confusion import ConfusionCounts, ConfusionTable
from .phonetic import IPA_LAYERS, AttributeTable, InventoryView, split_complex_segment

__all__ = ["EditStatistics", "EvaluationResults", "MultilingualEvaluationResults", "EvaluationMaps", "Evaluator", "LabelBatch", "levensthein_statistics",
           "levensthein_statistics_batch", "unicode_replacements", "Action", "UtteranceEdits", "levensthein_operations",
           "levensthein_operations_batch", "levensthein_substitutions", "to_substitutions", "PropertyWeighting",
           "levensthein_matrix", "levensthein_confusions_batch"]

TOTAL = "total"
STATISTICS_FIELDS = ("insertions", "deletions", "substitutions", "correct")  # the kernel's order


def _f32_ratio(numerator: np.float32, denominator: np.float32) -> float:
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float32(numerator) / np.float32(denominator))


@dataclass(frozen=True)
class EditStatistics:
    """Upstream's ``allophant.phonemes.EditStatistics`` (edit_distance.rs:283-360): counts of the first best edit path; rates
    in fp32 with upstream's order of operations."""
    insertions: int = 0
    deletions: int = 0
    substitutions: int = 0
    correct: int = 0

    @classmethod
    def zeros(cls) -> "EditStatistics":
        return cls(0, 0, 0, 0)

    def word_error_rate(self) -> float:
        """``(f32(S + D) + f32(I)) / (f32(S + D) + f32(C))``: NaN for all zeros, inf for insertions against nothing."""
        substituted_or_deleted = np.float32(self.substitutions + self.deletions)
        return _f32_ratio(substituted_or_deleted + np.float32(self.insertions), substituted_or_deleted + np.float32(self.correct))

    def _expected_count(self) -> np.float32:
        return np.float32(self.substitutions + self.deletions + self.correct)

    def substitution_rate(self) -> float:
        return _f32_ratio(np.float32(self.substitutions), self._expected_count())

    def insertion_rate(self) -> float:
        return _f32_ratio(np.float32(self.insertions), self._expected_count())

    def deletion_rate(self) -> float:
        return _f32_ratio(np.float32(self.deletions), self._expected_count())

    def __add__(self, other: "EditStatistics") -> "EditStatistics":
        if not isinstance(other, EditStatistics):
            return NotImplemented
        return EditStatistics(*(a + b for a, b in zip(self.astuple(), other.astuple())))

    def astuple(self) -> Tuple[int, int, int, int]:
        return (self.insertions, self.deletions, self.substitutions, self.correct)

    def to_dict(self) -> Dict[str, int]:
        return dict(zip(STATISTICS_FIELDS, self.astuple()))

    @classmethod
    def from_dict(cls, value: Dict[str, int]) -> "EditStatistics":
        if set(value) != set(STATISTICS_FIELDS):  # EditStatisticsField._deserialize
            raise ValueError("EditStatistics field mismatch, either missing or superfluous fields present")
        return cls(*(int(value[k]) for k in STATISTICS_FIELDS))

    def __str__(self) -> str:
        return (f"EditStatistics(insertions={self.insertions}, deletions={self.deletions}, "
                f"substitutions={self.substitutions}, correct={self.correct})")


@dataclass
class EvaluationResults:
    """Upstream's ``EvaluationResults``: per output name its error rate and statistics."""
    properties: List[str]
    error_rates: Dict[str, float]
    error_statistics: Dict[str, EditStatistics]

    @classmethod
    def from_statistics(cls, properties: Sequence[str], statistics: Dict[str, EditStatistics]) -> "EvaluationResults":
        return cls(list(properties), {name: s.word_error_rate() for name, s in statistics.items()}, dict(statistics))

    def to_dict(self) -> Dict:
        return {"properties": list(self.properties), "error_rates": dict(self.error_rates),
                "error_statistics": {name: s.to_dict() for name, s in self.error_statistics.items()}}

    @classmethod
    def from_dict(cls, value: Dict) -> "EvaluationResults":
        return cls(list(value["properties"]), {k: float(v) for k, v in value["error_rates"].items()},
                   {k: EditStatistics.from_dict(v) for k, v in value["error_statistics"].items()})

    def __format__(self, format_spec: str) -> str:
        return "\n".join(f"{name}: | {self.error_statistics[name]} | {self.error_rates[name] * 100:{format_spec + 'f'}}"
                         for name in self.properties)

    def __str__(self) -> str:
        return f"{self:.4}"


def _package_version() -> str:
    from . import __version__

    return __version__


@dataclass
class MultilingualEvaluationResults:
    """Upstream's ``MultilingualEvaluationResults``: per language (and ``"total"``) an ``EvaluationResults``."""
    evaluation_arguments: str
    results: Dict[str, EvaluationResults]
    package_version: str = field(default_factory=_package_version)

    @classmethod
    def from_statistics(cls, evaluation_arguments: str, properties: Sequence[str],
                        statistics: Dict[str, Dict[str, EditStatistics]]) -> "MultilingualEvaluationResults":
        """``evaluate`` (run.py:475-493): every language's results, then ``"total"``, the integer sum over the languages."""
        results: Dict[str, EvaluationResults] = {}
        totals: Dict[str, EditStatistics] = {}
        for language, language_statistics in statistics.items():
            for name, s in language_statistics.items():
                totals[name] = totals.get(name, EditStatistics.zeros()) + s
            results[language] = EvaluationResults.from_statistics(properties, language_statistics)
        results[TOTAL] = EvaluationResults.from_statistics(properties, totals)
        return cls(evaluation_arguments, results)

    def with_totals(self) -> "MultilingualEvaluationResults":
        """These results with ``"total"`` rebuilt from the languages."""
        languages = {k: v for k, v in self.results.items() if k != TOTAL}
        properties = next(iter(self.results.values())).properties if self.results else []
        rebuilt = MultilingualEvaluationResults.from_statistics(
            self.evaluation_arguments, properties, {k: v.error_statistics for k, v in languages.items()})
        rebuilt.package_version = self.package_version
        return rebuilt

    def to_dict(self) -> Dict:
        return {"evaluation_arguments": self.evaluation_arguments,
                "results": {k: v.to_dict() for k, v in self.results.items()}, "package_version": self.package_version}

    @classmethod
    def from_dict(cls, value: Dict) -> "MultilingualEvaluationResults":
        return cls(value["evaluation_arguments"], {k: EvaluationResults.from_dict(v) for k, v in value["results"].items()},
                   value.get("package_version", _package_version()))

    def dumps(self) -> str:
        return json.dumps(self.to_dict())

    def dump(self, file: IO[str]) -> None:
        file.write(self.dumps())

    @classmethod
    def loads(cls, text: str) -> "MultilingualEvaluationResults":
        return cls.from_dict(json.loads(text))

    @classmethod
    def load(cls, file: IO[str]) -> "MultilingualEvaluationResults":
        return cls.loads(file.read())

    def __format__(self, format_spec: str) -> str:
        lines = [f"Command: {self.evaluation_arguments}\nVersion: {self.package_version}"]
        lines += [f"{language}:\n{results:{format_spec}}" for language, results in self.results.items()]
        return "\n".join(lines)

    def __str__(self) -> str:
        return f"{self:.4}"


class Action(IntEnum):
    """Upstream's ``allophant.phonemes.Action`` (phonemes.pyi): the recorded edit operations."""
    INSERTION = 1
    DELETION = 2
    SUBSTITUTION = 3

    @staticmethod
    def from_int(integer: int) -> "Action":
        return Action(integer)


Operation = Tuple[Action, int, int]  # (action, i, j): the coordinates after the move
Substitution = Tuple[Action, str, str]  # (action, expected symbol or "", actual symbol or "")


@dataclass
class UtteranceEdits:
    """Upstream's ``UtteranceEdits`` (predictions.py:70-83): per output the expected symbols and the edit operations that turn
    them into the first candidate.  ``to_dict`` / ``to_json`` give mashumaro's shape: fields in this order, ``Action`` as its
    int, tuples as lists, ``json.dumps`` defaults (non-ASCII escaped)."""
    language: str
    utterance_id: str
    expected: Dict[str, List[str]]
    edit_operations: Dict[str, List[Substitution]]

    def to_dict(self) -> Dict:
        return {"language": self.language, "utterance_id": self.utterance_id,
                "expected": {name: list(symbols) for name, symbols in self.expected.items()},
                "edit_operations": {name: [[int(action), a, b] for action, a, b in operations]
                                    for name, operations in self.edit_operations.items()}}

    @classmethod
    def from_dict(cls, value: Dict) -> "UtteranceEdits":
        return cls(str(value["language"]), str(value["utterance_id"]),
                   {name: [str(s) for s in symbols] for name, symbols in value["expected"].items()},
                   {name: [(Action.from_int(action), str(a), str(b)) for action, a, b in operations]
                    for name, operations in value["edit_operations"].items()})

    def to_json(self) -> str:
        return json.dumps(self.to_dict())

    @classmethod
    def from_json(cls, text: str) -> "UtteranceEdits":
        return cls.from_dict(json.loads(text))


def to_substitutions(expected: Sequence[str], actual: Sequence[str], operations: Sequence[Tuple[int, int, int]]
                     ) -> List[Substitution]:
    """Upstream's ``phonemes.to_substitutions`` (edit_distance.rs:105-119), on the host: each (action, i, j) as (action,
    expected[i] or "", actual[j] or "")."""
    result = []
    for action, i, j in operations:
        action = Action(action)
        if action == Action.DELETION:
            result.append((action, expected[i], ""))
        elif action == Action.INSERTION:
            result.append((action, "", actual[j]))
        else:
            result.append((action, expected[i], actual[j]))
    return result


def unicode_replacements(table: AttributeTable, symbols: Sequence[str]) -> Dict[str, str]:
    """``--fix-unicode``: ``missing_inventory_mappings`` (phonetic_features.py:488-510) without segmentation -- a label
    symbol missing from the table maps to its NFC form when the table has that."""
    known = set(table.full_phonemes)
    mapping = {}
    for symbol in symbols:
        if symbol in known:
            continue
        combined = unicodedata.normalize("NFC", symbol)
        if combined not in known:
            raise ValueError(f"No suitable mapping found for segment {symbol!r}")
        mapping[symbol] = combined
    return mapping


class _MapBuilder:
    """Concatenated CSR maps (``map_offsets`` / ``map_values``) and their descriptors (first, entries)."""

    def __init__(self):
        self.offsets: List[int] = []
        self.values: List[int] = []

    def add(self, entries: Sequence[Sequence[int]]) -> Tuple[int, int]:
        first = len(self.offsets)
        for entry in entries:
            self.offsets.append(len(self.values))
            self.values.extend(entry)
        self.offsets.append(len(self.values))
        return first, len(entries)


def _ids(space: Dict[Hashable, int], symbols: Sequence[Hashable]) -> List[int]:
    return [space.setdefault(s, len(space)) for s in symbols]


def _library():
    handle = _lib.load()
    if not hasattr(handle, "amx_edit_statistics"):
        raise RuntimeError("liballophant_amx.so lacks amx_edit_statistics: rebuild the library")
    return handle


def _weighted_library():
    handle = _library()
    if not hasattr(handle, "amx_edit_weighted_statistics"):
        raise RuntimeError("liballophant_amx.so lacks amx_edit_weighted_statistics: rebuild the library")
    return handle


class _Weights(NamedTuple):
    """The cost arguments of the weighted kernels: per output a descriptor (first, V) into ``data``, the concatenated
    pairwise cost tables (V == 0: no table, ``a != b``)."""
    insertion_cost: float
    deletion_cost: float
    descriptors: Tensor  # int64 [O, 2]
    data: Optional[Tensor]  # uint8


def _device(device) -> torch.device:
    device = torch.device(device if device is not None else "cuda")
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("edit statistics run on the MI355X: there is no CPU path")
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


def _ptr(t: Optional[Tensor], offset: int = 0):
    """Device address of element ``offset`` of ``t`` (an empty tail still gets a non-null address)."""
    return C.c_void_p(t.data_ptr() + offset * t.element_size()) if t is not None else None


class _EditRows(NamedTuple):
    """What every row call of the edit family scores: the candidates, the labels and the maps between them."""
    tokens: Tensor  # int64 [O, N, K, T]
    counts: Tensor  # int32 [O, N, K], contiguous
    hyp_counts: Optional[Tensor]  # int32 [O, N], or None: all K candidates
    labels: Tensor  # the uploaded int32 block [offsets N + 1 | groups N | label ids]
    N: int
    G: int
    maps: Tensor  # the uploaded int32 block [map offsets | map values]
    n_offsets: int
    label_maps: Tensor  # int32 [O, 2]
    hyp_maps: Tensor  # int32 [H, O, 2]
    H: int
    max_expected: int
    max_actual: int

    def head(self, workspace: Tensor, candidates: bool = True) -> tuple:
        """The leading ctypes arguments of a row call on ``workspace``, the same for the six entries but for
        ``candidates=False``: an operations call has neither ``stride_k`` nor ``K``.  ``tokens`` have stride 1 along T
        (``unit_stride``)."""
        t, N = self.tokens, self.N
        O, N_, K, T = t.shape
        shape = (t.stride(0), t.stride(1), t.stride(2), O, N_, K, T) if candidates else (t.stride(0), t.stride(1), O, N_, T)
        return (t.device.index, _ptr(t), *shape, _ptr(self.counts), _ptr(self.hyp_counts), _ptr(self.labels),
                _ptr(self.labels, 2 * N + 1), _ptr(self.labels, N + 1), self.G, _ptr(self.maps), _ptr(self.maps, self.n_offsets),
                _ptr(self.label_maps), _ptr(self.hyp_maps), self.H, self.max_expected, self.max_actual, _ptr(workspace),
                workspace.numel())

    def unit_stride(self) -> "_EditRows":
        return self if self.tokens.stride(3) == 1 else self._replace(tokens=self.tokens.contiguous())

    def select(self, index: Tensor, label_maps: Tensor, hyp_maps: Tensor) -> "_EditRows":
        """The rows of the outputs ``index``, under those outputs' map descriptors."""
        return self._replace(tokens=self.tokens.index_select(0, index), counts=self.counts.index_select(0, index),
                             hyp_counts=None if self.hyp_counts is None else self.hyp_counts.index_select(0, index),
                             label_maps=label_maps, hyp_maps=hyp_maps)

    def first(self) -> "_EditRows":
        """Candidate 0 of every row: what the operations calls take."""
        return self._replace(tokens=self.tokens[:, :, :1], counts=self.counts[:, :, :1].contiguous())

    def workspace(self, codes: bool, workspace: Optional[Tensor] = None) -> Tensor:
        """``workspace`` if it holds what ``amx_edit_operations_workspace`` (``codes``) or ``amx_edit_workspace`` asks for
        these rows, a new one otherwise."""
        handle = _library()
        O, N_, K, _ = self.tokens.shape
        size = C.c_size_t()
        if codes:
            code = handle.amx_edit_operations_workspace(O * N_, self.max_expected, self.max_actual, C.byref(size))
        else:
            code = handle.amx_edit_workspace(O * N_ * K, self.max_expected, self.max_actual, C.byref(size))
        _lib.check(handle, None, code)
        if workspace is None or workspace.numel() < size.value:
            workspace = torch.empty(max(16, size.value), dtype=torch.uint8, device=self.tokens.device)
        return workspace


def _run(rows: _EditRows, workspace: Optional[Tensor], totals: Tensor, weights: Optional["_Weights"] = None
         ) -> Tuple[Tensor, Tensor, Tensor, Optional[Tensor]]:
    """One ``amx_edit_statistics`` call, or with ``weights`` one ``amx_edit_weighted_statistics`` call.  Returns (statistics,
    best, workspace, costs float32 [O, N, K] or None; NaN where nothing was scored)."""
    handle = _library() if weights is None else _weighted_library()
    rows = rows.unit_stride()
    device = rows.tokens.device
    O, N, K, _ = rows.tokens.shape
    workspace = rows.workspace(False, workspace)
    statistics = torch.empty(O, N, K, 4, dtype=torch.int32, device=device)
    best = torch.empty(O, N, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    head = rows.head(workspace)
    costs = None
    with torch.cuda.device(device):
        if weights is None:
            code = handle.amx_edit_statistics(*head, _ptr(statistics), _ptr(best), _ptr(totals), C.c_void_p(stream))
        else:
            costs = torch.full((O, N, K), float("nan"), dtype=torch.float32, device=device)
            code = handle.amx_edit_weighted_statistics(
                *head, weights.insertion_cost, weights.deletion_cost, _ptr(weights.descriptors), _ptr(weights.data),
                _ptr(statistics), _ptr(best), _ptr(totals), _ptr(costs), C.c_void_p(stream))
    _lib.check(handle, None, code)
    return statistics, best, workspace, costs


def _run_operations(rows: _EditRows, workspace: Optional[Tensor], weights: Optional["_Weights"] = None
                    ) -> Tuple[Tensor, Tensor, Tensor, Optional[Tensor]]:
    """One ``amx_edit_operations`` (with ``weights``: ``amx_edit_weighted_operations``) call on ``rows`` of one candidate
    (``first()``).  Returns (operations int32 [O, N, max_ops, 5], operation counts int32 [O, N], workspace, costs float32
    [O, N] or None; NaN where there is no path)."""
    handle = _library() if weights is None else _weighted_library()
    rows = rows.unit_stride()
    device = rows.tokens.device
    O, N, K, _ = rows.tokens.shape
    if K != 1:
        raise ValueError(f"the operations calls take one candidate per row, not {K}")
    workspace = rows.workspace(True, workspace)
    max_expected, max_actual = rows.max_expected, rows.max_actual
    max_ops = max(1, max_expected, max_actual) if weights is None else max(1, max_expected + max_actual)
    operations = torch.empty(O, N, max_ops, 5, dtype=torch.int32, device=device)
    operation_counts = torch.empty(O, N, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    head = rows.head(workspace, candidates=False)
    costs = None
    with torch.cuda.device(device):
        if weights is None:
            code = handle.amx_edit_operations(*head, max_ops, _ptr(operations), _ptr(operation_counts), C.c_void_p(stream))
        else:
            costs = torch.full((O, N), float("nan"), dtype=torch.float32, device=device)
            code = handle.amx_edit_weighted_operations(
                *head, weights.insertion_cost, weights.deletion_cost, _ptr(weights.descriptors), _ptr(weights.data), max_ops,
                _ptr(operations), _ptr(operation_counts), _ptr(costs), C.c_void_p(stream))
    _lib.check(handle, None, code)
    return operations, operation_counts, workspace, costs


def _upload(blocks: Sequence[np.ndarray], device: torch.device) -> Tuple[Tensor, List[int]]:
    """Concatenates int32 blocks into one pinned buffer and copies it with one non-blocking copy; returns the device tensor
    and each block's start."""
    starts, total = [], 0
    for b in blocks:
        starts.append(total)
        total += len(b)
    host = torch.empty(max(1, total), dtype=torch.int32, pin_memory=True)
    view = host.numpy()
    for start, b in zip(starts, blocks):
        view[start:start + len(b)] = b
    return host.to(device, non_blocking=True), starts


class LabelBatch(NamedTuple):
    """A batch's labels on the device: ``data`` int32 [offsets N + 1 | language indices N | label ids], and the longest
    label of any output once expanded (host-computed: it sizes the workspace)."""
    data: Tensor
    N: int
    max_expected: int


class EvaluationMaps:
    """The host half of ``Evaluator``: per output an id space (``spaces[o]``: string -> id) built from the strings upstream
    compares, the label map and the hypothesis maps into it, as concatenated CSR arrays (``offsets``, ``values``) with
    descriptors ``label_maps`` [O, 2] and ``hyp_maps`` [H, O, 2] (first, entries).  ``label_ids`` numbers the label symbols:
    every phoneme of the table and every replaced form.  Arguments as ``Evaluator``."""

    def __init__(self, table: AttributeTable, names: Sequence[str], inventory: Union[InventoryView, Sequence[str]],
                 languages: Sequence[str], split_complex: bool = False,
                 source_maps: Optional[Dict[str, Dict[str, str]]] = None, replacements: Optional[Dict[str, str]] = None):
        self.names = list(names)
        self.languages = list(languages)
        if not self.names or not self.languages:
            raise ValueError("evaluation needs at least one output and one language")
        inventory = list(inventory.inventory if isinstance(inventory, InventoryView) else inventory)
        self.table, self.inventory = table, inventory  # (what alignment.label_targets turns expected strings into classes with)
        replacements = dict(replacements or {})
        if source_maps is not None:
            missing = [lang for lang in self.languages if lang not in source_maps]
            if missing:
                raise ValueError(f"no source map for the languages {missing}")
        known = set(table.full_phonemes)
        self.label_ids: Dict[str, int] = {}
        _ids(self.label_ids, table.full_phonemes)
        _ids(self.label_ids, list(replacements))
        label_symbols = list(self.label_ids)

        def split(symbols: Sequence[str]) -> List[str]:
            return [p for s in symbols for p in split_complex_segment(s)] if split_complex else list(symbols)

        builder = _MapBuilder()
        self.H = len(self.languages) if source_maps is not None else 1
        self.label_maps = np.zeros((len(self.names), 2), dtype=np.int32)
        self.hyp_maps = np.zeros((self.H, len(self.names), 2), dtype=np.int32)
        self.label_lengths = np.zeros((len(self.names), len(label_symbols)), dtype=np.int64)
        self.spaces: List[Dict[str, int]] = []
        fanout = 0
        for o, name in enumerate(self.names):
            space: Dict[str, int] = {}
            self.spaces.append(space)
            if name in IPA_LAYERS:
                # run.py:399-411: the label itself (no replacement), split under --split-complex
                entries = [_ids(space, split([p])) for p in label_symbols]
            else:
                if name not in table.full_feature_names:
                    raise ValueError(f"Missing feature in attributes: {name!r}")
                entries = []
                for p in label_symbols:
                    target = replacements.get(p, p)
                    if target not in known:
                        raise ValueError(f"replacement {p!r} -> {target!r} names no phoneme of the attribute table")
                    entries.append(_ids(space, table.feature_contour(target, name)))
            self.label_lengths[o] = [len(e) for e in entries]
            self.label_maps[o] = builder.add(entries)
            for h in range(self.H):
                if name not in IPA_LAYERS:
                    if h == 0:  # attribute maps do not depend on the language: feature_values(name, token - 1)
                        entries = [[]] + [_ids(space, [c]) for c in table.feature_categories(name)]
                        fanout = max(fanout, 1)
                        self.hyp_maps[0, o] = builder.add(entries)
                    else:
                        self.hyp_maps[h, o] = self.hyp_maps[0, o]
                    continue
                source = None if source_maps is None else source_maps[self.languages[h]]
                if source is not None:
                    missing = [p for p in inventory if p not in source]
                    if missing:
                        raise ValueError(f"source map of {self.languages[h]!r} lacks {missing}")
                # inventory[token - 1], remapped, then split; the blank (token 0) expands to nothing
                entries = [[]] + [_ids(space, split([source[p] if source is not None else p])) for p in inventory]
                fanout = max(fanout, max(len(e) for e in entries))
                self.hyp_maps[h, o] = builder.add(entries)
        self.hyp_fanout = max(1, fanout)
        self.offsets = np.asarray(builder.offsets, dtype=np.int32)
        self.values = np.asarray(builder.values, dtype=np.int32)

    def _expand(self, descriptor, ids: Sequence[int], o: int) -> List[str]:
        first, entries = (int(v) for v in descriptor)
        names = {i: s for s, i in self.spaces[o].items()}
        out = []
        for e in ids:
            if not 0 <= e < entries:
                raise IndexError(f"id {e} outside a map of {entries} entries")
            out += [names[int(v)] for v in self.values[self.offsets[first + e]:self.offsets[first + e + 1]]]
        return out

    def expand_label(self, o: int, label: Sequence[str]) -> List[str]:
        """What the kernel compares as expected, as strings (host expansion through the label map of output ``o``)."""
        return self._expand(self.label_maps[o], [self.label_ids[s] for s in label], o)

    def expand_tokens(self, o: int, language: int, tokens: Sequence[int]) -> List[str]:
        """What the kernel compares as actual, as strings (host expansion of decoded token ids)."""
        return self._expand(self.hyp_maps[language if self.H > 1 else 0, o], [int(t) for t in tokens], o)


class Evaluator:
    """Accumulates upstream's ``evaluate`` statistics over decoded batches on the device.

    ``table``: the attribute table (its full feature columns give the label contours); ``names``: the outputs to score (a
    subset of the decoded ones, e.g. ``Predictions.outputs`` keys); ``inventory``: the phoneme inventory (or ``InventoryView``)
    the predictions were made under -- the ``phone`` / ``phoneme`` tokens index it; ``languages``: the totals slots, in
    order.  Options as upstream's ``evaluate``: ``split_complex`` (``--split-complex``), ``source_maps`` (language -> phoneme
    -> phoneme: remapping, which ``--no-remap`` turns off) and ``replacements`` (label phoneme -> table phoneme, applied before
    the attribute lookup: ``--fix-unicode``, see ``unicode_replacements``).

    ``weighting``: a ``PropertyWeighting``; the IPA outputs (``phone``, ``phoneme``) are then scored, chosen and listed under
    its costs (``add``, ``operations``, ``edits``), while attribute outputs keep unit costs.  Every symbol of an IPA output's
    id space (label phonemes, inventory, remapped and split forms) must be in its table: ``ValueError`` otherwise."""

    def __init__(self, table: AttributeTable, names: Sequence[str], inventory: Union[InventoryView, Sequence[str]],
                 languages: Sequence[str], split_complex: bool = False,
                 source_maps: Optional[Dict[str, Dict[str, str]]] = None, replacements: Optional[Dict[str, str]] = None,
                 device=None, weighting: Optional["PropertyWeighting"] = None, confusions: Union[bool, int] = False):
        self.device = _device(device)
        self.maps = EvaluationMaps(table, names, inventory, languages, split_complex, source_maps, replacements)
        self.weighting = weighting
        if weighting is not None:
            self._init_weighting(weighting)
        self.names, self.languages = self.maps.names, self.maps.languages
        self._n_offsets = len(self.maps.offsets)
        self._maps = torch.from_numpy(np.concatenate([self.maps.offsets, self.maps.values])).to(self.device)
        self._label_maps = torch.from_numpy(self.maps.label_maps.reshape(-1)).to(self.device)
        self._hyp_maps = torch.from_numpy(self.maps.hyp_maps.reshape(-1)).to(self.device)
        self.totals = torch.zeros(len(self.languages), len(self.names), 4, dtype=torch.int64, device=self.device)
        self._workspace: Optional[Tensor] = None
        self._ops_workspace: Optional[Tensor] = None
        self._rows: Optional[Tuple[Tensor, Tensor]] = None
        self._costs: Optional[Tensor] = None
        self._operation_costs: Optional[Tensor] = None
        # confusion tables: one accumulator for the uniform kernels' outputs, or one per part under a weighting (a key
        # holds the output's index within its call)
        self._confusions: Optional[List[Tuple[List[int], ConfusionCounts]]] = None
        self._confusion_events: Optional[Tensor] = None
        if confusions is not False:
            capacity = 2 ** 20 if confusions is True else int(confusions)
            parts = [list(range(len(self.names)))] if weighting is None else [index.tolist() for index, _, _, _ in self._parts]
            self._confusions = [(outputs, ConfusionCounts(self.device, capacity, self.languages, [self.names[o] for o in outputs],
                                                          [list(self.maps.spaces[o]) for o in outputs])) for outputs in parts]

    def _init_weighting(self, weighting: "PropertyWeighting") -> None:
        """Splits the outputs into the IPA ones, scored under ``weighting`` with one cost table per id space, and the
        attribute ones, scored by the uniform kernels; each part gets its own descriptors."""
        weighted = [o for o, name in enumerate(self.maps.names) if name in IPA_LAYERS]
        uniform = [o for o, name in enumerate(self.maps.names) if name not in IPA_LAYERS]
        missing = sorted({s for o in weighted for s in self.maps.spaces[o] if not weighting.has(s)})
        if missing:
            raise ValueError(f"the property table lacks the symbols {missing}")
        tables = [weighting.cost_table(list(self.maps.spaces[o]), self.device) for o in weighted]
        descriptors, first = [], 0
        for o, t in zip(weighted, tables):
            descriptors.append((first, len(self.maps.spaces[o])))
            first += t.numel()
        data = torch.cat(tables) if first else None
        self._parts = []
        for outputs, weights in ((uniform, None), (weighted, _Weights(weighting.insertion_cost, weighting.deletion_cost,
                                 torch.tensor(descriptors, dtype=torch.int64, device=self.device).reshape(-1, 2), data))):
            if outputs:
                index = torch.tensor(outputs, dtype=torch.long, device=self.device)
                label_maps = torch.from_numpy(np.ascontiguousarray(self.maps.label_maps[outputs]).reshape(-1)).to(self.device)
                hyp_maps = torch.from_numpy(np.ascontiguousarray(self.maps.hyp_maps[:, outputs]).reshape(-1)).to(self.device)
                self._parts.append((index, label_maps, hyp_maps, weights))
        self._part_workspaces: Dict[Tuple[int, bool], Optional[Tensor]] = {}

    def _add_weighted(self, rows: _EditRows) -> Tuple[Tuple[Tensor, Tensor], Tensor]:
        O, N, K, _ = rows.tokens.shape
        statistics = torch.empty(O, N, K, 4, dtype=torch.int32, device=self.device)
        best = torch.empty(O, N, dtype=torch.int32, device=self.device)
        costs = torch.empty(O, N, K, dtype=torch.float32, device=self.device)
        for p, (index, label_maps, hyp_maps, weights) in enumerate(self._parts):
            totals = torch.zeros(rows.G, len(index), 4, dtype=torch.int64, device=self.device)
            part = rows.select(index, label_maps, hyp_maps)
            part_statistics, part_best, self._part_workspaces[p, False], part_costs = _run(
                part, self._part_workspaces.get((p, False)), totals, weights)
            if self._confusions is not None:
                if p == 0:
                    self._confusion_events = torch.empty(O, N, dtype=torch.int32, device=self.device)
                self._confusion_events[index] = self._confusions[p][1].add_rows(part, part_best, weights)
            statistics.index_copy_(0, index, part_statistics)
            best.index_copy_(0, index, part_best)
            costs.index_copy_(0, index, _unit_costs(part_statistics) if part_costs is None else part_costs)
            self.totals.index_add_(1, index, totals)
        return (statistics, best), costs

    def _operations_weighted(self, rows: _EditRows) -> Tuple[Tensor, Tensor]:
        O, N, _, _ = rows.tokens.shape
        max_ops = max(1, rows.max_expected + rows.max_actual)
        operations = torch.empty(O, N, max_ops, 5, dtype=torch.int32, device=self.device)
        operation_counts = torch.empty(O, N, dtype=torch.int32, device=self.device)
        costs = torch.empty(O, N, dtype=torch.float32, device=self.device)
        for p, (index, label_maps, hyp_maps, weights) in enumerate(self._parts):
            part_operations, part_counts, self._part_workspaces[p, True], part_costs = _run_operations(
                rows.select(index, label_maps, hyp_maps), self._part_workspaces.get((p, True)), weights)
            operations[:, :, :part_operations.shape[2]].index_copy_(0, index, part_operations)
            operation_counts.index_copy_(0, index, part_counts)
            if part_costs is None:  # unit costs: one per record
                part_costs = torch.where(part_counts >= 0, part_counts.float(), torch.full_like(part_counts, float("nan"), dtype=torch.float32))
            costs.index_copy_(0, index, part_costs)
        self._operation_costs = costs
        return operations, operation_counts

    def reset(self) -> None:
        self.totals.zero_()
        for _, counts in self._confusions or []:
            counts.reset()

    def confusion_events(self) -> Tensor:
        """Of the last ``add`` with confusion tables: int32 [O, N], the number of events that each row's chosen candidate
        contributed; -1 for a row without a chosen candidate and -2 for a flagged row, which add nothing.  A device tensor."""
        if self._confusion_events is None:
            raise ValueError("nothing added with confusion tables yet")
        return self._confusion_events

    def confusions(self) -> ConfusionTable:
        """The confusion table of everything added since the last ``reset`` (``Evaluator(confusions=True)``): the events of
        the candidates that the statistics chose, per language and output, ids in ``maps.spaces[o]``.  One host
        synchronisation per accumulator; ``OverflowError`` if events were dropped (build the evaluator with a larger
        ``confusions=capacity``)."""
        if self._confusions is None:
            raise ValueError("this evaluator keeps no confusion tables: build it with confusions=True")
        columns: List[List[np.ndarray]] = [[] for _ in range(5)]
        for outputs, counts in self._confusions:
            part = counts.fetch()
            for column, values in zip(columns, (part.group, np.asarray(outputs, dtype=np.int64)[part.output], part.expected,
                                                part.actual, part.count)):
                column.append(values)
        return ConfusionTable(self.languages, self.names, [list(space) for space in self.maps.spaces],
                              *(np.concatenate(column) for column in columns))

    def encode_labels(self, labels: Sequence[Sequence[str]], languages: Sequence[Union[str, int]]) -> "LabelBatch":
        """Encodes a batch's labels (per utterance its phoneme strings) and languages (codes of ``languages`` or their
        indices) on the host, one dictionary lookup per symbol, and uploads them with one non-blocking copy from pinned
        memory.  ``add`` does this itself; call it ahead to capture ``add`` in a graph with the labels as a static input."""
        if len(labels) != len(languages):
            raise ValueError(f"{len(labels)} labels for {len(languages)} languages")
        N = len(labels)
        offsets = np.zeros(N + 1, dtype=np.int32)
        groups = np.empty(N, dtype=np.int32)
        ids: List[int] = []
        for n, (label, language) in enumerate(zip(labels, languages)):
            try:
                ids.extend(self.maps.label_ids[s] for s in label)
            except KeyError as e:
                raise ValueError(f"label symbol {e.args[0]!r} of utterance {n} is not in the attribute table") from None
            offsets[n + 1] = len(ids)
            groups[n] = language if isinstance(language, (int, np.integer)) else self.languages.index(language)
        ids_np = np.asarray(ids, dtype=np.int32)
        # the longest expanded label of any output: host data, so no device round trip
        cumulative = np.zeros((len(self.names), len(ids_np) + 1), dtype=np.int64)
        np.cumsum(self.maps.label_lengths[:, ids_np], axis=1, out=cumulative[:, 1:])
        max_expected = int((cumulative[:, offsets[1:]] - cumulative[:, offsets[:-1]]).max(initial=0))
        if max_expected > _lib.EDIT_MAX_LENGTH:
            raise ValueError(f"an expanded label has {max_expected} symbols; the limit is {_lib.EDIT_MAX_LENGTH}")
        data, _ = _upload([offsets, groups, ids_np], self.device)
        return LabelBatch(data, N, max_expected)

    def _edit_rows(self, decoded, tokens: Tensor, counts: Tensor, labels: Union[Sequence[Sequence[str]], "LabelBatch"],
                   languages: Optional[Sequence[Union[str, int]]]) -> _EditRows:
        """The rows of ``add`` and ``operations``: ``tokens`` [outputs of ``decoded``, N, K, T] and ``counts`` narrowed to
        the outputs of ``names``, with the encoded labels and this evaluator's maps."""
        outputs = [decoded.names.index(name) for name in self.names]
        hyp_counts = getattr(decoded, "hyp_counts", None)
        if tokens.device != self.device:
            raise ValueError(f"decoded results live on {tokens.device}, the evaluator on {self.device}")
        if outputs != list(range(len(decoded.names))):
            index = torch.tensor(outputs, dtype=torch.long, device=self.device)
            tokens, counts = tokens.index_select(0, index), counts.index_select(0, index)
            hyp_counts = None if hyp_counts is None else hyp_counts.index_select(0, index)
        counts = counts.to(torch.int32).contiguous()
        hyp_counts = None if hyp_counts is None else hyp_counts.to(torch.int32).contiguous()
        O, N, K, T = tokens.shape
        if not isinstance(labels, LabelBatch):
            if languages is None:
                raise ValueError("labels given as strings need their languages")
            labels = self.encode_labels(labels, languages)
        if N != labels.N:
            raise ValueError(f"{N} decoded utterances for {labels.N} labels")
        max_actual = min(T * self.maps.hyp_fanout, _lib.EDIT_MAX_LENGTH)
        return _EditRows(tokens, counts, hyp_counts, labels.data, N, len(self.languages), self._maps, self._n_offsets,
                         self._label_maps, self._hyp_maps, self.maps.H, labels.max_expected, max_actual)

    def add(self, decoded, labels: Union[Sequence[Sequence[str]], "LabelBatch"],
            languages: Optional[Sequence[Union[str, int]]] = None) -> None:
        """Scores ``decoded`` (``Decoded`` or ``BeamDecoded``, device-resident) against ``labels`` (per utterance its phoneme
        strings, with ``languages``; or a ``LabelBatch`` from ``encode_labels``) and adds each (output, utterance)'s best
        candidate to the totals of its language.  Stream-ordered: nothing waits for the device."""
        tokens, counts = decoded.tokens, decoded.counts
        if tokens.dim() == 3:  # greedy: one candidate
            tokens, counts = tokens.unsqueeze(2), counts.unsqueeze(2)
        rows = self._edit_rows(decoded, tokens, counts, labels, languages)
        if self.weighting is not None:
            self._rows, self._costs = self._add_weighted(rows)
            return
        statistics, best, self._workspace, _ = _run(rows, self._workspace, self.totals)
        self._rows, self._costs = (statistics, best), None
        if self._confusions is not None:  # the same stream, after the choice
            self._confusion_events = self._confusions[0][1].add_rows(rows, best)

    def operations(self, decoded, labels: Union[Sequence[Sequence[str]], "LabelBatch"],
                   languages: Optional[Sequence[Union[str, int]]] = None) -> Tuple[Tensor, Tensor]:
        """Upstream's ``levensthein_operations`` of the first candidate (for a ``BeamDecoded`` the best hypothesis) against
        the label, for every output of ``names`` and every utterance; arguments as ``add``.  Returns device tensors
        ``operations`` int32 [O, N, max_ops, 5] and ``counts`` int32 [O, N]: row (o, n) holds ``counts[o, n]`` records
        (action, i, j, expected id or -1, actual id or -1) in upstream's order, ids in ``maps.spaces[o]``; ``counts`` is -1
        for a row with no candidate and -2 for a row with an out-of-range token.  Stream-ordered: nothing waits for the
        device (capturable in a graph with a ``LabelBatch`` after one call outside the capture has sized the workspace)."""
        tokens, counts = decoded.tokens, decoded.counts
        if tokens.dim() == 4:  # beam: candidate 0, the highest-scoring hypothesis
            tokens, counts = tokens[:, :, 0], counts[:, :, 0]
        rows = self._edit_rows(decoded, tokens.unsqueeze(2), counts.unsqueeze(2), labels, languages)
        if self.weighting is not None:
            return self._operations_weighted(rows)
        operations, operation_counts, self._ops_workspace, _ = _run_operations(rows, self._ops_workspace)
        return operations, operation_counts

    def edits(self, decoded, labels: Sequence[Sequence[str]], languages: Sequence[Union[str, int]],
              utterance_ids: Sequence[str]) -> List[UtteranceEdits]:
        """Upstream's ``_compute_edits`` (run.py:502-521) on a decoded batch: per utterance an ``UtteranceEdits`` with, per
        output of ``names`` in that order, the expected symbols and the substitutions of the first candidate.  One host
        synchronisation.  A row with an out-of-range token or without a candidate raises ``ValueError``."""
        if not len(labels) == len(languages) == len(utterance_ids):
            raise ValueError(f"{len(labels)} labels, {len(languages)} languages and {len(utterance_ids)} utterance ids")
        operations, counts = self.operations(decoded, labels, languages)
        host_operations = torch.empty(operations.shape, dtype=torch.int32, pin_memory=True)
        host_counts = torch.empty(counts.shape, dtype=torch.int32, pin_memory=True)
        host_operations.copy_(operations, non_blocking=True)
        host_counts.copy_(counts, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        records, lengths = host_operations.numpy(), host_counts.numpy()
        symbols = [["" for _ in range(len(space))] for space in self.maps.spaces]
        for o, space in enumerate(self.maps.spaces):
            for symbol, i in space.items():
                symbols[o][i] = symbol
        edits = []
        for n, (label, language, utterance_id) in enumerate(zip(labels, languages, utterance_ids)):
            expected, substitutions = {}, {}
            for o, name in enumerate(self.names):
                count = int(lengths[o, n])
                if count < 0:
                    reason = "has no candidate" if count == -1 else "holds a token outside its map"
                    raise ValueError(f"output {name!r} of utterance {n} ({utterance_id!r}) {reason}")
                expected[name] = self.maps.expand_label(o, label)
                names = symbols[o]
                substitutions[name] = [(Action(action), names[a] if a >= 0 else "", names[b] if b >= 0 else "")
                                       for action, _, _, a, b in records[o, n, :count].tolist()]
            if not isinstance(language, str):
                language = self.languages[int(language)]
            edits.append(UtteranceEdits(language, str(utterance_id), expected, substitutions))
        return edits

    def rows(self) -> Tuple[Tensor, Tensor]:
        """Of the last ``add``: ``statistics`` int32 [O, N, K, 4] (insertions, deletions, substitutions, correct; -1 for a
        candidate past ``hyp_counts``, -2 for a row with an out-of-range token) and ``best`` int32 [O, N] (the chosen
        candidate, -1 for none, -2 for a flagged row), device tensors."""
        if self._rows is None:
            raise ValueError("nothing added yet")
        return self._rows

    def costs(self) -> Tensor:
        """Of the last ``add``, beside ``rows()``: float32 [O, N, K], every scored candidate's cost ``M[m][n]`` -- under the
        ``weighting`` for the IPA outputs, the number of operations for outputs scored with unit costs; NaN where ``rows()``
        holds -1 / -2.  A device tensor."""
        if self._rows is None:
            raise ValueError("nothing added yet")
        return _unit_costs(self._rows[0]) if self._costs is None else self._costs

    def statistics(self) -> Dict[str, Dict[str, EditStatistics]]:
        """language -> output -> accumulated ``EditStatistics`` (one host synchronisation)."""
        totals = self.totals.cpu().tolist()
        return {language: {name: EditStatistics(*totals[g][o]) for o, name in enumerate(self.names)}
                for g, language in enumerate(self.languages)}

    def results(self, evaluation_arguments: str = "") -> MultilingualEvaluationResults:
        """Upstream's ``evaluate`` output: every language, then ``"total"`` (one host synchronisation)."""
        return MultilingualEvaluationResults.from_statistics(evaluation_arguments, self.names, self.statistics())


def _unit_costs(statistics: Tensor) -> Tensor:
    """Under unit costs a path costs one per operation: I + D + S of [..., 4] statistics, NaN for rows flagged -1 / -2."""
    operations = statistics[..., :3].sum(-1).float()
    return torch.where(statistics[..., 0] >= 0, operations, torch.full_like(operations, float("nan")))


class _Pairs(NamedTuple):
    """Sequence pairs as one batch of the kernels: one id space, every id its own map entry."""
    tokens: Tensor  # int64 [1, N, 1, T]
    counts: Tensor  # int32 [1, N, 1]
    labels: Tensor  # the LabelBatch block
    maps: Tensor  # identity map: offsets V + 1 | values V
    descriptor: Tensor  # (0, V)
    V: int
    max_expected: int
    T: int
    symbols: List[Hashable]  # the id space: symbol of id v

    def rows(self) -> _EditRows:
        """One output, one group, the identity as both maps."""
        return _EditRows(self.tokens, self.counts, None, self.labels, self.tokens.shape[1], 1, self.maps, self.V + 1,
                         self.descriptor, self.descriptor, 1, self.max_expected, self.T)


def _pairs(expected: Sequence[Sequence[Hashable]], actual: Sequence[Sequence[Hashable]], device: torch.device) -> _Pairs:
    N = len(expected)
    space: Dict[Hashable, int] = {}
    label_ids = [_ids(space, e) for e in expected]
    hyp_ids = [_ids(space, a) for a in actual]
    longest = max(max(map(len, label_ids)), max(map(len, hyp_ids)))
    if longest > _lib.EDIT_MAX_LENGTH:
        raise ValueError(f"a sequence has {longest} symbols; the limit is {_lib.EDIT_MAX_LENGTH}")
    V = max(1, len(space))
    offsets = np.zeros(N + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(e) for e in label_ids])
    flat = np.asarray([i for e in label_ids for i in e], dtype=np.int32)
    block = np.concatenate([offsets, np.zeros(N, dtype=np.int32), flat])
    T = max(1, max(map(len, hyp_ids)))
    tokens = np.zeros((1, N, 1, T), dtype=np.int64)
    for n, a in enumerate(hyp_ids):
        tokens[0, n, 0, :len(a)] = a
    counts = np.asarray([len(a) for a in hyp_ids], dtype=np.int32).reshape(1, N, 1)
    identity = np.concatenate([np.arange(V + 1, dtype=np.int32), np.arange(V, dtype=np.int32)])  # entry e -> [e]
    descriptor = torch.tensor([0, V], dtype=torch.int32, device=device)
    return _Pairs(torch.from_numpy(tokens).to(device), torch.from_numpy(counts).to(device), torch.from_numpy(block).to(device),
                  torch.from_numpy(identity).to(device), descriptor, V, max(map(len, label_ids)), T, list(space))


def _pair_statistics(p: _Pairs, weights: Optional[_Weights] = None) -> List[EditStatistics]:
    totals = torch.zeros(1, 1, 4, dtype=torch.int64, device=p.tokens.device)
    statistics = _run(p.rows(), None, totals, weights)[0]
    return [EditStatistics(*row) for row in statistics.reshape(-1, 4).cpu().tolist()]


def _pair_operations(p: _Pairs, weights: Optional[_Weights] = None) -> List[Tuple[List[Operation], float]]:
    operations, counts, _, costs = _run_operations(p.rows(), None, weights)
    records, lengths = operations[0].cpu().numpy(), counts[0].cpu().tolist()
    costs = [float(length) for length in lengths] if costs is None else costs[0].cpu().tolist()  # unit costs: one per record
    return [([(Action(action), i, j) for action, i, j in records[n, :length, :3].tolist()], costs[n])
            for n, length in enumerate(lengths)]


def _pair_confusions(p: _Pairs, device: torch.device, weights: Optional[_Weights] = None, capacity: Optional[int] = None
                     ) -> Tuple[ConfusionCounts, Tensor]:
    """One confusion call over the pairs of ``p`` into a new table (by default large enough for every key the pairs can
    give); returns the accumulator and ``row_events`` int32 [1, N]."""
    if capacity is None:
        keys = min((p.V + 1) ** 2, int(p.counts.sum()) + p.labels.numel())  # distinct pairs; events
        capacity = 16
        while capacity < 2 * keys:
            capacity *= 2
    counts = ConfusionCounts(device, capacity, [TOTAL], ["pairs"], [p.symbols])
    return counts, counts.add_rows(p.rows(), None, weights)


def levensthein_statistics_batch(expected: Sequence[Sequence[Hashable]], actual: Sequence[Sequence[Hashable]],
                                 device=None) -> List[EditStatistics]:
    """``levensthein_statistics(expected[i], actual[i])`` for every pair, on the device (symbols compare by equality)."""
    if len(expected) != len(actual):
        raise ValueError("expected and actual differ in length")
    device = _device(device)
    return _pair_statistics(_pairs(expected, actual, device)) if len(expected) else []


def levensthein_statistics(expected: Sequence[Hashable], actual: Sequence[Hashable], device=None) -> EditStatistics:
    """Upstream's ``phonemes.levensthein_statistics(string_a=expected, string_b=actual)`` on the device."""
    return levensthein_statistics_batch([expected], [actual], device)[0]


def levensthein_operations_batch(expected: Sequence[Sequence[Hashable]], actual: Sequence[Sequence[Hashable]],
                                 device=None) -> List[Tuple[List[Operation], float]]:
    """``levensthein_operations(expected[i], actual[i])`` for every pair, on the device (symbols compare by equality)."""
    if len(expected) != len(actual):
        raise ValueError("expected and actual differ in length")
    device = _device(device)
    return _pair_operations(_pairs(expected, actual, device)) if len(expected) else []


def levensthein_confusions_batch(expected: Sequence[Sequence[Hashable]], actual: Sequence[Sequence[Hashable]],
                                 device=None) -> ConfusionTable:
    """The confusion table of the pairs (expected[i], actual[i]) under unit costs, on the device: one language (``"total"``)
    and one output (``"pairs"``), which ``ConfusionTable``'s methods default to."""
    if len(expected) != len(actual):
        raise ValueError("expected and actual differ in length")
    if len(expected) == 0:
        return ConfusionTable([TOTAL], ["pairs"], [[]], [], [], [], [], [])
    device = _device(device)
    return _pair_confusions(_pairs(expected, actual, device), device)[0].fetch()


def levensthein_operations(expected: Sequence[Hashable], actual: Sequence[Hashable], device=None
                           ) -> Tuple[List[Operation], float]:
    """Upstream's ``phonemes.levensthein_operations(string_a=expected, string_b=actual)`` on the device: the first best path's
    operations (action, i, j) in order, and the cost."""
    return levensthein_operations_batch([expected], [actual], device)[0]


def levensthein_substitutions(expected: Sequence[str], actual: Sequence[str], device=None) -> List[Substitution]:
    """Upstream's ``predictions.levensthein_substitutions``: ``to_substitutions`` of ``levensthein_operations``."""
    return to_substitutions(expected, actual, levensthein_operations(expected, actual, device)[0])


def _row(table, symbol) -> np.ndarray:
    """``table[symbol]`` as a 1-D array; ``KeyError`` naming the symbol when the table lacks it."""
    try:
        row = table[symbol]
    except (KeyError, IndexError, TypeError):
        raise KeyError(symbol) from None
    if isinstance(row, Tensor):
        row = row.detach().cpu().numpy()
    return np.asarray(row).reshape(-1)


class PropertyWeighting:
    """Upstream's ``allophant.phonemes.PropertyWeighting`` (edit_distance.rs:498-599) on the device: Levenshtein paths whose
    insertions and deletions cost ``insertion_cost`` / ``deletion_cost`` (fp32) and whose substitutions cost the number of
    positions in which ``property_table[a]`` and ``property_table[b]`` differ.  ``property_table`` is anything with
    ``__getitem__`` from a symbol to a 1-D row (tensor, array or list), e.g. ``AttributeTable.property_table()``.

    Upstream's first matrix row costs 1 per insertion whatever ``insertion_cost`` is; kept.  Beyond upstream: both costs must
    be finite and above 0, rows have one width of at most 255 columns, a column holds at most 256 distinct values, and a
    call compares at most 8192 distinct symbols (``ValueError``).  A symbol the table lacks raises ``KeyError``."""

    def __init__(self, insertion_cost: float, deletion_cost: float, property_table):
        self.insertion_cost = float(np.float32(insertion_cost))
        self.deletion_cost = float(np.float32(deletion_cost))
        for name, cost in (("insertion_cost", self.insertion_cost), ("deletion_cost", self.deletion_cost)):
            if not (np.isfinite(cost) and cost > 0):
                raise ValueError(f"{name} must be finite and above 0, not {cost}")
        if not hasattr(property_table, "__getitem__"):
            raise TypeError("property_table needs __getitem__")
        self.property_table = property_table

    def has(self, symbol) -> bool:
        try:
            _row(self.property_table, symbol)
        except KeyError:
            return False
        return True

    def codes(self, symbols: Sequence[Hashable]) -> np.ndarray:
        """The kernels' feature codes uint8 [V, F] of ``symbols``: per column the values numbered in order of first
        appearance (only equality matters)."""
        rows = [_row(self.property_table, s) for s in symbols]
        widths = {len(r) for r in rows}
        if len(widths) > 1:
            raise ValueError(f"property rows differ in width: {sorted(widths)}")
        F = widths.pop() if widths else 0
        if F > _lib.EDIT_MAX_FEATURES:
            raise ValueError(f"property rows have {F} columns; the limit is {_lib.EDIT_MAX_FEATURES}")
        if len(rows) > _lib.EDIT_MAX_SYMBOLS:
            raise ValueError(f"{len(rows)} distinct symbols; a cost table covers {_lib.EDIT_MAX_SYMBOLS}")
        codes = np.zeros((len(rows), F), dtype=np.uint8)
        for f in range(F):
            seen: Dict = {}
            for v, row in enumerate(rows):
                value = row[f].item()
                code = seen.setdefault(value, len(seen))
                if code > 255:
                    raise ValueError(f"property column {f} holds more than 256 distinct values")
                codes[v, f] = code
        return codes

    def cost_table(self, symbols: Sequence[Hashable], device: torch.device) -> Tensor:
        """The pairwise substitution costs uint8 [V * V] of ``symbols`` (ids in that order), built on the device."""
        codes = self.codes(symbols)
        V, F = codes.shape
        if V == 0:
            return torch.empty(0, dtype=torch.uint8, device=device)
        handle = _weighted_library()
        size = C.c_size_t()
        _lib.check(handle, None, handle.amx_edit_cost_table_bytes(V, C.byref(size)))
        table = torch.empty(size.value, dtype=torch.uint8, device=device)
        device_codes = torch.from_numpy(codes.reshape(-1)).to(device)
        with torch.cuda.device(device):
            code = handle.amx_edit_cost_table(device.index, _ptr(device_codes), V, F, _ptr(table),
                                              C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
        _lib.check(handle, None, code)
        return table

    def _prepare(self, expected, actual, device) -> Tuple[torch.device, "_Pairs", "_Weights"]:
        if len(expected) != len(actual):
            raise ValueError("expected and actual differ in length")
        symbols = list(dict.fromkeys(s for sequence in (*expected, *actual) for s in sequence))
        for s in symbols:  # KeyError before anything is launched
            _row(self.property_table, s)
        codes = self.codes(symbols)
        device = _device(device)
        p = _pairs(expected, actual, device)
        assert p.symbols == symbols
        table = self.cost_table(symbols, device)
        descriptors = torch.tensor([[0, len(symbols)]], dtype=torch.int64, device=device)
        return device, p, _Weights(self.insertion_cost, self.deletion_cost, descriptors, table if len(symbols) else None)

    def levensthein_statistics_batch(self, expected: Sequence[Sequence[Hashable]], actual: Sequence[Sequence[Hashable]],
                                     device=None) -> List[EditStatistics]:
        if len(expected) == 0 and len(actual) == 0:
            return []
        _, p, weights = self._prepare(expected, actual, device)
        return _pair_statistics(p, weights)

    def levensthein_statistics(self, expected: Sequence[Hashable], actual: Sequence[Hashable], device=None) -> EditStatistics:
        """Upstream's ``PropertyWeighting.levensthein_statistics(string_a=expected, string_b=actual)``."""
        return self.levensthein_statistics_batch([expected], [actual], device)[0]

    def levensthein_operations_batch(self, expected: Sequence[Sequence[Hashable]], actual: Sequence[Sequence[Hashable]],
                                     device=None) -> List[Tuple[List[Operation], float]]:
        if len(expected) == 0 and len(actual) == 0:
            return []
        _, p, weights = self._prepare(expected, actual, device)
        return _pair_operations(p, weights)

    def levensthein_operations(self, expected: Sequence[Hashable], actual: Sequence[Hashable], device=None
                               ) -> Tuple[List[Operation], float]:
        """Upstream's ``PropertyWeighting.levensthein_operations``: the first best path's operations (action, i, j) in order,
        and the fp32 cost."""
        return self.levensthein_operations_batch([expected], [actual], device)[0]

    def levensthein_confusions_batch(self, expected: Sequence[Sequence[Hashable]], actual: Sequence[Sequence[Hashable]],
                                     device=None) -> ConfusionTable:
        """The confusion table of the pairs on this weighting's paths (see the module-level function): a pair of different
        symbols with equal rows is a match of the path and an off-diagonal entry of the table."""
        if len(expected) == 0 and len(actual) == 0:
            return ConfusionTable([TOTAL], ["pairs"], [[]], [], [], [], [], [])
        device, p, weights = self._prepare(expected, actual, device)
        return _pair_confusions(p, device, weights)[0].fetch()

    def levensthein_matrix_batch(self, expected: Sequence[Sequence[Hashable]], actual: Sequence[Sequence[Hashable]],
                                 device=None) -> List[Tensor]:
        if len(expected) == 0 and len(actual) == 0:
            return []
        device, p, weights = self._prepare(expected, actual, device)
        return _matrices(device, expected, actual, p, weights)

    def levensthein_matrix(self, expected: Sequence[Hashable], actual: Sequence[Hashable], device=None) -> Tensor:
        """Upstream's ``PropertyWeighting.levensthein_matrix``: the (m + 1) x (n + 1) float32 cost matrix (a device tensor)."""
        return self.levensthein_matrix_batch([expected], [actual], device)[0]


def _matrices(device: torch.device, expected, actual, p: _Pairs, weights: _Weights) -> List[Tensor]:
    """One ``amx_edit_matrix`` call over the pairs of ``p``; each pair's (m + 1) x (n + 1) matrix."""
    handle = _weighted_library()
    N = len(expected)
    label_offsets = p.labels[:N + 1]
    actual_offsets = torch.zeros(N + 1, dtype=torch.int32, device=device)
    actual_offsets[1:] = torch.cumsum(p.counts.reshape(N), 0)
    # (one spare element: the buffer has an address even when every actual sequence is empty)
    actual_ids = torch.cat([p.tokens[0, n, 0, :len(a)] for n, a in enumerate(actual)] + [p.tokens.new_zeros(1)]).to(torch.int32)
    max_actual = max(map(len, actual))
    size = C.c_size_t()
    _lib.check(handle, None, handle.amx_edit_workspace(N, p.max_expected, max_actual, C.byref(size)))
    workspace = torch.empty(max(16, size.value), dtype=torch.uint8, device=device)
    matrix = torch.empty(N, p.max_expected + 1, max_actual + 1, dtype=torch.float32, device=device)
    status = torch.empty(N, dtype=torch.int32, device=device)
    V = int(weights.descriptors[0, 1]) if weights.data is not None else 0
    with torch.cuda.device(device):
        code = handle.amx_edit_matrix(
            device.index, _ptr(label_offsets), _ptr(p.labels, 2 * N + 1), _ptr(actual_offsets), _ptr(actual_ids), N,
            p.max_expected, max_actual, weights.insertion_cost, weights.deletion_cost, _ptr(weights.data), V, _ptr(workspace),
            workspace.numel(), _ptr(matrix), _ptr(status), C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    _lib.check(handle, None, code)
    if int(status.min()) < 0:
        raise RuntimeError("amx_edit_matrix flagged a row")
    return [matrix[n, :len(e) + 1, :len(a) + 1].clone() for n, (e, a) in enumerate(zip(expected, actual))]


def levensthein_matrix(expected: Sequence[Hashable], actual: Sequence[Hashable], device=None) -> Tensor:
    """Upstream's module-level ``phonemes.levensthein_matrix(string_a=expected, string_b=actual)``: unit costs, ``a != b``."""
    device = _device(device)
    p = _pairs([expected], [actual], device)
    weights = _Weights(1.0, 1.0, torch.zeros(1, 2, dtype=torch.int64, device=device), None)
    return _matrices(device, [expected], [actual], p, weights)[0]

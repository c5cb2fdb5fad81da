"""Confusion tables of evaluated batches: which phoneme is taken for which, what is deleted and inserted, and how often each
phoneme is right, per language and output.

``ConfusionCounts`` is the device half: a sparse table of (key, count) slots that the ``amx_edit_confusions`` kernel
(include/allophant_amx_edit.h) adds every aligned pair of the scored path to, matches included, and that lives on the device
across a corpus the way ``Evaluator.totals`` does.  ``ConfusionTable`` is the host half: the occupied slots decoded and
sorted, with the questions one asks of them (``pairs``, ``matrix``, ``statistics``, ``attribute_confusions``).

Epsilon -- the missing side of a deletion or an insertion -- is id -1 in the arrays and ``""`` among symbol strings, as
``to_substitutions`` writes it.
"""
from __future__ import annotations

import ctypes as C
import json
from typing import Dict, Hashable, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import lib as _lib

__all__ = ["ConfusionCounts", "ConfusionTable", "EPSILON"]

EPSILON = ""
KINDS = ("substitution", "deletion", "insertion", "correct")
_SYMBOL_BITS = _lib.EDIT_CONFUSION_SYMBOL_BITS
_SYMBOL_MASK = (1 << _SYMBOL_BITS) - 1


def _library():
    handle = _lib.load()
    if not hasattr(handle, "amx_edit_confusions"):
        raise RuntimeError("liballophant_amx.so lacks amx_edit_confusions: rebuild the library")
    return handle


def table_bytes(capacity: int) -> int:
    """``amx_edit_confusion_table_bytes``: ``ValueError`` unless ``capacity`` is a power of two from 16 to 2^28."""
    handle = _library()
    size = C.c_size_t()
    if handle.amx_edit_confusion_table_bytes(int(capacity), C.byref(size)) != 0:
        raise ValueError(f"a confusion table holds a power of two of 16 to 2^28 slots, not {capacity}")
    return size.value


def _ptr(t: Optional[Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class ConfusionTable:
    """The events of a corpus on the host: parallel int64 arrays ``group``, ``output``, ``expected``, ``actual``, ``count``,
    one entry per distinct (language index, output index, expected id, actual id), sorted by those four, epsilon as -1.
    ``languages`` and ``names`` label the first two, ``symbols[o][id]`` the ids of output ``o``."""

    def __init__(self, languages: Sequence[str], names: Sequence[str], symbols: Sequence[Sequence[Hashable]], group, output,
                 expected, actual, count):
        self.languages, self.names = list(languages), list(names)
        self.symbols = [list(s) for s in symbols]
        columns = [np.asarray(c, dtype=np.int64).reshape(-1) for c in (group, output, expected, actual, count)]
        if len({len(c) for c in columns}) != 1:
            raise ValueError("the columns of a confusion table differ in length")
        order = np.lexsort((columns[3], columns[2], columns[1], columns[0]))
        self.group, self.output, self.expected, self.actual, self.count = (c[order] for c in columns)
        if len(order) > 1:
            same = np.ones(len(order) - 1, dtype=bool)
            for c in (self.group, self.output, self.expected, self.actual):
                same &= c[1:] == c[:-1]
            if same.any():  # one entry per key: equal keys are summed
                first = np.concatenate([[True], ~same])
                sums = np.add.reduceat(self.count, np.flatnonzero(first))
                self.group, self.output, self.expected, self.actual = (c[first] for c in (self.group, self.output, self.expected, self.actual))
                self.count = sums
        if len(self.count):
            if self.group.min() < 0 or self.group.max() >= len(self.languages) or self.output.min() < 0 or self.output.max() >= len(self.names):
                raise ValueError("a confusion entry names a language or output outside the table's")
            if min(self.expected.min(), self.actual.min()) < -1:
                raise ValueError("a confusion entry holds a symbol id below -1")
            for o in range(len(self.names)):
                rows = self.output == o
                if rows.any() and max(self.expected[rows].max(), self.actual[rows].max()) >= len(self.symbols[o]):
                    raise ValueError(f"a confusion entry of output {self.names[o]!r} names a symbol outside its id space")

    # ------------------------------------------------------------------------------------------------------------------
    def _index(self, language, output) -> Tuple[int, int]:
        def find(value, values, what):
            if value is None:
                if len(values) != 1:
                    raise ValueError(f"name the {what}: the table has {len(values)}")
                return 0
            if isinstance(value, (int, np.integer)):  # an index, as `languages` of Evaluator.add may be
                if not 0 <= value < len(values):
                    raise KeyError(value)
                return int(value)
            try:
                return values.index(value)
            except ValueError:
                raise KeyError(value) from None
        return find(language, self.languages, "language"), find(output, self.names, "output")

    def _name(self, o: int, ident: int):
        return EPSILON if ident < 0 else self.symbols[o][ident]

    def _rows(self, g: int, o: int, kind: Optional[str] = None) -> np.ndarray:
        rows = (self.group == g) & (self.output == o)
        if kind is None:
            return rows
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS} or None, not {kind!r}")
        e, a = self.expected, self.actual
        if kind == "deletion":
            return rows & (e >= 0) & (a < 0)
        if kind == "insertion":
            return rows & (e < 0) & (a >= 0)
        both = rows & (e >= 0) & (a >= 0)
        return both & (e == a) if kind == "correct" else both & (e != a)

    def pairs(self, language=None, output=None, k: Optional[int] = None, kind: Optional[str] = "substitution"
              ) -> List[Tuple[Hashable, Hashable, int]]:
        """(expected symbol, actual symbol, count) of one language and output, most frequent first, ties by the symbols;
        ``kind`` keeps substitutions (different symbols), deletions, insertions or correct pairs, ``None`` all; ``k`` the
        first k."""
        g, o = self._index(language, output)
        rows = np.flatnonzero(self._rows(g, o, kind))
        found = [(self._name(o, int(self.expected[r])), self._name(o, int(self.actual[r])), int(self.count[r])) for r in rows]
        found.sort(key=lambda t: (-t[2], str(t[0]), str(t[1])))
        return found if k is None else found[:k]

    def matrix(self, language=None, output=None) -> Tuple[List[Hashable], np.ndarray]:
        """(symbols, counts): the symbols that occur on either side in id order, epsilon (``""``) last, and int64
        counts[expected, actual] over them (the last row insertions, the last column deletions)."""
        g, o = self._index(language, output)
        rows = self._rows(g, o)
        e, a, c = self.expected[rows], self.actual[rows], self.count[rows]
        ids = np.unique(np.concatenate([e, a]))
        ids = ids[ids >= 0]
        position = {int(v): p for p, v in enumerate(ids)}
        position[-1] = len(ids)
        counts = np.zeros((len(ids) + 1, len(ids) + 1), dtype=np.int64)
        for x, y, v in zip(e.tolist(), a.tolist(), c.tolist()):
            counts[position[x], position[y]] += v
        return [self.symbols[o][int(v)] for v in ids] + [EPSILON], counts

    def statistics(self, weighting=None):
        """language -> output -> the ``EditStatistics`` that the events imply.  Different symbols are substitutions; with a
        ``weighting`` (``PropertyWeighting``) those whose property rows are equal are correct, as its costs score them."""
        from .evaluation import EditStatistics

        result = {}
        for g, language in enumerate(self.languages):
            per_output = {}
            for o, name in enumerate(self.names):
                sums = {kind: int(self.count[self._rows(g, o, kind)].sum()) for kind in KINDS}
                if weighting is not None:
                    for r in np.flatnonzero(self._rows(g, o, "substitution")):
                        pair = [self.symbols[o][int(self.expected[r])], self.symbols[o][int(self.actual[r])]]
                        if not all(weighting.has(s) for s in pair):  # (an attribute output: scored under unit costs)
                            continue
                        codes = weighting.codes(pair)
                        if (codes[0] == codes[1]).all():
                            sums["substitution"] -= int(self.count[r])
                            sums["correct"] += int(self.count[r])
                per_output[name] = EditStatistics(sums["insertion"], sums["deletion"], sums["substitution"], sums["correct"])
            result[language] = per_output
        return result

    def attribute_confusions(self, table, language=None, output=None) -> Dict[str, Tuple[List[str], np.ndarray]]:
        """Per feature column of ``table`` (an ``AttributeTable``): (values, counts), the phoneme pairs of one language and
        output projected through the phonemes' feature rows -- counts[expected value, actual value] over the values that
        occur, a contour written as its categories joined by ``","``.  Host arithmetic; deletions and insertions have no
        second phoneme and are left out.  ``ValueError`` for a symbol that the table lacks."""
        g, o = self._index(language, output)
        rows = np.flatnonzero(self._rows(g, o) & (self.expected >= 0) & (self.actual >= 0))
        known = set(table.full_phonemes)
        used = sorted({int(v) for v in self.expected[rows]} | {int(v) for v in self.actual[rows]})
        missing = [self.symbols[o][v] for v in used if self.symbols[o][v] not in known]
        if missing:
            raise ValueError(f"the attribute table lacks the symbols {missing}")
        result = {}
        for feature in table.full_feature_names:
            value = {v: ",".join(table.feature_contour(self.symbols[o][v], feature)) for v in used}
            values = sorted(set(value.values()))
            position = {v: p for p, v in enumerate(values)}
            counts = np.zeros((len(values), len(values)), dtype=np.int64)
            for r in rows:
                counts[position[value[int(self.expected[r])]], position[value[int(self.actual[r])]]] += int(self.count[r])
            result[feature] = (values, counts)
        return result

    # ------------------------------------------------------------------------------------------------------------------
    def total(self) -> int:
        return int(self.count.sum())

    def entries(self) -> List[Tuple[int, int, int, int, int]]:
        return list(zip(*(c.tolist() for c in (self.group, self.output, self.expected, self.actual, self.count))))

    def __len__(self) -> int:
        return len(self.count)

    def __eq__(self, other) -> bool:
        if not isinstance(other, ConfusionTable):
            return NotImplemented
        return (self.languages, self.names, self.symbols, self.entries()) == (other.languages, other.names, other.symbols,
                                                                              other.entries())

    def __add__(self, other: "ConfusionTable") -> "ConfusionTable":
        """The events of both tables; they must share languages, outputs and id spaces."""
        if not isinstance(other, ConfusionTable):
            return NotImplemented
        if (self.languages, self.names, self.symbols) != (other.languages, other.names, other.symbols):
            raise ValueError("confusion tables over different languages, outputs or id spaces do not add")
        columns = [np.concatenate([x, y]) for x, y in zip((self.group, self.output, self.expected, self.actual, self.count),
                                                          (other.group, other.output, other.expected, other.actual, other.count))]
        return ConfusionTable(self.languages, self.names, self.symbols, *columns)

    def to_dict(self) -> Dict:
        return {"languages": list(self.languages), "outputs": list(self.names), "symbols": [list(s) for s in self.symbols],
                "entries": [list(e) for e in self.entries()]}

    @classmethod
    def from_dict(cls, value: Dict) -> "ConfusionTable":
        entries = np.asarray(value["entries"], dtype=np.int64).reshape(-1, 5)
        return cls(value["languages"], value["outputs"], value["symbols"], *(entries[:, c] for c in range(5)))

    def dumps(self) -> str:
        return json.dumps(self.to_dict())

    @classmethod
    def loads(cls, text: str) -> "ConfusionTable":
        return cls.from_dict(json.loads(text))


class ConfusionCounts:
    """The device accumulator: ``capacity`` (key, count) slots (a power of two, 16 to 2^28) and the two counters (events
    added, events dropped) of include/allophant_amx_edit.h.  ``languages``, ``names`` and ``symbols`` (per output, the symbol
    of each id) label what ``fetch`` returns; ``names`` also fixes the number of outputs that the keys are decoded with."""

    def __init__(self, device=None, capacity: int = 2 ** 20, languages: Optional[Sequence[str]] = None,
                 names: Optional[Sequence[str]] = None, symbols: Optional[Sequence[Sequence[Hashable]]] = None):
        device = torch.device(device if device is not None else "cuda")
        if device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("confusion tables are counted on the MI355X: there is no CPU path")
        self.device = device if device.index is not None else torch.device("cuda", torch.cuda.current_device())
        self.languages = None if languages is None else list(languages)
        self.names = None if names is None else list(names)
        self.symbols = None if symbols is None else [list(s) for s in symbols]
        self.table = self._new_table(capacity)
        self.counters = torch.zeros(2, dtype=torch.int64, device=self.device)  # (uint64 on the device; far below 2^63)
        self._workspace: Optional[Tensor] = None
        self._shape: Optional[Tuple[int, int]] = None  # (groups, outputs) of the keys, fixed by the first rows added

    def _new_table(self, capacity: int) -> Tensor:
        assert table_bytes(capacity) == capacity * 16
        return torch.zeros(capacity, 2, dtype=torch.int64, device=self.device)

    @property
    def capacity(self) -> int:
        return self.table.shape[0]

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def add_rows(self, rows, best: Optional[Tensor] = None, weights=None) -> Tensor:
        """One ``amx_edit_confusions`` call (with ``weights``: ``amx_edit_weighted_confusions``) over ``rows``, the
        ``evaluation._EditRows`` that the statistics were computed on, for the candidates ``best`` int32 [O, N] (None:
        candidate 0).  Returns ``row_events`` int32 [O, N].  Stream-ordered: nothing waits for the device."""
        handle = _library()
        rows = rows.unit_stride()
        O, N, _, _ = rows.tokens.shape
        G = rows.G
        if self.names is not None and len(self.names) != O:
            raise ValueError(f"{O} outputs for a table over {len(self.names)}")
        if self.languages is not None and len(self.languages) != G:
            raise ValueError(f"{G} groups for a table over {len(self.languages)} languages")
        if self._shape not in (None, (G, O)):
            raise ValueError(f"{G} groups x {O} outputs added to a table over {self._shape}")
        self._shape = (G, O)
        self._workspace = rows.workspace(True, self._workspace)
        row_events = torch.empty(O, N, dtype=torch.int32, device=self.device)
        head = rows.head(self._workspace)
        tail = (_ptr(best), _ptr(self.table), self.capacity, _ptr(row_events), _ptr(self.counters), self._stream())
        with torch.cuda.device(self.device):
            if weights is None:
                code = handle.amx_edit_confusions(*head, *tail)
            else:
                code = handle.amx_edit_weighted_confusions(*head, weights.insertion_cost, weights.deletion_cost,
                                                           _ptr(weights.descriptors), _ptr(weights.data), *tail)
        _lib.check(handle, None, code)
        return row_events

    def _merge_from(self, src: Tensor) -> None:
        handle = _library()
        with torch.cuda.device(self.device):
            code = handle.amx_edit_confusion_merge(self.device.index, _ptr(src), src.shape[0], _ptr(self.table), self.capacity,
                                                   _ptr(self.counters), self._stream())
        _lib.check(handle, None, code)

    def grow(self, capacity: int) -> None:
        """Moves every entry into a new table of ``capacity`` slots (stream-ordered).  A smaller table than the entries need
        counts the rest as dropped."""
        old, dropped = self.table, self.counters[1].clone()
        self.table = self._new_table(capacity)
        self.counters.zero_()
        self._merge_from(old)
        self.counters[1] += dropped

    def merge(self, other: "ConfusionCounts") -> None:
        """Adds ``other``'s events to this table (same device, same groups and outputs)."""
        if other is self or other.device != self.device:
            raise ValueError("a table merges with another table on its device")
        if None not in (self._shape, other._shape) and self._shape != other._shape:
            raise ValueError(f"tables over {other._shape} and {self._shape} (groups, outputs) do not merge")
        self._shape = self._shape or other._shape
        self._merge_from(other.table)
        self.counters[1] += other.counters[1]

    def reset(self) -> None:
        self.table.zero_()
        self.counters.zero_()

    def events(self) -> Tuple[int, int]:
        """(events added, events dropped) so far (one host synchronisation)."""
        added, dropped = self.counters.cpu().tolist()
        return added, dropped

    def raw(self) -> Tuple[np.ndarray, np.ndarray]:
        """The occupied slots, sorted by key: (keys uint64, counts uint64) on the host (one host synchronisation).  Sorted,
        a table is bitwise reproducible; slot positions are not."""
        occupied = self.table[self.table[:, 0] != 0].cpu().numpy()
        keys, counts = occupied[:, 0].view(np.uint64), occupied[:, 1].view(np.uint64)
        order = np.argsort(keys, kind="stable")
        return keys[order], counts[order]

    def fetch(self) -> ConfusionTable:
        """The table on the host (one host synchronisation).  ``OverflowError`` naming the count if any event was dropped:
        dropped events are lost, so the table would be silently partial (``grow`` before adding, or start over larger)."""
        added, dropped = self.events()
        if dropped:
            raise OverflowError(f"{dropped} events found no slot in a confusion table of {self.capacity} slots "
                                f"({added} were added): they are lost")
        keys, counts = self.raw()
        G, O = self._shape or (len(self.languages or [None]), len(self.names or [None]))
        slot = (keys >> np.uint64(2 * _SYMBOL_BITS)).astype(np.int64) - 1
        expected = ((keys >> np.uint64(_SYMBOL_BITS)) & np.uint64(_SYMBOL_MASK)).astype(np.int64) - 1
        actual = (keys & np.uint64(_SYMBOL_MASK)).astype(np.int64) - 1
        languages = self.languages if self.languages is not None else [str(g) for g in range(G)]
        names = self.names if self.names is not None else [str(o) for o in range(O)]
        symbols = self.symbols
        if symbols is None:
            top = int(max(expected.max(initial=-1), actual.max(initial=-1))) + 1
            symbols = [[str(v) for v in range(top)] for _ in names]
        return ConfusionTable(languages, names, symbols, slot // O, slot % O, expected, actual, counts.astype(np.int64))

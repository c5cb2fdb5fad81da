"""Per-utterance phoneme inventories for models with the embedding-composition head.

Upstream predicts such a model under ONE inventory per call and therefore splits every batch by language
(``_filter_split_raw_batches_by_language``, one ``feature_matrix`` per batch: reference run.py:712-713, 742-753).  A composed
phoneme's logit depends on its own feature row only (acoustic_model.py:219-234), so one pass under the UNION of the languages'
inventories holds every language's logits; ``Estimator.predict_languages`` runs that pass and restricts each utterance's
composed output to its own language on the device (``amx_restrict_outputs``).  ``LanguageInventories`` is the host side: the
union, each language's place in it, and the membership bit table the kernel reads.

Two index spaces: the UNION space (class 0 the blank, class ``1 + u`` the union's u-th phoneme), which the predictions and
every decoder on them speak, and upstream's PER-LANGUAGE space (class 0 the blank, class ``1 + j`` the j-th phoneme of the
language's own inventory).  ``columns(language)[j]`` is the union class of the language's class ``j``.

Out of scope: a restriction fused into the forward pass, a grouped per-language GEMM, the data-parallel gather of such
predictions and a compact per-language layout in the C ABI.
"""
from __future__ import annotations

from typing import Dict, List, Mapping, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from .phonetic import BLANK_OFFSET, AttributeTable


class LanguageInventories:
    """The union of several languages' phoneme inventories (the ``language_inventories`` of reference run.py:686-693) and each
    language's columns in it.  Built by ``from_matrices`` or ``from_table``.

    ``languages``: the names, in order (an utterance's dense language id indexes them); ``union_tfi``: int64 ``[U, F]``, the
    ``target_feature_indices`` of the union pass, whose composed output has ``U + 1`` classes with the blank at column 0;
    ``union_symbols``: the union's phonemes where a table was given, else ``None``; ``bits``: the host membership table,
    uint64 ``[languages, (U + 1 + 63) // 64]`` (bit ``c % 64`` of word ``c // 64``: class ``c`` belongs to the language; the blank
    belongs to all)."""

    def __init__(self, languages: Sequence[str], union_tfi: Tensor, rows: Sequence[Sequence[int]],
                 union_symbols: Optional[Sequence[str]] = None):
        self.languages: List[str] = list(languages)
        if not self.languages:
            raise ValueError("at least one language is needed")
        if len(set(self.languages)) != len(self.languages):
            raise ValueError("a language is listed twice")
        self.union_tfi = union_tfi.detach().to("cpu", torch.int64).contiguous()
        self.union_symbols: Optional[List[str]] = None if union_symbols is None else list(union_symbols)
        self._index = {language: i for i, language in enumerate(self.languages)}
        classes = self.classes
        self._columns: List[Tensor] = []
        self._inverse: List[Tensor] = []
        self.bits = np.zeros((len(self.languages), (classes + 63) // 64), dtype=np.uint64)
        for i, own in enumerate(rows):
            columns = torch.tensor([0] + [BLANK_OFFSET + int(u) for u in own], dtype=torch.int64)
            inverse = torch.full((classes,), -1, dtype=torch.int64)
            inverse[columns] = torch.arange(columns.numel())
            self._columns.append(columns)
            self._inverse.append(inverse)
            for c in columns.tolist():
                self.bits[i, c // 64] |= np.uint64(1) << np.uint64(c % 64)
        self._device_bits: Dict[torch.device, Tensor] = {}

    # -- construction ------------------------------------------------------------------------------------------------
    @classmethod
    def from_matrices(cls, matrices: Mapping[str, Tensor]) -> "LanguageInventories":
        """From ``{language: target_feature_indices [P_l, F]}``, each what upstream's per-language ``predict`` takes.  The union
        holds the distinct rows in order of first appearance; a row listed twice within a language raises, and so does an
        ``F`` that differs between languages.  An empty language (``[0, F]``) is allowed: it has the blank only."""
        if not matrices:
            raise ValueError("at least one language is needed")
        width = None
        union: Dict[tuple, int] = {}
        rows: List[List[int]] = []
        for language, tfi in matrices.items():
            tfi = torch.as_tensor(tfi)
            if tfi.dim() != 2:
                raise ValueError(f"language {language!r}: target_feature_indices must be [phones, features]")
            if width is None:
                width = tfi.shape[1]
            elif tfi.shape[1] != width:
                raise ValueError(f"language {language!r} has {tfi.shape[1]} features, the languages before it {width}")
            own: List[int] = []
            seen = set()
            for j, row in enumerate(tfi.to("cpu", torch.int64).tolist()):
                key = tuple(row)
                if key in seen:
                    raise ValueError(f"language {language!r} lists the phoneme of row {j} twice")
                seen.add(key)
                own.append(union.setdefault(key, len(union)))
            rows.append(own)
        union_tfi = torch.tensor(list(union), dtype=torch.int64).reshape(len(union), width)
        return cls(list(matrices), union_tfi, rows)

    @classmethod
    def from_table(cls, table: AttributeTable, inventories: Mapping[str, Sequence[str]]) -> "LanguageInventories":
        """From an ``AttributeTable`` and ``{language: [phoneme, ...]}``.  The union holds the distinct symbols in order of
        first appearance, one column each (two symbols with equal feature rows keep a column each); a symbol listed twice within
        a language raises, a symbol the table lacks raises like ``composition_feature_matrix``."""
        if not inventories:
            raise ValueError("at least one language is needed")
        union: Dict[str, int] = {}
        rows: List[List[int]] = []
        for language, inventory in inventories.items():
            inventory = list(inventory)
            duplicates = sorted({p for p in inventory if inventory.count(p) > 1})
            if duplicates:
                raise ValueError(f"language {language!r} lists {duplicates} twice")
            rows.append([union.setdefault(p, len(union)) for p in inventory])
        return cls(list(inventories), table.composition_feature_matrix(list(union)), rows, list(union))

    # -- the two index spaces ------------------------------------------------------------------------------------------
    @property
    def classes(self) -> int:
        """Classes of the union pass's composed output: the union's phonemes and the blank."""
        return self.union_tfi.shape[0] + BLANK_OFFSET

    def index(self, language: Union[str, int]) -> int:
        """The dense id of a language name (an id in range is returned as it is)."""
        if isinstance(language, str):
            if language not in self._index:
                raise ValueError(f"unknown language {language!r}; the inventories hold {self.languages}")
            return self._index[language]
        if not 0 <= int(language) < len(self.languages):
            raise IndexError(f"language id {int(language)} outside the {len(self.languages)} languages")
        return int(language)

    def language_ids(self, languages) -> Tensor:
        """One dense id per utterance (host int32) from names, ids or a tensor of ids, each checked."""
        if isinstance(languages, Tensor):
            languages = languages.detach().cpu().tolist()
        return torch.tensor([self.index(language) for language in languages], dtype=torch.int32)

    def columns(self, language: Union[str, int]) -> Tensor:
        """int64 ``[P_l + 1]``: the union class of the language's j-th class, the blank first (upstream's per-language index
        space in, union space out)."""
        return self._columns[self.index(language)]

    def symbols(self, language: Union[str, int]) -> List[str]:
        """The language's inventory as given to ``from_table``."""
        if self.union_symbols is None:
            raise ValueError("these inventories were built from matrices: they know no symbols")
        return [self.union_symbols[c - BLANK_OFFSET] for c in self.columns(language).tolist()[1:]]

    def tfi(self, language: Union[str, int]) -> Tensor:
        """The language's own ``target_feature_indices``, what upstream's per-language ``predict`` takes."""
        return self.union_tfi[self.columns(language)[1:] - BLANK_OFFSET]

    def to_language_indices(self, tokens, language: Union[str, int]):
        """Union token ids -> upstream's per-language ids (a tensor gives an int64 tensor on its device, anything else a
        list).  A token outside the language raises."""
        inverse = self._inverse[self.index(language)]
        return self._map(tokens, inverse, f"a class outside the inventory of {self.languages[self.index(language)]!r}")

    def from_language_indices(self, tokens, language: Union[str, int]):
        """Upstream's per-language ids -> union token ids, e.g. for targets written in a language's own space."""
        return self._map(tokens, self.columns(language), "an id outside the language's classes")

    @staticmethod
    def _map(tokens, table: Tensor, complaint: str):
        as_tensor = isinstance(tokens, Tensor)
        ids = tokens.detach().to("cpu", torch.int64) if as_tensor else torch.tensor([int(t) for t in tokens], dtype=torch.int64)
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= table.numel()):
            raise ValueError(f"tokens hold {complaint}")
        mapped = table[ids]
        if mapped.numel() and int(mapped.min()) < 0:
            raise ValueError(f"tokens hold {complaint}")
        return mapped.to(tokens.device) if as_tensor else mapped.tolist()

    # -- what the kernel reads -------------------------------------------------------------------------------------------
    def device_bits(self, device) -> Tensor:
        """``bits`` on ``device`` (its 64-bit words as an int64 tensor), uploaded once per device."""
        device = torch.device(device)
        if device not in self._device_bits:
            self._device_bits[device] = torch.from_numpy(self.bits.view(np.int64).copy()).to(device)
        return self._device_bits[device]

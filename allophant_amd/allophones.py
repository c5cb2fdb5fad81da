"""Structure of the allophone layer (reference ``AllophoneMapping.__init__``, allophant/network/acoustic_model.py:105-136).

A ``LanguageAllophoneMappings`` dump (``allophones``: language index -> {phoneme index: [shared phone indices]},
``languages``, ``shared_phones``; phonetic_features.py:40-44) determines, per language, which (phone, phoneme) pairs of
the ``[P+1, Q+1]`` allophone matrix the layer may use.  Upstream keeps that structure in two non-persistent buffers built at
construction -- ``_initialization`` (the 0 / 1 matrix) and ``_allophone_mask`` (its complement) -- and an ``index_map`` from
language code to matrix index; the trained values are the ``_allophone_matrices`` parameter of the state dict.  This module
rebuilds the three from the dump alone, bitwise as upstream does:

* the matrix index of a language follows the iteration order of ``allophones`` (``enumerate(allophones.items())``), not the
  language index;
* every language listed in ``allophones`` gets the blank diagonal ``[0, 0] = 1`` (blank offset 1) and
  ``[allophone + 1, phoneme + 1] = 1`` for each of its ``phoneme -> [allophones]``;
* a language of ``languages`` without an entry in ``allophones`` leaves an all-zero matrix (everything masked, even blank).

Keys may be ints or, in a mapping that went through JSON, strings (``"0"``), as ``phonetic.AttributeTable._restrict``
accepts them.  Indices outside the matrix raise ``ValueError`` (upstream would index a wrong row or fail inside torch).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, Mapping

import torch
from torch import Tensor

BLANK_OFFSET = 1


@dataclass
class AllophoneStructure:
    """``initialization`` fp32 ``[L, P+1, Q+1]`` (upstream ``_initialization``), ``mask`` bool ``[L, P+1, Q+1]`` (upstream
    ``_allophone_mask``: True = masked), ``index_map`` language code -> matrix index (upstream ``index_map``)."""

    initialization: Tensor
    mask: Tensor
    index_map: Dict[str, int]


def _index(key: Any, what: str) -> int:
    if isinstance(key, bool):
        raise ValueError(f"{what} index must be an integer, got {key!r}")
    if isinstance(key, int):
        return key
    if isinstance(key, str):
        try:
            return int(key)
        except ValueError:
            pass
    raise ValueError(f"{what} index must be an integer, got {key!r}")


def _field(mapping: Any, name: str):
    if isinstance(mapping, Mapping):
        if name not in mapping:
            raise ValueError(f"language_allophones lacks {name!r}")
        return mapping[name]
    if not hasattr(mapping, name):
        raise ValueError(f"language_allophones lacks {name!r}")
    return getattr(mapping, name)


def build_structure(language_allophones: Any, shared_phone_count: int, phoneme_count: int) -> AllophoneStructure:
    """Structure of ``AllophoneMapping(shared_phone_count, phoneme_count, 1, language_allophones)``: both counts include the
    blank (P+1 phones, Q+1 phonemes), as upstream passes them (acoustic_model.py:451-457).  ``language_allophones`` is a
    ``LanguageAllophoneMappings`` object or its dict dump."""
    allophones = _field(language_allophones, "allophones")
    languages = list(_field(language_allophones, "languages"))
    if not isinstance(allophones, Mapping):
        raise ValueError("language_allophones.allophones must map language indices to {phoneme: [allophones]}")
    P1, Q1 = int(shared_phone_count), int(phoneme_count)
    if P1 < BLANK_OFFSET or Q1 < BLANK_OFFSET:
        raise ValueError("the allophone matrices need room for the blank")
    n_lang = len(languages)
    if len(allophones) > n_lang:
        raise ValueError(f"language_allophones maps {len(allophones)} languages, but lists {n_lang}")
    matrix = torch.zeros(n_lang, P1, Q1)
    index_map: Dict[str, int] = {}
    for dense, (language_key, per_language) in enumerate(allophones.items()):
        language = _index(language_key, "language")
        if not 0 <= language < n_lang:
            raise ValueError(f"language index {language_key!r} outside the {n_lang} languages")
        if not isinstance(per_language, Mapping):
            raise ValueError(f"allophones of language {language_key!r} must map phonemes to lists of allophones")
        language_matrix = matrix[dense]
        language_matrix[:BLANK_OFFSET, :BLANK_OFFSET].fill_diagonal_(1)
        index_map[languages[language]] = dense
        for phoneme_key, phones in per_language.items():
            phoneme = _index(phoneme_key, "phoneme")
            if not 0 <= phoneme < Q1 - BLANK_OFFSET:
                raise ValueError(f"phoneme index {phoneme_key!r} outside the {Q1 - BLANK_OFFSET} phonemes of the model")
            if isinstance(phones, (str, bytes)) or not hasattr(phones, "__iter__"):
                raise ValueError(f"allophones of phoneme {phoneme_key!r} must be a list of shared phone indices")
            for phone_key in phones:
                phone = _index(phone_key, "shared phone")
                if not 0 <= phone < P1 - BLANK_OFFSET:
                    raise ValueError(f"shared phone index {phone_key!r} outside the {P1 - BLANK_OFFSET} shared phones of the model")
                language_matrix[phone + BLANK_OFFSET, phoneme + BLANK_OFFSET] = 1
    return AllophoneStructure(matrix, ~matrix.bool(), index_map)

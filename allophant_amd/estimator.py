"""Drop-in façade over ``liballophant_amx``: the reference's ``Estimator`` / ``Batch`` / ``Predictions`` names, shapes and
error behaviour for the prediction path.

Mirrors (reference file:line):
  * ``Batch``                allophant/dataset_processing.py:49-85
  * ``Predictions``          allophant/network/acoustic_model.py:908-926
  * ``Estimator.predict``    allophant/estimator.py:1035-1046
  * ``Estimator.restore``    allophant/estimator.py:1085-1126 (checkpoint dict schema estimator.py:199-249)
  * ``GreedyCTCDecoder``     allophant/predictions.py:189-207
  * ``BeamCTCDecoder``, ``_ctc_decoder``, ``feature_decoders``  allophant/predictions.py:210-254
  * ``Estimator.map_allophones``  allophant/estimator.py:1048-1049 -> AllophoneMapping.map_allophones
                             (allophant/network/acoustic_model.py:142-159)
  * ``Estimator.sample_rate``  allophant/estimator.py:940; ``Estimator.resample`` applies ``resample.resample_batch``

PyTorch is used only as plumbing (device memory for inputs/outputs, the current HIP stream); all arithmetic happens in the
HIP kernels behind the C ABI.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from dataclasses import dataclass
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import alignment as _alignment
from . import ctc as _ctc
from . import graph_alignment as _graph_alignment
from . import lib as _lib
from . import phonotactics as _phonotactics
from . import scoring as _scoring
from . import search as _search
from . import spec as _spec
from . import variants as _variants
from .alignment import Aligned, Alignment, ctc_forced_align, label_targets, segments  # noqa: F401  (the façade's names)
from .graph_alignment import (GraphAligned, GraphAlignment, TargetGraph, ctc_graph_align,  # noqa: F401  (the façade's graph names)
                              slot_targets)
from .scoring import Rescored, Score, Scored, ctc_score  # noqa: F401  (the façade's scoring names)
from .search import Found, Hit, ctc_search, pick_hits, query_targets  # noqa: F401  (the façade's search names)
from .phonotactics import PhonotacticLM  # noqa: F401  (the façade's language-model name)
from .variants import Alternatives, Variants, ctc_variants  # noqa: F401  (the façade's variant names)


@dataclass
class Batch:
    """``Batch(audio_features [N, L] f32 zero right-padded, lengths [N] i64 samples, language_ids [N])``."""

    audio_features: Tensor
    lengths: Tensor
    language_ids: Tensor

    def pin_memory(self):
        self.audio_features = self.audio_features.pin_memory()
        self.lengths = self.lengths.pin_memory()
        self.language_ids = self.language_ids.pin_memory()
        return self

    def to(self, device, non_blocking: bool = False, copy: bool = False):
        moved = self.__class__(
            self.audio_features.to(device, non_blocking=non_blocking, copy=copy),
            self.lengths.to(device, non_blocking=non_blocking, copy=copy),
            self.language_ids.to(device, non_blocking=non_blocking, copy=copy),
        )
        if getattr(self, "_padded", False):
            moved._padded = True  # a slice of a larger batch (parallel.shard_batch(keep_length=True)): L may exceed max(lengths)
        slot = getattr(self, "_pinned_slot", None)
        if slot is not None:
            if moved.audio_features.device.type == "cuda" and non_blocking:
                # an asynchronous copy out of a `batching.PinnedCollator` slot: the collator refills the slot only behind
                # this event
                event = torch.cuda.Event()
                event.record(torch.cuda.current_stream(moved.audio_features.device))
                slot[0].mark_in_flight(self, event)
            elif moved.audio_features.data_ptr() == self.audio_features.data_ptr():
                moved._pinned_slot = slot  # same storage (a no-op move): still the collator's slot
        return moved

    def cuda(self, non_blocking: bool = False, copy: bool = False):
        return self.to("cuda", non_blocking, copy)

    def size(self) -> int:
        return len(self)

    def __len__(self) -> int:
        return self.lengths.numel()

    def __repr__(self) -> str:
        return "{}(Features: ({}; {}))".format(self.__class__.__name__, self.audio_features.shape, self.audio_features.dtype)


@dataclass
class Predictions:
    """``outputs``: name -> [T, N, C] (log-)probabilities, time-major; ``lengths``: [N] int64 output frames."""

    outputs: Dict[str, Tensor]
    lengths: Tensor
    # flat device buffer the outputs are views of (kept for the on-device greedy decoder); not part of the reference API
    _flat: Optional[Tensor] = dataclasses.field(default=None, repr=False, compare=False)
    _geometry: Optional[Tuple[int, int]] = dataclasses.field(default=None, repr=False, compare=False)
    # the `target_feature_indices` the outputs were computed under (their phoneme block is that many phones wide)
    _inventory: Optional[Tensor] = dataclasses.field(default=None, repr=False, compare=False)
    # assembled by parallel.gather_flat_predictions: one status word per rank (device tensor; non-zero = that rank reported a
    # range error -- AMX_ERANGE -- with its shard).  Left on the device so that the gather never synchronises the host.
    _status: Optional[Tensor] = dataclasses.field(default=None, repr=False, compare=False)
    # set by Estimator.predict_languages: (int32 device language id per utterance, the LanguageInventories); the composed
    # output is then the union inventory's, each utterance restricted to its own language (-inf elsewhere)
    _languages: Optional[Tuple[Tensor, Any]] = dataclasses.field(default=None, repr=False, compare=False)

    def __len__(self) -> int:
        return len(self.lengths)

    def check_ranks(self) -> None:
        """Data-parallel predictions only: raises ``FloatingPointError`` if a rank reported activations beyond the range of the
        planes with the shard it contributed (reads one small tensor back: call it where the host reads the results anyway)."""
        if self._status is not None:
            bad = [r for r, st in enumerate(self._status.tolist()) if st]
            if bad:
                raise FloatingPointError(f"rank(s) {bad} reported a range error (AMX_ERANGE) with their shard of this batch")

    def task_count(self) -> int:
        return len(self.outputs)


class CTCHypothesis(NamedTuple):
    """Field-compatible with ``torchaudio.models.decoder.CTCHypothesis`` as used by the reference decoder."""

    tokens: Tensor
    words: List[str]
    score: float
    timesteps: Tensor


class Decoded(NamedTuple):
    """Greedy CTC alignments of a batch, one row per output: ``tokens`` / ``timesteps`` ``[O, N, T]`` int64 of which the
    first ``counts[o, n]`` entries are valid, ``counts`` ``[O, N]`` int32, ``scores`` ``[O, N]`` fp32 (sum of the per-frame
    maxima, predictions.py:205).  Device tensors when produced by ``Estimator.greedy_decode_device``."""
    names: List[str]
    tokens: Tensor
    timesteps: Tensor
    counts: Tensor
    scores: Tensor

    def select(self, names: List[str]) -> "Decoded":
        rows = [self.names.index(name) for name in names]
        index = torch.tensor(rows, dtype=torch.long, device=self.tokens.device)
        return Decoded(list(names), self.tokens.index_select(0, index), self.timesteps.index_select(0, index),
                       self.counts.index_select(0, index), self.scores.index_select(0, index))

    def hypotheses(self) -> Dict[str, List[List[CTCHypothesis]]]:
        """Host form: per output and utterance ``[CTCHypothesis(tokens, [], score, timesteps)]`` like the reference."""
        counts_h, scores_h = self.counts.cpu(), self.scores.cpu()
        tokens_h, timesteps_h = self.tokens.cpu(), self.timesteps.cpu()
        result: Dict[str, List[List[CTCHypothesis]]] = {}
        for o, name in enumerate(self.names):
            hyps = []
            for n in range(counts_h.shape[1]):
                k = int(counts_h[o, n])
                hyps.append([CTCHypothesis(tokens_h[o, n, :k].clone(), [], float(scores_h[o, n]), timesteps_h[o, n, :k].clone())])
            result[name] = hyps
        return result



def _beam_hypotheses(tokens: Tensor, timesteps: Tensor, counts: Tensor, scores: Tensor, hyp_counts: Tensor
                     ) -> List[List[CTCHypothesis]]:
    """Host form of beam-search rows: ``tokens`` / ``timesteps`` ``[R, n_best, T]``, ``counts`` / ``scores`` ``[R, n_best]``,
    ``hyp_counts`` ``[R]`` -> per row the list of its hypotheses, best first."""
    tokens_h, timesteps_h, counts_h = tokens.cpu(), timesteps.cpu(), counts.cpu()
    scores_h, hyp_h = scores.cpu(), hyp_counts.cpu()
    result = []
    for r in range(hyp_h.shape[0]):
        hyps = []
        for h in range(int(hyp_h[r])):
            k = int(counts_h[r, h])
            hyps.append(CTCHypothesis(tokens_h[r, h, :k].clone(), [], float(scores_h[r, h]), timesteps_h[r, h, :k].clone()))
        result.append(hyps)
    return result


class BeamDecoded(NamedTuple):
    """CTC beam-search results of a batch, one row per output: ``tokens`` / ``timesteps`` ``[O, N, n_best, T]`` int64 of which
    the first ``counts[o, n, h]`` entries are valid (timesteps 1-based), ``counts`` ``[O, N, n_best]`` int32, ``scores``
    ``[O, N, n_best]`` fp64 (descending), ``hyp_counts`` ``[O, N]`` int32 hypotheses found.  Device tensors when produced by
    ``Estimator.beam_decode_device``."""
    names: List[str]
    tokens: Tensor
    timesteps: Tensor
    counts: Tensor
    scores: Tensor
    hyp_counts: Tensor

    def hypotheses(self) -> Dict[str, List[List[CTCHypothesis]]]:
        """Host form: per output and utterance the reference's list of up to ``n_best`` ``CTCHypothesis``."""
        O, N, B, T = self.tokens.shape
        rows = _beam_hypotheses(self.tokens.reshape(O * N, B, T), self.timesteps.reshape(O * N, B, T),
                                self.counts.reshape(O * N, B), self.scores.reshape(O * N, B), self.hyp_counts.reshape(O * N))
        return {name: rows[o * N:(o + 1) * N] for o, name in enumerate(self.names)}


def _spec_to_structs(spec: Dict[str, Any], precision: str):
    cfg = _lib.AmxConfig()
    cfg.abi_version = _lib.AMX_ABI_VERSION
    n = len(spec["conv_kernel"])
    if n > _lib.AMX_MAX_CONV:
        raise ValueError("too many conv layers")
    cfg.n_conv = n
    cfg.conv_dim = spec["conv_dim"]
    for i in range(n):
        cfg.conv_kernel[i] = spec["conv_kernel"][i]
        cfg.conv_stride[i] = spec["conv_stride"][i]
    cfg.hidden, cfg.layers, cfg.heads, cfg.ffn = spec["hidden"], spec["layers"], spec["heads"], spec["ffn"]
    cfg.pos_kernel, cfg.pos_groups = spec["pos_kernel"], spec["pos_groups"]
    cfg.eps = spec["eps"]
    cfg.do_normalize = int(spec.get("do_normalize", True))
    cfg.dependency_blanks = int(spec.get("dependency_blanks", True))
    cfg.embedding_size = int(spec.get("embedding_size") or 0)
    cfg.allophone_layer = int(bool(spec.get("allophone_layer", False)))
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"unknown precision {precision!r}; expected one of {sorted(_lib.PRECISIONS)}")
    cfg.precision = _lib.PRECISIONS[precision]
    norm = spec.get("feat_extract_norm", "layer")
    if norm not in ("layer", "group"):
        raise ValueError(f"`feat_extract_norm` is {norm}, but has to be one of ['group', 'layer']")  # transformers' own message
    cfg.feat_extract_norm = _lib.NORM_GROUP if norm == "group" else _lib.NORM_LAYER
    cfg.conv_bias = int(bool(spec.get("conv_bias", True)))
    cfg.stable_layer_norm = int(bool(spec.get("stable_layer_norm", True)))
    cfg.use_attention_mask = int(bool(spec.get("use_attention_mask", True)))
    cfg.adapter_attn_dim = int(spec.get("adapter_attn_dim") or 0)

    classes = spec["classes"]
    index = {c["name"]: i for i, c in enumerate(classes)}
    descs = (_lib.AmxClassDesc * len(classes))()
    for i, c in enumerate(classes):
        if len(c["name"].encode()) >= _lib.AMX_NAME_LEN:
            raise ValueError(f"classifier name too long: {c['name']}")
        descs[i].name = c["name"].encode()
        descs[i].size = c["size"]
        composed = c["name"] == _spec.PHONEME and cfg.embedding_size
        allophone = c["name"] == _spec.PHONEME and cfg.allophone_layer
        out_classes = spec.get("shared_phones", c["size"]) if allophone else c["size"]
        descs[i].out_features = cfg.embedding_size if composed else out_classes + _spec.BLANK_OFFSET
        layer = c.get("time_layer")
        descs[i].time_heads = int(layer.get("num_heads", 1)) if layer else 0
        descs[i].time_positional = int(bool(layer.get("positional_embeddings", False))) if layer else 0
        deps = c["dependencies"]
        if len(deps) > _lib.AMX_MAX_DEPS:
            raise ValueError("too many dependencies")
        descs[i].n_deps = len(deps)
        for j, d in enumerate(deps):
            m = _spec.OUTPUT_PATTERN.match(d)
            if m:
                descs[i].deps[j] = _lib.DEP_OUTPUT if m.group(1) is None else _lib.dep_output_layer(int(m.group(1)))
            else:
                if d not in index:
                    raise ValueError(f"unknown dependency {d!r}")
                descs[i].deps[j] = index[d]
    return cfg, descs


SAMPLE_RATE = 16000  # the audio rate of every reference model (checkpoint.py checks it on restore)
ALLOPHONE_MATRICES_KEY = "_projection._layers.phoneme._allophone_layer._allophone_matrices"
_NO_ALLOPHONE_LAYER = "Can't map phones to allophones with a model without an allophone layer"  # acoustic_model.py:546


def _allophone_field(mapping, name: str):
    return mapping.get(name) if isinstance(mapping, dict) else getattr(mapping, name, None)


class Estimator:
    """Prediction-side replacement of the reference ``Estimator`` running on one MI355X.

    ``precision``: ``"f16x3"`` (default; fp32-grade split-precision MFMA, meets the 1e-3 logit gate), ``"bf16x3"``,
    ``"f16"`` or ``"bf16"`` (single-plane throughput modes; error measured in tests/ and DESIGN.md).
    """

    def __init__(self, spec: Dict[str, Any], state_dict: Dict[str, Tensor], device: str | torch.device = "cuda:0",
                 precision: str = "f16x3"):
        _spec.validate(spec)
        self._spec = spec
        self._lib = _lib.load()
        self._device = torch.device(device)
        if self._device.type != "cuda":
            raise RuntimeError("allophant_amd runs on an MI355X only (device must be cuda:N); there is no CPU fallback")
        self._index = self._device.index if self._device.index is not None else torch.cuda.current_device()
        self._precision = precision
        cfg, descs = _spec_to_structs(spec, precision)
        keep = []
        tensors = (_lib.AmxTensor * len(state_dict))()
        # the trained allophone matrices stay on the host: set_allophones compresses them under the mapping's structure
        self._allophone_values: Optional[Tensor] = None
        for i, (k, v) in enumerate(state_dict.items()):
            t = v.detach().to("cpu", torch.float32).contiguous()
            keep.append(t)
            if k == ALLOPHONE_MATRICES_KEY:
                self._allophone_values = t
            tensors[i].name = k.encode()
            tensors[i].data = C.cast(t.data_ptr(), C.POINTER(C.c_float))
            tensors[i].numel = t.numel()
        handle = C.c_void_p()
        code = self._lib.amx_create(C.byref(handle), self._index, C.byref(cfg), descs, len(descs), tensors, len(state_dict))
        _lib.check(self._lib, None, code)
        self._handle = handle
        self._classes = [c["name"] for c in spec["classes"]]
        self._allophone_shape: Optional[Tuple[int, int, int]] = None  # (languages, P+1, Q+1) of the installed structure
        self._allophone_index_map: Optional[Dict[str, int]] = None
        self._inventory: Optional[Tensor] = None
        self._training_inventory: Optional[Tensor] = None
        cats = spec.get("composition_categories")
        self._category_offsets = None
        if spec.get("embedding_size"):
            if cats is None:
                raise ValueError("composition models need `composition_categories` (number of values per feature)")
            self._category_offsets = torch.tensor([1] + list(cats), dtype=torch.int64).cumsum(0)[:-1].contiguous()

    # -- reference-compatible surface ------------------------------------------------------------------------------
    @property
    def classes(self) -> List[str]:
        return self._classes

    @property
    def precision(self) -> str:
        return self._precision

    @property
    def device_bytes(self) -> int:
        return int(self._lib.amx_device_bytes(self._handle))

    @property
    def sample_rate(self) -> int:
        """The rate ``predict`` expects (reference estimator.py:940; every upstream model is trained at 16 kHz)."""
        return SAMPLE_RATE

    def resample(self, batch: Batch, sample_rates) -> Batch:
        """``resample.resample_batch(batch, sample_rates, self.sample_rate)`` on this estimator's device: a padded batch at
        source rates (one per utterance, mixed freely) -> the 16 kHz batch ``predict`` takes, in one launch.  Upstream
        resamples each utterance on the host before ``predict`` (README recipe; speech_corpus.py ``Resample(sr, 16000)``)."""
        from .resample import resample_batch

        if batch.audio_features.device != self._device:
            batch = batch.to(self._device)
        return resample_batch(batch, sample_rates, self.sample_rate)

    @classmethod
    def restore(cls, checkpoint_or_path, device: str = "cuda:0", precision: str = "f16x3"):
        """Builds an estimator from a checkpoint dict in the reference ``Checkpoint`` schema (estimator.py:199-249) or a
        path to one saved with ``torch.save``.  Returns ``(estimator, attribute_indexer)`` like the reference
        (estimator.py:1085-1126): the indexer is an ``allophant_amd.phonetic.AttributeTable`` rebuilt from the table text
        embedded in ``phonetic_indexer_state`` (``composition_feature_matrix``, ``phoneme_inventory``,
        ``composition_features``), or ``None`` for checkpoints without one."""
        from .checkpoint import indexer_from_checkpoint, spec_from_checkpoint

        if not isinstance(checkpoint_or_path, dict):
            checkpoint_or_path = torch.load(checkpoint_or_path, map_location="cpu", weights_only=True)
        spec = spec_from_checkpoint(checkpoint_or_path)
        indexer, training = indexer_from_checkpoint(checkpoint_or_path)
        estimator = cls(spec, checkpoint_or_path["model_state"], device, precision)
        if spec.get("embedding_size") and indexer is not None and training:
            # `predict(batch)` without target_feature_indices falls back to the training inventory upstream
            # (`_dense_feature_table`, acoustic_model.py:214-221); it is a non-persistent buffer there, rebuilt from the
            # indexer at construction, so it is rebuilt from the embedded table here as well
            estimator.set_training_inventory(indexer.composition_feature_matrix(training))
        language_allophones = (checkpoint_or_path.get("phonetic_indexer_state") or {}).get("language_allophones")
        if spec.get("allophone_layer") and language_allophones:
            # upstream rebuilds the allophone layer's structure from the same dump (`Allophant.from_config` ->
            # AllophoneMapping.__init__), with or without an embedded attribute table
            estimator.set_allophones(language_allophones)
        return estimator, indexer

    def set_training_inventory(self, target_feature_indices: Tensor) -> None:
        """The inventory ``predict(batch)`` uses when called without ``target_feature_indices`` (upstream: the
        ``_dense_feature_table`` buffer of ``EmbeddingCompositionLayer``, acoustic_model.py:214-221)."""
        if not self._spec.get("embedding_size"):
            raise ValueError("model has no embedding composition layer")
        self._training_inventory = target_feature_indices.detach().to("cpu", torch.int64).contiguous()

    # -- allophone layer ---------------------------------------------------------------------------------------------
    def set_allophones(self, language_allophones) -> None:
        """Installs the allophone layer of ``map_allophones``: the structure (``_allophone_mask``) comes from the
        ``LanguageAllophoneMappings`` dump like upstream's ``AllophoneMapping.__init__`` (acoustic_model.py:105-136), the
        values from the state dict's trained ``_allophone_matrices``.  A second call replaces the first."""
        from .allophones import build_structure

        if not self._spec.get("allophone_layer"):
            raise ValueError(_NO_ALLOPHONE_LAYER)
        if self._allophone_values is None:
            raise ValueError(f"the state dict lacks {ALLOPHONE_MATRICES_KEY}")
        if not hasattr(self._lib, "amx_set_allophones"):
            raise RuntimeError(f"{_lib.LIB_PATH} predates the allophone layer (amx_set_allophones): rebuild it")
        P1, Q1 = self._allophone_widths()
        values = self._allophone_values
        shared = list(_allophone_field(language_allophones, "shared_phones") or [])
        if shared and len(shared) + _spec.BLANK_OFFSET != P1:
            raise ValueError(f"language_allophones lists {len(shared)} shared phones, the model predicts {P1 - _spec.BLANK_OFFSET}")
        structure = build_structure(language_allophones, P1, Q1)
        n_lang = structure.mask.shape[0]
        if tuple(values.shape) != (n_lang, P1, Q1):
            raise ValueError(f"_allophone_matrices is {list(values.shape)}, the mapping and the model need {[n_lang, P1, Q1]}")
        mask = structure.mask.to(torch.uint8).contiguous()
        with torch.cuda.device(self._device):
            code = self._lib.amx_set_allophones(self._handle, n_lang, P1, Q1, C.cast(values.data_ptr(), C.POINTER(C.c_float)),
                                                C.cast(mask.data_ptr(), C.POINTER(C.c_uint8)))
        _lib.check(self._lib, self._handle, code)
        self._allophone_shape = (n_lang, P1, Q1)
        self._allophone_index_map = structure.index_map

    @property
    def allophone_languages(self) -> Dict[str, int]:
        """Language code -> matrix index of the installed allophone layer (upstream ``AllophoneMapping.index_map``): the
        ``language_ids`` ``map_allophones`` takes."""
        if self._allophone_index_map is None:
            raise ValueError(_NO_ALLOPHONE_LAYER if not self._spec.get("allophone_layer") else
                             "no allophone mapping installed: restore from a checkpoint with language_allophones or call set_allophones()")
        return dict(self._allophone_index_map)

    def _allophone_widths(self) -> Tuple[int, int]:
        phoneme = next(c for c in self._spec["classes"] if c["name"] == _spec.PHONEME)
        return int(self._spec.get("shared_phones", phoneme["size"])) + _spec.BLANK_OFFSET, int(phoneme["size"]) + _spec.BLANK_OFFSET

    def map_allophones(self, phone_logits: Tensor, language_ids) -> Tensor:
        """``Estimator.map_allophones`` (reference estimator.py:1048-1049, AllophoneMapping.map_allophones
        acoustic_model.py:142-159): language-specific phoneme outputs ``[T, N, Q+1]`` from phone outputs ``[T, N, P+1]``
        (``predict(...).outputs["phone"]`` goes in as it is; any strides with a unit class stride), on the device and the
        current stream.  ``out[t, n, q] = max_p(x[t, n, p] * W[l, p, q])`` over the allophones p of phoneme q in language
        ``l = int(language_ids[n])`` (Python indexing: -1 is the last language), ``finfo(float32).min`` standing in for every
        masked pair; bitwise upstream's values.  Not renormalised.  There is no CPU path."""
        if not self._spec.get("allophone_layer"):
            raise ValueError(_NO_ALLOPHONE_LAYER)
        if phone_logits.device.type != "cuda":
            raise RuntimeError("allophant_amd maps allophones on an MI355X only (phone_logits must be a cuda tensor); there is no CPU fallback")
        if self._allophone_shape is None:
            raise RuntimeError("no allophone mapping installed: restore from a checkpoint with language_allophones or call set_allophones()")
        if phone_logits.device != self._device:
            raise ValueError(f"phone_logits is on {phone_logits.device}, the estimator on {self._device}")
        if phone_logits.dim() != 3:
            raise ValueError("phone_logits must be [T, N, P+1]")
        n_lang, P1, Q1 = self._allophone_shape
        T, N, width = phone_logits.shape
        if width != P1:
            raise ValueError(f"phone_logits has {width} classes, the allophone layer maps {P1} (shared phones + blank): a "
                             "custom composition inventory has no allophone matrices")
        if phone_logits.dtype != torch.float32:
            phone_logits = phone_logits.float()
        if phone_logits.stride(2) != 1:
            phone_logits = phone_logits.contiguous()
        ids_host = language_ids.detach().cpu() if isinstance(language_ids, Tensor) else language_ids
        ids = [int(v) for v in ids_host]  # upstream: map(int, language_ids)
        if len(ids) != N:
            raise ValueError(f"{len(ids)} language ids for {N} utterances")
        for i, v in enumerate(ids):
            if not -n_lang <= v < n_lang:
                raise IndexError(f"index {v} is out of bounds for dimension 0 with size {n_lang}")
            ids[i] = v % n_lang
        out = torch.empty(T, N, Q1, dtype=torch.float32, device=self._device)
        if N == 0 or T == 0:
            return out
        with torch.cuda.device(self._device):
            dense = torch.tensor(ids, dtype=torch.int32).to(self._device)
            stream = torch.cuda.current_stream(self._device).cuda_stream
            code = self._lib.amx_map_allophones(
                self._handle, C.c_void_p(phone_logits.data_ptr()), phone_logits.stride(0), phone_logits.stride(1),
                C.c_void_p(dense.data_ptr()), N, T, C.c_void_p(out.data_ptr()), C.c_void_p(stream))
        _lib.check(self._lib, self._handle, code)
        return out

    def _set_inventory(self, tfi: Tensor) -> None:
        tfi_cpu = tfi.detach().to("cpu", torch.int64).contiguous()
        if self._inventory is not None and self._inventory.shape == tfi_cpu.shape and torch.equal(self._inventory, tfi_cpu):
            return
        if tfi_cpu.dim() != 2 or tfi_cpu.shape[1] != self._category_offsets.numel():
            raise ValueError(
                f"target_feature_indices must be [phones, {self._category_offsets.numel()}] (composition_feature_matrix)")
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream(self._device).cuda_stream
            code = self._lib.amx_set_inventory(
                self._handle, C.cast(tfi_cpu.data_ptr(), C.POINTER(C.c_int64)), tfi_cpu.shape[0], tfi_cpu.shape[1],
                C.cast(self._category_offsets.data_ptr(), C.POINTER(C.c_int64)), C.c_void_p(stream))
        _lib.check(self._lib, self._handle, code)
        self._inventory = tfi_cpu

    def _select_inventory(self, target_feature_indices: Optional[Tensor]) -> None:
        """What ``predict`` does with its ``target_feature_indices``: a composition model runs under them, or under the training
        inventory when there are none."""
        if self._spec.get("embedding_size"):
            if target_feature_indices is None:
                if self._training_inventory is None:
                    raise ValueError(
                        "composition models need `target_feature_indices`: the training inventory table is a "
                        "non-persistent buffer upstream (acoustic_model.py:214-221); restore the estimator from a checkpoint "
                        "that embeds its attribute table, or call set_training_inventory()")
                target_feature_indices = self._training_inventory
            self._set_inventory(target_feature_indices)

    def _output_layout(self, N: int, L: int):
        """``amx_output_layout`` of a batch of ``N`` rows padded to ``L`` samples under the selected inventory: the output
        descriptors, the frames ``T`` and the floats of the flat buffer."""
        n_out, T, total = C.c_int(), C.c_int64(), C.c_int64()
        code = self._lib.amx_output_layout(self._handle, N, L, None, C.byref(n_out), C.byref(T), C.byref(total))
        _lib.check(self._lib, self._handle, code)
        descs = (_lib.AmxOutputDesc * n_out.value)()
        code = self._lib.amx_output_layout(self._handle, N, L, descs, C.byref(n_out), C.byref(T), C.byref(total))
        _lib.check(self._lib, self._handle, code)
        return descs, int(T.value), int(total.value)

    def predict(self, batch: Batch, target_feature_indices: Optional[Tensor] = None, log_probabilities: bool = True,
                _keep_hidden: bool = False, _timing: bool = False, _no_pack: bool = False, _no_graph: bool = False,
                _out: Optional[Tensor] = None) -> Predictions:
        """``Estimator.predict`` (reference estimator.py:1035-1046).  ``_no_pack`` (test hook) keeps the padded row layout
        through the encoder layers of a ragged batch (``AMX_FLAG_NO_PACK``); ``_no_graph`` (test hook) enqueues the pass launch
        by launch (``AMX_FLAG_NO_GRAPH``); ``_out`` (test / benchmark hook) is a flat fp32 device buffer to write the outputs into.

        Safe by default: the reference computes in fp32; here an activation beyond the range of the fp16 planes turns into
        non-finite logits.  Such a batch raises ``FloatingPointError`` from the first ``predict`` / ``synchronize`` issued after
        the offending pass has finished on the GPU (no host synchronisation is added: see ``amx_forward``)."""
        self._select_inventory(target_feature_indices)
        audio = batch.audio_features
        if audio.dim() != 2:
            raise ValueError("audio_features must be [N, L]")
        audio = audio.to(self._device, torch.float32).contiguous()
        lengths = batch.lengths.detach().to("cpu", torch.int64).contiguous()
        N, L = audio.shape
        if lengths.numel() != N:
            raise ValueError("lengths must have one entry per utterance")
        padded = bool(getattr(batch, "_padded", False))  # a block of a larger batch that keeps the global padded length
        if N > 0 and int(lengths.max()) != L and not (padded and int(lengths.max()) <= L):
            raise ValueError("the batch must be padded to exactly max(lengths) (reference utils.py:62-63, acoustic_model.py:765-767)")
        with torch.cuda.device(self._device):
            descs, T, total = self._output_layout(N, L)
            if _out is not None:
                if _out.dtype != torch.float32 or _out.device != self._device or _out.numel() < total or not _out.is_contiguous():
                    raise ValueError("_out must be a contiguous fp32 buffer on the estimator's device with room for every output")
                flat = _out.view(-1)[: total]
            else:
                flat = torch.empty(total, dtype=torch.float32, device=self._device)
            out_lengths = torch.empty(N, dtype=torch.int64)
            flags = 0 if log_probabilities else _lib.FLAG_RAW_LOGITS
            if _keep_hidden:
                flags |= _lib.FLAG_KEEP_HIDDEN
            if _timing:
                flags |= _lib.FLAG_TIMING
            if _no_pack:
                flags |= _lib.FLAG_NO_PACK
            if padded:
                flags |= _lib.FLAG_PADDED
            if _no_graph:
                flags |= _lib.FLAG_NO_GRAPH
            stream = torch.cuda.current_stream(self._device).cuda_stream
            n_max = int(self._lib.amx_max_utterances(self._handle, L))
            if N <= n_max:
                code = self._lib.amx_forward(
                    self._handle, C.c_void_p(audio.data_ptr()), C.cast(lengths.data_ptr(), C.POINTER(C.c_int64)), N, L,
                    C.c_void_p(flat.data_ptr()), C.cast(out_lengths.data_ptr(), C.POINTER(C.c_int64)), flags,
                    C.c_void_p(stream))
                _lib.check(self._lib, self._handle, code)
            else:
                # a plane of the batch would pass 4 GiB (32-bit plane offsets in the kernels): run it as slices of
                # utterances padded to the same L -- no operator mixes utterances, so the results are those of one call
                if n_max < 1:
                    raise ValueError(f"utterances of {L} samples are too long for one forward pass")
                # the slices add to one range-check count (`check_finite`): the first one restarts it like any forward pass,
                # the later ones continue it (AMX_FLAG_CONTINUE) -- launch-only, no host synchronisation
                blocks = {d.offset: d.classes for d in descs}
                for lo in range(0, N, n_max):
                    hi = min(N, lo + n_max)
                    n = hi - lo
                    part_total = sum(T * n * c for c in blocks.values())
                    part = torch.empty(part_total, dtype=torch.float32, device=self._device)
                    part_lengths = torch.empty(n, dtype=torch.int64)
                    slice_lengths = lengths[lo:hi].contiguous()  # named: must outlive the call that reads its storage
                    code = self._lib.amx_forward(
                        self._handle, C.c_void_p(audio[lo:hi].data_ptr()),
                        C.cast(slice_lengths.data_ptr(), C.POINTER(C.c_int64)), n, L,
                        C.c_void_p(part.data_ptr()), C.cast(part_lengths.data_ptr(), C.POINTER(C.c_int64)),
                        flags | _lib.FLAG_PADDED | (_lib.FLAG_CONTINUE if lo > 0 else 0), C.c_void_p(stream))
                    _lib.check(self._lib, self._handle, code)
                    out_lengths[lo:hi] = part_lengths
                    src = 0
                    for offset, c in blocks.items():  # blocks in output order: offsets ascend with the part's own
                        flat[offset: offset + T * N * c].view(T, N, c)[:, lo:hi] = \
                            part[src: src + T * n * c].view(T, n, c)
                        src += T * n * c
                    part.record_stream(torch.cuda.current_stream(self._device))
            # keep `audio` alive until the asynchronous kernels have consumed it
            flat.record_stream(torch.cuda.current_stream(self._device))
            audio.record_stream(torch.cuda.current_stream(self._device))
        self._geom = (N, T)
        outputs: Dict[str, Tensor] = {}
        for d in descs:
            c = d.classes
            outputs[d.name.decode()] = flat[d.offset: d.offset + T * N * c].view(T, N, c)
        return Predictions(outputs, out_lengths.to(batch.lengths.device), flat, (N, L), self._inventory)

    def predict_long(self, batch: Batch, target_feature_indices: Optional[Tensor] = None, log_probabilities: bool = True,
                     window_seconds: float = 10.0, context_seconds: float = 1.0, batch_windows: int = 32,
                     _no_graph: bool = False) -> Predictions:
        """``predict`` for recordings of any length up to 2^20 frames (5.8 h), as HF's CTC pipeline does it with
        ``chunk_length_s`` / ``stride_length_s``: every recording of the padded batch ``[R, Lmax]`` is cut into windows of
        ``int(window_seconds * sample_rate)`` samples that overlap by twice the context of
        ``int(context_seconds * sample_rate) // hop`` frames (``longform.plan_windows``; the last window of a recording is
        right-aligned, not short).  The windows of all recordings run through ``predict`` in slices of at most ``batch_windows``
        rows, and each window's frames between its contexts -- at the ends of a recording, up to the end -- are copied into the
        recording's output.  A slice is gathered (``amx_long_gather``), predicted and stitched (``amx_long_stitch``) on the
        current stream, in one fixed pair of device buffers: equal slices replay one recorded graph.  The call itself adds no
        host synchronisation (the window table and the lengths go up from pinned memory: two small blocks per call from
        torch's caching host allocator); each slice is a forward pass and takes one of the handle's four pinned length slots
        (``amx_forward``), so from the fifth slice on the launch of a slice waits for the slice four before it.  Measured
        under a stalled stream (tests/test_gpu_run_ahead.py): a call of four slices on a handle whose earlier passes have
        completed returns before the device starts; a call of ten slices does not.

        The result is an ordinary ``Predictions`` of the whole batch (layout of ``amx_output_layout(R, Lmax)``, ``lengths`` the
        recordings' frames, zeros beyond them; a recording below the receptive field has length 0): ``greedy_decode``,
        ``beam_decode``, ``align``, ``score``, ``search`` and ``Evaluator`` take it unchanged (``search`` keeps its
        ``N * Q * T < 2^31`` limit; ``align`` takes up to 262 143 targets per row, a whole transcript, and ``score`` keeps its
        4095).  Recordings that each fit one window, at most ``batch_windows`` of them, give the bits of
        ``predict(batch)``.

        What a window cannot see: ``do_normalize`` normalises each window on its own samples, as it does each utterance the
        model was trained on; a time-layer head attends within its window; and a model that is sensitive to padding (group-norm
        extractor, no attention mask) sees less than one hop of it, in a recording's last window only.  The defaults are HF's
        customary proportions, not a measurement.  Not covered: the data-parallel gather of such predictions and
        ``predict_languages`` on long rows."""
        from . import longform

        self._select_inventory(target_feature_indices)
        audio = batch.audio_features
        if audio.dim() != 2:
            raise ValueError("audio_features must be [N, L]")
        audio = audio.to(self._device, torch.float32).contiguous()
        lengths = batch.lengths.detach().to("cpu", torch.int64).contiguous()
        R, Lmax = audio.shape
        if lengths.numel() != R:
            raise ValueError("lengths must have one entry per utterance")
        if R > 0 and int(lengths.max()) != Lmax and not (getattr(batch, "_padded", False) and int(lengths.max()) <= Lmax):
            raise ValueError("the batch must be padded to exactly max(lengths) (reference utils.py:62-63, acoustic_model.py:765-767)")
        if batch_windows < 1:
            raise ValueError(f"batch_windows must be at least 1, got {batch_windows}")
        window = int(window_seconds * self.sample_rate)
        plan = longform.plan_windows(lengths.tolist(), self._spec, window, int(context_seconds * self.sample_rate) // math.prod(
            self._spec["conv_stride"]))
        W = len(plan)
        with torch.cuda.device(self._device):
            descs, T, total = self._output_layout(R, Lmax)  # (raises for a batch without a frame, and past 2^20 frames)
            if W == 0:  # (a padded batch: Lmax holds a frame, no recording does)
                raise ValueError("utterances are shorter than the receptive field of the feature extractor")
            rows = min(int(batch_windows), int(self._lib.amx_max_utterances(self._handle, window)))
            if rows < 1:
                raise ValueError(f"windows of {window} samples are too long for one forward pass")
            rows = min(rows, W)
            samples = torch.from_numpy(plan.windows[:, longform.SAMPLES].astype("int64"))
            longest = int(samples.max())
            flat = torch.zeros(total, dtype=torch.float32, device=self._device)
            window_audio = torch.empty(rows * longest, dtype=torch.float32, device=self._device)
            window_out = torch.empty(self._output_layout(rows, longest)[2], dtype=torch.float32, device=self._device)
            # (pinned and asynchronous: a copy out of pageable memory would wait for everything the stream holds)
            windows = torch.from_numpy(plan.windows).pin_memory().to(self._device, non_blocking=True)
            device_lengths = lengths.pin_memory().to(self._device, non_blocking=True)
            status = torch.empty(2, W, dtype=torch.int32, device=self._device)
            where = {d.name: d.offset for d in descs}
            for lo in range(0, W, rows):
                hi = min(W, lo + rows)
                part = Batch(window_audio[: (hi - lo) * int(samples[lo:hi].max())].view(hi - lo, -1), samples[lo:hi].contiguous(),
                             torch.zeros(hi - lo, dtype=torch.long))
                part._padded = True
                longform.gather_windows(audio, device_lengths, windows[lo:hi], plan.hop, part.audio_features, status[0, lo:hi])
                piece = self.predict(part, target_feature_indices, log_probabilities, _no_graph=_no_graph, _out=window_out)
                # the blocks of the slice against those of the batch, by name ("phone" shares the block of "phoneme")
                blocks = {(o.storage_offset(), where[name.encode()], o.shape[2]) for name, o in piece.outputs.items()}
                src_T = next(iter(piece.outputs.values())).shape[0]
                longform.stitch_windows(window_out, src_T, windows[lo:hi], sorted(blocks), flat, R, T, status[1, lo:hi])
            stream = torch.cuda.current_stream(self._device)
            for t in (audio, window_audio, window_out, windows, device_lengths, status):
                t.record_stream(stream)
        outputs: Dict[str, Tensor] = {}
        for d in descs:
            outputs[d.name.decode()] = flat[d.offset: d.offset + T * R * d.classes].view(T, R, d.classes)
        frames = torch.from_numpy(plan.frames.copy()).to(batch.lengths.device)
        return Predictions(outputs, frames, flat, (R, Lmax), self._inventory)

    def predict_languages(self, batch: Batch, inventories, languages: Optional[Sequence] = None, log_probabilities: bool = True,
                          _no_graph: bool = False) -> Predictions:
        """``predict`` for a batch that mixes languages (composition models; upstream splits such a batch by language and
        predicts each part under its own inventory, run.py:712-713, 742-753): ONE pass under ``inventories.union_tfi``, then
        ``amx_restrict_outputs`` in place on the composed output (``"phoneme"``; ``"phone"`` shares its block) on the same
        stream.  ``inventories`` is a ``LanguageInventories``; ``languages`` holds one name (or dense id) per utterance, and
        left as ``None``, ``batch.language_ids`` are dense indices into ``inventories.languages``.

        For utterance ``n`` of language ``l`` the composed output then holds, at the union classes ``inventories.columns(l)``,
        what upstream's ``predict(part, tfi_l)`` holds (the log-softmax over the language's own classes, or with
        ``log_probabilities=False`` the raw logits), and -inf at every other class; frames beyond ``lengths`` are 0 as ever,
        and every other output is untouched.  ``greedy_decode``, ``align``, ``score``, ``rescore_device``, ``search``,
        ``Evaluator`` (with the union as its inventory) and ``hypothesis_symbols`` (with ``union_symbols``) take such
        predictions unchanged and speak union class indices (``LanguageInventories.to_language_indices`` gives upstream's);
        ``beam_decode`` decodes each language over its own classes.  Not covered: the data-parallel gather of such
        predictions."""
        if not self._spec.get("embedding_size"):
            raise ValueError("model has no embedding composition layer")
        if not hasattr(self._lib, "amx_restrict_outputs"):
            raise RuntimeError(f"{_lib.LIB_PATH} predates per-utterance inventories (amx_restrict_outputs): rebuild it")
        ids = inventories.language_ids(batch.language_ids if languages is None else languages)
        if ids.numel() != len(batch):
            raise ValueError(f"{ids.numel()} languages for {len(batch)} utterances")
        predictions = self.predict(batch, inventories.union_tfi, log_probabilities, _no_graph=_no_graph)
        block = predictions.outputs[_spec.PHONEME]
        T, N, classes = block.shape
        if classes != inventories.classes:
            raise ValueError(f"the composed output has {classes} classes, the union inventory {inventories.classes}")
        with torch.cuda.device(self._device):
            meta = torch.cat([predictions.lengths.detach().to("cpu", torch.int32), ids]).to(self._device)
            status = torch.empty(max(1, N), dtype=torch.int32, device=self._device)
            bits = inventories.device_bits(self._device)
            code = self._lib.amx_restrict_outputs(
                self._index, C.c_void_p(block.data_ptr()), block.stride(0), block.stride(1), classes,
                C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 4 * N), C.c_void_p(bits.data_ptr()),
                len(inventories.languages), N, T, _lib.RESTRICT_NORMALIZE if log_probabilities else 0,
                C.c_void_p(block.data_ptr()), block.stride(0), block.stride(1), C.c_void_p(status.data_ptr()),
                C.c_void_p(torch.cuda.current_stream(self._device).cuda_stream))
            _lib.check(self._lib, None, code)
            stream = torch.cuda.current_stream(self._device)
            meta.record_stream(stream), status.record_stream(stream)
        predictions._languages = (meta[N:], inventories)
        return predictions

    def _predictions_call(self, predictions: Predictions):
        """What every call over the output buffer of ``predictions`` starts with: selects their inventory and returns the
        output names, ``N``, ``L``, ``T``, ``O``, the host int64 frame lengths with their pointer, and the stream."""
        if predictions._flat is None or predictions._geometry is None:
            raise ValueError("predictions were not produced by this estimator")
        N, L = predictions._geometry
        if predictions._inventory is not None:
            # the block layout depends on the inventory size: run under the inventory of THESE predictions, whatever
            # later predict() calls selected (a cached inventory is re-selected without device work)
            self._set_inventory(predictions._inventory)
        names = list(predictions.outputs.keys())
        T = next(iter(predictions.outputs.values())).shape[0]
        frame_lengths = predictions.lengths.detach().to("cpu", torch.int64).contiguous()
        return (names, N, L, T, len(names), frame_lengths, C.cast(frame_lengths.data_ptr(), C.POINTER(C.c_int64)),
                torch.cuda.current_stream(self._device).cuda_stream)

    @staticmethod
    def _target_rows(predictions: Predictions, targets: Dict[str, Sequence[Sequence[int]]], names: List[str], N: int,
                     verb: str) -> List[Sequence[int]]:
        """``targets`` (output name -> one row per utterance) as rows ``o * N + n``, empty for an output without an entry;
        ``verb`` is what the caller does with them ("align", "score")."""
        unknown = [name for name in targets if name not in predictions.outputs]
        if unknown:
            raise ValueError(f"targets name the outputs {unknown}, the predictions hold {names}")
        rows: List[Sequence[int]] = []
        for name in names:
            per_utterance = targets.get(name)
            if per_utterance is not None and len(per_utterance) != N:
                raise ValueError(f"output {name!r}: {len(per_utterance)} target rows for {N} utterances")
            rows += [[] for _ in range(N)] if per_utterance is None else list(per_utterance)
        if N == 0:
            raise ValueError(f"predictions hold no utterances: nothing to {verb}")
        return rows

    def greedy_decode_device(self, predictions: Predictions) -> "Decoded":
        """On-device ``GreedyCTCDecoder`` over every output of ``predictions`` (reference predictions.py:194-207 applied
        per classifier as in run.py:767-774); the result stays in HBM (``Decoded``: no host copy, no synchronisation), which
        is what the data-parallel path gathers instead of log-probabilities (``parallel.gather_decoded``)."""
        names, N, L, T, O, _, lengths_pointer, stream = self._predictions_call(predictions)
        with torch.cuda.device(self._device):
            tokens = torch.empty(O, N, T, dtype=torch.int64, device=self._device)
            timesteps = torch.empty_like(tokens)
            counts = torch.empty(O, N, dtype=torch.int32, device=self._device)
            scores = torch.empty(O, N, dtype=torch.float32, device=self._device)
            code = self._lib.amx_greedy_ctc(
                self._handle, C.c_void_p(predictions._flat.data_ptr()), lengths_pointer, N, L, C.c_void_p(tokens.data_ptr()),
                C.c_void_p(timesteps.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(scores.data_ptr()),
                C.c_void_p(stream))
            _lib.check(self._lib, self._handle, code)
        return Decoded(names, tokens, timesteps, counts, scores)

    def greedy_decode(self, predictions: Predictions) -> Dict[str, List[List[CTCHypothesis]]]:
        """``greedy_decode_device`` fetched to the host as the reference's hypothesis lists.  Only token ids / timesteps /
        scores cross PCIe."""
        return self.greedy_decode_device(predictions).hypotheses()

    def beam_decode_device(self, predictions: Predictions, beam_width: int, n_best: int = 1,
                           exp_emissions: bool = True, *, lm=None, lm_weight: float = 1.0, token_score: float = 0.0,
                           lm_ids=None) -> "BeamDecoded":
        """On-device ``BeamCTCDecoder`` (reference predictions.py:210-235) over every output of ``predictions``, as the
        reference's decode loop applies it per classifier (run.py:767-785).  ``exp_emissions`` (default, like upstream's
        ``log_emissions.exp()``) adds probabilities; False adds the log-probabilities as given.  The result stays in HBM.

        ``lm`` (a ``PhonotacticLM``, or a sequence of them with one ``lm_ids`` index per utterance, -1 for none) fuses a
        phonotactic bigram into the search of the phoneme / phone outputs whose class count is the model's
        (``amx_beam_ctc_lm_emissions``: every new token adds ``lm_weight * lm[previous, token] + token_score``, the end
        ``lm_weight * lm[last, end]``); their rows replace those of the plain decode, every other output is unchanged.  For
        ``predict_languages`` predictions ``lm`` speaks union classes and each language's rows run under
        ``lm.restrict(columns)``.  Fusion is meant for ``exp_emissions=False``: with upstream's sums of probabilities a
        log-probability term is on another scale."""
        names, N, L, T, O, _, lengths_pointer, stream = self._predictions_call(predictions)
        _check_beam(beam_width, n_best)
        fusion = None
        if lm is not None:
            _phonotactics.check_scalars(lm_weight, token_score)
            fusion = (*_phonotactics.lm_call(lm, lm_ids, N), float(lm_weight), float(token_score))
        with torch.cuda.device(self._device):
            size = C.c_size_t()
            _lib.check(self._lib, None, self._lib.amx_beam_ctc_workspace(beam_width, O * N, T, C.byref(size)))
            workspace = torch.empty(max(1, size.value), dtype=torch.uint8, device=self._device)
            tokens = torch.empty(O, N, n_best, T, dtype=torch.int64, device=self._device)
            timesteps = torch.empty_like(tokens)
            counts = torch.empty(O, N, n_best, dtype=torch.int32, device=self._device)
            scores = torch.empty(O, N, n_best, dtype=torch.float64, device=self._device)
            hyp_counts = torch.empty(O, N, dtype=torch.int32, device=self._device)
            code = self._lib.amx_beam_ctc(
                self._handle, C.c_void_p(predictions._flat.data_ptr()), lengths_pointer, N, L, beam_width, n_best,
                _lib.BEAM_EXP_EMISSIONS if exp_emissions else 0, C.c_void_p(workspace.data_ptr()), size.value,
                C.c_void_p(tokens.data_ptr()), C.c_void_p(timesteps.data_ptr()), C.c_void_p(counts.data_ptr()),
                C.c_void_p(scores.data_ptr()), C.c_void_p(hyp_counts.data_ptr()), C.c_void_p(stream))
            _lib.check(self._lib, self._handle, code)
        decoded = BeamDecoded(names, tokens, timesteps, counts, scores, hyp_counts)
        if predictions._languages is not None:
            decoded = self._beam_decode_languages(predictions, decoded, beam_width, n_best, exp_emissions, fusion)
        elif fusion is not None:
            decoded = self._beam_decode_fused(predictions, decoded, beam_width, n_best, exp_emissions, fusion)
        return decoded

    @staticmethod
    def _fused_outputs(predictions: Predictions, names: List[str], classes: int) -> List[int]:
        """The outputs a language model of ``classes`` classes is fused into: phoneme / phone blocks of that class count."""
        found = [o for o, name in enumerate(names)
                 if name in (_spec.PHONEME, _spec.PHONE) and predictions.outputs[name].shape[2] == classes]
        if not found:
            raise ValueError(f"no phoneme or phone output has the language model's {classes} classes")
        return found

    def _beam_decode_fused(self, predictions: Predictions, decoded: "BeamDecoded", beam_width: int, n_best: int,
                           exp_emissions: bool, fusion) -> "BeamDecoded":
        """The rest of ``beam_decode_device`` under a language model: the phoneme / phone rows decoded again through
        ``amx_beam_ctc_lm_emissions``, which reads the output's block in place through its strides."""
        lms, lm_ids, lm_weight, token_score = fusion
        if any(m.blank != 0 for m in lms):
            raise ValueError("the outputs' blank is class 0: the language model's must be too")
        with torch.cuda.device(self._device):
            stack = _phonotactics.PhonotacticLM.stack(lms).to(self._device)
            for o in self._fused_outputs(predictions, decoded.names, lms[0].classes):
                block = predictions.outputs[decoded.names[o]]  # [T, N, C]
                rows = _beam_ctc_rows(block.transpose(0, 1), predictions.lengths, beam_width, n_best, 0, exp_emissions,
                                      (stack, lm_ids, lm_weight, token_score))
                for whole, piece in zip(decoded[1:], rows):
                    whole[o] = piece
        return decoded

    def _beam_decode_languages(self, predictions: Predictions, decoded: "BeamDecoded", beam_width: int, n_best: int,
                               exp_emissions: bool, fusion=None) -> "BeamDecoded":
        """The rest of ``beam_decode_device`` for ``predict_languages`` predictions.  Upstream hands the decoder probabilities as
        scores, so a class of probability 0 is still a candidate, while upstream's per-language decoder does not have the
        class at all: the composed outputs are decoded again per language, over the language's utterances and its own columns
        of the restricted block (the emissions path), the tokens mapped back to union ids, and the rows of ``decoded``
        replaced.  With ``fusion`` (language models over the union classes) each language's rows run under the models
        restricted to its columns."""
        ids, inventories = predictions._languages
        ids_host = ids.cpu().tolist()
        fused = None
        if fusion is not None:
            lms, lm_ids, lm_weight, token_score = fusion
            if any(m.blank != 0 for m in lms):
                raise ValueError("the outputs' blank is class 0: the language model's must be too")
            fused = self._fused_outputs(predictions, decoded.names, lms[0].classes)
        with torch.cuda.device(self._device):
            lengths = predictions.lengths.to(self._device)
            for o, name in enumerate(decoded.names):
                if name not in (_spec.PHONEME, _spec.PHONE):
                    continue
                block = predictions.outputs[name]  # [T, N, C]
                for language in sorted(set(ids_host)):
                    columns = inventories.columns(language).to(self._device)
                    if columns.numel() < 2:
                        raise ValueError(f"beam search needs a phoneme in the inventory of {inventories.languages[language]!r}")
                    rows_of = [n for n, l in enumerate(ids_host) if l == language]
                    own = torch.tensor(rows_of, dtype=torch.int64, device=self._device)
                    compact = block.index_select(1, own).index_select(2, columns).transpose(0, 1).contiguous()
                    table = None
                    if fused is not None and o in fused:
                        stack = _phonotactics.PhonotacticLM.stack([m.restrict(columns) for m in lms]).to(self._device)
                        table = (stack, lm_ids[rows_of], lm_weight, token_score)
                    tokens, *rest = _beam_ctc_rows(compact, lengths[own], beam_width, n_best, 0, exp_emissions, table)
                    # per-language ids -> union ids (the entries past `counts` are not tokens: clamped into the table)
                    decoded.tokens[o, own] = columns[tokens.clamp_(0, columns.numel() - 1)]
                    for whole, piece in zip(decoded[2:], rest):
                        whole[o, own] = piece
        return decoded

    def beam_decode(self, predictions: Predictions, beam_width: int, n_best: int = 1, exp_emissions: bool = True, *, lm=None,
                    lm_weight: float = 1.0, token_score: float = 0.0, lm_ids=None) -> Dict[str, List[List[CTCHypothesis]]]:
        """``beam_decode_device`` fetched to the host: per output and utterance up to ``n_best`` hypotheses, best first."""
        return self.beam_decode_device(predictions, beam_width, n_best, exp_emissions, lm=lm, lm_weight=lm_weight,
                                       token_score=token_score, lm_ids=lm_ids).hypotheses()

    def align_device(self, predictions: Predictions, targets: Dict[str, Sequence[Sequence[int]]],
                     long: Optional[bool] = None) -> "_alignment.Aligned":
        """On-device CTC forced alignment (``amx_ctc_align``) of every output of ``predictions`` against ``targets``: output
        name -> one class-index sequence per utterance (``alignment.label_targets`` builds them from labels).  An output
        without an entry is aligned against nothing and left out of ``Aligned.present``.  The result stays in HBM.  ``long``
        as in ``alignment.ctc_forced_align``: a call whose largest row has more than ``ALIGN_MAX_TARGET`` targets (a whole
        transcript on a ``predict_long`` result, up to ``ALIGN_LONG_MAX_TARGET``) runs ``amx_ctc_align_long``."""
        names, N, L, T, O, frame_lengths, lengths_pointer, stream = self._predictions_call(predictions)
        rows = self._target_rows(predictions, targets, names, N, "align")
        limit = _alignment.ALIGN_MAX_TARGET if long is False else _alignment.ALIGN_LONG_MAX_TARGET
        offsets, ids, counts = _alignment.pack_targets(rows, limit=limit)
        max_target = max(counts)
        long = _alignment.use_long(max_target, long)
        entry = self._lib.amx_ctc_align_long if long else self._lib.amx_ctc_align
        with torch.cuda.device(self._device):
            meta = torch.cat([offsets, ids, torch.zeros(1, dtype=torch.int32)]).to(self._device)
            b = _alignment.allocate(self._lib, O * N, T, max_target, self._device, long)
            code = entry(
                self._handle, C.c_void_p(predictions._flat.data_ptr()), lengths_pointer, N, L, C.c_void_p(meta.data_ptr()),
                C.c_void_p(meta.data_ptr() + 4 * (O * N + 1)), max_target, *b.pointers(), C.c_void_p(stream))
            _lib.check(self._lib, self._handle, code)
        return _alignment.Aligned(names, [name for name in names if name in targets], b.paths.view(O, N, T),
                                  b.frame_scores.view(O, N, T), b.spans.view(O, N, max_target, 2),
                                  b.span_scores.view(O, N, max_target), b.totals.view(O, N), b.status.view(O, N),
                                  frame_lengths.tolist(), [counts[o * N:(o + 1) * N] for o in range(O)])

    def align(self, predictions: Predictions, targets: Dict[str, Sequence[Sequence[int]]], long: Optional[bool] = None
              ) -> Dict[str, List[Optional["_alignment.Alignment"]]]:
        """``align_device`` fetched to the host: per output with targets and utterance an ``Alignment`` (``None`` where no
        alignment exists)."""
        return self.align_device(predictions, targets, long).alignments()

    def align_graph_device(self, predictions: Predictions, graphs: Dict[str, Sequence["_graph_alignment.TargetGraph"]]
                           ) -> "_graph_alignment.GraphAligned":
        """On-device CTC forced alignment over pronunciation graphs (``amx_ctc_align_graph``) of every output of
        ``predictions``: ``graphs`` maps an output name to one ``TargetGraph`` per utterance (``TargetGraph.from_slots`` over
        ``graph_alignment.slot_targets`` builds them from symbols).  An output without an entry is aligned against the graph
        of no nodes and left out of ``GraphAligned.present``.  The result stays in HBM."""
        names, N, L, T, O, frame_lengths, lengths_pointer, stream = self._predictions_call(predictions)
        rows = self._target_rows(predictions, graphs, names, N, "align")
        rows = [row if isinstance(row, _graph_alignment.TargetGraph) else _graph_alignment.TargetGraph.chain(row) for row in rows]
        packed, starts, counts = _graph_alignment.pack_graphs(rows)
        max_nodes = max(counts)
        with torch.cuda.device(self._device):
            meta = packed.to(self._device)
            b = _graph_alignment.allocate(self._lib, O * N, T, max_nodes, self._device)
            code = self._lib.amx_ctc_align_graph(
                self._handle, C.c_void_p(predictions._flat.data_ptr()), lengths_pointer, N, L,
                *_graph_alignment.graph_pointers(meta, starts), max_nodes, *b.pointers(), C.c_void_p(stream))
            _lib.check(self._lib, self._handle, code)
        return _graph_alignment.GraphAligned(
            names, [name for name in names if name in graphs], b.paths.view(O, N, T), b.frame_scores.view(O, N, T),
            b.spans.view(O, N, max_nodes, 2), b.span_scores.view(O, N, max_nodes), b.totals.view(O, N), b.status.view(O, N),
            frame_lengths.tolist(), [rows[o * N:(o + 1) * N] for o in range(O)])

    def align_graph(self, predictions: Predictions, graphs: Dict[str, Sequence["_graph_alignment.TargetGraph"]]
                    ) -> Dict[str, List[Optional["_graph_alignment.GraphAlignment"]]]:
        """``align_graph_device`` fetched to the host: per output with graphs and utterance a ``GraphAlignment`` (``None``
        where no path exists)."""
        return self.align_graph_device(predictions, graphs).alignments()

    def _score_call(self, call, predictions: Predictions, candidates: int, meta: Tensor, max_target: int, posteriors: bool):
        """``amx_ctc_score`` over every output of ``predictions`` (``call`` is their ``_predictions_call``): ``meta`` holds the
        device int32 offsets ``[O * N * candidates + 1]`` followed by the ids.  Returns the buffers."""
        _, N, L, T, O, _, lengths_pointer, stream = call
        rows = O * N * candidates
        b = _scoring.allocate(self._lib, rows, T, max_target, self._device, posteriors)
        code = self._lib.amx_ctc_score(
            self._handle, C.c_void_p(predictions._flat.data_ptr()), lengths_pointer, N, L, candidates,
            C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 4 * (rows + 1)), max_target, *b.pointers(),
            C.c_void_p(stream))
        _lib.check(self._lib, self._handle, code)
        return b

    def score_device(self, predictions: Predictions, targets: Dict[str, Sequence[Sequence[int]]],
                     posteriors: bool = False) -> "_scoring.Scored":
        """On-device CTC forward-backward scoring (``amx_ctc_score``) of every output of ``predictions`` against ``targets``,
        given as ``align_device`` takes them: the log-likelihood of each target sequence and, per target, its posterior
        occupancy, position and score sums (with ``posteriors`` also the state posteriors of every frame).  An output without
        an entry is scored against nothing and left out of ``Scored.present``.  The result stays in HBM, leading shape
        ``[O, N, 1]``."""
        call = names, N, _, T, O, frame_lengths, _, _ = self._predictions_call(predictions)
        offsets, ids, counts = _scoring.pack_targets(self._target_rows(predictions, targets, names, N, "score"))
        max_target = max(counts)
        with torch.cuda.device(self._device):
            meta = torch.cat([offsets, ids, torch.zeros(1, dtype=torch.int32)]).to(self._device)
            b = self._score_call(call, predictions, 1, meta, max_target, posteriors)
        return _scoring.scored(b, (O, N, 1), T, max_target, names, [name for name in names if name in targets],
                               frame_lengths.tolist(), counts)

    def score(self, predictions: Predictions, targets: Dict[str, Sequence[Sequence[int]]], posteriors: bool = False
              ) -> Dict[str, List[Optional["_scoring.Score"]]]:
        """``score_device`` fetched to the host: per output with targets and utterance a ``Score`` (``None`` where the targets
        have no path through the frames)."""
        return {name: [row[0] for row in rows] for name, rows in self.score_device(predictions, targets, posteriors).scores().items()}

    def rescore_device(self, predictions: Predictions, beam_decoded: "BeamDecoded") -> "_scoring.Rescored":
        """The exact log P(hypothesis | emissions) of every hypothesis of ``beam_decoded`` (``beam_decode_device`` of these
        predictions), whose own scores are those of a pruned search, and the softmax over each n-best list.  The targets are
        packed on the device from ``tokens`` / ``counts``; the host synchronises once, for their sizes."""
        call = self._predictions_call(predictions)
        names, N = call[:2]
        O, Nb, B, T = beam_decoded.tokens.shape
        if beam_decoded.names != names or Nb != N or N == 0:
            raise ValueError("beam_decoded does not belong to these predictions")
        with torch.cuda.device(self._device):
            present = torch.arange(B, device=self._device).view(1, 1, B) < beam_decoded.hyp_counts.view(O, N, 1)
            counts = torch.where(present, beam_decoded.counts, torch.zeros_like(beam_decoded.counts)).reshape(-1).to(torch.int64)
            ends = torch.cumsum(counts, 0)
            total, max_target = (int(v) for v in torch.stack([ends[-1], counts.max()]).cpu())  # the one synchronisation
            if max_target > _scoring.SCORE_MAX_TARGET:
                raise ValueError(f"at most {_scoring.SCORE_MAX_TARGET} targets per row on the device, got {max_target}")
            at = torch.arange(total, device=self._device)
            row = torch.searchsorted(ends, at, right=True)
            ids = beam_decoded.tokens.reshape(-1, T)[row, at - (ends - counts)[row]]
            meta = torch.cat([torch.zeros(1, dtype=torch.int64, device=self._device), ends, ids,
                              torch.zeros(1, dtype=torch.int64, device=self._device)]).to(torch.int32)
            b = self._score_call(call, predictions, B, meta, max_target, False)
            ll = torch.where(present, b.log_likelihood.view(O, N, B), torch.full((), -math.inf, device=self._device))
            return _scoring.Rescored(names, ll, torch.nan_to_num(torch.softmax(ll, -1), nan=0.0), b.status.view(O, N, B))

    def search_device(self, predictions: Predictions, queries: Sequence[Sequence[int]], output: str,
                      curves: bool = False) -> "_search.Found":
        """On-device CTC search (``amx_ctc_search_emissions``) of every utterance of ``predictions.outputs[output]`` for every
        query (class indices of that output under the predictions' own inventory, e.g. from ``query_targets``): where each
        query occurs best, and with ``curves`` the best occurrence ending at every frame (``Found.hits``).  The output's
        ``[T, N, C]`` tensor is read in place through its transposed view; the result stays in HBM."""
        if output not in predictions.outputs:
            raise ValueError(f"unknown output {output!r}, the predictions hold {list(predictions.outputs.keys())}")
        return _search.ctc_search(predictions.outputs[output].transpose(0, 1), predictions.lengths, queries, 0, curves)

    def search(self, predictions: Predictions, queries: Sequence[Sequence[int]], output: str
               ) -> List[List[Optional["_search.Hit"]]]:
        """``search_device`` fetched to the host: per utterance and query the best ``Hit`` (``None`` where the query does not
        occur)."""
        return self.search_device(predictions, queries, output).best()

    def variants_device(self, predictions: Predictions, targets, output: str) -> "_variants.Variants":
        """On-device CTC scoring of every one-edit variant (``amx_ctc_variants_emissions``) of each utterance's transcript on
        ``predictions.outputs[output]``: each symbol substituted by each class or deleted, and each class inserted into each
        gap.  ``targets`` are as for ``score_device``, restricted to this output: its rows (class indices under the
        predictions' own inventory, e.g. from ``label_targets``), or a dict that holds them under ``output``.  The output's
        ``[T, N, C]`` tensor is read in place through its transposed view; the result stays in HBM."""
        if output not in predictions.outputs:
            raise ValueError(f"unknown output {output!r}, the predictions hold {list(predictions.outputs.keys())}")
        if isinstance(targets, dict):
            if list(targets) != [output]:
                raise ValueError(f"variants take the targets of the one output {output!r}, got {list(targets)}")
            targets = targets[output]
        return _variants.ctc_variants(predictions.outputs[output].transpose(0, 1), predictions.lengths, targets, 0)

    def variants(self, predictions: Predictions, targets, output: str, threshold: float = 0.0
                 ) -> List[Optional[List["_variants.Finding"]]]:
        """``variants_device`` fetched to the host: per utterance the single edits that beat the transcript by more than
        ``threshold`` nats (``Variants.diagnose``), ``None`` for an utterance of no frames whose transcript is not empty."""
        return self.variants_device(predictions, targets, output).diagnose(threshold)

    def debug_fetch(self, what: str, index: int = 0) -> Tensor:
        """Test hook: intermediates of the last ``predict(..., _keep_hidden=True)`` as CPU fp32 tensors.  Without the flag a pass
        still hands out ``"hidden"`` i where a classifier reads ``OUTPUT_i`` and, for the pre-LN encoder, the final one, in the
        [N, T] layout whatever rows the pass ran on (frames beyond an utterance of rows packed early: zeros)."""
        code_of = {"conv": 0, "hidden": 1, "logits": 2}
        n_t = self._last_geometry()
        if what == "conv":
            shape = (n_t[0], n_t[1], self._spec["conv_dim"])
        elif what == "hidden":
            shape = (n_t[0], n_t[1], self._spec["hidden"])
        else:
            shape = None
        ld = C.c_int64(0)
        if shape is None:
            buf = torch.empty(n_t[0] * n_t[1] * 4096, dtype=torch.float32)
        else:
            buf = torch.empty(shape, dtype=torch.float32)
        code = self._lib.amx_debug_fetch(self._handle, code_of[what], index, C.c_void_p(buf.data_ptr()), buf.numel(), C.byref(ld))
        _lib.check(self._lib, self._handle, code)
        if shape is None:
            return buf[: n_t[0] * n_t[1] * ld.value].view(n_t[0] * n_t[1], ld.value)
        return buf

    def _debug_scribble(self, word16: int) -> None:
        """Test hook (``amx_debug_scribble``): fills every data workspace of the handle, over its whole allocation, with the
        16-bit word ``word16`` repeated, in stream order.  The next ``predict`` must give the bits it gives on a fresh handle."""
        if not hasattr(self._lib, "amx_debug_scribble"):
            raise RuntimeError("this build of liballophant_amx has no amx_debug_scribble")
        stream = torch.cuda.current_stream(self._device).cuda_stream
        with torch.cuda.device(self._device):
            _lib.check(self._lib, self._handle, self._lib.amx_debug_scribble(self._handle, int(word16), C.c_void_p(stream)))

    def _last_geometry(self) -> Tuple[int, int]:
        if not hasattr(self, "_geom"):
            raise RuntimeError("no forward pass yet")
        return self._geom

    def timing_fetch(self) -> Dict[str, Tuple[float, int]]:
        """Measurement hook: {kernel class: (total ms, launches)} of the ``predict(..., _timing=True)`` calls since the
        previous fetch, from HIP events recorded on the launch stream."""
        n = len(_lib.KERNEL_CLASSES)
        ms = (C.c_float * n)()
        launches = (C.c_int32 * n)()
        _lib.check(self._lib, self._handle, self._lib.amx_timing_fetch(self._handle, ms, launches, n))
        return {k: (float(ms[i]), int(launches[i])) for i, k in enumerate(_lib.KERNEL_CLASSES)}

    def graph_info(self) -> Tuple[int, int]:
        """(forward passes recorded into HIP graphs, passes replayed from one) so far -- ``amx_graph_info``."""
        if _lib.AMX_ABI_VERSION < 5:
            return 0, 0
        captures, replays = C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib, self._handle, self._lib.amx_graph_info(self._handle, C.byref(captures), C.byref(replays)))
        return int(captures.value), int(replays.value)

    def pass_info(self) -> Dict[str, int]:
        """Which optional forms the last ``predict`` took (``amx_pass_info``): ``ln_fold`` 1 = LayerNorm folded into the encoder
        products, ``packed`` 0 / 1 / 2 = padded rows / packed layers / packed from the feature projection on, ``graph`` 0 / 1 / 2
        = eager / recorded / replayed, ``rows`` = frames the encoder layers worked on, ``id`` = number of the pass, ``attention`` = the
        form of the attention kernels (0 / 1: 8- / 4-wave workgroups, 2: 4 waves with the key split, 3: the long-key kernel, 4 / 5:
        a head dimension other than 64 on 64- / 128-wide rows), ``conv0`` = the kernels of conv layer 0 (see ``conv0_route``)."""
        if _lib.AMX_ABI_VERSION < 6:
            return {}
        n = len(_lib.PASS_INFO)
        info = (C.c_int32 * n)()
        _lib.check(self._lib, self._handle, self._lib.amx_pass_info(self._handle, info, n))
        return {k: int(info[i]) for i, k in enumerate(_lib.PASS_INFO)}

    def conv0_route(self) -> Dict[str, Any]:
        """The kernels conv layer 0 of this model runs in (``AMX_PASS_INFO_CONV0``; fixed when the estimator is built): ``apply``
        ``"mfma"`` (matrix pipe) or ``"scalar"`` with the ``kw`` taps and ``cpl`` channels per lane the kernel is instantiated for,
        and ``stats``, where the normalisation statistics come from (``lib.CONV0_STATS``)."""
        code = self.pass_info()["conv0"]
        kw, cpl = code // 100 % 100, code % 100
        return {"apply": "scalar" if cpl else "mfma", "kw": kw, "cpl": cpl, "stats": _lib.CONV0_STATS[code // 10000]}

    def check_finite(self) -> None:
        """Range check of the last ``predict`` (``amx_check_finite``; no upstream counterpart -- the reference computes in
        fp32): waits for the stream and raises ``FloatingPointError`` when a valid frame holds non-finite logits, i.e. an
        activation left the range of the fp16 planes (|x| <= 65504) or the audio was not finite.  Weights cannot cause it:
        they are packed under per-tensor power-of-two scales.  ``precision="bf16x3"`` has the range of fp32."""
        stream = torch.cuda.current_stream(self._device).cuda_stream
        _lib.check(self._lib, self._handle, self._lib.amx_check_finite(self._handle, C.c_void_p(stream), None))

    def synchronize(self) -> None:
        """Waits for the stream; raises ``FloatingPointError`` if a pass issued since the last report left the range of the
        planes (``amx_synchronize`` -> ``AMX_ERANGE``)."""
        stream = torch.cuda.current_stream(self._device).cuda_stream
        _lib.check(self._lib, self._handle, self._lib.amx_synchronize(self._handle, C.c_void_p(stream)))

    def close(self) -> None:
        if getattr(self, "_handle", None):
            self._lib.amx_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GreedyCTCDecoder:
    """``GreedyCTCDecoder`` with the reference's signature (predictions.py:189-207), decoding on the device:

        decoder = GreedyCTCDecoder()
        hypotheses = decoder(outputs.transpose(1, 0), model_outputs.lengths)     # run.py:767-774, README.md:120-125

    ``log_emissions`` is a ``[N, T, C]`` fp32 tensor on an MI355X (any strides with a unit class stride: the transposed
    view of a ``[T, N, C]`` output is read in place, no copy), ``lengths`` the ``[N]`` frame lengths.  Returns, per
    utterance, ``[CTCHypothesis(tokens, [], score, timesteps)]`` like the reference.  There is no CPU path.

    Also accepted, for the whole-prediction form: ``GreedyCTCDecoder(estimator)(predictions)`` decodes every output of a
    ``Predictions`` object in one launch (``Estimator.greedy_decode``)."""

    def __init__(self, blank_index_or_estimator=0, blank_index: Optional[int] = None):
        self._estimator = None
        if isinstance(blank_index_or_estimator, Estimator):
            self._estimator = blank_index_or_estimator
            self._blank_index = 0 if blank_index is None else int(blank_index)
            if self._blank_index != 0:
                raise ValueError("the CTC blank of model outputs is index 0 (config.py:555)")
        else:
            self._blank_index = int(blank_index_or_estimator)

    def __call__(self, log_emissions, lengths: Optional[Tensor] = None):
        if isinstance(log_emissions, Predictions):
            if self._estimator is None:
                raise ValueError("decoding a Predictions object needs GreedyCTCDecoder(estimator)")
            return self._estimator.greedy_decode(log_emissions)
        if lengths is None:
            raise TypeError("__call__() missing 1 required positional argument: 'lengths'")
        return greedy_ctc_decode(log_emissions, lengths, self._blank_index)


def greedy_ctc_decode(log_emissions: Tensor, lengths: Tensor, blank_index: int = 0) -> List[List[CTCHypothesis]]:
    """``GreedyCTCDecoder.__call__`` (reference predictions.py:194-207) through ``amx_greedy_ctc_emissions``."""
    log_emissions, N, T, Cn = _ctc.emissions(log_emissions, "decodes")
    lib = _lib.load()
    device = log_emissions.device
    _ctc.check_classes(Cn, blank_index)
    if N == 0:
        return []
    with torch.cuda.device(device):
        frame_lengths, index, stream = _ctc.frame(log_emissions, lengths.detach())  # (the lengths are required here)
        tokens = torch.empty(N, T, dtype=torch.int64, device=device)
        timesteps = torch.empty_like(tokens)
        counts = torch.empty(N, dtype=torch.int32, device=device)
        scores = torch.empty(N, dtype=torch.float32, device=device)
        code = lib.amx_greedy_ctc_emissions(
            index, C.c_void_p(log_emissions.data_ptr()), log_emissions.stride(0), log_emissions.stride(1),
            C.c_void_p(frame_lengths.data_ptr()), N, T, Cn, blank_index, C.c_void_p(tokens.data_ptr()),
            C.c_void_p(timesteps.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(scores.data_ptr()),
            C.c_void_p(stream))
        _lib.check(lib, None, code)
        counts_h, scores_h, tokens_h, timesteps_h = counts.cpu(), scores.cpu(), tokens.cpu(), timesteps.cpu()
    result = []
    for n in range(N):
        k = int(counts_h[n])
        result.append([CTCHypothesis(tokens_h[n, :k].clone(), [], float(scores_h[n]), timesteps_h[n, :k].clone())])
    return result


def _check_beam(beam_width: int, n_best: int) -> None:
    if n_best > beam_width:
        raise ValueError("N-best can not exceed beam width")
    if not 1 <= beam_width <= _lib.BEAM_MAX_WIDTH:
        raise ValueError(f"beam_width must be 1 to {_lib.BEAM_MAX_WIDTH} on the device, got {beam_width}")
    if n_best < 1:
        raise ValueError(f"n_best must be at least 1, got {n_best}")


class BeamCTCDecoder:
    """``BeamCTCDecoder`` with the reference's signature (predictions.py:210-229), decoding on the device:

        decoder = BeamCTCDecoder(["<blank>", *categories], beam_width, n_best)
        hypotheses = decoder(outputs.transpose(1, 0), model_outputs.lengths)

    Upstream this is torchaudio's flashlight ``ctc_decoder`` (lexicon-free, no LM, blank = silence, log_add) called on
    ``log_emissions.exp()``; here ``amx_beam_ctc_emissions`` reads the fp32 ``[N, T, C]`` tensor in place (any strides with a
    unit class stride) and exponentiates each value as it is read.  Returns, per utterance, up to ``n_best``
    ``CTCHypothesis(tokens, [], score, timesteps)``, best first.  There is no CPU path.

    ``lm`` (keyword-only, a ``PhonotacticLM`` over the decoder's tokens) fuses a phonotactic bigram into the search, see
    ``beam_ctc_decode``; upstream's decoder has no such argument."""

    def __init__(self, tokens: List[str], beam_width: int, n_best: int = 1, blank_index: int = 0, *, lm=None,
                 lm_weight: float = 1.0, token_score: float = 0.0) -> None:
        _check_beam(beam_width, n_best)
        self._tokens = list(tokens)
        if not 0 <= blank_index < len(self._tokens):
            raise ValueError("blank_index out of range")
        self._beam_width = int(beam_width)
        self._n_best = int(n_best)
        self._blank_index = int(blank_index)
        if lm is not None:
            _phonotactics.check_scalars(lm_weight, token_score)
            if not isinstance(lm, PhonotacticLM) or lm.classes != len(self._tokens) or lm.blank != self._blank_index:
                raise ValueError(f"lm must be a PhonotacticLM over the decoder's {len(self._tokens)} tokens and its blank")
        self._lm, self._lm_weight, self._token_score = lm, float(lm_weight), float(token_score)

    def __call__(self, log_emissions: Tensor, lengths: Optional[Tensor] = None) -> List[List[CTCHypothesis]]:
        if log_emissions.dim() == 3 and log_emissions.shape[2] != len(self._tokens):
            raise ValueError(f"emissions have {log_emissions.shape[2]} classes, the decoder {len(self._tokens)} tokens")
        return beam_ctc_decode(log_emissions, lengths, self._beam_width, self._n_best, self._blank_index, lm=self._lm,
                               lm_weight=self._lm_weight, token_score=self._token_score)


def beam_ctc_decode(log_emissions: Tensor, lengths: Optional[Tensor], beam_width: int, n_best: int = 1, blank_index: int = 0,
                    exp_emissions: bool = True, *, lm=None, lm_weight: float = 1.0, token_score: float = 0.0,
                    lm_ids=None) -> List[List[CTCHypothesis]]:
    """``BeamCTCDecoder.__call__`` (reference predictions.py:231-233) through ``amx_beam_ctc_emissions``; ``exp_emissions``
    False adds the values as given instead of their exponentials.

    With ``lm`` (a ``PhonotacticLM`` over the emissions' classes, or a sequence of them with one ``lm_ids`` index per
    utterance, -1 for none) the search runs through ``amx_beam_ctc_lm_emissions``: a new token ``n`` after the prefix ``P``
    adds ``lm_weight * lm[last(P), n] + token_score``, the end ``lm_weight * lm[last(P), end]``, and the scores are the
    fused totals.  Meant for ``exp_emissions=False``."""
    log_emissions, N, _, Cn = _ctc.emissions(log_emissions, "decodes")
    _check_beam(beam_width, n_best)
    fusion = None
    if lm is not None:
        _phonotactics.check_scalars(lm_weight, token_score)
        lms, ids = _phonotactics.lm_call(lm, lm_ids, N)
        if any(m.classes != Cn or m.blank != blank_index for m in lms):
            raise ValueError(f"the language model must have the emissions' {Cn} classes and blank {blank_index}")
        if Cn > _lib.BEAM_LM_MAX_CLASSES:
            raise ValueError(f"beam search with a language model takes at most {_lib.BEAM_LM_MAX_CLASSES} classes")
    _lib.load()
    _ctc.check_classes(Cn, blank_index)
    if N == 0:
        return []
    if lm is not None:
        fusion = (PhonotacticLM.stack(lms).to(log_emissions.device), ids, float(lm_weight), float(token_score))
    return _beam_hypotheses(*_beam_ctc_rows(log_emissions, lengths, beam_width, n_best, blank_index, exp_emissions, fusion))


def _beam_ctc_rows(log_emissions: Tensor, lengths: Optional[Tensor], beam_width: int, n_best: int, blank_index: int,
                   exp_emissions: bool, fusion=None) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """``amx_beam_ctc_emissions`` over ``[N, T, C]`` emissions, ``N >= 1``: the device tensors ``tokens`` / ``timesteps``
    ``[N, n_best, T]``, ``counts`` / ``scores`` ``[N, n_best]`` and ``hyp_counts`` ``[N]``.  With ``fusion`` (the device stack
    ``[n_lm, C + 1, C + 1]``, the int32 host ``lm_ids`` ``[N]``, ``lm_weight``, ``token_score``) through
    ``amx_beam_ctc_lm_emissions``."""
    log_emissions, N, T, Cn = _ctc.emissions(log_emissions, "decodes")
    _check_beam(beam_width, n_best)
    lib = _lib.load()
    device = log_emissions.device
    _ctc.check_classes(Cn, blank_index)
    if fusion is not None and not hasattr(lib, "amx_beam_ctc_lm_emissions"):
        raise RuntimeError(f"{_lib.LIB_PATH} predates beam search with a language model (amx_beam_ctc_lm_emissions): rebuild it")
    with torch.cuda.device(device):
        frame_lengths, index, stream = _ctc.frame(log_emissions, lengths)
        size = C.c_size_t()
        _lib.check(lib, None, lib.amx_beam_ctc_workspace(beam_width, N, T, C.byref(size)))
        workspace = torch.empty(max(1, size.value), dtype=torch.uint8, device=device)
        tokens = torch.empty(N, n_best, T, dtype=torch.int64, device=device)
        timesteps = torch.empty_like(tokens)
        counts = torch.empty(N, n_best, dtype=torch.int32, device=device)
        scores = torch.empty(N, n_best, dtype=torch.float64, device=device)
        hyp_counts = torch.empty(N, dtype=torch.int32, device=device)
        head = (index, C.c_void_p(log_emissions.data_ptr()), log_emissions.stride(0), log_emissions.stride(1),
                C.c_void_p(frame_lengths.data_ptr()), N, T, Cn, blank_index, beam_width, n_best,
                _lib.BEAM_EXP_EMISSIONS if exp_emissions else 0)
        tail = (C.c_void_p(workspace.data_ptr()), size.value, C.c_void_p(tokens.data_ptr()), C.c_void_p(timesteps.data_ptr()),
                C.c_void_p(counts.data_ptr()), C.c_void_p(scores.data_ptr()), C.c_void_p(hyp_counts.data_ptr()), C.c_void_p(stream))
        if fusion is None:
            code = lib.amx_beam_ctc_emissions(*head, *tail)
        else:
            stack, lm_ids, lm_weight, token_score = fusion
            if stack.dim() != 3 or tuple(stack.shape[1:]) != (Cn + 1, Cn + 1) or stack.dtype != torch.float32:
                raise ValueError(f"the language-model stack must be fp32 [n_lm, {Cn + 1}, {Cn + 1}]")
            stack = stack.to(device).contiguous()
            ids = lm_ids.to(device=device, dtype=torch.int32).contiguous()
            code = lib.amx_beam_ctc_lm_emissions(*head, C.c_void_p(stack.data_ptr()), stack.shape[0], C.c_void_p(ids.data_ptr()),
                                                 lm_weight, token_score, *tail)
            current = torch.cuda.current_stream(device)
            stack.record_stream(current), ids.record_stream(current)
        _lib.check(lib, None, code)
        return tokens, timesteps, counts, scores, hyp_counts


def _ctc_decoder(categories, beam_width: int = 1, n_best: int = 1):
    """``predictions._ctc_decoder`` (reference predictions.py:236-242): greedy for a beam of one, else a beam-search decoder
    over ``["<blank>", *categories]``."""
    if n_best > beam_width:
        raise ValueError("N-best can not exceed beam width")
    if beam_width == 1:
        return GreedyCTCDecoder()
    return BeamCTCDecoder(["<blank>", *categories], beam_width, n_best)


def feature_decoders(indexer, beam_width: int = 1, feature_names=None, n_best: int = 1) -> Dict[str, Any]:
    """``predictions.feature_decoders`` (reference predictions.py:245-254): one decoder per feature name of ``indexer`` (an
    ``AttributeTable`` or anything with ``feature_names``, and ``feature_categories`` for a beam): ``GreedyCTCDecoder`` for
    ``beam_width == 1``, else ``BeamCTCDecoder`` over ``["<blank>", *indexer.feature_categories(name)]``."""
    if n_best > beam_width:
        raise ValueError("N-best can not exceed beam width")
    names = indexer.feature_names if feature_names is None else feature_names
    if beam_width == 1:
        return {name: GreedyCTCDecoder() for name in names}
    return {name: _ctc_decoder(indexer.feature_categories(name), beam_width, n_best) for name in names}

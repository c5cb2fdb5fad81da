"""Stage-local evaluation of ``Estimator.predict`` (CPU only): every stage of the path as a function of its own input, written
once and evaluated three ways -- float64 (the truth), plain fp32 (context), and fp32 with every matrix product taken as
hi.hi + lo.hi + hi.lo on 16-bit planes (what the split-precision kernels are meant to compute).

The stages restate ``oracle/allophant_oracle.py`` (``feature_encoder``, ``wav2vec2_hidden_states``, ``projection_forward``,
``time_layer_forward``) with a product hook in place of ``F.linear`` / ``F.conv1d`` / ``@``; tests/test_stage_util.py pins them to the
oracle.  The oracle's dtype-generic helpers are used as they are.

  conv    normalised audio [N, L]        -> conv_out [N, T, C]      the 7-layer extractor, layer-norm and group-norm family
  front   conv_out                       -> hidden[0]               feature-projection LayerNorm, projection, frame mask, the
                                                                    weight-normed grouped positional convolution (last frame
                                                                    dropped, GELU); post-LN: + the encoder LayerNorm
  layer   hidden[i]                      -> hidden[i + 1]           pre-LN (the last layer includes the final LayerNorm, as
                                                                    hidden_states[layers] does) and post-LN
  heads   hidden[layers] (+ hidden[i])   -> logits, log-probs       projections, composition, dependency concatenation with
                                                                    softmax, time-layer heads, log-softmax
  entry   audio [N, L]                   -> hidden[0]               normalisation + conv + front   } what a pass without the keep
  tail    hidden[layers - 1] (+ taps)    -> logits, log-probs       the last layer + heads         } flag leaves to look at

Products (the names ``Evaluation(drop=(name, "lo_x" | "lo_w"))`` takes): ``conv1`` .. ``conv6`` and ``pos_conv`` as implicit
GEMMs, ``feature_projection``, per layer ``q_proj k_proj v_proj qk pv out_proj ffn1 ffn2``, per classifier ``<name>.linear``,
``<name>.compose`` and for a time layer ``<name>.input_projection .in_proj .qk .pv .out_proj``.  Conv layer 0 is not a split
product (the device evaluates it to fp32 grade from fp64 tables): it runs in the evaluation's dtype.

Everything is batch-major ([N, T, ...]); the metric is ``max_abs_valid``: max abs over the valid frames.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from allophant_amd import spec as S, synthetic
from oracle import allophant_oracle as O

AM = "_acoustic_model._model."
PROJ = "_projection._layers."
PLANES = {"f16x3": torch.float16, "bf16x3": torch.bfloat16}
_cast: list = []  # [state dict, its float64 copy]


class Evaluation:
    """How a stage is evaluated.  ``mode``: "truth" (float64), "fp32", "f16x3" or "bf16x3" (fp32 with split products; planes
    ``x.half()`` / ``(x - hi).half()``, or ``.bfloat16()``).  ``drop = (product, "lo_x" | "lo_w")`` leaves the cross term with
    the low plane of the activation / of the weight out of that one product.  ``seen`` lists the products evaluated."""

    def __init__(self, mode: str = "fp32", drop: Optional[Tuple[str, str]] = None):
        if mode not in ("truth", "fp32") and mode not in PLANES:
            raise ValueError(mode)
        if drop is not None and (mode not in PLANES or drop[1] not in ("lo_x", "lo_w")):
            raise ValueError("a cross term can only be dropped from a split product")
        self.mode = mode
        self.dtype = torch.float64 if mode == "truth" else torch.float32
        self.plane = PLANES.get(mode)
        self.drop = drop
        self.seen: List[str] = []

    def weights(self, state: Dict[str, Tensor]) -> Dict[str, Tensor]:
        """``state`` in the evaluation's dtype (the float64 copy of the last state dict is kept: a case evaluates many stages of one)"""
        if self.dtype == torch.float32:
            return state
        if _cast and _cast[0] is state:
            return _cast[1]
        _cast[:] = [state, {k: v.to(self.dtype) if v.is_floating_point() else v for k, v in state.items()}]
        return _cast[1]

    def _split(self, x: Tensor) -> Tuple[Tensor, Tensor]:
        hi = x.to(self.plane).float()
        return hi, (x - hi).to(self.plane).float()

    def matmul(self, name: str, x: Tensor, w: Tensor) -> Tensor:
        """``x @ w`` (x the activation [..., M, K], w [..., K, N]) as product ``name``."""
        if name not in self.seen:
            self.seen.append(name)
        if self.plane is None:
            return x @ w
        xh, xl = self._split(x)
        wh, wl = self._split(w)
        out = xh @ wh
        if self.drop != (name, "lo_x"):
            out = out + xl @ wh
        if self.drop != (name, "lo_w"):
            out = out + xh @ wl
        return out

    def linear(self, name: str, x: Tensor, weight: Tensor, bias: Optional[Tensor] = None) -> Tensor:
        out = self.matmul(name, x, weight.t())
        return out if bias is None else out + bias


def max_abs_valid(got: Tensor, want: Tensor, frame_lengths: Sequence[int]) -> float:
    """max |got - want| over the first ``frame_lengths[n]`` frames of every utterance of two [N, T, ...] tensors"""
    worst = 0.0
    for n, t in enumerate(int(v) for v in frame_lengths):
        worst = max(worst, float((got[n, :t].double() - want[n, :t].double()).abs().max()))
    return worst


def normalize(audio: Tensor, lengths: Tensor, spec: Dict[str, Any], ev: Evaluation) -> Tensor:
    """the input normalisation in front of the conv stage (acoustic_model.py:762-767), in the evaluation's dtype"""
    x = audio.to(ev.dtype)
    if not spec.get("do_normalize", True):
        return x
    return O.zero_mean_unit_var_norm(x, lengths, O.mask_sequence(lengths, audio.shape[1]))


# ----------------------------------------------------------------------------------------------------------------------------
# conv
# ----------------------------------------------------------------------------------------------------------------------------
def conv_stage(x: Tensor, state: Dict[str, Tensor], spec: Dict[str, Any], ev: Evaluation, first: int = 0,
               last: Optional[int] = None) -> Tensor:
    """Conv layers ``first`` .. ``last - 1`` of the extractor (default: all).  ``x``: normalised audio [N, L] for ``first == 0``,
    else the output [N, T, C] of layer ``first - 1``.  Returns [N, T', C].  Layers >= 1 are implicit GEMMs, summed tap by tap."""
    sd = ev.weights(state)
    group = spec.get("feat_extract_norm", "layer") == "group"
    kernels, strides = spec["conv_kernel"], spec["conv_stride"]
    h = x.to(ev.dtype)
    for i in range(first, len(kernels) if last is None else last):
        k, s = kernels[i], strides[i]
        p = f"{AM}feature_extractor.conv_layers.{i}."
        w = sd[p + "conv.weight"]
        bias = sd[p + "conv.bias"] if spec.get("conv_bias", True) else None
        if i == 0:
            h = F.conv1d(h.unsqueeze(1), w, bias, stride=s)  # [N, C, T]
            if group:  # GroupNorm of one channel per group: statistics over the time of the padded tensor
                h = F.group_norm(h, h.shape[1], sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], 1e-5)
            h = h.transpose(1, 2)
        else:
            rows = (h.shape[1] - k) // s + 1
            out = None
            for j in range(k):
                tap = ev.matmul(f"conv{i}", h[:, j: j + s * (rows - 1) + 1: s], w[:, :, j].t())
                out = tap if out is None else out + tap
            h = out if bias is None else out + bias
        if not group:
            h = F.layer_norm(h, (h.shape[-1],), sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], 1e-5)
        h = F.gelu(h)
    return h


# ----------------------------------------------------------------------------------------------------------------------------
# front
# ----------------------------------------------------------------------------------------------------------------------------
def front_stage(conv_out: Tensor, frame_lengths: Tensor, state: Dict[str, Tensor], spec: Dict[str, Any], ev: Evaluation) -> Tensor:
    """conv_out [N, T, C] -> hidden[0] [N, T, D]"""
    sd = ev.weights(state)
    eps = spec["eps"]
    feats = conv_out.to(ev.dtype)
    N, T, C = feats.shape
    p = AM + "feature_projection."
    h = F.layer_norm(feats, (C,), sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], eps)
    h = ev.linear("feature_projection", h, sd[p + "projection.weight"], sd[p + "projection.bias"])
    if spec.get("use_attention_mask", True):
        h = h * (torch.arange(T).unsqueeze(0) < frame_lengths.unsqueeze(1)).unsqueeze(-1)
    D = h.shape[-1]
    k, groups = spec["pos_kernel"], spec["pos_groups"]
    cg = D // groups
    weight = O._pos_conv_weight(sd)  # [D, cg, k]
    # Conv1d(padding = k // 2) and, for an even k, its last frame dropped: frame t reads padded frames t .. t + k - 1
    windows = F.pad(h, (0, 0, k // 2, k // 2)).unfold(1, k, 1)[:, :T]  # [N, T, D, k]
    pos = torch.cat([
        ev.matmul("pos_conv", windows[:, :, g * cg:(g + 1) * cg].reshape(N, T, cg * k),
                  weight[g * cg:(g + 1) * cg].reshape(cg, cg * k).t())
        for g in range(groups)], -1) + sd[AM + "encoder.pos_conv_embed.conv.bias"]
    h = h + F.gelu(pos)
    if not spec.get("stable_layer_norm", True):
        h = F.layer_norm(h, (D,), sd[AM + "encoder.layer_norm.weight"], sd[AM + "encoder.layer_norm.bias"], eps)
    return h


# ----------------------------------------------------------------------------------------------------------------------------
# encoder layer
# ----------------------------------------------------------------------------------------------------------------------------
def stream_planes(x: Tensor, ev: Evaluation) -> Tensor:
    """The residual stream as the LayerNorm fold of the two-plane modes holds it between the products of a layer: planes
    of u = (x - p) * s, read back as (hi + lo) / s + p -- 22 significant bits about the pivot on fp16 planes, 16 on bf16 planes.
    The device takes p and s from the row's PREVIOUS statistics (mean; a power of two with 1 < sigma * s <= 2); here they are the
    row's own, which puts the rounding at the same size.  The truth and the fp32 evaluation keep the stream as it is."""
    if ev.plane is None:
        return x
    pivot = x.mean(-1, keepdim=True)
    scale = torch.exp2(torch.floor(torch.log2(2.0 / x.std(-1, unbiased=False, keepdim=True))))
    hi, lo = ev._split((x - pivot) * scale)
    return (hi + lo) / scale + pivot


def layer_stage(h: Tensor, frame_lengths: Tensor, state: Dict[str, Tensor], spec: Dict[str, Any], ev: Evaluation, index: int,
                fold: bool = False) -> Tensor:
    """hidden[index] [N, T, D] -> hidden[index + 1].  ``fold`` (pre-LN): the emulation keeps the stream in planes where a pass
    with ``ln_fold == 1`` does -- as the layer receives it and behind the out-projection; what FFN2 adds lands in fp32 rows."""
    sd = ev.weights(state)
    eps = spec["eps"]
    stable = bool(spec.get("stable_layer_norm", True))
    h = h.to(ev.dtype)
    N, T, D = h.shape
    H = spec["heads"]
    dh = D // H
    p = f"{AM}encoder.layers.{index}."

    def norm(x, prefix):
        return F.layer_norm(x, (D,), sd[prefix + ".weight"], sd[prefix + ".bias"], eps)

    bias = torch.zeros(N, 1, 1, T, dtype=ev.dtype)
    if spec.get("use_attention_mask", True):
        padded = torch.arange(T).unsqueeze(0) >= frame_lengths.unsqueeze(1)
        bias.masked_fill_(padded[:, None, None, :], torch.finfo(torch.float32).min)
    if fold:
        h = stream_planes(h, ev)
    a = norm(h, p + "layer_norm") if stable else h
    q, kk, v = (ev.linear(f"{n}_proj", a, sd[p + f"attention.{n}_proj.weight"], sd[p + f"attention.{n}_proj.bias"])
                .view(N, T, H, dh).transpose(1, 2) for n in ("q", "k", "v"))
    scores = ev.matmul("qk", q, kk.transpose(2, 3)) * (dh ** -0.5) + bias
    attn = ev.matmul("pv", torch.softmax(scores, -1), v).transpose(1, 2).reshape(N, T, D)
    h = h + ev.linear("out_proj", attn, sd[p + "attention.out_proj.weight"], sd[p + "attention.out_proj.bias"])
    if fold:
        h = stream_planes(h, ev)

    def ffn(x):
        x = F.gelu(ev.linear("ffn1", x, sd[p + "feed_forward.intermediate_dense.weight"], sd[p + "feed_forward.intermediate_dense.bias"]))
        return ev.linear("ffn2", x, sd[p + "feed_forward.output_dense.weight"], sd[p + "feed_forward.output_dense.bias"])

    if stable:
        h = h + ffn(norm(h, p + "final_layer_norm"))
        if index == spec["layers"] - 1:
            h = norm(h, AM + "encoder.layer_norm")
    else:
        h = norm(h, p + "layer_norm")
        h = norm(h + ffn(h), p + "final_layer_norm")
    return h


# ----------------------------------------------------------------------------------------------------------------------------
# heads
# ----------------------------------------------------------------------------------------------------------------------------
def positions(frames: int, size: int, dtype: torch.dtype) -> Tensor:
    """``O.sinusoidal_positions``: the ARGUMENT frame * base is the fp32 product upstream forms (that rounding defines the table);
    sine and cosine of it are taken in ``dtype``"""
    component = torch.exp(torch.arange(0, size, 2, dtype=torch.float) * -(math.log(10000) / size))
    argument = (torch.arange(frames, dtype=torch.float).unsqueeze(1) * torch.stack([component] * 2, 1).view(-1)).to(dtype)
    argument[:, 0::2] = torch.sin(argument[:, 0::2])
    argument[:, 1::2] = torch.cos(argument[:, 1::2])
    return argument


def _time_layer(u: Tensor, frame_lengths: Tensor, sd: Dict[str, Tensor], prefix: str, name: str, heads: int, positional: bool,
                ev: Evaluation) -> Tensor:
    """``O.time_layer_forward`` on batch-major ``u`` [N, T, in]"""
    x = ev.linear(name + ".input_projection", u, sd[prefix + "input_projection.weight"], sd[prefix + "input_projection.bias"])
    x = F.layer_norm(x, (x.shape[-1],), sd[prefix + "layer_norm.weight"], sd[prefix + "layer_norm.bias"], 1e-5)
    N, T, C = x.shape
    if positional:
        x = x + positions(T, C, ev.dtype)
    qkv = ev.linear(name + ".in_proj", x, sd[prefix + "attention.in_proj_weight"], sd[prefix + "attention.in_proj_bias"])
    dh = C // heads
    q, k, v = (t.reshape(N, T, heads, dh).transpose(1, 2) for t in qkv.split(C, -1))
    scores = ev.matmul(name + ".qk", q / math.sqrt(dh), k.transpose(-1, -2))
    padded = torch.arange(T).unsqueeze(0) >= frame_lengths.unsqueeze(1)
    scores = scores.masked_fill(padded[:, None, None, :], float("-inf"))
    o = ev.matmul(name + ".pv", torch.softmax(scores, -1), v).transpose(1, 2).reshape(N, T, C)
    return ev.linear(name + ".out_proj", o, sd[prefix + "attention.out_proj.weight"], sd[prefix + "attention.out_proj.bias"])


def heads_stage(hidden: Dict[int, Tensor], frame_lengths: Tensor, state: Dict[str, Tensor], spec: Dict[str, Any], tfi: Optional[Tensor],
                category_offsets: Optional[Tensor], ev: Evaluation) -> Tuple[Dict[str, Tensor], Dict[str, Tensor]]:
    """``O.projection_forward`` + log-softmax, batch-major.  ``hidden``: layer index -> [N, T, D] for ``spec["layers"]`` (``OUTPUT``)
    and every ``OUTPUT_i`` a class depends on (``hidden_inputs``).  Returns (logits, log-probabilities), name -> [N, T, C]."""
    sd = ev.weights(state)
    outputs: Dict[str, Tensor] = {f"{O.OUTPUT}_{i}": h.to(ev.dtype) for i, h in hidden.items()}
    outputs[O.OUTPUT] = outputs[f"{O.OUTPUT}_{spec['layers']}"]
    blanks = bool(spec.get("dependency_blanks", True))
    classes = spec["classes"]
    logits: Dict[str, Tensor] = {}
    for ci in O.topological_order(classes):
        node = classes[ci]
        name, deps = node["name"], node["dependencies"]
        parts = []
        for d in deps:
            if O.OUTPUT_PATTERN.match(d):
                parts.append(outputs[d])
            else:
                parts.append(torch.softmax(outputs[d] if blanks else outputs[d][..., O.BLANK_OFFSET:], -1))
        u = parts[0] if len(deps) == 1 and O.OUTPUT_PATTERN.match(deps[0]) else torch.cat(parts, -1)
        p = f"{PROJ}{name}."
        layer = node.get("time_layer")
        if layer:
            y = _time_layer(u, frame_lengths, sd, p + "_time_distributed_layer.", name, int(layer.get("num_heads", 1)),
                            bool(layer.get("positional_embeddings", False)), ev)
        else:
            y = ev.linear(name + ".linear", u, sd[p + "_time_distributed_layer.weight"], sd[p + "_time_distributed_layer.bias"])
        emb_key = p + "_composition_layer._attribute_embeddings.weight"
        if emb_key in sd:
            composed = O.composed_embeddings(sd[emb_key], tfi, category_offsets)  # [E, P + 1]
            y = ev.matmul(name + ".compose", y, composed) / math.sqrt(composed.shape[0])
        if name == O.PHONEME and spec.get("allophone_layer", False):
            logits[O.PHONE] = y
            outputs[O.PHONE] = y
        logits[name] = y
        outputs[name] = y
    return logits, {k: F.log_softmax(v, -1) for k, v in logits.items()}


# ----------------------------------------------------------------------------------------------------------------------------
# combined stages: what a pass WITHOUT the keep flag leaves to look at (tests/test_gpu_stage_production.py)
# ----------------------------------------------------------------------------------------------------------------------------
def entry_stage(audio: Tensor, lengths: Tensor, frame_lengths: Tensor, state: Dict[str, Tensor], spec: Dict[str, Any],
                ev: Evaluation) -> Tensor:
    """audio [N, L] -> hidden[0]: normalisation, conv and front in one (such a pass does not keep the conv output)"""
    return front_stage(conv_stage(normalize(audio, lengths, spec, ev), state, spec, ev), frame_lengths, state, spec, ev)


def tail_stage(h: Tensor, taps: Dict[int, Tensor], frame_lengths: Tensor, state: Dict[str, Tensor], spec: Dict[str, Any],
               tfi: Optional[Tensor], category_offsets: Optional[Tensor], ev: Evaluation) -> Tuple[Dict[str, Tensor], Dict[str, Tensor]]:
    """hidden[layers - 1] -> (logits, log-probabilities): the last encoder layer and the heads in one, for the post-LN encoder,
    whose hidden[layers] such a pass does not keep.  ``taps``: the other hidden states the heads read (``OUTPUT_i``, i < layers)."""
    last = layer_stage(h, frame_lengths, state, spec, ev, spec["layers"] - 1)
    return heads_stage({**taps, spec["layers"]: last}, frame_lengths, state, spec, tfi, category_offsets, ev)


def hidden_inputs(spec: Dict[str, Any]) -> List[int]:
    """the hidden states the heads read: ``layers`` (``OUTPUT``) and every ``OUTPUT_i`` named by a class"""
    wanted = {spec["layers"]}
    for node in spec["classes"]:
        for d in node["dependencies"]:
            m = O.OUTPUT_PATTERN.match(d)
            if m and m.group(1) is not None:
                wanted.add(int(m.group(1)))
    return sorted(wanted)


def heads_case_spec(dependency_blanks: bool) -> Dict[str, Any]:
    """The tiny hierarchical model of the heads case: a time-layer head with positions on ``OUTPUT`` (``syllabic``), a linear head
    on the concatenation of its softmax with ``OUTPUT_1`` (``long``), a plain head (``nasal``), and a composed phoneme head
    behind a time layer on ``cat(OUTPUT, softmax(...) x 3)``."""
    spec = S.hierarchical_spec(S.tiny_encoder(2), ["syllabic", "long", "nasal"], embedding_size=32, train_phonemes=12, n_features=6,
                               dependency_blanks=dependency_blanks)
    by_name = {c["name"]: c for c in spec["classes"]}
    by_name["syllabic"].update(size=5, time_layer={"num_heads": 3, "positional_embeddings": True})
    by_name["long"].update(dependencies=["syllabic", "OUTPUT_1"])
    by_name[S.PHONEME]["time_layer"] = {"num_heads": 2, "positional_embeddings": True}
    S.validate(spec)
    return spec


# ----------------------------------------------------------------------------------------------------------------------------
# heads models: the geometry switches of the row kernels of the heads, of ``create_heads`` and of the composition product that
# ``heads_case_spec`` and the encoder cases do not cross (tests/test_gpu_stage_heads.py; CPU proof: tests/test_stage_util.py).
# Each returns (spec, state dict, inventories); an uncomposed model has the one inventory ``None``.
# ----------------------------------------------------------------------------------------------------------------------------
def heads_audio(seed: int) -> Tuple[Tensor, Tensor]:
    """The batch of every heads model: three ragged utterances of at most 3 s and a fourth of 400 samples -- 149 frames (more than
    128 keys, not a multiple of 4) down to exactly one frame, i.e. a time-layer row of one valid key"""
    audio, lengths = synthetic.make_audio(3, 48000, seed=seed, ragged=True)
    one_frame = synthetic.make_audio(1, 400, seed=seed + 1)[0]
    audio = torch.cat([audio, F.pad(one_frame, (0, audio.shape[1] - 400))])
    return audio, torch.cat([lengths, torch.tensor([400])])


def _sized(spec: Dict[str, Any], sizes: Dict[str, int]) -> None:
    for c in spec["classes"]:
        if c["name"] in sizes:
            c["size"] = sizes[c["name"]]


def narrow_wide_model():
    """Log-softmax outputs of 2, 7, 8 | 9, 10 classes (lane-local up to 8, whole-wave beyond), phoneme outputs of 4 (lane-local), 64
    and 65 classes (one wave stride, and one past it) from three inventories, a composition with K = 40 inside a 32-element group
    of its 64-wide planes and N = 4 / 64 / 65, five direct heads in one stack."""
    sizes = {"a1": 1, "a6": 6, "a7": 7, "a8": 8, "a9": 9}
    spec = S.multitask_spec(S.tiny_encoder(1), list(sizes), embedding_size=40, train_phonemes=12, n_features=6, allophone_layer=True)
    _sized(spec, sizes)
    S.validate(spec)
    return spec, synthetic.make_state_dict(spec, seed=31), [synthetic.make_inventory(spec, p, seed=31) for p in (3, 63, 64)]


def large_inventory_model():
    """The released head shape: a 640-wide composition with 37 features into 201 and 1026 classes (N odd and four-digit, the
    log-softmax over hundreds and over more than 1024 columns), next to two 4-class heads."""
    spec = S.multitask_spec(S.tiny_encoder(1), ["syllabic", "long"], embedding_size=640, train_phonemes=64, n_features=37)
    S.validate(spec)
    return spec, synthetic.make_state_dict(spec, seed=32), [synthetic.make_inventory(spec, p, seed=32) for p in (200, 1025)]


def many_outputs_model():
    """71 outputs: 70 attribute heads of 2 .. 10 classes (the second round of the lane-local log-softmax, which walks 64 outputs at
    a time) and a plain phoneme head of 41, all direct: one stack whose N is the sum of the widths (454)."""
    names = [f"attribute{i:02d}" for i in range(70)]
    spec = S.baseline_spec(S.tiny_encoder(1), 40)
    spec["classes"] = [{"name": n, "size": 1 + i % 9, "dependencies": [S.OUTPUT]} for i, n in enumerate(names)] + spec["classes"]
    S.validate(spec)
    return spec, synthetic.make_state_dict(spec, seed=33), [None]


def wide_dependency_model(dependency_blanks: bool, encoder: Optional[Dict[str, Any]] = None):
    """``concat_kernel``: a softmax part of 71 (70 without the blanks) columns, hidden-state parts that are not first
    (``[wide, OUTPUT_0, other]``, ``[OUTPUT, wide, second, OUTPUT_1]``), concatenated widths of 224 (no zero fill) and 353 (one past
    a multiple of 32 and of 8) with the blanks, 222 and 351 without; ``create_heads``: direct heads before (``wide``, ``other``)
    and after (``late``) a dependent one, so two stacks.  Classifiers on ``OUTPUT_0`` / ``OUTPUT_1``: a pass without the keep
    flag hands out every hidden state.  ``encoder``: two layers (default: the tiny one)."""
    enc = dict(encoder or S.tiny_encoder(2))
    assert enc["layers"] == 2
    spec = S.hierarchical_spec(enc, ["wide", "other", "second", "late"], embedding_size=32, train_phonemes=12, n_features=6,
                               dependency_blanks=dependency_blanks)
    _sized(spec, {"wide": 70, "other": 24, "second": 25, "late": 4})
    by_name = {c["name"]: c for c in spec["classes"]}
    by_name["second"]["dependencies"] = ["wide", "OUTPUT_0", "other"]
    by_name[S.PHONEME]["dependencies"] = [S.OUTPUT, "wide", "second", "OUTPUT_1"]
    S.validate(spec)
    return spec, synthetic.make_state_dict(spec, seed=34), [synthetic.make_inventory(spec, 9, seed=34)]


def narrow_layout_model(dependency_blanks: bool = True):
    """``wide_dependency_model`` on an encoder whose conv and FFN widths (24, 72) are no multiples of 32: separate planes, rows
    padded to 8 instead of 32 (``kalign``)"""
    enc = S.tiny_encoder(2)
    enc.update(conv_dim=24, ffn=72)
    return wide_dependency_model(dependency_blanks, enc)


TIME_LAYER_COMPOSITIONS = ((64, 1), (192, 2), (160, 1))  # embedding size, heads of the phoneme head: head dimensions 64, 96, 160


def time_layer_model(embedding_size: int, heads: int):
    """``time_attention_kernel`` / ``time_ln_pe_kernel``: time-layer heads of (width, heads) (6, 6), (6, 2), (10, 2), (40, 1) --
    head dimensions 1 (64 key groups), 3 and 5 (idle lanes), 40 -- with positions except on ``t62``, which reads the softmax of
    ``t66`` in front of ``OUTPUT``; widths below 64 in rows padded to 32 / 64.  The composed phoneme head behind a time layer of
    head dimension 64, 96 (a partial second round of 64 columns) or 160 (three rounds): ``TIME_LAYER_COMPOSITIONS``."""
    sizes = {"t66": 5, "t62": 5, "t102": 9, "t401": 39}
    spec = S.hierarchical_spec(S.tiny_encoder(1), list(sizes), embedding_size=embedding_size, train_phonemes=12, n_features=6)
    _sized(spec, sizes)
    by_name = {c["name"]: c for c in spec["classes"]}
    by_name["t66"]["time_layer"] = {"num_heads": 6, "positional_embeddings": True}
    by_name["t62"].update(dependencies=["t66", S.OUTPUT], time_layer={"num_heads": 2, "positional_embeddings": False})
    by_name["t102"]["time_layer"] = {"num_heads": 2, "positional_embeddings": True}
    by_name["t401"]["time_layer"] = {"num_heads": 1, "positional_embeddings": True}
    by_name[S.PHONEME].update(dependencies=[S.OUTPUT, "t102"], time_layer={"num_heads": heads, "positional_embeddings": True})
    S.validate(spec)
    return spec, synthetic.make_state_dict(spec, seed=35 + heads), [synthetic.make_inventory(spec, 9, seed=35)]


# name -> factory: the cases of tests/test_stage_util.py (CPU proof) and of tests/test_gpu_stage_heads.py
HEADS_MODELS = {
    "narrow_wide": narrow_wide_model,
    "large_inventory": large_inventory_model,
    "many_outputs": many_outputs_model,
    "wide_dependency": lambda: wide_dependency_model(True),
    "wide_dependency/no_blanks": lambda: wide_dependency_model(False),
    "narrow_layout": narrow_layout_model,
    **{f"time_layers/dh{e // h}": (lambda e=e, h=h: time_layer_model(e, h)) for e, h in TIME_LAYER_COMPOSITIONS},
}


def tapped_spec(encoder: Dict[str, Any], **heads: int) -> Dict[str, Any]:
    """The two-layer hierarchical model of the production cases: ``syllabic`` reads ``OUTPUT_0`` and the phoneme head reads
    ``cat(OUTPUT, softmax(syllabic), softmax(long), OUTPUT_1)``, so a pass keeps every hidden state a classifier reads and
    ``debug_fetch("hidden", i)`` hands them out without the keep flag."""
    enc = dict(encoder, layers=2)
    spec = S.hierarchical_spec(enc, ["syllabic", "long"], **heads)
    spec["classes"][0]["dependencies"] = ["OUTPUT_0"]
    spec["classes"][-1]["dependencies"] = ["OUTPUT", "syllabic", "long", "OUTPUT_1"]
    S.validate(spec)
    return spec


# hidden, heads, groups of the positional convolution: head dimensions 40 and 8 (attention form 4: rows of 64 columns), 96 (form 5,
# six 16-column steps of Q.K^T) and 128 (form 5, the full width) on the tiny encoder -- the models of tests/test_gpu_head_dim.py
HEAD_DIM_MODELS = ((80, 2, 2), (64, 8, 4), (192, 2, 4), (256, 2, 4))


def head_dim_encoder(hidden: int, heads: int, groups: int) -> Dict[str, Any]:
    enc = S.tiny_encoder(2)
    enc.update(hidden=hidden, heads=heads, ffn=2 * hidden, pos_groups=groups)
    return enc


def head_dim_model(hidden: int, heads: int, groups: int):
    """(spec, state dict, inventory) of ``test_head_dims_against_oracle`` for one entry of ``HEAD_DIM_MODELS``"""
    spec = S.multitask_spec(head_dim_encoder(hidden, heads, groups), ["syllabic", "long"], embedding_size=16, train_phonemes=9,
                            n_features=5, allophone_layer=True)
    spec["shared_phones"] = 11
    S.validate(spec)
    return spec, synthetic.make_state_dict(spec, seed=hidden + heads), synthetic.make_inventory(spec, 7, seed=3)


def post_ln_tapped_spec() -> Dict[str, Any]:
    """``tapped_spec`` at wav2vec2-base width with the post-LN encoder and the attention mask.  12 groups in the positional
    convolution instead of 16: 64 channels per group is what the window kernel takes, and the post-LN encoder packs its rows
    only behind that kernel."""
    enc = S.wav2vec2_base_encoder()
    enc.update(use_attention_mask=True, pos_groups=12)
    return tapped_spec(enc, embedding_size=64, train_phonemes=9, n_features=5)


# (case of tests/test_stage_util.py, mode, stage) -> the weakest lost cross term measured there, in units of e_emu: below 5.0 (the
# floor of the listed products, 4.5, plus 10 % for the summation order of the host's BLAS) the stage-local gate does not claim
# to see a lost term, so neither the separation proof nor a GPU case asserts on that stage.  Both are the second layer under the
# LayerNorm fold on bf16 planes, where the stream's 16 bits about the pivot set e_emu (4.8e-5 / 5.5e-5); weakest: lo(Q) of Q.K^T.
NOT_CLAIMED = {
    ("xlsr_1b", "bf16x3", "layer1/fold"): 4.9,
    ("xlsr_2b", "bf16x3", "layer1/fold"): 4.6,
}


def against(got, truth, frame_lengths: Sequence[int]) -> float:
    """``max_abs_valid`` of a stage's output (a tensor, or name -> tensor for the heads) against its truth"""
    if isinstance(truth, dict):
        return max(max_abs_valid(got[k], truth[k], frame_lengths) for k in truth)
    return max_abs_valid(got, truth, frame_lengths)


def shortest_longest_and(lengths: Tensor, more: int) -> List[int]:
    """utterance indices for the truth of a large batch: the shortest, the longest and ``more`` spread between them by length"""
    order = torch.argsort(lengths).tolist()
    inner = [order[(j + 1) * (len(order) - 1) // (more + 1)] for j in range(more)]
    return sorted({order[0], order[-1], *inner})


def judged(run, device_out, frame_lengths: Sequence[int], precision: str,
           each: Optional[Dict[str, Tuple[float, float]]] = None) -> Tuple[float, float]:
    """One stage of a GPU case: ``run(ev)`` evaluates it from the device's input; returns (the device's error, e_emu of
    ``precision``), both against the float64 truth over the valid frames.  ``each`` (the heads, name -> tensor): filled with the
    same pair per output."""
    with torch.inference_mode():
        truth = run(Evaluation("truth"))
        emulated = run(Evaluation(precision))
        if each is not None:
            for k in truth:
                each[k] = (max_abs_valid(device_out[k], truth[k], frame_lengths), max_abs_valid(emulated[k], truth[k], frame_lengths))
        return against(device_out, truth, frame_lengths), against(emulated, truth, frame_lengths)


def report(name: str, precision: str, found: Dict[str, Tuple[float, float]]) -> None:
    """the ``[stage-local]`` lines of a GPU case: per stage the device's error, e_emu and their ratio"""
    for stage, (error, e_emu) in found.items():
        print(f"[stage-local] {name} {precision} {stage}: device {error:.3g}  e_emu {e_emu:.3g}  ratio {error / e_emu:.2f}")

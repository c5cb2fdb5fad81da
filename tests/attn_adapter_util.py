"""Encoder layers with attention adapters (``adapter_attn_dim``, the fine-tuned MMS encoders), restated for the stage-local tests.

``layer_stage`` is ``stage_util.layer_stage`` for a pre-LN layer that ends in a ``Wav2Vec2AttnAdapterLayer`` (transformers
``Wav2Vec2EncoderLayerStableLayerNorm.forward``):

    h <- h + out_proj(attention(LN1(h)))
    h <- h + FFN(LN2(h))
    h <- h + W2 relu(W1 LN_a(h) + b1) + b2          LN_a = nn.LayerNorm(D) at torch's default eps 1e-5, not layer_norm_eps

hidden[index + 1] is the stream behind the adapter; the final encoder LayerNorm follows the LAST layer's adapter.  The products of
the layer go through the ``Evaluation`` hook as before; the adapter's two products are plain products in the evaluation's dtype
(the device computes them in fp32 FMAs on the fp32 stream: no planes, no cross terms).  Models without adapters, and post-LN
models -- which transformers builds without them whatever the config says -- take ``stage_util.layer_stage`` itself, so the
function can stand in for it anywhere (the GPU tests put it in its place).

``defect`` evaluates a layer with one mistake an implementation of the adapter could make; tests/test_attn_adapter.py shows that
each of them moves the layer stage by >= 7.5 x e_emu, i.e. that the GPU gate of 3 x e_emu sees them.

tests/golden/g19_tiny_attn_adapter.npz (tools/gen_attn_adapter_golden.py: the real reference) pins this restatement.
"""
from __future__ import annotations

from typing import Any, Dict, Optional

import torch
import torch.nn.functional as F
from torch import Tensor

from allophant_amd import spec as S, synthetic
from tests import stage_util as SU
from tests.golden_util import Golden

AM = SU.AM
ADAPTER_LN_EPS = 1e-5
DEFECTS = ("skipped", "no_relu", "no_b2", "no_beta", "before_ffn", "after_final_norm")
_plain_layer_stage = SU.layer_stage  # (kept: the GPU tests put ``layer_stage`` below in its place)


def adapter_term(h: Tensor, sd: Dict[str, Tensor], prefix: str, defect: Optional[str] = None) -> Tensor:
    """``Wav2Vec2AttnAdapterLayer.forward`` of ``h`` [..., D] in ``h``'s dtype"""
    beta = None if defect == "no_beta" else sd[prefix + "norm.bias"]
    x = F.layer_norm(h, (h.shape[-1],), sd[prefix + "norm.weight"], beta, ADAPTER_LN_EPS)
    x = F.linear(x, sd[prefix + "linear_1.weight"], sd[prefix + "linear_1.bias"])
    if defect != "no_relu":
        x = torch.relu(x)
    return F.linear(x, sd[prefix + "linear_2.weight"], None if defect == "no_b2" else sd[prefix + "linear_2.bias"])


def layer_stage(h: Tensor, frame_lengths: Tensor, state: Dict[str, Tensor], spec: Dict[str, Any], ev: SU.Evaluation, index: int,
                fold: bool = False, defect: Optional[str] = None) -> Tensor:
    """hidden[index] [N, T, D] -> hidden[index + 1] of an encoder whose pre-LN layers end in attention adapters"""
    if not S.adapter_attn_dim(spec):
        assert defect is None
        return _plain_layer_stage(h, frame_lengths, state, spec, ev, index, fold)
    assert not fold, "a pass with attention adapters does not fold its LayerNorms"
    if defect is not None and defect not in DEFECTS:
        raise ValueError(defect)
    sd = ev.weights(state)
    eps = spec["eps"]
    h = h.to(ev.dtype)
    N, T, D = h.shape
    H = spec["heads"]
    dh = D // H
    p = f"{AM}encoder.layers.{index}."
    last = index == spec["layers"] - 1

    def norm(x, prefix):
        return F.layer_norm(x, (D,), sd[prefix + ".weight"], sd[prefix + ".bias"], eps)

    def adapter(x):
        return x if defect == "skipped" else x + adapter_term(x, sd, p + "adapter_layer.", defect)

    bias = torch.zeros(N, 1, 1, T, dtype=ev.dtype)
    if spec.get("use_attention_mask", True):
        padded = torch.arange(T).unsqueeze(0) >= frame_lengths.unsqueeze(1)
        bias.masked_fill_(padded[:, None, None, :], torch.finfo(torch.float32).min)
    a = norm(h, p + "layer_norm")
    q, kk, v = (ev.linear(f"{n}_proj", a, sd[p + f"attention.{n}_proj.weight"], sd[p + f"attention.{n}_proj.bias"])
                .view(N, T, H, dh).transpose(1, 2) for n in ("q", "k", "v"))
    scores = ev.matmul("qk", q, kk.transpose(2, 3)) * (dh ** -0.5) + bias
    attn = ev.matmul("pv", torch.softmax(scores, -1), v).transpose(1, 2).reshape(N, T, D)
    h = h + ev.linear("out_proj", attn, sd[p + "attention.out_proj.weight"], sd[p + "attention.out_proj.bias"])
    if defect == "before_ffn":
        h = adapter(h)
    x = F.gelu(ev.linear("ffn1", norm(h, p + "final_layer_norm"), sd[p + "feed_forward.intermediate_dense.weight"],
                         sd[p + "feed_forward.intermediate_dense.bias"]))
    h = h + ev.linear("ffn2", x, sd[p + "feed_forward.output_dense.weight"], sd[p + "feed_forward.output_dense.bias"])
    if defect == "after_final_norm" and last:
        return adapter(norm(h, AM + "encoder.layer_norm"))
    if defect != "before_ffn":
        h = adapter(h)
    return norm(h, AM + "encoder.layer_norm") if last else h


def hidden_states(audio: Tensor, lengths: Tensor, state: Dict[str, Tensor], spec: Dict[str, Any], ev: SU.Evaluation):
    """(every hidden state [N, T, D] of ``spec`` on ``audio``, the frame lengths): the stages chained in one evaluation"""
    frames = torch.tensor(S.frame_lengths(lengths.tolist(), spec))
    hidden = [SU.entry_stage(audio, lengths, frames, state, spec, ev)]
    for i in range(spec["layers"]):
        hidden.append(layer_stage(hidden[-1], frames, state, spec, ev, i))
    return hidden, frames


def golden_state(g: Golden) -> Dict[str, Tensor]:
    """the state dict of a g19 golden: procedural (``synthetic.make_state_dict``), the stored adapter tensors compared with it"""
    state = synthetic.make_state_dict(g.spec, seed=g.seed)
    stored = {k[2:]: torch.from_numpy(g.z[k]) for k in g.z.files if k.startswith("w/")}
    assert stored.keys() == {k for k in state if ".adapter_layer." in k}
    for k, v in stored.items():
        assert torch.equal(v, state[k]), f"procedural weights changed for {k}"
    return state


def adapter_encoder(encoder: Dict[str, Any], dim: int, layers: int = 2) -> Dict[str, Any]:
    return dict(encoder, layers=layers, adapter_attn_dim=dim)


def width_model(encoder: Dict[str, Any], dim: int = 16, tapped: bool = False, seed: int = 0):
    """two layers of ``encoder`` with adapters of width ``dim``, the heads of the stage-local width cases (``tapped``: of the
    production cases): (spec, state dict, inventory)"""
    if tapped:
        spec = SU.tapped_spec(adapter_encoder(encoder, dim))
    else:
        spec = S.multitask_spec(adapter_encoder(encoder, dim), ["syllabic", "long"], allophone_layer=True)
        spec["shared_phones"] = 80
    S.validate(spec)
    return spec, synthetic.make_state_dict(spec, seed=seed), synthetic.make_inventory(spec, 27, seed=seed)


def small_model(hidden: int, heads: int, groups: int, dim: int):
    """``stage_util.head_dim_model`` with adapters of width ``dim``"""
    spec = S.multitask_spec(adapter_encoder(SU.head_dim_encoder(hidden, heads, groups), dim), ["syllabic", "long"], embedding_size=16,
                            train_phonemes=9, n_features=5, allophone_layer=True)
    spec["shared_phones"] = 11
    S.validate(spec)
    return spec, synthetic.make_state_dict(spec, seed=hidden + heads + dim), synthetic.make_inventory(spec, 7, seed=3)

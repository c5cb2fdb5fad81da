"""Writes tests/golden/g19_tiny_attn_adapter.npz and g19b_tiny_attn_adapter_postln.npz by running the REAL reference
(kgnlp/allophant on transformers' ``Wav2Vec2Model``, imported through oracle/ref_import.py) on a tiny encoder whose config
names ``adapter_attn_dim``:

    python tools/gen_attn_adapter_golden.py        # needs the reference sources; a few seconds

g19:  pre-LN layers (``do_stable_layer_norm=True``), ``adapter_attn_dim`` 5: every ``Wav2Vec2EncoderLayerStableLayerNorm`` ends in
      a ``Wav2Vec2AttnAdapterLayer``.  The ``long`` classifier reads ``OUTPUT_1``, so the reference's own projection consumes a
      hidden state behind an adapter.  A ragged batch of 3 utterances; stored: the adapter weights (the others are procedural:
      the whole tiny state dict would exceed the size limit of a committed file), every hidden state, the log-probabilities, the
      logits and the reference's greedy CTC alignments.
g19b: the same field on post-LN layers (``do_stable_layer_norm=False``, the wav2vec2-base family): transformers builds
      ``Wav2Vec2EncoderLayer`` without an adapter, the state dict has no ``adapter_layer`` key (asserted here) and the field changes
      nothing.

oracle/ref_import.py writes the config.json of the HF model directory from a spec and does not know the field; its writer is
wrapped here so that the file it has produced is rewritten with ``adapter_attn_dim`` added.  Both files have the layout of
oracle/gen_golden.py (``tests/golden_util.Golden`` loads them).  Only data is stored.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from allophant_amd import spec as S, synthetic  # noqa: E402
from oracle import allophant_oracle as O, ref_import  # noqa: E402
from oracle.gen_golden import _load_into_reference  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
ADAPTER_DIM = 5


def _np(t):
    return t.detach().cpu().numpy()


def _json(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def _with_adapter_attn_dim(write):
    """``write_hf_model_dir`` followed by a rewrite of its config.json that also names ``adapter_attn_dim``"""
    def wrapped(spec, directory):
        write(spec, directory)
        path = os.path.join(directory, "config.json")
        with open(path) as f:
            config = json.load(f)
        config["adapter_attn_dim"] = spec.get("adapter_attn_dim")
        with open(path, "w") as f:
            json.dump(config, f)
        return directory
    return wrapped


def case_spec(stable: bool):
    encoder = S.tiny_encoder(2)
    encoder["adapter_attn_dim"] = ADAPTER_DIM
    if not stable:
        encoder.update(stable_layer_norm=False)
    spec = S.multitask_spec(encoder, ["syllabic", "long", "nasal"], embedding_size=16, train_phonemes=9, n_features=5)
    next(c for c in spec["classes"] if c["name"] == "long")["dependencies"] = ["OUTPUT_1"]
    S.validate(spec)
    return spec


def run_case(name: str, stable: bool, seed: int):
    spec = case_spec(stable)
    train_table = synthetic.make_inventory(spec, 9, seed=seed + 100)
    for f, ncat in enumerate(spec["composition_categories"]):
        train_table[:ncat, f] = torch.arange(ncat)
    estimator, model = ref_import.build_reference_estimator(spec, train_table)
    hf_model = model._acoustic_model._model
    assert hf_model.config.adapter_attn_dim == ADAPTER_DIM
    adapter_keys = [k for k in model.state_dict() if ".adapter_layer." in k]
    if stable:
        assert type(hf_model.encoder.layers[0]).__name__ == "Wav2Vec2EncoderLayerStableLayerNorm"
        assert len([k for k in adapter_keys if ".encoder.layers." in k]) == 6 * spec["layers"], adapter_keys
    else:
        assert type(hf_model.encoder.layers[0]).__name__ == "Wav2Vec2EncoderLayer"
        assert not adapter_keys, adapter_keys  # the post-LN layer class builds no adapter: the field has no effect
    state = synthetic.make_state_dict(spec, seed=seed)
    assert bool([k for k in state if ".adapter_layer." in k]) == stable
    _load_into_reference(model, state)
    n, length, audio_seed = 3, 6000, 1900 + seed
    audio, lengths = synthetic.make_audio(n, length, seed=audio_seed, ragged=True)
    tfi = synthetic.make_inventory(spec, 7, seed=seed)
    pred = ref_import.reference_predict(estimator, audio, lengths, tfi, True)
    raw = ref_import.reference_predict(estimator, audio, lengths, tfi, False)
    with torch.inference_mode():
        mask = O.mask_sequence(lengths)
        hf = hf_model(O.zero_mean_unit_var_norm(audio, lengths, mask), mask.long(), output_hidden_states=True)
    from allophant.predictions import GreedyCTCDecoder

    data = {
        "spec_json": _json(spec), "seed": np.int64(seed), "audio": _np(audio),
        "audio_args": np.array([n, length, audio_seed, 1], dtype=np.int64), "lengths": _np(lengths),
        "frame_lengths": _np(pred.lengths), "output_names": _json(list(pred.outputs.keys())),
        "tfi": _np(tfi), "category_offsets": _np(synthetic.category_offsets(spec)),
    }
    # the weights are procedural (synthetic.make_state_dict(spec, seed)); the adapter's own tensors are stored as well, so that a
    # change of their generator shows as such (the whole state dict of the tiny model would be 1.4 MB: over the size limit)
    for k, v in state.items():
        if ".adapter_layer." in k:
            data["w/" + k] = _np(v)
    decoder = GreedyCTCDecoder()
    for k in pred.outputs:
        data["logprobs/" + k] = _np(pred.outputs[k])
        data["logits/" + k] = _np(raw.outputs[k])
        for i, h in enumerate(decoder(pred.outputs[k].transpose(1, 0).contiguous(), pred.lengths)):
            data[f"tokens/{k}/{i}"] = _np(h[0].tokens)
            data[f"timesteps/{k}/{i}"] = _np(h[0].timesteps)
            data[f"score/{k}/{i}"] = np.float32(h[0].score.item())
    assert len(hf.hidden_states) == spec["layers"] + 1
    for i, h in enumerate(hf.hidden_states):
        data[f"hidden/{i}"] = _np(h)
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **data)
    stream = float(hf.hidden_states[1][0, : int(pred.lengths[0])].std())
    print(f"[{name}] wrote {path} ({os.path.getsize(path) / 1e3:.0f} kB); outputs {list(pred.outputs)}, frames {pred.lengths.tolist()}, "
          f"std of hidden[1] {stream:.2f}, adapter tensors {len(adapter_keys)}")


def main():
    ref_import.write_hf_model_dir = _with_adapter_attn_dim(ref_import.write_hf_model_dir)
    run_case("g19_tiny_attn_adapter", True, seed=19)
    run_case("g19b_tiny_attn_adapter_postln", False, seed=19)


if __name__ == "__main__":
    main()

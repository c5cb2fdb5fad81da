"""Writes tests/golden/g17_allophone_mapping.npz by running the REAL reference ``AllophoneMapping``
(allophant/network/acoustic_model.py:89-171, imported through oracle/ref_import.py) in the build container.

    python tools/gen_allophone_golden.py        # needs the reference sources; a few seconds

Part 1 -- the layer alone: a hand-written ``LanguageAllophoneMappings`` (4 languages, 23 shared phones, 17 phonemes; keys out
of order, one language without an entry, phonemes without allophones, phonemes with 1 to 5 allophones), trained values with
noise everywhere (also at masked positions), exact zeros and negative weights, and [37, 6, 24] inputs with NaN, -inf, 1e38
and a denormal planted at masked and unmasked positions; mapped under int ids (with -1) and float-typed ids.

Part 2 -- end to end: a tiny reference model whose allophone layer is built from the same mapping and values; its phone
log-probabilities, the mapped outputs and the reference's greedy CTC alignments of those.

Upstream's ``HierarchicalProjection.map_allophones`` (acoustic_model.py:541-546) looks for the ``AllophoneMapping`` directly in
``_layers["phoneme"]``, where a ``HierarchicalClassifier`` sits, and so raises for every model; the mapping itself is the
layer's own ``map_allophones``, which is what is called here (and what ``allophant_amd.Estimator.map_allophones`` computes).
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from allophant_amd import spec as S, synthetic  # noqa: E402
from oracle import ref_import  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g17_allophone_mapping.npz")
P, Q = 23, 17
LANGUAGES = ["spa", "ita", "deu", "fin"]
KEY = "_projection._layers.phoneme._allophone_layer._allophone_matrices"

# language index -> {phoneme: [shared phones]}; language 1 ("ita") has no entry; keys out of order
MAPPING = {
    2: {0: [0], 3: [3, 4], 16: [22, 21, 20, 19, 18], 5: [5], 7: [8, 9, 10], 1: [1, 2], 11: [12, 13, 14, 15]},
    0: {4: [6], 0: [0, 1], 9: [11, 12, 13, 14, 15], 2: [2], 12: [17, 16], 15: [20]},
    3: {1: [3], 6: [7, 8, 9, 10], 10: [0, 22], 13: [18, 19, 21], 14: [16]},
}


def _np(t):
    return t.detach().cpu().numpy()


def _json(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def main():
    ref_import.install()
    from allophant.network.acoustic_model import AllophoneMapping

    torch.manual_seed(17)
    structure = types.SimpleNamespace(allophones=MAPPING, languages=LANGUAGES, shared_phones=[f"p{i}" for i in range(P)])
    layer = AllophoneMapping(P + 1, Q + 1, 1, structure)
    init = layer._initialization.clone()
    mask = layer._allophone_mask.clone()
    # trained values: the initial matrix plus noise everywhere (masked positions too), negatives, some exact zeros where unmasked
    values = init + 0.4 * torch.randn(init.shape)
    unmasked = (~mask).nonzero()
    zeros = unmasked[torch.randperm(len(unmasked))[:6]]
    values[zeros[:, 0], zeros[:, 1], zeros[:, 2]] = 0.0
    values[2, 0, 0] = -0.75  # a negative blank weight
    with torch.no_grad():
        layer._allophone_matrices.copy_(values)

    T, N = 37, 6
    x = torch.randn(T, N, P + 1).log_softmax(-1)
    ids = torch.tensor([0, 3, -1, 2, 1, 0])
    ids_float = torch.tensor([2.0, 0.7, 3.9, 1.2, 0.0, 2.5])  # int() truncates like the reference's map(int, ...)
    # planted specials: per utterance, a phone unused by its language (masked in every column) and one it uses
    dense = [int(i) % len(LANGUAGES) for i in ids]
    for n, l in enumerate(dense):
        used = (~mask[l, 1:, 1:]).any(1).nonzero().flatten() + 1
        unused = mask[l, 1:, 1:].all(1).nonzero().flatten() + 1
        specials = [float("nan"), float("-inf"), 1e38, 1e-40]
        for k, v in enumerate(specials):
            if len(unused):
                x[3 + k, n, int(unused[(n + k) % len(unused)])] = v
            if len(used):
                x[9 + 2 * k, n, int(used[(n + k) % len(used)])] = v
        x[20, n, 0] = specials[n % 4]  # the blank row
    with torch.no_grad():
        out = layer.map_allophones(x, ids)
        out_float = layer.map_allophones(x, ids_float)
    assert torch.isnan(out).any() and (out == torch.finfo(torch.float32).min).any()

    data = {
        "mapping_json": _json({"allophones": {str(k): {str(q): v for q, v in m.items()} for k, m in MAPPING.items()},
                               "languages": LANGUAGES, "shared_phones": structure.shared_phones}),
        "mapping_int_order": np.array([k for k in MAPPING], dtype=np.int64),
        "matrices": _np(values), "mask": _np(mask), "initialization": _np(init),
        "index_map_json": _json(layer.index_map),
        "inputs": _np(x), "ids": _np(ids), "ids_float": _np(ids_float), "outputs": _np(out), "outputs_float": _np(out_float),
    }

    # ---- part 2: a tiny reference model with this allophone layer ----
    spec = S.multitask_spec(S.tiny_encoder(2), ["syllabic", "long"], embedding_size=None, train_phonemes=Q, allophone_layer=True)
    spec["shared_phones"] = P
    seed = 17
    estimator, model = ref_import.build_reference_estimator(spec, torch.zeros(P, 1, dtype=torch.int64))
    model._projection._layers["phoneme"]._allophone_layer = layer
    state = synthetic.make_state_dict(spec, seed=seed)
    state[KEY] = values.clone()
    model.load_state_dict(state)
    model.eval()
    audio, lengths = synthetic.make_audio(3, 6000, seed=1700, ragged=True)
    pred = ref_import.reference_predict(estimator, audio, lengths, None, True)
    e2e_ids = torch.tensor([1, 0, 3])
    with torch.no_grad():
        mapped = layer.map_allophones(pred.outputs["phone"], e2e_ids)
    from allophant.predictions import GreedyCTCDecoder

    hyps = GreedyCTCDecoder()(mapped.transpose(1, 0).contiguous(), pred.lengths)
    data.update({
        "e2e/spec_json": _json(spec), "e2e/seed": np.int64(seed), "e2e/audio": _np(audio), "e2e/lengths": _np(lengths),
        "e2e/ids": _np(e2e_ids), "e2e/frame_lengths": _np(pred.lengths), "e2e/phone": _np(pred.outputs["phone"]),
        "e2e/mapped": _np(mapped),
    })
    for i, h in enumerate(hyps):
        data[f"e2e/tokens/{i}"] = _np(h[0].tokens)
        data[f"e2e/timesteps/{i}"] = _np(h[0].timesteps)
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e3:.0f} kB); NaN outputs {int(torch.isnan(out).sum())}, "
          f"finfo.min outputs {int((out == torch.finfo(torch.float32).min).sum())}, e2e tokens {[len(h[0].tokens) for h in hyps]}")


if __name__ == "__main__":
    main()

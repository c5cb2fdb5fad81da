"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/g16_reference_models.json: what LIVE reference ``Allophant`` modules
(built by oracle/ref_import.py for the specs of tests/test_reference_binding.py) expose to the reference-side binding
(``spec.spec_from_reference_model`` / ``spec.training_inventory_of_reference_model``), so that
those tests run from the committed fixture alone.

Recorded per model, with the reference's own values:

* ``model._acoustic_model``: the ``transformers.Wav2Vec2Config`` fields of ``_model.config`` the binding reads, and the
  pre-processor flags ``_normalize`` / ``_use_attention_mask`` (acoustic_model.py:796-826);
* ``model._classes`` and ``model._projection``: ``_ordered_nodes`` (names of each node's dependencies),
  ``_dependency_blanks``, ``_uses_allophone_mapping`` (acoustic_model.py:353-466);
* per head of ``_projection._layers``: its time-distributed layer (``nn.Linear``: ``out_features``;
  ``ProjectingMultiheadAttention``: ``input_projection.out_features``, ``attention.num_heads``, whether it has
  ``positional_embeddings``), the composition layer (``_dense_feature_table``, ``_category_offsets``, rows of
  ``_attribute_embeddings``) and the shape of the allophone layer's ``_allophone_matrices``;
* the keys of ``model.state_dict()``.

An attribute the live object lacks is recorded as absent (null), so that ``getattr`` defaults are exercised as they are
on the live model.
"""
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402

ref_import.install()

import torch  # noqa: E402

from allophant_amd import spec as S, synthetic  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g16_reference_models.json")
CONFIG_FIELDS = ("conv_dim", "conv_kernel", "conv_stride", "hidden_size", "num_hidden_layers", "num_attention_heads",
                 "intermediate_size", "num_conv_pos_embeddings", "num_conv_pos_embedding_groups", "layer_norm_eps",
                 "feat_extract_norm", "conv_bias", "do_stable_layer_norm")
MISSING = object()


def _plain(value):
    if value is MISSING:
        return None
    if isinstance(value, (list, tuple)):
        return [_plain(v) for v in value]
    if isinstance(value, torch.Tensor):
        return value.tolist()
    return value


def cases():
    """(name, spec, training phonemes) of every model the tests bind to; the same constructions as the tests."""
    multitask = S.multitask_spec(S.tiny_encoder(2), ["syllabic", "long", "nasal"], embedding_size=16, train_phonemes=9,
                                 n_features=5, n_values=3, allophone_layer=True)
    multitask["shared_phones"] = 11
    hierarchical = S.hierarchical_spec(S.tiny_encoder(2), ["syllabic", "long"], embedding_size=16, train_phonemes=8,
                                       n_features=4, dependency_blanks=False)
    by_name = {c["name"]: c for c in hierarchical["classes"]}
    by_name["syllabic"]["dependencies"] = ["OUTPUT_1"]
    by_name["long"].update(dependencies=["syllabic", "OUTPUT"], time_layer={"num_heads": 2, "positional_embeddings": True})
    S.validate(hierarchical)
    enc = S.tiny_encoder(2)
    enc.update(feat_extract_norm="group", conv_bias=False, stable_layer_norm=False, use_attention_mask=False)
    return [("multitask_allophones", multitask, 11), ("hierarchical_time_layer", hierarchical, 8),
            ("baseline", S.baseline_spec(S.tiny_encoder(1), 14), 14), ("groupnorm_postln", S.baseline_spec(enc, 12), 12)]


def reference_model(spec, n_train):
    """The live model, built as tests/test_reference_binding.py built it (training table: synthetic seed 5, every category
    occurring)."""
    table = None
    if spec.get("embedding_size") or spec.get("allophone_layer"):
        table = synthetic.make_inventory(spec, n_train, seed=5)
        for f, ncat in enumerate(spec["composition_categories"]):
            table[:ncat, f] = torch.arange(ncat)  # every category occurs: n_f == max + 1 (acoustic_model.py:196-207)
    _estimator, model = ref_import.build_reference_estimator(spec, table)
    return model


def record(model):
    acoustic = model._acoustic_model
    config = acoustic._model.config
    projection = model._projection
    heads = {}
    for name in model._classes:
        head = projection._layers[name]
        layer = head._time_distributed_layer
        if hasattr(layer, "input_projection"):
            entry = {"time_layer": {"input_projection_out_features": int(layer.input_projection.out_features),
                                    "num_heads": int(layer.attention.num_heads),
                                    "positional_embeddings": layer.positional_embeddings is not None}}
        else:
            entry = {"out_features": int(layer.out_features)}
        composition = getattr(head, "_composition_layer", None)
        if composition is not None:
            entry["composition"] = {"dense_feature_table": composition._dense_feature_table.tolist(),
                                    "category_offsets": composition._category_offsets.tolist(),
                                    "attribute_embedding_rows": int(composition._attribute_embeddings.weight.shape[0])}
        allophones = getattr(head, "_allophone_layer", None)
        if allophones is not None:
            entry["allophone_matrices_shape"] = list(allophones._allophone_matrices.shape)
        heads[name] = entry
    return {
        "config": {k: _plain(getattr(config, k, MISSING)) for k in CONFIG_FIELDS},
        "normalize": _plain(getattr(acoustic, "_normalize", MISSING)),
        "use_attention_mask": _plain(getattr(acoustic, "_use_attention_mask", MISSING)),
        "classes": list(model._classes),
        "ordered_nodes": [[name, [d.name for d in deps]] for name, deps in projection._ordered_nodes],
        "dependency_blanks": bool(projection._dependency_blanks),
        "uses_allophone_mapping": _plain(getattr(projection, "_uses_allophone_mapping", MISSING)),
        "heads": heads,
        "state_dict_keys": sorted(model.state_dict()),
    }


def main():
    warnings.simplefilter("ignore")
    golden = {name: record(reference_model(spec, n_train)) for name, spec, n_train in cases()}
    with open(OUT, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}: {', '.join(golden)}")


if __name__ == "__main__":
    main()

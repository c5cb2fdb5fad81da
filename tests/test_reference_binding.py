"""The pieces of the reference-side binding that run without a GPU: deriving the spec and the
training inventory from a reference model.  The models are the ones the REAL reference built for these specs (through
oracle/ref_import.py), as recorded in tests/golden/g16_reference_models.json by oracle/gen_binding_golden.py: every
attribute the binding reads, with the reference's own values, and the keys of the model's state_dict.  Each test rebuilds
that model as plain objects and binds to it."""
import json
import os
from types import SimpleNamespace

import torch

from allophant_amd import spec as S, synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_reference_models.json")


def _recorded_model(record):
    """A stand-in for the live ``Allophant`` module with exactly the recorded attributes (absent ones stay absent)."""
    def present(**attrs):
        return SimpleNamespace(**{k: v for k, v in attrs.items() if v is not None})

    acoustic = present(_model=SimpleNamespace(config=present(**record["config"])), _normalize=record["normalize"],
                       _use_attention_mask=record["use_attention_mask"])
    layers = {}
    for name, head in record["heads"].items():
        if "time_layer" in head:
            t = head["time_layer"]
            layer = SimpleNamespace(input_projection=SimpleNamespace(out_features=t["input_projection_out_features"]),
                                    attention=SimpleNamespace(num_heads=t["num_heads"]),
                                    positional_embeddings=object() if t["positional_embeddings"] else None)
        else:
            layer = SimpleNamespace(out_features=head["out_features"])
        entry = SimpleNamespace(_time_distributed_layer=layer)
        if "composition" in head:
            c = head["composition"]
            entry._composition_layer = SimpleNamespace(
                _dense_feature_table=torch.tensor(c["dense_feature_table"]), _category_offsets=torch.tensor(c["category_offsets"]),
                _attribute_embeddings=SimpleNamespace(weight=torch.empty(c["attribute_embedding_rows"], 0)))
        if "allophone_matrices_shape" in head:
            entry._allophone_layer = SimpleNamespace(_allophone_matrices=torch.empty(head["allophone_matrices_shape"]))
        layers[name] = entry
    projection = present(_layers=layers, _dependency_blanks=record["dependency_blanks"],
                         _uses_allophone_mapping=record["uses_allophone_mapping"],
                         _ordered_nodes=[(name, [SimpleNamespace(name=d) for d in deps]) for name, deps in record["ordered_nodes"]])
    keys = record["state_dict_keys"]
    return SimpleNamespace(_acoustic_model=acoustic, _classes=list(record["classes"]), _projection=projection,
                           state_dict=lambda: dict.fromkeys(keys))


def _reference_model(case, spec, n_train):
    """The reference model recorded under `case` and the training inventory it was built with (synthetic seed 5, every
    category occurring), or None for models without a composition layer."""
    with open(GOLDEN) as f:
        record = json.load(f)[case]
    table = None
    if spec.get("embedding_size") or spec.get("allophone_layer"):
        table = synthetic.make_inventory(spec, n_train, seed=5)
        for f, ncat in enumerate(spec["composition_categories"]):
            table[:ncat, f] = torch.arange(ncat)  # every category occurs: n_f == max + 1 (acoustic_model.py:196-207)
    return _recorded_model(record), table


def _comparable(spec):
    keys = ("conv_dim", "conv_kernel", "conv_stride", "hidden", "layers", "heads", "ffn", "pos_kernel", "pos_groups", "eps",
            "do_normalize", "dependency_blanks", "embedding_size", "allophone_layer", "composition_categories")
    out = {k: spec.get(k) for k in keys}
    out["variant"] = (spec.get("feat_extract_norm", "layer"), bool(spec.get("conv_bias", True)),
                      bool(spec.get("stable_layer_norm", True)), bool(spec.get("use_attention_mask", True)))
    out["classes"] = [{"name": c["name"], "dependencies": list(c["dependencies"]), "time_layer": c.get("time_layer")}
                      for c in spec["classes"]]
    out["embedding_size"] = out["embedding_size"] or None
    return out


def test_spec_from_a_live_reference_model_multitask_allophones():
    spec = S.multitask_spec(S.tiny_encoder(2), ["syllabic", "long", "nasal"], embedding_size=16, train_phonemes=9,
                            n_features=5, n_values=3, allophone_layer=True)
    spec["shared_phones"] = 11
    model, table = _reference_model("multitask_allophones", spec, 11)
    derived = S.spec_from_reference_model(model)
    assert _comparable(derived) == _comparable(spec)
    assert derived["shared_phones"] == 11
    sizes = {c["name"]: c["size"] for c in derived["classes"]}
    assert sizes["syllabic"] == 3 and sizes["long"] == 3
    assert torch.equal(S.training_inventory_of_reference_model(model), table)
    # the state_dict of that model carries exactly the keys the packer reads
    state = synthetic.make_state_dict(spec, seed=0)
    assert set(state) <= set(model.state_dict())


def test_spec_from_a_live_reference_model_hierarchical_time_layer():
    spec = S.hierarchical_spec(S.tiny_encoder(2), ["syllabic", "long"], embedding_size=16, train_phonemes=8, n_features=4,
                               dependency_blanks=False)
    by_name = {c["name"]: c for c in spec["classes"]}
    by_name["syllabic"]["dependencies"] = ["OUTPUT_1"]
    by_name["long"].update(dependencies=["syllabic", "OUTPUT"], time_layer={"num_heads": 2, "positional_embeddings": True})
    S.validate(spec)
    model, table = _reference_model("hierarchical_time_layer", spec, 8)
    derived = S.spec_from_reference_model(model)
    assert _comparable(derived) == _comparable(spec)
    assert {c["name"]: c["size"] for c in derived["classes"]} == {c["name"]: c["size"] for c in spec["classes"]}
    assert torch.equal(S.training_inventory_of_reference_model(model), table)


def test_spec_from_a_live_reference_model_baseline():
    spec = S.baseline_spec(S.tiny_encoder(1), 14)
    model, _ = _reference_model("baseline", spec, 14)
    derived = S.spec_from_reference_model(model)
    assert _comparable(derived) == _comparable(spec)
    assert derived["classes"][0]["size"] == 14 and S.training_inventory_of_reference_model(model) is None


def test_spec_from_a_live_reference_model_groupnorm_postln():
    """The reference builds whatever ``model_id`` names (acoustic_model.py:775-826): a group-norm / post-LN wav2vec 2.0 whose
    preprocessor has return_attention_mask=False comes out as that variant, and its state_dict has no conv bias and a norm
    behind conv layer 0 only."""
    enc = S.tiny_encoder(2)
    enc.update(feat_extract_norm="group", conv_bias=False, stable_layer_norm=False, use_attention_mask=False)
    spec = S.baseline_spec(enc, 12)
    model, _ = _reference_model("groupnorm_postln", spec, 12)
    derived = S.spec_from_reference_model(model)
    assert _comparable(derived) == _comparable(spec)
    assert derived["feat_extract_norm"] == "group" and derived["use_attention_mask"] is False
    state = synthetic.make_state_dict(spec, seed=0)
    reference_keys = set(model.state_dict())
    assert set(state) <= reference_keys
    extractor = {k for k in reference_keys if ".feature_extractor." in k}
    assert extractor == {k for k in state if ".feature_extractor." in k}  # no bias, one norm: exactly the generated keys

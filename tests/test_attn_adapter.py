"""Attention adapters (``adapter_attn_dim``: the fine-tuned MMS encoders) on the CPU: the restatement of an adapter layer pinned to
the real reference (golden g19), the description of such a model (spec, synthetic weights, checkpoints), and the proof that the
stage-local gate of the GPU tests (3 x e_emu, tests/test_gpu_attn_adapter.py) sees a wrong adapter.

Separation, in the manner of tests/test_stage_util.py: a layer stage evaluated with one defect of the adapter -- skipped, without
its ReLU, without ``b2``, without the beta of its LayerNorm, in front of the FFN residual instead of behind it, behind the final
LayerNorm instead of in front of it -- lies >= 7.5 x e_emu from the float64 truth, e_emu being the error of the intact
split-precision emulation.  Shown on the tiny model of g19 and on two layers at XLS-R 1B width with the released dimension 16.
"""
import ctypes as C

import pytest
import torch

from allophant_amd import checkpoint, spec as S, synthetic
from oracle import allophant_oracle as O
from tests import attn_adapter_util as AU, stage_util as SU
from tests.golden_util import Golden, max_abs_valid_bm, max_abs_valid_tm
from tests.test_stage_util import SEPARATION

AM = SU.AM
HIDDEN_TOLERANCE = 2e-5  # what tests/test_oracle_golden.py allows the tiny goldens' hidden states and log-probabilities


@pytest.fixture(scope="module")
def g19():
    return Golden("g19_tiny_attn_adapter")


# ----------------------------------------------------------------------------------------------------------------------------
# the restatement against the reference
# ----------------------------------------------------------------------------------------------------------------------------
def test_layer_stage_matches_reference(g19):
    """every layer from the reference's own hidden state, and the chain from the audio, against g19's hidden states"""
    spec, state = g19.spec, AU.golden_state(g19)
    assert spec["adapter_attn_dim"] == 5 and g19.hidden_indices() == [0, 1, 2]
    ev = SU.Evaluation("fp32")
    with torch.inference_mode():
        for i in range(spec["layers"]):
            got = AU.layer_stage(g19.hidden(i), g19.frame_lengths, state, spec, ev, i)
            assert max_abs_valid_bm(got, g19.hidden(i + 1), g19.frame_lengths) < HIDDEN_TOLERANCE, i
        hidden, frames = AU.hidden_states(g19.audio, g19.lengths, state, spec, ev)
        assert torch.equal(frames, g19.frame_lengths)
        for i, h in enumerate(hidden):
            assert max_abs_valid_bm(h, g19.hidden(i), frames) < HIDDEN_TOLERANCE, i
        # the adapter is a visible share of the stream: without it the layer misses the reference by far more than rounding
        without = AU.layer_stage(g19.hidden(0), frames, state, spec, ev, 0, defect="skipped")
        assert max_abs_valid_bm(without, g19.hidden(1), frames) > 0.5


def test_heads_on_adapter_states_match_reference(g19):
    """log-probabilities, logits and greedy alignments from the restated hidden states (``long`` reads ``OUTPUT_1``, a state behind
    an adapter)"""
    spec, state = g19.spec, AU.golden_state(g19)
    ev = SU.Evaluation("fp32")
    with torch.inference_mode():
        hidden, frames = AU.hidden_states(g19.audio, g19.lengths, state, spec, ev)
        taps = {i: hidden[i] for i in SU.hidden_inputs(spec)}
        assert sorted(taps) == [1, 2]
        logits, logp = SU.heads_stage(taps, frames, state, spec, g19.tfi, g19.category_offsets, ev)
    assert list(logp) == g19.output_names == S.output_names(spec)
    for k in g19.output_names:
        assert max_abs_valid_tm(logp[k].transpose(0, 1), g19.logprobs(k), frames) < HIDDEN_TOLERANCE, k
        assert max_abs_valid_tm(logits[k].transpose(0, 1), g19.logits(k), frames) < HIDDEN_TOLERANCE, k
        for i, (tokens, timesteps, _score) in enumerate(O.greedy_ctc(logp[k].contiguous(), frames)):
            want_tokens, want_timesteps, _ = g19.tokens(k, i)
            assert torch.equal(tokens, want_tokens) and torch.equal(timesteps, want_timesteps), (k, i)


def test_post_ln_reference_ignores_the_field():
    """g19b: ``do_stable_layer_norm=False`` with ``adapter_attn_dim`` set -- the reference built no adapter (no such tensor in its
    state dict), so the oracle, which knows none, reproduces it; and the restatement falls through to the plain layer"""
    g = Golden("g19b_tiny_attn_adapter_postln")
    assert g.spec["adapter_attn_dim"] == 5 and g.spec["stable_layer_norm"] is False and S.adapter_attn_dim(g.spec) == 0
    state = AU.golden_state(g)
    assert not [k for k in state if "adapter_layer" in k]
    with torch.inference_mode():
        out, frames, inter = O.predict(g.audio, g.lengths, state, g.spec, g.tfi, g.category_offsets, True, keep_intermediates=True)
        for k in g.output_names:
            assert max_abs_valid_tm(out[k], g.logprobs(k), g.frame_lengths) < HIDDEN_TOLERANCE, k
        for i in g.hidden_indices():
            assert max_abs_valid_bm(inter["hidden_states"][i], g.hidden(i), g.frame_lengths) < HIDDEN_TOLERANCE, i
        got = AU.layer_stage(g.hidden(0), frames, state, g.spec, SU.Evaluation("fp32"), 0)
        assert max_abs_valid_bm(got, g.hidden(1), frames) < HIDDEN_TOLERANCE


# ----------------------------------------------------------------------------------------------------------------------------
# spec, synthetic weights, checkpoints
# ----------------------------------------------------------------------------------------------------------------------------
def adapter_spec(dim=16, **encoder):
    return S.baseline_spec(dict(S.tiny_encoder(2), adapter_attn_dim=dim, **encoder), 9)


@pytest.mark.parametrize("dim", [None, 0, 1, 16, 64])
def test_validate_accepts(dim):
    S.validate(adapter_spec(dim))
    assert S.adapter_attn_dim(adapter_spec(dim)) == (dim or 0)


@pytest.mark.parametrize("dim", [-1, 65, 2.0, "16", True])
def test_validate_refuses(dim):
    with pytest.raises(ValueError, match="adapter_attn_dim"):
        S.validate(adapter_spec(dim))


def test_synthetic_adapter_tensors():
    spec = adapter_spec(6)
    state = synthetic.make_state_dict(spec, seed=3)
    D = spec["hidden"]
    shapes = {"norm.weight": (D,), "norm.bias": (D,), "linear_1.weight": (6, D), "linear_1.bias": (6,), "linear_2.weight": (D, 6),
              "linear_2.bias": (D,)}
    for i in range(spec["layers"]):
        for name, shape in shapes.items():
            tensor = state[f"{AM}encoder.layers.{i}.adapter_layer.{name}"]
            assert tuple(tensor.shape) == shape and tensor.dtype == torch.float32, (i, name)
            assert float(tensor.abs().min()) > 0  # no bias is zero, no gamma is one: none can be dropped unseen
        assert float((state[f"{AM}encoder.layers.{i}.adapter_layer.norm.weight"] - 1).abs().min()) > 0
    assert len([k for k in state if ".adapter_layer." in k]) == 6 * spec["layers"]
    # the other tensors are those of the same model without adapters; 0 / None / post-LN layers: no adapter tensors at all
    plain = synthetic.make_state_dict(adapter_spec(None), seed=3)
    assert {k for k in state if ".adapter_layer." not in k} == set(plain) and all(torch.equal(plain[k], state[k]) for k in plain)
    for other in (adapter_spec(0), adapter_spec(6, stable_layer_norm=False)):
        assert not [k for k in synthetic.make_state_dict(other, seed=3) if "adapter_layer" in k]


def test_spec_to_structs_passes_the_dimension():
    from allophant_amd import estimator, lib

    assert lib.AMX_ABI_VERSION == 7 or "AMX_ABI_OVERRIDE" in __import__("os").environ
    # ABI 7: the last 32-bit member of amx_config is the pair (use_attention_mask, adapter_attn_dim), 16 bits each -- the size of the
    # struct and the offsets of the older members are those of ABI 6
    assert lib.AmxConfig._fields_[-1][0] == "adapter_attn_dim" and C.sizeof(lib.AmxConfig) == 140
    assert lib.AmxConfig.use_attention_mask.offset == 136 and lib.AmxConfig.adapter_attn_dim.offset == 138
    cfg, _ = estimator._spec_to_structs(adapter_spec(None), "f16x3")
    assert C.cast(C.byref(cfg, 136), C.POINTER(C.c_int32))[0] == 1  # what a build of ABI <= 6 reads as its mask flag
    for dim, want in ((None, 0), (0, 0), (16, 16)):
        cfg, _ = estimator._spec_to_structs(adapter_spec(dim), "f16x3")
        assert cfg.adapter_attn_dim == want


def test_model_ids():
    for model_id in ("facebook/mms-1b-all", "facebook/mms-1b-fl102", "facebook/mms-1b-l1107"):
        encoder = checkpoint.MODEL_ID_ENCODERS[model_id]()
        assert encoder == dict(S.xlsr_1b_encoder(), adapter_attn_dim=16)
    assert "adapter_attn_dim" not in checkpoint.MODEL_ID_ENCODERS["facebook/mms-1b"]()


def _checkpoint(spec, state, described):
    """a checkpoint of ``state`` whose encoder description names ``described`` as the adapter dimension (None: does not name one)"""
    ckpt = checkpoint.make_checkpoint(spec, state, synthetic_encoder=True)
    ckpt["additional"]["amx_encoder"].pop("adapter_attn_dim", None)
    if described is not None:
        ckpt["additional"]["amx_encoder"]["adapter_attn_dim"] = described
    return ckpt


def test_checkpoint_infers_the_dimension_from_the_weights():
    """a state dict in the reference's naming (the HF keys ``encoder.layers.{i}.adapter_layer.*`` under the acoustic model's prefix)
    with adapters is accepted: named or not, the dimension is what ``linear_1.weight`` says"""
    spec = adapter_spec(6)
    state = synthetic.make_state_dict(spec, seed=4)
    for described in (None, 0, 6):
        restored = checkpoint.spec_from_checkpoint(_checkpoint(spec, state, described))
        assert restored["adapter_attn_dim"] == 6 and S.adapter_attn_dim(restored) == 6
    # a checkpoint that says nothing and has no adapters stays without
    plain = adapter_spec(None)
    restored = checkpoint.spec_from_checkpoint(_checkpoint(plain, synthetic.make_state_dict(plain, seed=4), None))
    assert not restored.get("adapter_attn_dim")


def test_checkpoint_reports_mismatches():
    spec = adapter_spec(6)
    state = synthetic.make_state_dict(spec, seed=4)
    with pytest.raises(ValueError, match="adapter_attn_dim described as 16"):
        checkpoint.spec_from_checkpoint(_checkpoint(spec, state, 16))
    without = {k: v for k, v in state.items() if "adapter_layer" not in k}
    with pytest.raises(ValueError, match="adapter_attn_dim=6 but the state dict has no"):
        checkpoint.spec_from_checkpoint(_checkpoint(spec, without, 6))
    partial = {k: v for k, v in state.items() if "layers.1.adapter_layer" not in k}
    with pytest.raises(ValueError, match="1 of 2 encoder layers carry an attention adapter"):
        checkpoint.spec_from_checkpoint(_checkpoint(spec, partial, None))
    post_ln = adapter_spec(6, stable_layer_norm=False)
    with pytest.raises(ValueError, match="post-LN layers"):
        checkpoint.spec_from_checkpoint(_checkpoint(post_ln, state, None))
    # post-LN with the field named and no adapter tensors: accepted, no effect -- as upstream
    restored = checkpoint.spec_from_checkpoint(_checkpoint(post_ln, synthetic.make_state_dict(post_ln, seed=4), 6))
    assert S.adapter_attn_dim(restored) == 0


# ----------------------------------------------------------------------------------------------------------------------------
# separation: a wrong adapter lies far outside the stage-local gate
# ----------------------------------------------------------------------------------------------------------------------------
def tiny_case():
    g = Golden("g19_tiny_attn_adapter")
    return g.spec, AU.golden_state(g), g.audio, g.lengths


def width_case():
    spec, state, _ = AU.width_model(S.xlsr_1b_encoder(), 16)
    audio, lengths = synthetic.make_audio(2, 48000, seed=1234, ragged=True)
    return spec, state, audio, lengths


_cases = {}


@pytest.fixture(params=["tiny", "xlsr_1b"])
def case(request):
    """(name, spec, state, hidden states of the fp32 evaluation, frames, per layer and mode: truth and e_emu)"""
    name = request.param
    if name not in _cases:
        spec, state, audio, lengths = {"tiny": tiny_case, "xlsr_1b": width_case}[name]()
        with torch.inference_mode():
            hidden, frames = AU.hidden_states(audio, lengths, state, spec, SU.Evaluation("fp32"))
            truth = [AU.layer_stage(hidden[i], frames, state, spec, SU.Evaluation("truth"), i) for i in range(spec["layers"])]
        _cases[name] = (name, spec, state, hidden, frames, truth, {})
    return _cases[name]


def test_adapter_term_is_visible(case):
    """the synthetic scales: the adapter's term is a visible share of the stream it is added to (std >= a fifth of the stream's)"""
    name, spec, state, hidden, frames, _, _ = case
    with torch.inference_mode():
        for i in range(spec["layers"]):
            # the stream the adapter of layer i sees: the layer without its adapter (and, for the last one, without the final norm)
            probe = dict(spec, layers=spec["layers"] + 1)
            stream = AU.layer_stage(hidden[i], frames, state, probe, SU.Evaluation("fp32"), i, defect="skipped")
            term = AU.adapter_term(stream, state, f"{AM}encoder.layers.{i}.adapter_layer.")
            n = int(frames[0])
            ratio = float(term[0, :n].std() / stream[0, :n].std())
            print(f"[attn-adapter] {name} layer{i}: std of the stream {float(stream[0, :n].std()):.2f}, of the adapter's term "
                  f"{float(term[0, :n].std()):.2f}")
            assert ratio > 0.2, (name, i, ratio)


@pytest.mark.parametrize("mode", ["f16x3", "bf16x3"])
def test_every_adapter_defect_is_separated(case, mode):
    name, spec, state, hidden, frames, truth, e_emus = case
    failures = []
    with torch.inference_mode():
        for i in range(spec["layers"]):
            if (i, mode) not in e_emus:
                e_emus[i, mode] = SU.against(AU.layer_stage(hidden[i], frames, state, spec, SU.Evaluation(mode), i), truth[i], frames)
            e_emu = e_emus[i, mode]
            for defect in AU.DEFECTS:
                if defect == "after_final_norm" and i != spec["layers"] - 1:
                    continue
                got = AU.layer_stage(hidden[i], frames, state, spec, SU.Evaluation(mode), i, defect=defect)
                ratio = SU.against(got, truth[i], frames) / e_emu
                print(f"[attn-adapter] {name} {mode} layer{i}: {defect}: {ratio:.3g} x e_emu ({e_emu:.3g})")
                if ratio < SEPARATION:
                    failures.append((name, mode, i, defect, ratio))
    assert not failures, failures

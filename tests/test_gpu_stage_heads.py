"""The classifier heads at every head geometry, held to the stage-local budget of tests/test_gpu_stage_local.py.

The heads stage -- ``concat_kernel``, ``time_ln_pe_kernel``, ``time_attention_kernel`` and ``logsoftmax_out_kernel``, the head
products laid out by ``create_heads`` and the composition product -- is judged by the other stage-local files at a handful of
shapes only (outputs of 4 .. 28 classes, compositions 16 .. 640 wide, time-layer head dimensions 2 and 16, one concatenated input).
Here the same gate,

    max |device_out - truth|  <=  3 x e_emu      over all outputs of the heads, from the device's own hidden states,

is put on the models of ``stage_util`` (``narrow_wide_model`` ... ``time_layer_model``), each of which names in its docstring the
switches of those kernels it crosses: the lane-local / whole-wave boundary of the log-softmax and its strides, softmax parts wider
than a wave, hidden-state parts that are not first, the zero fill of the concatenated rows, both plane layouts, two stacks of
direct heads, a composition whose K ends inside a 32-element group, inventories of 4 .. 1026 classes, time-layer head dimensions
1 .. 160.  tests/test_stage_util.py shows on the CPU, for every product of every one of these models, that one lost cross term puts
the heads at >= 7.5 x e_emu.

Every model runs on the tiny encoder (one or two layers) with the batch of ``stage_util.heads_audio``: 149, two ragged counts and
exactly one frame.  The gate is on the heads; the lines of the other stages, which run kernels that other files judge, are printed
only.  Also held here: raw logits, inventories installed on a handle that has run another (and the way back, bit for bit), exact
zeros beyond the lengths of every output, and the log-softmax on rows packed from the feature projection on.
"""
import pytest
import torch

from allophant_amd import spec as S
from tests import stage_util as SU
from tests import test_gpu_stage_production as production
from tests.test_gpu_parity import _custom_ragged
from tests.test_gpu_stage_local import amd, assert_within_budget, device_pass, stage_ratios  # noqa: F401  (``amd``: the fixture)

pytestmark = pytest.mark.gpu

AUDIO_SEED = 97
PINS = {"ln_fold": 0, "packed": 0}

MODELS = SU.HEADS_MODELS


def raw_logits_too(model):
    """the models that get a second pass with ``log_probabilities=False``"""
    return model == "narrow_wide" or model.startswith("time_layers/")


def heads_only(found):
    return {stage: pair for stage, pair in found.items() if stage.startswith("heads")}


def assert_zero_beyond_lengths(name, got):
    """the contract of ``logsoftmax_out_kernel``: every output, narrow or wide, is exactly zero at t >= lengths[n]"""
    frames = got["frames"].tolist()
    assert min(frames) < max(frames)
    for output, values in got["outputs"].items():
        for n, t in enumerate(frames):
            assert not values[n, t:].any(), (name, output, n)


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
@pytest.mark.parametrize("model", list(MODELS))
def test_heads_model(amd, model, precision):
    """One handle per model: every inventory in turn (each after the first on a handle that has run another), log-probabilities
    and -- narrow / wide and time layers -- raw logits; then the first inventory again, which must give its first bits."""
    raw_too = raw_logits_too(model)
    spec, state, inventories = MODELS[model]()
    audio, lengths = SU.heads_audio(AUDIO_SEED)
    picks = range(audio.shape[0])
    est = amd.Estimator(spec, state, "cuda:0", precision)
    try:
        first = None
        for tfi in inventories:
            name = model if len(inventories) == 1 else f"{model}/{tfi.shape[0]}"
            got = device_pass(amd, spec, state, tfi, audio, lengths, precision, PINS, est=est)
            assert_zero_beyond_lengths(name, got)
            found = stage_ratios(name, got, spec, state, tfi, audio, lengths, precision, picks, conv_key=model, per_output=True)
            if raw_too:
                raw = device_pass(amd, spec, state, tfi, audio, lengths, precision, PINS, log_probabilities=False, est=est)
                assert_zero_beyond_lengths(name, raw)
                found.update(heads_only(stage_ratios(name, raw, spec, state, tfi, audio, lengths, precision, picks,
                                                     log_probabilities=False, conv_key=model, per_output=True)))
            assert_within_budget(name, heads_only(found))
            first = first or got
        if len(inventories) > 1:
            again = device_pass(amd, spec, state, inventories[0], audio, lengths, precision, PINS, est=est)
            assert set(again["outputs"]) == set(first["outputs"])
            for output, values in first["outputs"].items():
                assert torch.equal(again["outputs"][output], values), (model, output)
    finally:
        est.close()


PACKED_EARLY = 2  # ``pass_info()["packed"]``: rows packed from the feature projection on, the heads and the log-softmax included


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_heads_on_packed_rows(amd, precision):
    """A pass without ``_keep_hidden`` whose log-softmax reads packed rows (the ``row_off`` branch).  The tiny encoder never packs
    early: that takes the window positional convolution, i.e. 64 channels per group and enough utterances to fill the chip.  So
    this is the smallest geometry of tests/test_gpu_stage_production.py that does -- the tiny encoder with two groups, 96 utterances
    of at most 1.5 s -- under the wide-dependency graph, whose classifiers on ``OUTPUT_0`` / ``OUTPUT_1`` make the pass hand out
    every hidden state.  Truth for the shortest, the longest and one more utterance."""
    enc = S.tiny_encoder(2)
    enc["pos_groups"] = 2
    spec, state, (tfi,) = SU.wide_dependency_model(True, enc)
    audio, lengths = _custom_ragged(96, 1.5, seed=77)
    got = production.device_pass(amd, spec, state, tfi, audio, lengths, precision, {"packed": PACKED_EARLY, "ln_fold": 0})
    assert_zero_beyond_lengths("packed", got)
    found = production.stage_ratios("heads/packed", got, spec, state, tfi, audio, lengths, precision,
                                    SU.shortest_longest_and(lengths, 1), per_output=True)
    assert_within_budget("heads/packed", heads_only(found))

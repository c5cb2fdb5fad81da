"""Encoders with attention adapters (``adapter_attn_dim``: the fine-tuned MMS encoders) on the device, held to the stage-local
budget of tests/test_gpu_stage_local.py and to the reference (golden g19).

Method and helpers are those of tests/test_gpu_stage_local.py (``device_pass`` with an ``expect`` dictionary, ``stage_ratios``,
``assert_within_budget`` with its ``FACTOR``) and, for passes without the keep flag, of tests/test_gpu_stage_production.py: per
stage, from the device's own input to it, max |device - float64 truth| <= 3 x e_emu.  The layer stage is
``attn_adapter_util.layer_stage`` -- the layer WITH its adapter, pinned to the reference by tests/test_attn_adapter.py -- put in
the place of ``stage_util.layer_stage`` for the duration of a test (the ``adapter_stage`` fixture).  tests/test_attn_adapter.py
shows that an adapter that is skipped, lacks its ReLU, ``b2`` or the beta of its LayerNorm, or sits on the wrong side of the FFN
residual or of the final LayerNorm lands at >= 1e4 x e_emu: every such mistake fails the layer stage here.

What the cases reach: the adapter kernel with its weights in registers (dimension 5, 16, 1) and read per row (64); one wave per
row (hidden 80: a row that is no multiple of 64 columns, and 128), five and eight waves (1280, 1920); the launch that also writes
the next layer's planes and the last layer's, which does not; padded rows, rows packed behind the positional convolution and from
the feature projection on; FFN2 with K chunks in front of the adapter (2 x 3 s at 1B / 2B width); a recorded and replayed pass.
``pass_info()["ln_fold"]`` is 0 throughout: adapter models do not fold their LayerNorms, also where the same model without
adapters does (``test_no_fold_where_the_plain_model_folds``).
"""
import pytest
import torch

from allophant_amd import spec as S, synthetic
from oracle import allophant_oracle as O
from tests import attn_adapter_util as AU, stage_util as SU
from tests import test_gpu_stage_production as production
from tests.golden_util import Golden, max_abs_valid_tm
from tests.test_gpu_parity import GATE, _custom_ragged
from tests.test_gpu_stage_local import amd, assert_within_budget, device_pass, stage_ratios  # noqa: F401  (``amd``: the fixture)
from tests.test_gpu_stage_widths import ENCODERS, FOLDS_FROM

pytestmark = pytest.mark.gpu
PRECISIONS = ["f16x3", "bf16x3"]


@pytest.fixture
def adapter_stage(monkeypatch):
    """``stage_ratios`` of both helper modules evaluate layers through ``SU.layer_stage``: the adapter layer in its place"""
    monkeypatch.setattr(SU, "layer_stage", AU.layer_stage)


@pytest.fixture(scope="module")
def g19():
    g = Golden("g19_tiny_attn_adapter")
    return g, AU.golden_state(g)


_width_models = {}


def width_model(width, tapped=False):
    if (width, tapped) not in _width_models:
        _width_models[width, tapped] = AU.width_model(ENCODERS[width](), 16, tapped)
    return _width_models[width, tapped]


def assert_reference_parity(amd, est, pred, g):
    """the project's parity gate: log-probabilities within 1e-3 of the reference's on valid frames, greedy alignments equal"""
    assert list(pred.outputs) == g.output_names and torch.equal(pred.lengths.cpu(), g.frame_lengths)
    worst = max(max_abs_valid_tm(pred.outputs[k].cpu(), g.logprobs(k), g.frame_lengths) for k in g.output_names)
    print(f"[attn-adapter] {g.name}: max |log-prob - reference| = {worst:.3g}")
    assert worst < GATE, worst
    decoded = est.greedy_decode(pred)
    for k in g.output_names:
        for i in range(len(g.lengths)):
            tokens, timesteps, _ = g.tokens(k, i)
            assert torch.equal(decoded[k][i][0].tokens, tokens) and torch.equal(decoded[k][i][0].timesteps, timesteps), (k, i)


# ----------------------------------------------------------------------------------------------------------------------------
# the keep-hidden pass: padded rows, every stage on its own
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_tiny_golden(amd, adapter_stage, g19, precision):
    """the tiny encoder (hidden 128) with dimension 5 on the ragged batch of g19: stage budget, the reference's log-probabilities
    and alignments, no fold"""
    g, state = g19
    got = device_pass(amd, g.spec, state, g.tfi, g.audio, g.lengths, precision, {"ln_fold": 0, "packed": 0, "graph": 0})
    found = stage_ratios("adapter/tiny", got, g.spec, state, g.tfi, g.audio, g.lengths, precision, (0, 1, 2), conv_key="adapter/tiny")
    assert_within_budget("adapter/tiny", found)
    est = amd.Estimator(g.spec, state, "cuda:0", precision)
    try:
        pred = est.predict(amd.Batch(g.audio.cuda(), g.lengths, torch.zeros(3, dtype=torch.long)), g.tfi)
        assert est.pass_info()["ln_fold"] == 0
        assert_reference_parity(amd, est, pred, g)
    finally:
        est.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("dim", [1, 64])
def test_row_of_80_columns(amd, adapter_stage, dim, precision):
    """hidden 80 (20 of a wave's 64 column blocks in use) with the smallest and the largest dimension: 1 in registers, 64 read
    per row in four groups of 16"""
    spec, state, tfi = AU.small_model(80, 2, 2, dim)
    audio, lengths = synthetic.make_audio(5, 24000, seed=80, ragged=True)
    got = device_pass(amd, spec, state, tfi, audio, lengths, precision, {"ln_fold": 0, "packed": 0})
    name = f"adapter/d80/a{dim}"
    found = stage_ratios(name, got, spec, state, tfi, audio, lengths, precision, SU.shortest_longest_and(lengths, 2), conv_key=name)
    assert_within_budget(name, found)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("width", list(ENCODERS))
def test_short_batch_at_width(amd, adapter_stage, width, precision):
    """2 x 3 s ragged on padded rows at 1B / 2B width, dimension 16: 298 rows, where FFN2 takes K chunks -- not deferred to a
    LayerNorm in front of an adapter -- and the adapter's workgroups have five / eight waves"""
    spec, state, tfi = width_model(width)
    audio, lengths = synthetic.make_audio(2, 48000, seed=1234, ragged=True)
    got = device_pass(amd, spec, state, tfi, audio, lengths, precision, {"ln_fold": 0, "packed": 0, "rows": 298})
    name = f"adapter/{width}/short"
    assert_within_budget(name, stage_ratios(name, got, spec, state, tfi, audio, lengths, precision, (0, 1), conv_key=name))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("width", list(ENCODERS))
def test_no_fold_where_the_plain_model_folds(amd, adapter_stage, width, precision):
    """the equal-length batch of 10 s utterances from which the same model WITHOUT adapters reports ``ln_fold`` 1
    (``FOLDS_FROM``): 0 here, the row passes and the adapter on 256-row product tiles.  Truth for the first and the last."""
    spec, state, tfi = width_model(width)
    n = FOLDS_FROM[width]
    audio, lengths = synthetic.make_audio(n, 160000, seed=778)
    got = device_pass(amd, spec, state, tfi, audio, lengths, precision, {"ln_fold": 0, "packed": 0, "rows": n * 499})
    name = f"adapter/{width}/large"
    found = stage_ratios(name, got, spec, state, tfi, audio, lengths, precision, (0, n - 1), conv_key=name)
    assert_within_budget(name, found)


# ----------------------------------------------------------------------------------------------------------------------------
# the pass without the keep flag: packed rows; the hidden states the classifiers tap are those behind the adapters
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_packed_layers(amd, adapter_stage, precision):
    """3 s + 2 s + 1.2 s at 1B width, ``stage_util.tapped_spec`` (classifiers on ``OUTPUT_0`` and ``OUTPUT_1``): the layers and their
    adapters on 307 packed rows, the last adapter in front of the unpacking and the final LayerNorm.  ``layer0`` judges the
    tapped hidden state 1 against the layer WITH its adapter."""
    spec, state, tfi = width_model("xlsr_1b", tapped=True)
    lengths = torch.tensor([48000, 32000, 19200])
    audio = synthetic.make_audio(3, 48000, seed=1234)[0]
    audio = audio * (torch.arange(48000).unsqueeze(0) < lengths.unsqueeze(1))
    got = production.device_pass(amd, spec, state, tfi, audio, lengths, precision, {"packed": 1, "ln_fold": 0, "rows": 149 + 99 + 59})
    name = "adapter/xlsr_1b/packed layers"
    found = production.stage_ratios(name, got, spec, state, tfi, audio, lengths, precision, (0, 1, 2), entry_key=name)
    assert set(found) == {"entry", "layer0", "layer1", "heads"}
    assert_within_budget(name, found)


def test_packed_early_replayed(amd, adapter_stage):
    """6 utterances of 2 .. 8 s at XLS-R 300M width: packed from the feature projection on, the third pass replayed from the
    recording of the second.  Truth for the shortest, the longest and one more."""
    spec, state, tfi = AU.width_model(S.xlsr_300m_encoder(), 16, tapped=True)
    audio, lengths = _custom_ragged(6, 8.0, seed=77)
    got = production.device_pass(amd, spec, state, tfi, audio, lengths, "f16x3", {"packed": 2, "ln_fold": 0, "graph": 2}, passes=3)
    name = "adapter/xlsr/packed early"
    found = production.stage_ratios(name, got, spec, state, tfi, audio, lengths, "f16x3", SU.shortest_longest_and(lengths, 1))
    assert_within_budget(name, found)


# ----------------------------------------------------------------------------------------------------------------------------
# reproducibility, the post-LN family, refusals
# ----------------------------------------------------------------------------------------------------------------------------
def test_replay_and_repeats_are_bitwise(amd, g19):
    """the g19 batch: a replayed recording gives the bits of the eager pass, and so does every repetition"""
    g, state = g19
    est = amd.Estimator(g.spec, state, "cuda:0", "f16x3")
    try:
        batch = amd.Batch(g.audio.cuda(), g.lengths, torch.zeros(3, dtype=torch.long))
        eager = est.predict(batch, g.tfi, _no_graph=True)
        assert est.pass_info()["graph"] == 0
        want = eager._flat.clone()
        again = est.predict(batch, g.tfi, _no_graph=True)
        assert torch.equal(again._flat, want)
        pred = est.predict(batch, g.tfi)
        seen = set()
        for _ in range(3):
            pred = est.predict(batch, g.tfi, _out=pred._flat)
            seen.add(est.pass_info()["graph"])
            assert torch.equal(pred._flat, want)
        assert 2 in seen, seen  # at least one of them was replayed from a recording
        est.check_finite()
    finally:
        est.close()


def test_post_ln_model_ignores_the_field(amd):
    """g19b: post-LN layers with ``adapter_attn_dim`` set -- the reference built no adapter; the device gives the reference's
    outputs, bit for bit those of the same model without the field"""
    g = Golden("g19b_tiny_attn_adapter_postln")
    state = AU.golden_state(g)
    batch = amd.Batch(g.audio.cuda(), g.lengths, torch.zeros(3, dtype=torch.long))
    est = amd.Estimator(g.spec, state, "cuda:0", "f16x3")
    try:
        pred = est.predict(batch, g.tfi)
        assert_reference_parity(amd, est, pred, g)
        with_field = pred._flat.clone()
    finally:
        est.close()
    plain = {k: v for k, v in g.spec.items() if k != "adapter_attn_dim"}
    est = amd.Estimator(plain, state, "cuda:0", "f16x3")
    try:
        assert torch.equal(est.predict(batch, g.tfi)._flat, with_field)
    finally:
        est.close()


def test_create_refusals(amd, g19):
    """``amx_create`` names the adapter tensor that is missing or mis-shaped, and refuses adapter tensors it would have to drop"""
    g, state = g19
    prefix = f"{SU.AM}encoder.layers.1.adapter_layer."
    for name in ("norm.weight", "norm.bias", "linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias"):
        missing = {k: v for k, v in state.items() if k != prefix + name}
        with pytest.raises(ValueError, match="missing tensor.*layers.1.adapter_layer." + name):
            amd.Estimator(g.spec, missing, "cuda:0", "f16x3")
    wrong = dict(state)
    wrong[prefix + "linear_1.weight"] = torch.zeros(6, g.spec["hidden"])
    with pytest.raises(ValueError, match=r"layers.1.adapter_layer.linear_1.weight has 768 elements, expected 640"):
        amd.Estimator(g.spec, wrong, "cuda:0", "f16x3")
    wrong = dict(state)
    wrong[prefix + "linear_2.bias"] = torch.zeros(g.spec["hidden"] + 8)
    with pytest.raises(ValueError, match=r"layers.1.adapter_layer.linear_2.bias has 136 elements, expected 128"):
        amd.Estimator(g.spec, wrong, "cuda:0", "f16x3")
    for dim in (None, 0):
        with pytest.raises(ValueError, match="adapter_layer.*adapter_attn_dim is 0"):
            amd.Estimator(dict(g.spec, adapter_attn_dim=dim), state, "cuda:0", "f16x3")
    with pytest.raises(ValueError, match="adapter_layer.*post-LN"):
        amd.Estimator(dict(g.spec, stable_layer_norm=False), state, "cuda:0", "f16x3")
    with pytest.raises(ValueError, match="adapter_attn_dim"):
        amd.Estimator(dict(g.spec, adapter_attn_dim=65), state, "cuda:0", "f16x3")

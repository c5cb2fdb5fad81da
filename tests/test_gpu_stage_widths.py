"""The XLS-R 1B / 2B widths and head dimensions other than 64, held to the stage-local budget of tests/test_gpu_stage_local.py.

Every case of that file and of tests/test_gpu_stage_production.py runs at hidden 1024 or 768 with heads of 64 columns, or on the
tiny model.  What is instantiated separately for the other released widths ran only under the 1e-3 gate of
tests/test_gpu_head_dim.py, which a lost cross term passes:

* the attention instances for head dimensions other than 64 -- ``pass_info()["attention"]`` 4 (rows of 64 columns, head dimension
  8 ... 56) and 5 (rows of 128 columns) with its three instances: five 16-column steps of the score chain for up to 80 columns
  (XLS-R 1B), six for up to 96, and the full width (120: XLS-R 2B; 128) -- each on padded rows and on row offsets;
* the row kernels' instance for rows wider than 1024, the LayerNorm fold with 20 / 30 column blocks per row, the grouped
  implicit-GEMM positional convolution at 80 / 120 channels per group, and the GEMM routes of N, K = 1280, 1920, 5120, 7680.

Same gate, same method: per stage, from the device's own input to it, max |device - float64 truth| <= 3 x e_emu.  The keep-hidden
cases use ``device_pass`` / ``stage_ratios`` of tests/test_gpu_stage_local.py, the cases without the flag those of
tests/test_gpu_stage_production.py (models of ``stage_util.tapped_spec``; ``entry`` stands for conv + front).  tests/test_stage_util.py
shows on the CPU, for the same models (``xlsr_1b``, ``xlsr_2b``, ``dh40``, ``dh8``, ``dh96``, ``dh128``), that a cross term lost from any
product -- Q.K^T and P.V of every attention instance among them -- lands at >= 7.5 x e_emu, or at >= 6.0 where listed there.  The
one exception is the second layer under the LayerNorm fold on bf16 planes (4.9 / 4.6 x at 1B / 2B width,
``stage_util.NOT_CLAIMED``): the folded bf16x3 cases print that layer's ratio and assert on every other stage.

Routes, as ``pass_info()`` reports them on an MI355X and as every case pins them: equal-length batches of 10 s utterances fold from
24 utterances on at 1B width (16 do not) and from 16 on at 2B width; the window positional convolution does not take 80 or 120
channels per group, so a ragged batch packs behind the grouped one (``packed`` 1), never from the feature projection on.
"""
import pytest
import torch

from allophant_amd import spec as S, synthetic
from tests import stage_util as SU
from tests import test_gpu_stage_production as production
from tests.test_gpu_parity import _custom_ragged
from tests.test_gpu_stage_local import amd, assert_within_budget, device_pass, stage_ratios  # noqa: F401  (``amd``: the fixture)

pytestmark = pytest.mark.gpu

ENCODERS = {"xlsr_1b": S.xlsr_1b_encoder, "xlsr_2b": S.xlsr_2b_encoder}
FOLDS_FROM = {"xlsr_1b": 24, "xlsr_2b": 16}  # utterances of 10 s, equal lengths: the smallest of 16, 24 that report ``ln_fold`` 1
HEAD_DIM_ATTENTION = {40: 4, 8: 4, 96: 5, 128: 5}
_models = {}


def width_model(width, tapped=False):
    """two layers at the width of XLS-R 1B / 2B, the heads and seeds of the XLS-R case (``tapped``: of the production cases)"""
    if (width, tapped) not in _models:
        if tapped:
            spec = SU.tapped_spec(ENCODERS[width]())
        else:
            spec = S.multitask_spec(dict(ENCODERS[width](), layers=2), ["syllabic", "long"], allophone_layer=True)
            spec["shared_phones"] = 80
        _models[width, tapped] = spec, synthetic.make_state_dict(spec, seed=0), synthetic.make_inventory(spec, 27, seed=0)
    return _models[width, tapped]


def head_dim_tapped_model(hidden, heads, groups):
    spec = SU.tapped_spec(SU.head_dim_encoder(hidden, heads, groups), embedding_size=16, train_phonemes=9, n_features=5)
    return spec, synthetic.make_state_dict(spec, seed=hidden + heads), synthetic.make_inventory(spec, 7, seed=3)


def head_dim_batch(hidden):
    """5 ragged utterances of 0.75 ... 1.5 s, 15 ... 30 % padding: what tests/test_stage_util.py takes for the same model"""
    return synthetic.make_audio(5, 24000, seed=hidden, ragged=True)


def claimed(case, precision, found, folded):
    """``found`` without the stages that the separation proof does not claim for this case and mode"""
    def proof_name(stage):
        return stage + "/fold" if folded and stage.startswith("layer") else stage

    return {stage: v for stage, v in found.items() if (case, precision, proof_name(stage)) not in SU.NOT_CLAIMED}


# ----------------------------------------------------------------------------------------------------------------------------
# the keep-hidden pass: padded rows, every stage on its own
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
@pytest.mark.parametrize("width", list(ENCODERS))
def test_short_batch(amd, width, precision):
    """2 x 3 s ragged on padded rows: the row kernels for rows wider than 1024, the grouped positional convolution at 80 / 120
    channels per group, tile / DMA GEMMs at N, K = 1280 ... 7680 with K chunks, attention on 128-wide rows with the score chain
    stopping at 80 columns (1B) or running all of them (2B: 120)"""
    spec, state, tfi = width_model(width)
    audio, lengths = synthetic.make_audio(2, 48000, seed=1234, ragged=True)
    got = device_pass(amd, spec, state, tfi, audio, lengths, precision, {"attention": 5, "ln_fold": 0, "packed": 0, "rows": 298})
    name = f"{width}/short"
    assert_within_budget(name, stage_ratios(name, got, spec, state, tfi, audio, lengths, precision, (0, 1), conv_key=name))


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
@pytest.mark.parametrize("width", list(ENCODERS))
def test_fold_batch(amd, width, precision):
    """``ln_fold == 1`` at 1B / 2B width: producers and consumers of the LayerNorm fold with 20 / 30 column blocks per row, the
    ping-pong GEMM on these shapes, attention as above on a full chip.  Truth for the first and the last utterance.  bf16x3: the
    second folded layer is printed, not asserted (``stage_util.NOT_CLAIMED``)."""
    spec, state, tfi = width_model(width)
    n = FOLDS_FROM[width]
    audio, lengths = synthetic.make_audio(n, 160000, seed=778)
    got = device_pass(amd, spec, state, tfi, audio, lengths, precision, {"attention": 5, "ln_fold": 1, "packed": 0, "rows": n * 499})
    name = f"{width}/fold"
    found = stage_ratios(name, got, spec, state, tfi, audio, lengths, precision, (0, n - 1), conv_key=name)
    assert_within_budget(name, claimed(width, precision, found, folded=True))


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
@pytest.mark.parametrize("hidden,heads,groups", SU.HEAD_DIM_MODELS)
def test_head_dims(amd, hidden, heads, groups, precision):
    """head dimensions 40 and 8 (rows of 64 columns), 96 (the only case that reaches the six-step score chain) and 128 on the tiny
    encoder, padded rows.  Truth for the shortest, the longest and two more."""
    spec, state, tfi = SU.head_dim_model(hidden, heads, groups)
    audio, lengths = head_dim_batch(hidden)
    dh = hidden // heads
    got = device_pass(amd, spec, state, tfi, audio, lengths, precision, {"attention": HEAD_DIM_ATTENTION[dh], "ln_fold": 0, "packed": 0})
    name = f"dh{dh}"
    found = stage_ratios(name, got, spec, state, tfi, audio, lengths, precision, SU.shortest_longest_and(lengths, 2), conv_key=name)
    assert_within_budget(name, found)


# ----------------------------------------------------------------------------------------------------------------------------
# the pass without the keep flag: packed rows, attention by row offsets
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,precision", [("xlsr_1b", "f16x3"), ("xlsr_1b", "bf16x3"), ("xlsr_2b", "f16x3")])
def test_packed_layers(amd, width, precision):
    """3 s + 2 s + 1.2 s (149 / 99 / 59 frames): the layers on 307 packed rows, the attention instances of 1B / 2B width on row
    offsets.  ``packed`` is 1: the rows are packed behind the grouped positional convolution.  Truth for all three."""
    spec, state, tfi = width_model(width, tapped=True)
    lengths = torch.tensor([48000, 32000, 19200])
    audio = synthetic.make_audio(3, 48000, seed=1234)[0]
    audio = audio * (torch.arange(48000).unsqueeze(0) < lengths.unsqueeze(1))
    got = production.device_pass(amd, spec, state, tfi, audio, lengths, precision,
                                 {"packed": 1, "attention": 5, "ln_fold": 0, "rows": 149 + 99 + 59})
    name = f"{width}/packed layers"
    found = production.stage_ratios(name, got, spec, state, tfi, audio, lengths, precision, (0, 1, 2), entry_key=name)
    assert_within_budget(name, found)


@pytest.mark.parametrize("hidden,heads,groups", [(80, 2, 2), (192, 2, 4)])
def test_packed_head_dims(amd, hidden, heads, groups):
    """head dimensions 40 and 96 on the tiny encoder without the keep flag: 273 / 293 packed rows (``packed`` 1), the 64-column
    and the six-step 128-column attention instances on row offsets.  Truth for four of the five utterances."""
    spec, state, tfi = head_dim_tapped_model(hidden, heads, groups)
    audio, lengths = head_dim_batch(hidden)
    dh = hidden // heads
    got = production.device_pass(amd, spec, state, tfi, audio, lengths, "f16x3",
                                 {"packed": 1, "attention": HEAD_DIM_ATTENTION[dh], "ln_fold": 0})
    name = f"dh{dh}/packed layers"
    found = production.stage_ratios(name, got, spec, state, tfi, audio, lengths, "f16x3", SU.shortest_longest_and(lengths, 2))
    assert_within_budget(name, found)


def test_fold_on_packed_rows_1b(amd):
    """16 utterances of 2.5 ... 10 s at 1B width: 5124 of 7984 rows valid, which both packs (``packed`` 1) and takes the LayerNorm
    fold -- its producer tiles end inside utterances, 20 column blocks per row.  (16 ... 24 utterances of 5 ... 10 s pack and do not
    fold at this width.)  Truth for the shortest, the longest and one more."""
    spec, state, tfi = width_model("xlsr_1b", tapped=True)
    audio, lengths = _custom_ragged(16, 10.0, seed=77)
    got = production.device_pass(amd, spec, state, tfi, audio, lengths, "f16x3",
                                 {"packed": 1, "attention": 5, "ln_fold": 1, "rows": 5124})
    found = production.stage_ratios("xlsr_1b/fold/packed", got, spec, state, tfi, audio, lengths, "f16x3",
                                    SU.shortest_longest_and(lengths, 1))
    assert_within_budget("xlsr_1b/fold/packed", found)

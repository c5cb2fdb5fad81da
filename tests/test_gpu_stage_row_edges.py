"""The partial last row tile of every product of an encoder layer, held to the stage-local budget of tests/test_gpu_stage_local.py.

The other stage-local files reach the encoder products at a handful of row counts, so each product's last row tile ends wherever
those happen to put it.  What the kernels do there is a path of its own: the ping-pong kernel picks its epilogue per wave group of
``HALF`` rows and sends every group that crosses ``M`` to ``pp_epilogue_generic`` (row masks, the (b, t) walk of the QKV scatter,
rows beyond ``M`` clamped to ``M - 1`` in the LayerNorm-fold producer with only the stores predicated, ``row_coef[m]`` per row in
the consumer), its operand DMA clamps rows the same way, and the split-K fix-ups, the LDS-DMA tiles and the register-staged tiles
have row tails of their own.  A wrong row coefficient, a bias missing on the masked rows, a store one row too far or a clamped
row's statistics leaking into a valid row puts the rows concerned far above ``3 x e_emu`` -- if those rows are judged.

tests/row_edge_util.py holds the cases: batches of XLS-R width (two layers, ``xlsr_model()``) whose row count ends a chosen number
of rows into the last tile, by family (fold on 256-row and on 128-row tiles, plain 128-row tiles, the routing thresholds, short
products with K chunks, utterances of 7 / 8 / 9 frames in the padded layout).  tests/test_gemm_routes.py proves on the CPU that
each case reaches the kernel, tile, residue and fold role it declares; here ``pass_info()`` pins ``rows``, ``packed`` and
``ln_fold``.  Every batch ends in the same short utterances (the tail, the last of one frame): packed rows lie in utterance
order, so the tail is the last partial tile and the boundary in front of it, and only the tail is judged -- its truth and e_emu
do not depend on what stands in front of it, and the bodies are never evaluated on the CPU.

Method and helpers are those of tests/test_gpu_stage_production.py (no ``_keep_hidden``; hidden 0, 1 and 2 are all handed out).
Beyond the gate every case asserts ``check_finite()``, exact zeros beyond each utterance's length in every output and, on rows
packed early, in every fetched hidden state, and that a second pass of the batch into the same output buffer gives the bits of
a first pass (a race on clamped rows would show there).  DESIGN.md, "Stage-local error budget", records the ratios.
"""
import pytest
import torch

from tests import row_edge_util as RE
from tests.test_gpu_stage_local import amd, assert_within_budget  # noqa: F401  (``amd``: the module's fixture)
from tests.test_gpu_stage_production import device_pass, stage_ratios, xlsr_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def xlsr():
    return xlsr_model()


def assert_zero_beyond_lengths(name, got, hidden_too):
    """every output -- and, where the pass defines it (rows packed early), every fetched hidden state -- is exactly zero at
    t >= frames[n], for every utterance of the batch"""
    frames = got["frames"].tolist()
    tensors = dict(got["outputs"])
    if hidden_too:
        tensors.update({f"hidden{i}": h for i, h in enumerate(got["hidden"])})
    for what, values in tensors.items():
        for n, t in enumerate(frames):
            assert not values[n, t:].any(), (name, what, n)


def assert_same_bits(name, first, second):
    for i, (a, b) in enumerate(zip(first["hidden"], second["hidden"])):
        frames = first["frames"].tolist()
        for n, t in enumerate(frames):  # (packed layers leave the padding of a kept state undefined: the valid frames)
            assert torch.equal(a[n, :t], b[n, :t]), (name, f"hidden{i}", n)
    assert set(first["outputs"]) == set(second["outputs"])
    for output, values in first["outputs"].items():
        assert torch.equal(values, second["outputs"][output]), (name, output)


def only(got, audio, lengths, picks):
    """the pass, the audio and the lengths restricted to utterances ``picks`` and cut to the longest of them: what
    ``stage_ratios`` evaluates on the CPU is then the judged utterances alone, not their padding up to the body's length"""
    frames = got["frames"][picks]
    t, samples = int(frames.max()), int(lengths[picks].max())
    cut = {"hidden": [h[picks, :t] for h in got["hidden"]], "outputs": {k: v[picks, :t] for k, v in got["outputs"].items()},
           "frames": frames, "ln_fold": got["ln_fold"]}
    return cut, audio[picks, :samples], lengths[picks]


@pytest.mark.parametrize("name,precision", RE.GPU_CASES)
def test_row_edge(amd, xlsr, name, precision):
    """One case of tests/row_edge_util.py: a first pass on a fresh handle, then on another handle two passes into one output
    buffer; the second one is judged stage by stage over the tail (padded family: the first utterance and the last
    two) and must equal the first pass bit for bit."""
    case = RE.CASES[name]
    spec, state, tfi = xlsr
    audio, lengths, picks = RE.batch(case)
    pins = {"rows": case.M, "packed": case.packed, "ln_fold": case.ln_fold}
    first = device_pass(amd, spec, state, tfi, audio, lengths, precision, pins)
    got = device_pass(amd, spec, state, tfi, audio, lengths, precision, pins, passes=2)
    assert first["frames"].tolist() == RE.utterance_frames(case) == got["frames"].tolist()
    for each in (first, got):
        assert_zero_beyond_lengths(name, each, hidden_too=case.packed == 2)
    assert_same_bits(name, first, got)
    cut, cut_audio, cut_lengths = only(got, audio, lengths, picks)
    # (the tail is the same audio in every case of a family, and of every family with the same tail: one truth of its entry stage)
    entry_key = f"row edges/{len(case.tail)}" if case.tail else None
    found = stage_ratios(name, cut, spec, state, tfi, cut_audio, cut_lengths, precision, range(len(picks)), entry_key=entry_key)
    assert set(found) == {"entry", "layer0", "layer1", "heads"}
    assert_within_budget(name, found)

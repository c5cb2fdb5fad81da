"""Every stage of the HIP path against float64, judged alone and at split-precision accuracy.

The parity tests gate everything at 1e-3 against the fp32 oracle, 20 to 100 times above what the two-plane modes deliver: a
product that lost one of its cross terms (hi.lo or lo.hi), or ran in plain fp16 altogether, passes them.  Here each stage (conv
extractor, front, every encoder layer, heads: tests/stage_util.py) is evaluated on the CPU from the DEVICE's own input to that
stage -- ``debug_fetch("conv" | "hidden", i)`` of one ``predict(..., _keep_hidden=True)`` -- so that nothing accumulates over
stages, once in float64 (the truth) and once with every product as hi.hi + lo.hi + hi.lo on 16-bit planes (error ``e_emu``
against the truth).  Gate, per stage, over the valid frames of the picked utterances:

    max |device_out - truth|  <=  3 x e_emu

The emulation has the kernels' planes and their three products, not their summation order or fast GELU / exp: hence 3.  One
approximation of the kernels is in it because the factor does not cover it: under the LayerNorm fold the two-plane modes keep the
residual stream as planes of (x - pivot) * scale between the products of a layer (``stage_util.stream_planes``) -- 16 bits on bf16
planes, which alone puts a folded bf16x3 layer at 5e-5, four times its unfolded error; on fp16 planes (22 bits) it is invisible.  tests/test_stage_util.py shows on the CPU that one lost cross term in
any one product puts a stage at >= 7.5 x e_emu, i.e. >= 2.5 x above this gate.  The ratio device error / e_emu of every (case,
stage) is printed; DESIGN.md, "Stage-local error budget", records them.

The cases are the smallest geometries that reach each family of kernels; ``pass_info()`` pins the route where it reports it.

Every case here runs ``_keep_hidden``, i.e. padded and eager, with the conv stage in its two-pass form.  What a pass without the
flag takes instead -- packed rows, the conv extractor's per-utterance tiles, the fused pass behind the last conv layer, the
recorded graph -- is held to the same gate by tests/test_gpu_stage_production.py (packed and padded rows are the same bits only on
the tiny model, so the budget does not carry over by itself).  The XLS-R 1B / 2B widths and head dimensions other than 64, whose
attention, row-kernel, fold and positional-convolution instances no case here reaches, are held to it by
tests/test_gpu_stage_widths.py.  The heads stage at the geometries no case here reaches -- both paths and every stride of the
log-softmax, wide and late parts of the concatenation, a second stack of direct heads, compositions of 4 .. 1026 classes,
time-layer head dimensions 1 .. 160 -- is held to it by tests/test_gpu_stage_heads.py, with the helpers of this file.  Where a row
count ends inside the last row tile of a product -- every residue at which the edge epilogues, the fix-ups and the short tiles take
another path, and both sides of the routing thresholds -- is held to it by tests/test_gpu_stage_row_edges.py.

Not covered: the single-plane modes (``f16``, ``bf16``): no cross terms to lose; they keep their own bounds.
"""
import pytest
import torch

from allophant_amd import spec as S, synthetic
from tests import stage_util as SU

pytestmark = pytest.mark.gpu
FACTOR = 3.0


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import estimator, lib

    assert lib.load() is not None
    return estimator


def device_pass(amd, spec, state, tfi, audio, lengths, precision, expect, log_probabilities=True, est=None):
    """one ``predict(..., _keep_hidden=True)``: the conv output, every hidden state and the outputs, on the host, batch-major.
    ``est``: an estimator of the caller's that has run other passes (and stays open) instead of a fresh one"""
    n = audio.shape[0]
    own = est is None
    if own:
        est = amd.Estimator(spec, state, "cuda:0", precision)
    try:
        pred = est.predict(amd.Batch(audio.cuda(), lengths, torch.zeros(n, dtype=torch.long)), tfi, log_probabilities, _keep_hidden=True)
        info = est.pass_info()
        est.check_finite()
        for key, value in expect.items():
            assert info[key] == value, (key, value, info)  # the case reaches the kernels it is there for
        return {"conv": est.debug_fetch("conv"),
                "hidden": [est.debug_fetch("hidden", i) for i in range(spec["layers"] + 1)],
                "outputs": {k: v.cpu().transpose(0, 1) for k, v in pred.outputs.items()},
                "frames": pred.lengths.cpu(), "ln_fold": info["ln_fold"] == 1}
    finally:
        if own:
            est.close()


_conv_truth, _conv_e_emu = {}, {}  # the conv stage's input is the audio: its truth and e_emu do not depend on the device


def stage_ratios(name, got, spec, state, tfi, audio, lengths, precision, picks, log_probabilities=True, conv_key=None,
                 per_output=False):
    """``got``: a ``device_pass``.  Per stage, from the device's input to it and over utterances ``picks``: the truth, e_emu of
    ``precision`` and the device's error; prints and returns {stage: (device error, e_emu)}.  ``conv_key``: runs that differ in
    nothing the conv stage sees (precision apart) share its truth and e_emu under this key.  ``per_output``: also prints the
    pair of every output of the heads (``heads/<output>``), for information: the gate is on the joint one."""
    picks = list(picks)
    frames = got["frames"][picks]
    offsets = synthetic.category_offsets(spec) if spec.get("embedding_size") else None
    assert torch.equal(got["frames"], torch.tensor(S.frame_lengths(lengths.tolist(), spec)))
    found = {}

    def judge(stage, run, device_out):
        found[stage] = SU.judged(run, device_out, frames, precision)

    def conv(ev):
        return SU.conv_stage(SU.normalize(audio[picks], lengths[picks], spec, ev), state, spec, ev)

    with torch.inference_mode():
        key = (conv_key, tuple(picks))
        truth = _conv_truth.get(key) if conv_key else None
        if truth is None:
            truth = _conv_truth[key] = conv(SU.Evaluation("truth"))
        e_emu = _conv_e_emu.get(key + (precision,)) if conv_key else None
        if e_emu is None:
            e_emu = _conv_e_emu[key + (precision,)] = SU.against(conv(SU.Evaluation(precision)), truth, frames)
        found["conv"] = (SU.against(got["conv"][picks], truth, frames), e_emu)
    judge("front", lambda ev: SU.front_stage(got["conv"][picks], frames, state, spec, ev), got["hidden"][0][picks])
    for i in range(spec["layers"]):
        # (a pass that folded the LayerNorm kept the stream in planes between the products: the emulation does the same)
        judge(f"layer{i}", lambda ev, i=i: SU.layer_stage(got["hidden"][i][picks], frames, state, spec, ev, i, fold=got["ln_fold"]),
              got["hidden"][i + 1][picks])
    heads_in = {i: got["hidden"][i][picks] for i in SU.hidden_inputs(spec)}
    heads, each = "heads" if log_probabilities else "heads (logits)", {}
    found[heads] = SU.judged(lambda ev: SU.heads_stage(heads_in, frames, state, spec, tfi, offsets, ev)[1 if log_probabilities else 0],
                             {k: v[picks] for k, v in got["outputs"].items()}, frames, precision, each if per_output else None)
    SU.report(name, precision, found)
    SU.report(name, precision, {f"{heads}/{k}": v for k, v in each.items()})
    return found


def assert_within_budget(name, found):
    over = {stage: (error, e_emu, error / e_emu) for stage, (error, e_emu) in found.items() if not error <= FACTOR * e_emu}
    assert not over, (name, over)


def xlsr_model(seed=0):
    """XLS-R width, two layers, two attribute heads and the composed phoneme head behind an allophone layer"""
    enc = S.xlsr_300m_encoder()
    enc["layers"] = 2
    spec = S.multitask_spec(enc, ["syllabic", "long"], allophone_layer=True)
    spec["shared_phones"] = 80
    return spec, synthetic.make_state_dict(spec, seed=seed), synthetic.make_inventory(spec, 27, seed=seed)


@pytest.fixture(scope="module")
def xlsr():
    return xlsr_model()


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_short_batch(amd, xlsr, precision):
    """2 x 3 s ragged, fewer than 384 rows: tile / DMA GEMMs with K chunks, the fix-up merged into the row norm, the grouped-GEMM
    positional convolution, short-key attention on 4-wave workgroups"""
    spec, state, tfi = xlsr
    audio, lengths = synthetic.make_audio(2, 48000, seed=1234, ragged=True)
    got = device_pass(amd, spec, state, tfi, audio, lengths, precision, {"ln_fold": 0, "packed": 0, "graph": 0, "attention": 1})
    assert_within_budget("short", stage_ratios("short", got, spec, state, tfi, audio, lengths, precision, (0, 1)))


def test_mid_batch(amd, xlsr):
    """4 x 10 s: 128-row ping-pong tiles on both widths, DMA tiles, no fold, 4-wave attention with the key split"""
    spec, state, tfi = xlsr
    audio, lengths = synthetic.make_audio(4, 160000, seed=55)
    got = device_pass(amd, spec, state, tfi, audio, lengths, "f16x3", {"ln_fold": 0, "packed": 0, "attention": 2, "rows": 4 * 499})
    assert_within_budget("mid", stage_ratios("mid", got, spec, state, tfi, audio, lengths, "f16x3", (0, 1, 2, 3)))


def fold_batch(layout):
    """16 x 10 s; "padded": every third utterance 9000 samples shorter -- too little padding to pack, so the fold runs on the
    padded layout with its padded frames, edge blocks and row masks (as tests/test_gpu_fold_range.py)"""
    audio, lengths = synthetic.make_audio(16, 160000, seed=778)
    if layout == "padded":
        lengths[1::3] -= 9000
        for i in range(16):
            audio[i, int(lengths[i]):] = 0
    return audio, lengths


@pytest.mark.parametrize("layout", ["equal", "padded"])
@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_fold_batch(amd, xlsr, precision, layout):
    """``ln_fold == 1``: producers and consumers of the LayerNorm fold, 256-row tiles, the window positional convolution, 8-wave
    attention.  Truth for four utterances: the first, the last and two more (shaved ones in the padded layout: 1 and 10)."""
    spec, state, tfi = xlsr
    audio, lengths = fold_batch(layout)
    got = device_pass(amd, spec, state, tfi, audio, lengths, precision, {"ln_fold": 1, "packed": 0, "attention": 0, "rows": 16 * 499})
    found = stage_ratios(f"fold/{layout}", got, spec, state, tfi, audio, lengths, precision, (0, 1, 10, 15), conv_key=f"fold/{layout}")
    assert_within_budget(f"fold/{layout}", found)


def test_long_utterance(amd, xlsr):
    """1 x 60 s: the window positional convolution with a partial last tile, 2999 keys per query.  One utterance does not fill the
    chip, so it keeps the 8-wave attention kernel (``attention_form``); ``test_long_key_attention`` reaches the long-key one."""
    spec, state, tfi = xlsr
    audio, lengths = synthetic.make_audio(1, 960000, seed=60)
    got = device_pass(amd, spec, state, tfi, audio, lengths, "f16x3", {"ln_fold": 0, "packed": 0, "attention": 0, "rows": 2999})
    assert_within_budget("long", stage_ratios("long", got, spec, state, tfi, audio, lengths, "f16x3", (0,)))


def test_long_key_attention(amd, xlsr):
    """6 x 20 s, the last one 9000 samples shorter: 999 frames (>= 960) on a full chip is what ``attention_form`` gives the
    long-key kernel (form 3), here with masked keys.  Truth for the first and the last utterance."""
    spec, state, tfi = xlsr
    audio, lengths = synthetic.make_audio(6, 320000, seed=61)
    lengths[5] -= 9000
    audio[5, int(lengths[5]):] = 0
    got = device_pass(amd, spec, state, tfi, audio, lengths, "f16x3", {"packed": 0, "attention": 3, "rows": 6 * 999})
    assert_within_budget("long keys", stage_ratios("long keys", got, spec, state, tfi, audio, lengths, "f16x3", (0, 5)))


@pytest.mark.parametrize("masked", [False, True])
def test_post_ln_family(amd, masked):
    """wav2vec2-base shape, two layers, 8 x 5 s ragged: the group-norm extractor, post-LN layers, 48 channels per group of the
    positional convolution; with and without the attention mask.  Truth for utterances 0, 3, 5 and 7."""
    enc = S.wav2vec2_base_encoder()
    enc["layers"] = 2
    enc["use_attention_mask"] = masked
    spec = S.multitask_spec(enc, ["syllabic", "long"], allophone_layer=True)
    spec["shared_phones"] = 80
    state = synthetic.make_state_dict(spec, seed=23)
    tfi = synthetic.make_inventory(spec, 27, seed=23)
    audio, lengths = synthetic.make_audio(8, 80000, seed=82, ragged=True)
    got = device_pass(amd, spec, state, tfi, audio, lengths, "f16x3", {"ln_fold": 0, "packed": 0})
    name = f"post-LN/{'masked' if masked else 'unmasked'}"
    found = stage_ratios(name, got, spec, state, tfi, audio, lengths, "f16x3", (0, 3, 5, 7), conv_key="post-LN")
    assert_within_budget(name, found)


@pytest.mark.parametrize("blanks", [True, False])
def test_hierarchical_heads(amd, blanks):
    """tiny encoder, 3 x 2 s ragged, the hierarchical model of ``stage_util.heads_case_spec``: ``concat_kernel`` with and without
    the blanks, ``time_ln_pe`` / ``time_attention``, the composition -- log-probabilities and, from a second pass, raw logits"""
    spec = SU.heads_case_spec(blanks)
    state = synthetic.make_state_dict(spec, seed=21)
    tfi = synthetic.make_inventory(spec, 9, seed=5)
    audio, lengths = synthetic.make_audio(3, 32000, seed=41, ragged=True)
    name = f"heads/{'blanks' if blanks else 'no blanks'}"
    got = device_pass(amd, spec, state, tfi, audio, lengths, "f16x3", {"ln_fold": 0, "packed": 0})
    found = stage_ratios(name, got, spec, state, tfi, audio, lengths, "f16x3", (0, 1, 2), conv_key=name)
    raw = device_pass(amd, spec, state, tfi, audio, lengths, "f16x3", {"ln_fold": 0, "packed": 0}, log_probabilities=False)
    again = stage_ratios(name, raw, spec, state, tfi, audio, lengths, "f16x3", (0, 1, 2), log_probabilities=False, conv_key=name)
    found["heads (logits)"] = again["heads (logits)"]
    assert_within_budget(name, found)

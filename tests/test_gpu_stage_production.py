"""The pass that production runs -- no ``_keep_hidden`` -- held to the stage-local budget of tests/test_gpu_stage_local.py.

``_keep_hidden`` switches off most of what a real batch takes: packed rows (the encoder layers on the valid frames only, attention
by per-utterance row offsets, from the feature projection on when the window positional convolution runs: ``packed`` 1 / 2), the
conv extractor's per-utterance tiles, the fused pass behind the last conv layer (LayerNorm + GELU + the projection's LayerNorm in
one kernel) and the recorded graph.  At XLS-R width the packed row count picks other tile heights and K chunks than the padded
one, so the budget shown on the keep pass does not carry over by itself.  Here the same gate,

    max |device_out - truth|  <=  3 x e_emu      per stage, from the device's own input to it,

is put on passes without the flag.  What such a pass leaves to look at: ``debug_fetch("hidden", i)`` hands out hidden state i
whenever a classifier reads ``OUTPUT_i`` and, for the pre-LN encoder, the final one; so the model (``stage_util.tapped_spec``) has
classifiers on ``OUTPUT_0`` and ``OUTPUT_1``.  The conv output is not kept: ``entry`` (audio -> hidden[0]) takes the place of conv
and front.  The post-LN encoder does not keep hidden[layers]: ``tail`` (last layer + heads) takes the place of both.
tests/test_stage_util.py shows the separation condition for the two combined stages as for the others.

Every case pins its route through ``pass_info()``.  ``test_fetch_of_packed_rows_*`` ties the fetch itself (the unpacking by row
offsets) to the padded pass on the tiny model, where both layouts give the same bits: a wrong row offset cannot pass as kernel
error here, nor kernel error as a fetch bug.

Not held: the single-plane modes (``f16``, ``bf16``: no cross terms to lose; they keep their own bounds).  The row counts here end
each product's last row tile wherever they happen to; tests/test_gpu_stage_row_edges.py holds the chosen residues, with these helpers.
"""
import pytest
import torch

from allophant_amd import spec as S, synthetic
from tests import stage_util as SU
from tests.test_gpu_parity import _custom_ragged
from tests.test_gpu_stage_local import amd, assert_within_budget  # noqa: F401  (``amd``: the module's fixture)

pytestmark = pytest.mark.gpu


def device_pass(amd, spec, state, tfi, audio, lengths, precision, expect, log_probabilities=True, passes=1):
    """``passes`` x ``predict`` of one batch without ``_keep_hidden`` (the later ones from the same device audio into the same
    output buffer: a recording is keyed on both), then every hidden state such a pass hands out and the outputs of the last one,
    on the host, batch-major"""
    n = audio.shape[0]
    est = amd.Estimator(spec, state, "cuda:0", precision)
    try:
        batch = amd.Batch(audio.cuda(), lengths, torch.zeros(n, dtype=torch.long))
        pred = est.predict(batch, tfi, log_probabilities)
        for _ in range(passes - 1):
            pred = est.predict(batch, tfi, log_probabilities, _out=pred._flat)
        info = est.pass_info()
        est.check_finite()
        for key, value in expect.items():
            assert info[key] == value, (key, value, info)  # the case reaches the kernels it is there for
        kept = spec["layers"] + 1 if spec.get("stable_layer_norm", True) else spec["layers"]
        return {"hidden": [est.debug_fetch("hidden", i) for i in range(kept)],
                "outputs": {k: v.cpu().transpose(0, 1) for k, v in pred.outputs.items()},
                "frames": pred.lengths.cpu(), "ln_fold": info["ln_fold"] == 1}
    finally:
        est.close()


_entry_truth, _entry_e_emu = {}, {}  # the entry stage's input is the audio: its truth and e_emu do not depend on the device


def stage_ratios(name, got, spec, state, tfi, audio, lengths, precision, picks, log_probabilities=True, entry_key=None,
                 per_output=False):
    """``got``: a ``device_pass``.  Per stage (``entry``, every ``layer<i>`` and ``heads``; post-LN: the last layer and the heads
    as ``tail``), from the device's input to it and over utterances ``picks``: the truth, e_emu of ``precision`` and the device's
    error; prints and returns {stage: (device error, e_emu)}.  ``entry_key``: runs that differ in nothing the entry stage sees
    (precision apart) share its truth and e_emu under this key.  ``per_output``: also prints the pair of every output of the
    heads (``heads/<output>``), for information."""
    picks = list(picks)
    frames = got["frames"][picks]
    offsets = synthetic.category_offsets(spec)
    each = {}
    layers, hidden = spec["layers"], got["hidden"]
    assert torch.equal(got["frames"], torch.tensor(S.frame_lengths(lengths.tolist(), spec)))
    found = {}

    def entry(ev):
        return SU.entry_stage(audio[picks], lengths[picks], frames, state, spec, ev)

    with torch.inference_mode():
        key = (entry_key, tuple(picks))
        truth = _entry_truth.get(key) if entry_key else None
        if truth is None:
            truth = _entry_truth[key] = entry(SU.Evaluation("truth"))
        e_emu = _entry_e_emu.get(key + (precision,)) if entry_key else None
        if e_emu is None:
            e_emu = _entry_e_emu[key + (precision,)] = SU.against(entry(SU.Evaluation(precision)), truth, frames)
        found["entry"] = (SU.against(hidden[0][picks], truth, frames), e_emu)
    for i in range(len(hidden) - 1):
        # (a pass that folded the LayerNorm kept the stream in planes between the products: the emulation does the same)
        found[f"layer{i}"] = SU.judged(lambda ev, i=i: SU.layer_stage(hidden[i][picks], frames, state, spec, ev, i, fold=got["ln_fold"]),
                                       hidden[i + 1][picks], frames, precision)
    which = 1 if log_probabilities else 0
    outputs = {k: v[picks] for k, v in got["outputs"].items()}
    suffix = "" if log_probabilities else " (logits)"
    taps = {i: hidden[i][picks] for i in SU.hidden_inputs(spec) if i < len(hidden)}
    if len(hidden) == layers + 1:
        found["heads" + suffix] = SU.judged(lambda ev: SU.heads_stage(taps, frames, state, spec, tfi, offsets, ev)[which], outputs,
                                            frames, precision, each if per_output else None)
    else:
        found["tail" + suffix] = SU.judged(
            lambda ev: SU.tail_stage(hidden[layers - 1][picks], taps, frames, state, spec, tfi, offsets, ev)[which], outputs, frames, precision)
    SU.report(name, precision, found)
    SU.report(name, precision, {f"heads{suffix}/{k}": v for k, v in each.items()})
    return found


def xlsr_model(time_layer=False):
    """XLS-R width, two layers, ``stage_util.tapped_spec``; ``time_layer``: the ``long`` head behind a time layer"""
    spec = SU.tapped_spec(S.xlsr_300m_encoder())
    if time_layer:
        next(c for c in spec["classes"] if c["name"] == "long")["time_layer"] = {"num_heads": 2, "positional_embeddings": True}
        S.validate(spec)
    return spec, synthetic.make_state_dict(spec, seed=0), synthetic.make_inventory(spec, 27, seed=0)


@pytest.fixture(scope="module")
def xlsr():
    return xlsr_model()


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_packed_layers(amd, xlsr, precision):
    """3 s + 2 s + 1.2 s (149 / 99 / 59 frames, 31 % padding): too small a grid for the window positional convolution, so the rows
    are packed behind the grouped-GEMM one (``pack_rows_kernel``), the layers run on 307 rows with attention by row offsets, and
    the rows are unpacked before the final LayerNorm.  Truth for all three."""
    spec, state, tfi = xlsr
    lengths = torch.tensor([48000, 32000, 19200])
    audio = synthetic.make_audio(3, 48000, seed=1234)[0]
    audio = audio * (torch.arange(48000).unsqueeze(0) < lengths.unsqueeze(1))
    got = device_pass(amd, spec, state, tfi, audio, lengths, precision, {"packed": 1, "ln_fold": 0, "rows": 149 + 99 + 59})
    found = stage_ratios("packed layers", got, spec, state, tfi, audio, lengths, precision, (0, 1, 2), entry_key="packed layers")
    assert_within_budget("packed layers", found)


PACKED_EARLY_ATTENTION = 0  # the form ``pass_info()`` reports for these 1283 packed rows: 256-query workgroups of 8 waves


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_packed_early(amd, xlsr, precision):
    """6 utterances of 2 .. 8 s, the batch ``test_packed_rows_give_the_bits_of_the_padded_layout`` packs early: the last conv
    layer's LayerNorm pass gathers the valid frames (the fused conv tail), feature projection, window positional convolution,
    layers, final LayerNorm, heads and log-softmax on packed rows, conv tiles per utterance.  Truth for the shortest, the longest
    and one more.  On fp16 planes also the raw logits (a second pass) and the same pass replayed from its recording."""
    spec, state, tfi = xlsr
    audio, lengths = _custom_ragged(6, 8.0, seed=77)
    picks = SU.shortest_longest_and(lengths, 1)
    pins = {"packed": 2, "ln_fold": 0, "attention": PACKED_EARLY_ATTENTION}
    got = device_pass(amd, spec, state, tfi, audio, lengths, precision, {**pins, "graph": 0})
    found = stage_ratios("packed early", got, spec, state, tfi, audio, lengths, precision, picks, entry_key="packed early")
    if precision == "f16x3":
        raw = device_pass(amd, spec, state, tfi, audio, lengths, precision, pins, log_probabilities=False)
        again = stage_ratios("packed early", raw, spec, state, tfi, audio, lengths, precision, picks, log_probabilities=False,
                             entry_key="packed early")
        found["heads (logits)"] = again["heads (logits)"]
    assert_within_budget("packed early", found)


def test_replay_on_packed_rows(amd, xlsr):
    """the packed-early batch a third time on one handle: replayed from the recording of the second pass"""
    spec, state, tfi = xlsr
    audio, lengths = _custom_ragged(6, 8.0, seed=77)
    got = device_pass(amd, spec, state, tfi, audio, lengths, "f16x3", {"packed": 2, "graph": 2}, passes=3)
    found = stage_ratios("packed early/replay", got, spec, state, tfi, audio, lengths, "f16x3", SU.shortest_longest_and(lengths, 1),
                         entry_key="packed early")
    assert_within_budget("packed early/replay", found)


def fold_batch():
    """16 utterances of 5 .. 10 s, 6631 of 7984 rows valid: the smallest of 8, 10, 12, 14, 16 such utterances whose packed rows take
    the LayerNorm fold (the route of every product of a layer has to allow it: 20 do, 24 do not)"""
    return synthetic.make_audio(16, 160000, seed=4000, ragged=True)


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_fold_on_packed_rows(amd, xlsr, precision):
    """``ln_fold == 1`` on rows packed early: producer tiles of the LayerNorm fold that end inside utterances, its consumers,
    256-row tiles chosen for the packed row count.  Truth for the shortest, the longest and two in between."""
    spec, state, tfi = xlsr
    audio, lengths = fold_batch()
    got = device_pass(amd, spec, state, tfi, audio, lengths, precision, {"ln_fold": 1, "packed": 2, "rows": 6631})
    found = stage_ratios("fold/packed", got, spec, state, tfi, audio, lengths, precision, SU.shortest_longest_and(lengths, 2),
                         entry_key="fold/packed")
    assert_within_budget("fold/packed", found)


def test_packed_with_a_time_layer_head(amd):
    """the packed-early batch with the ``long`` head behind a time layer, whose attention walks (utterance, frame) pairs: that
    blocks the early packing, so the window positional convolution runs padded, the layers on packed rows at XLS-R width, and
    the rows are unpacked before the final LayerNorm.  Truth for three utterances."""
    spec, state, tfi = xlsr_model(time_layer=True)
    audio, lengths = _custom_ragged(6, 8.0, seed=77)
    got = device_pass(amd, spec, state, tfi, audio, lengths, "f16x3", {"packed": 1, "ln_fold": 0})
    found = stage_ratios("packed/time layer", got, spec, state, tfi, audio, lengths, "f16x3", SU.shortest_longest_and(lengths, 1),
                         entry_key="packed early")
    assert_within_budget("packed/time layer", found)


def test_production_equal_lengths(amd, xlsr):
    """4 x 10 s of equal lengths, the fourth pass of one handle (the first one, which zeroes the Q / K / V planes, has a key of its
    own): the fused conv tail on the padded layout, replayed from the recording.  Truth for two utterances."""
    spec, state, tfi = xlsr
    audio, lengths = synthetic.make_audio(4, 160000, seed=55)
    got = device_pass(amd, spec, state, tfi, audio, lengths, "f16x3", {"packed": 0, "graph": 2, "rows": 4 * 499}, passes=4)
    assert_within_budget("production", stage_ratios("production", got, spec, state, tfi, audio, lengths, "f16x3", (0, 3)))


def test_post_ln(amd):
    """wav2vec2-base width, post-LN, masked, 64 channels per group of the positional convolution (``stage_util.post_ln_tapped_spec``),
    8 utterances of 1.5 .. 6 s: the group-norm extractor, and the post-LN encoder on rows packed early (it packs early or not at
    all).  hidden[2] is not kept: ``entry``, ``layer0`` and ``tail``.  Truth for three utterances."""
    spec = SU.post_ln_tapped_spec()
    state = synthetic.make_state_dict(spec, seed=23)
    tfi = synthetic.make_inventory(spec, 11, seed=23)
    audio, lengths = _custom_ragged(8, 6.0, seed=82)
    got = device_pass(amd, spec, state, tfi, audio, lengths, "f16x3", {"packed": 2, "ln_fold": 0})
    found = stage_ratios("post-LN/packed", got, spec, state, tfi, audio, lengths, "f16x3", SU.shortest_longest_and(lengths, 1))
    assert set(found) == {"entry", "layer0", "tail"}
    assert_within_budget("post-LN/packed", found)


@pytest.mark.parametrize("early", [False, True])
def test_fetch_of_packed_rows_is_the_padded_pass(amd, early):
    """The tiny model's packed and padded passes give the same bits, so ``debug_fetch("hidden", i)`` of a default pass must EQUAL
    that of a ``_no_pack`` pass on the valid frames.  ``early``: 96 utterances and 64 channels per group of the positional
    convolution, which packs from the feature projection on -- there the fetch itself unpacks by the pass's row offsets and hands
    out zeros beyond the lengths.  (Packed layers: the kept states are in the padded layout already, padding undefined.)"""
    enc = S.tiny_encoder(2)
    if early:
        enc["pos_groups"] = 2
    spec = SU.tapped_spec(enc, embedding_size=16, train_phonemes=9, n_features=5)
    state = synthetic.make_state_dict(spec, seed=5)
    tfi = synthetic.make_inventory(spec, 11, seed=5)
    n = 96 if early else 7
    audio, lengths = _custom_ragged(n, 1.5, seed=77)
    est = amd.Estimator(spec, state, "cuda:0", "f16x3")
    try:
        batch = amd.Batch(audio.cuda(), lengths, torch.zeros(n, dtype=torch.long))
        fetched = []
        for no_pack, packed in ((False, 2 if early else 1), (True, 0)):
            pred = est.predict(batch, tfi, _no_pack=no_pack)
            est.check_finite()
            assert est.pass_info()["packed"] == packed, est.pass_info()
            fetched.append([est.debug_fetch("hidden", i) for i in range(spec["layers"] + 1)])
        frames = pred.lengths.tolist()
        assert min(frames) < max(frames)
        for i, (default, padded) in enumerate(zip(*fetched)):
            for u, f in enumerate(frames):
                assert torch.equal(default[u, :f], padded[u, :f]), (i, u)
                if early:
                    assert not default[u, f:].any(), (i, u)
    finally:
        est.close()

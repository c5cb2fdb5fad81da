"""Residual jumps on the LayerNorm fold.

The fold keeps the residual stream of a large pre-LN batch only as 16-bit planes of ``u = (x - pivot) * s``, with the pivot and
the power of two ``s`` taken from the row's PREVIOUS statistics (``ln_plane_scale`` in amx_rowops.hip).  A sublayer that moves
one element by many of those standard deviations -- the "massive activations" trained wav2vec 2.0 / XLS-R checkpoints develop
suddenly in one early layer -- then writes a plane value far beyond what the row's statistics predicted, and an fp16 plane ends
at 65504.  The unfolded path (short batches) keeps the stream in fp32 and normalises before it writes planes, so it has no such
limit.  The outlier family of test_gpu_range.py cannot show this: its 1e3 sits in the feature-projection bias, in front of the
fold's first (exact) row statistics.

Here one channel of the bias of ``attention.out_proj`` or ``feed_forward.output_dense`` of layer 1 or 22 is raised by
``m x sigma`` (tests/jump_util.py: sigma the smallest valid-row sigma of the oracle's hidden state at that layer).  The same
checkpoint must meet the oracle on batches that fold -- equal lengths, a ragged batch on the padded layout (padded frames have
a smaller sigma than valid ones, and the same jump reaches them too), a ragged batch on packed rows -- and on one that does not
(2 x 3 s): a result must not depend on the batch it came in.  Beyond the stated headroom the fp16 modes must refuse loudly
(``FloatingPointError``), never answer wrongly.
"""
import pytest
import torch

from allophant_amd import synthetic
from tests.jump_util import jump_state, short_batch

pytestmark = pytest.mark.gpu
GATE = 1e-3
F16_BOUND = 6e-2  # test_gpu_timed_path.py: the single-plane fp16 mode's bound on log-probs
@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import estimator, lib

    assert lib.load() is not None
    return estimator


def _fold_batch(layout):
    """equal: 16 x 10 s.  padded: the same with a few utterances 9000 samples shorter -- too little padding to pack the rows, so
    the fold runs on the padded layout with its padded frames (as test_layer_norm_fold_in_every_mode's shaved batch).  packed:
    31 ragged utterances of up to 12.9 s, 15 478 frames on packed rows (test_random_large_geometries_against_oracle's seed 0)."""
    if layout == "packed":
        return synthetic.make_audio(31, 206191, seed=4000, ragged=True)
    audio, lengths = synthetic.make_audio(16, 160000, seed=778)
    if layout == "padded":
        lengths[1::3] -= 9000
        for i in range(16):
            audio[i, int(lengths[i]):] = 0
    return audio, lengths


def _against_oracle_alone(pred, audio, lengths, state, spec, tfi, picks):
    """worst |log-prob - oracle| over the valid frames of utterances `picks`, each run alone through the oracle"""
    from oracle import allophant_oracle as O

    offsets = synthetic.category_offsets(spec)
    worst = 0.0
    for i in picks:
        ref, ref_len = O.predict(audio[i:i + 1, :int(lengths[i])].contiguous(), lengths[i:i + 1], state, spec, tfi, offsets)
        t_i = int(ref_len[0])
        assert int(pred.lengths[i]) == t_i
        worst = max(worst, max((pred.outputs[k][:t_i, i].cpu() - ref[k][:t_i, 0]).abs().max().item() for k in ref))
    return worst


def _run_fold(amd, spec, state, precision, layout="equal", picks=(0, 9)):
    tfi = synthetic.make_inventory(spec, 27, seed=3)
    audio, lengths = _fold_batch(layout)
    n = audio.shape[0]
    est = amd.Estimator(spec, state, "cuda:0", precision)
    try:
        pred = est.predict(amd.Batch(audio.cuda(), lengths, torch.zeros(n, dtype=torch.long)), tfi)
        info = est.pass_info()
        assert info["ln_fold"] == 1 and (info["packed"] != 0) == (layout == "packed"), info
        est.check_finite()
        return _against_oracle_alone(pred, audio, lengths, state, spec, tfi, picks), info
    finally:
        est.close()


# (layer, sublayer, m): every m and both sublayers, both ends of the stack
FOLD_CASES = [
    (1, "out_proj", 1e3),
    (1, "ffn2", 1e4),
    (22, "out_proj", 1e4),
    (1, "out_proj", 3e4),
    (22, "ffn2", 3e4),
]


@pytest.mark.parametrize("layer,sublayer,multiple", FOLD_CASES)
def test_fold_survives_residual_jump(amd, layer, sublayer, multiple):
    """16 x 10 s (the fold), f16x3: a jump of m sigma in one channel stays finite and meets the oracle on utterances 0 and 9"""
    spec, state = jump_state(layer, sublayer, multiple)
    worst, _ = _run_fold(amd, spec, state, "f16x3")
    assert worst < GATE, (layer, sublayer, multiple, worst)


@pytest.mark.parametrize("layer,sublayer,multiple", [(1, "ffn2", 1e4), (1, "ffn2", 3e4), (0, "out_proj", 1e4)])
def test_fold_survives_residual_jump_on_padded_layout(amd, layer, sublayer, multiple):
    """the same on a ragged batch in the padded layout.  Its padded frames have 2 .. 7 times less sigma than the valid ones (layer 1:
    ~0.5 against ~1.07; hidden state 0: 0.15 .. 0.21), so under the valid rows' headroom the jump would overflow them first and
    reach the valid frames through the attention (a masked P = 0 times a non-finite V row is NaN).  Utterance 10 is a shortened
    one."""
    spec, state = jump_state(layer, sublayer, multiple)
    worst, info = _run_fold(amd, spec, state, "f16x3", layout="padded", picks=(0, 10))
    assert worst < GATE, (layer, sublayer, multiple, info, worst)


def test_fold_survives_residual_jump_on_packed_rows(amd):
    """the 3e4-sigma jump on a ragged batch whose rows are packed: the fold's producer tiles end inside utterances"""
    spec, state = jump_state(1, "ffn2", 3e4)
    audio, lengths = _fold_batch("packed")
    shortest = int(torch.argmin(lengths))
    worst, info = _run_fold(amd, spec, state, "f16x3", layout="packed", picks=(0, shortest))
    assert worst < GATE, (info, worst)


@pytest.mark.parametrize("layer,sublayer,multiple", [(1, "ffn2", 1e4), (22, "out_proj", 3e4)])
def test_unfolded_batch_meets_the_same_checkpoint(amd, layer, sublayer, multiple):
    """2 x 3 s: the same checkpoints without the fold (LayerNorm in fp32 before the planes) -- the outcome of a checkpoint does
    not depend on the size of its batch"""
    from oracle import allophant_oracle as O

    spec, state = jump_state(layer, sublayer, multiple)
    tfi = synthetic.make_inventory(spec, 27, seed=3)
    audio, lengths = short_batch()
    ref, ref_len = O.predict(audio, lengths, state, spec, tfi, synthetic.category_offsets(spec))
    est = amd.Estimator(spec, state, "cuda:0", "f16x3")
    try:
        pred = est.predict(amd.Batch(audio.cuda(), lengths, torch.zeros(2, dtype=torch.long)), tfi)
        assert est.pass_info()["ln_fold"] == 0
        est.check_finite()
    finally:
        est.close()
    assert torch.equal(pred.lengths.cpu(), ref_len)
    worst = 0.0
    for k in ref:
        got = pred.outputs[k].cpu()
        valid = (torch.arange(got.shape[0]).unsqueeze(1) < ref_len.unsqueeze(0)).unsqueeze(-1)
        worst = max(worst, torch.where(valid, (got - ref[k]).abs(), 0.0).max().item())
    assert worst < GATE, (layer, sublayer, multiple, worst)


@pytest.mark.parametrize("precision,tolerance", [("f16", F16_BOUND), ("bf16x3", GATE)])
def test_fold_residual_jump_in_other_modes(amd, precision, tolerance):
    """the 1e4-sigma jump on the fold in the single-plane fp16 mode (its stream stays fp32, its planes do not) and in bf16x3"""
    spec, state = jump_state(1, "ffn2", 1e4)
    worst, _ = _run_fold(amd, spec, state, precision)
    assert worst < tolerance, (precision, worst)


BEYOND = 1e5  # past the headroom of ln_plane_scale for every row: sigma * s <= 2 puts the jump at >= 1e5 / 1.07 in the plane


def test_jump_beyond_the_headroom_is_refused_not_silent(amd):
    """a jump the fp16 planes cannot hold: f16x3 on the fold raises FloatingPointError; bf16x3 (fp32 range) meets the oracle,
    once the oracle's own fp32 result has been checked against its fp64 evaluation"""
    from oracle import allophant_oracle as O

    spec, state = jump_state(1, "ffn2", BEYOND)
    tfi = synthetic.make_inventory(spec, 27, seed=3)
    audio, lengths = _fold_batch("equal")
    offsets = synthetic.category_offsets(spec)
    # the reference itself: fp32 against fp64 on utterance 0
    ref32, len32 = O.predict(audio[:1].contiguous(), lengths[:1], state, spec, tfi, offsets)
    with torch.inference_mode():
        state64 = {k: v.double() if v.is_floating_point() else v for k, v in state.items()}
        prev = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)
        try:
            ref64, len64 = O.predict(audio[:1].double(), lengths[:1], state64, spec, tfi, offsets)
        finally:
            torch.set_default_dtype(prev)
    assert torch.equal(len32, len64)
    own = max((ref32[k].double() - ref64[k]).abs().max().item() for k in ref32)
    assert own < 1e-4, own

    est = amd.Estimator(spec, state, "cuda:0", "f16x3")
    try:
        est.predict(amd.Batch(audio.cuda(), lengths, torch.zeros(16, dtype=torch.long)), tfi)
        assert est.pass_info()["ln_fold"] == 1
        with pytest.raises(FloatingPointError, match="bf16x3"):
            est.check_finite()
    finally:
        est.close()
    wide = amd.Estimator(spec, state, "cuda:0", "bf16x3")
    try:
        pred = wide.predict(amd.Batch(audio.cuda(), lengths, torch.zeros(16, dtype=torch.long)), tfi)
        assert wide.pass_info()["ln_fold"] == 1
        wide.check_finite()
        worst = _against_oracle_alone(pred, audio, lengths, state, spec, tfi, (0, 9))
    finally:
        wide.close()
    assert worst < GATE, worst

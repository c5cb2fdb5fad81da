"""The inputs and references of ``test_gpu_attention_sharp.py``, checked on the CPU (``attention_util.py``): the helpers do what
they say, every case reaches the deferred-maximum rescale of the attention kernels (``rescale_rows``: 0 rows with the suite's
usual weights, at least 2 % / 10 % of the rows at the case's two q factors), and the fp32 oracle stays within 1e-4 -- a tenth of the
1e-3 gate -- of its own fp64 evaluation on the hidden states of every case, so that it is a yardstick the gate can be applied to."""
import math

import pytest
import torch

import attention_util as A
from allophant_amd import spec as S, synthetic

CASE_FACTORS = [(case.name, factor) for case in A.CASES for factor in case.factors]


def _scores_to_qk(scores):
    """q, k ([1, 1, T, T]) whose ``rescale_rows`` scores are ``scores`` [T, T] (log2 units): k = identity, q = scores / scale."""
    t = scores.shape[0]
    scale = t ** -0.5 * A.LOG2E
    return (scores.double() / scale).view(1, 1, t, t), torch.eye(t, dtype=torch.float64).view(1, 1, t, t)


def test_rescale_rows_follows_the_rule():
    # 8 keys in tiles of 2; the rows are queries: [tile maxima] -> fires?
    rows = torch.tensor([
        [0, -1, 8, 3, 2, 1, 0, 0],       # second tile reaches +8: not MORE than 8 -> no
        [0, -1, 8.5, 3, 2, 1, 0, 0],     # +8.5 -> yes
        [0, 0, 5, 5, 10, 10, 15, 15],    # climbs by 5 per tile, the running value stays at the first tile's: 10 > 0 + 8 -> yes
        [0, 0, 5, 5, 8, 8, 3, 3],        # never more than 8 above the first tile -> no
        [20, 0, 5, 5, 27, 8, 3, 3],      # the first tile sets the level -> no
        [0, 0, 0, 0, -50, -50, -41, -41],  # with one run: no; with two halves the second starts afresh at -50: -41 > -50 + 8 -> yes
        [0, 0, 0, 0, 0, 0, 0, 100],      # -> yes (in the second half as well)
        [0, 0, 0, 0, -30, -30, -21, -21],  # the same
    ], dtype=torch.float64)
    q, k = _scores_to_qk(rows)
    fired, total, top = A.rescale_rows(q, k, [8], tile=2, halves=1)
    assert (fired, total) == (3, 8) and top == pytest.approx(100.0)
    assert A.rescale_rows(q, k, [8], tile=2, halves=2)[:2] == (4, 8)   # row 2: 15 against 10 is no rescale; rows 5 and 7 are
    # only valid keys and queries count: 5 frames -> tiles (0 1) (2 3) (4), rows 0 .. 4
    assert A.rescale_rows(q, k, [5], tile=2, halves=1)[:2] == (2, 5)
    # one tile per half: nothing can fire
    assert A.rescale_rows(q, k, [8], tile=4, halves=2)[0] == 0
    # a half without tiles (one tile in all) is skipped
    assert A.rescale_rows(q, k, [2], tile=2, halves=2)[:2] == (0, 2)
    # sunk_rows: only the first tile counts, and only below -128
    low = torch.zeros(8, 8, dtype=torch.float64)
    low[1] = -129.0
    low[2] = -128.0
    low[3, :2] = torch.tensor([-200.0, -100.0], dtype=torch.float64)
    low[4, :2] = -130.0
    low[5, 2:] = -500.0
    assert A.sunk_rows(*_scores_to_qk(low), [8], tile=2) == 2   # rows 1 and 4


def test_sharpen_and_shift_touch_what_they_should():
    spec = A.tiny_spec()
    state = synthetic.make_state_dict(spec, seed=3)
    same = A.sharpen(state, spec, 1)
    assert same.keys() == state.keys() and all(torch.equal(same[k], state[k]) for k in state)
    sharp = A.sharpen(state, spec, 16)
    changed = sorted(k for k in state if not torch.equal(sharp[k], state[k]))
    assert changed == sorted(f"{A.AM}encoder.layers.{i}.attention.q_proj.{leaf}" for i in range(2) for leaf in ("weight", "bias"))
    assert all(torch.equal(sharp[k], state[k] * 16) for k in changed)
    shifted = A.shift_keys(state, spec, 8.0)
    changed = sorted(k for k in state if not torch.equal(shifted[k], state[k]))
    assert changed == [f"{A.AM}encoder.layers.{i}.attention.k_proj.bias" for i in range(2)]
    assert all(((shifted[k] - state[k]).abs() - 8.0).abs().max() < 1e-5 for k in changed)
    with pytest.raises(AssertionError):
        A.sharpen(state, spec, 12)


def test_samples_for_frames():
    spec = A.tiny_spec()
    for frames in (1, 64, 65, 129, 960, 999):
        assert S.frame_lengths([A.samples_for_frames(spec, frames)], spec) == [frames]
    audio, lengths = A.CASE["long_key"].batch(A.wide_spec())
    assert S.frame_lengths(lengths.tolist(), spec) == [999, 993, 992, 991, 961, 960] and audio.shape == (6, int(lengths[0]))
    assert [f % 64 for f in (999, 993, 992, 991, 961, 960)] == [39, 33, 32, 31, 1, 0]


@pytest.mark.parametrize("name", ["key_split", "w8"])
def test_the_usual_weights_never_rescale(name):
    """Factor 1 -- the weights every other parity test uses -- at tiny and at XLS-R width (T = 399): no row ever exceeds its
    first-tile maximum by 2^8."""
    ref = A.reference(name, 1)
    print(f"{name} factor 1: {ref.fired} of {ref.rows} rows fire, max |score| {ref.top_score:.1f} log2 units")
    assert ref.fired == 0 and ref.rows > 1000


@pytest.mark.parametrize("name,factor", CASE_FACTORS)
def test_case_reaches_the_rescale_and_its_reference_is_sound(name, factor):
    case = A.CASE[name]
    ref = A.reference(name, factor)
    share = ref.fired / ref.rows
    print(f"{name} factor {factor}: {ref.fired} of {ref.rows} rows fire ({100 * share:.1f} %), max |score| {ref.top_score:.0f} log2 units, "
          f"fp32 oracle against fp64 {ref.oracle_noise:.1e}")
    assert share >= (0.02 if factor == case.factors[0] else 0.10)
    assert ref.oracle_noise < A.NOISE_BOUND
    assert all(torch.isfinite(v).all() for v in ref.logprobs.values())


@pytest.mark.parametrize("name", A.SHIFT_CASES)
def test_key_shift_leaves_the_function_alone(name):
    """``shift_keys``: the fp64 evaluation does not move (scores of ~1e3 at 1.1e-16 relative, a few hundred operations deep: far below
    1e-9), the raw scores do, and the fp32 oracle stays within its noise bound at SHIFT."""
    plain = A.reference(name, A.SHIFT_FACTOR)
    moved = A.reference(name, A.SHIFT_FACTOR, A.SHIFT)
    print(f"{name} shift {A.SHIFT}: max |score| {plain.top_score:.0f} -> {moved.top_score:.0f} log2 units, fp32 oracle against fp64 "
          f"{moved.oracle_noise:.1e}")
    for i in range(1, 3):
        assert A.valid_max(plain.hidden64[i], moved.hidden64[i], plain.frames) < 1e-9
    assert moved.top_score > 4 * plain.top_score
    # q . b is negative for half of the rows, and some of them start below -128 log2 units (one would do: its NaN reaches every
    # frame one layer on; the bar is that of the rescale at the lower factor)
    print(f"    rows whose first tile lies below -128: {plain.sunk} -> {moved.sunk} of {moved.rows}")
    assert plain.sunk == 0 and moved.sunk >= 0.02 * moved.rows
    assert (moved.fired, moved.rows) == (plain.fired, plain.rows)
    assert moved.oracle_noise < A.NOISE_BOUND


def test_key_shift_is_the_largest_the_oracle_supports():
    """SHIFT is the LARGEST power of two at which the fp32 oracle stays within 1e-4 of fp64 on both batches: at twice the value it
    no longer does on one of them (checked on the small batch, where it fails)."""
    spec = A.tiny_spec()
    case = A.CASE["key_split"]
    state = A.shift_keys(A.sharpen(synthetic.make_state_dict(spec, seed=case.seed), spec, A.SHIFT_FACTOR), spec, 2 * A.SHIFT)
    audio, lengths = case.batch(spec)
    from oracle import allophant_oracle as O

    hidden64, frames = A.fp64_hidden_states(audio, lengths, state, spec)
    worst = 0.0
    with torch.inference_mode():
        for i in range(len(lengths)):
            n = int(lengths[i])
            hidden32 = O.wav2vec2_hidden_states(audio[i:i + 1, :n].contiguous(), lengths[i:i + 1], state, spec)[0]
            for j in (1, 2):
                worst = max(worst, (hidden32[j][0].double() - hidden64[j][i, : int(frames[i])]).abs().max().item())
    print(f"shift {2 * A.SHIFT}: fp32 oracle against fp64 {worst:.1e}")
    assert worst >= A.NOISE_BOUND

"""Every route ``conv0_route`` (csrc/amx_conv0.hip) can return besides the matrix-pipe ones, against the CPU oracle.

``test_gpu_conv0.py`` covers the matrix pipe (C = 512, k = 10, small strides: fp64 table and covariance statistics) and the
golden vectors the scalar kernel at ``CPL = 1, KW = 10``.  The cases here are the smallest models that reach the other
instantiations: each is ``tiny_encoder(layers=1)`` with the first layer's width, kernel, stride and norm overridden, two
utterances (one ragged) just long enough for the last conv layer to yield ``FRAMES`` frames, and asserts the route it got
(``Estimator.conv0_route()``) before it compares the conv extractor's output with the oracle's ``conv_out``.

Gates: those of ``test_gpu_conv0.py`` -- 1e-3 in the split modes, 6e-2 in the single-plane modes; valid frames only in the masked
(layer-norm) family, every frame in the group-norm family, whose statistics run over the padded length.

``test_widths_without_a_kernel_are_refused``: a ``conv_dim`` of 64 or more that is not 64, 128, 256 or 512 has no instantiation of
the scalar kernel (a lane owns ``conv_dim / 64`` channels, built for 1, 2, 4 and 8); ``amx_create`` refuses it.
"""
import pytest
import torch

from allophant_amd import spec as S, synthetic

pytestmark = pytest.mark.gpu

FRAMES = 6  # of the last conv layer, for the longer utterance

# (conv_dim, first kernel, first stride, norm, precision) -> Estimator.conv0_route()
CASES = [
    ((48, 10, 5, "layer", "f16x3"), dict(apply="scalar", kw=10, cpl=1, stats="none")),    # idle lanes
    ((64, 10, 5, "layer", "f16x3"), dict(apply="scalar", kw=10, cpl=1, stats="none")),    # full wave
    ((128, 10, 5, "layer", "f16x3"), dict(apply="scalar", kw=10, cpl=2, stats="none")),   # vector prologue, packed pipe
    ((128, 10, 5, "layer", "bf16"), dict(apply="scalar", kw=10, cpl=2, stats="none")),
    ((256, 8, 4, "layer", "f16x3"), dict(apply="scalar", kw=16, cpl=4, stats="none")),    # padded taps, predicated prologue
    ((512, 8, 4, "layer", "f16x3"), dict(apply="scalar", kw=16, cpl=8, stats="none")),
    ((512, 10, 48, "layer", "f16x3"), dict(apply="scalar", kw=10, cpl=8, stats="none")),  # matrix-pipe LDS too large; whole-line stores
    ((512, 10, 8, "group", "f16x3"), dict(apply="scalar", kw=10, cpl=8, stats="recompute8")),
    ((128, 12, 6, "group", "f16x3"), dict(apply="scalar", kw=16, cpl=2, stats="recompute")),
]


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import estimator, lib

    assert lib.load() is not None
    return estimator


def _spec(conv_dim, kernel, stride, norm):
    enc = S.tiny_encoder(layers=1)
    enc["conv_dim"] = conv_dim
    enc["conv_kernel"][0], enc["conv_stride"][0] = kernel, stride
    if norm == "group":  # the family as wav2vec2-base has it
        enc.update(feat_extract_norm="group", conv_bias=False, stable_layer_norm=False, use_attention_mask=False)
    return S.baseline_spec(enc, 12)


def _samples_for(spec, frames):
    """The shortest utterance whose last conv layer has ``frames`` frames."""
    t = frames
    for k, s in zip(reversed(spec["conv_kernel"]), reversed(spec["conv_stride"])):
        t = (t - 1) * s + k
    return t


@pytest.mark.parametrize("shape,route", CASES, ids=["-".join(map(str, c[0])) for c in CASES])
def test_route_against_oracle(amd, shape, route):
    from oracle import allophant_oracle as O

    conv_dim, kernel, stride, norm, precision = shape
    spec = _spec(conv_dim, kernel, stride, norm)
    state = synthetic.make_state_dict(spec, seed=31)
    length = _samples_for(spec, FRAMES)
    audio, lengths = synthetic.make_audio(2, length, seed=41)
    lengths[1] = _samples_for(spec, FRAMES - 2) + 1
    audio[1, int(lengths[1]):] = 0.0
    _, ref_len, inter = O.predict(audio, lengths, state, spec, keep_intermediates=True)
    assert ref_len.tolist() == [FRAMES, FRAMES - 2]
    est = amd.Estimator(spec, state, "cuda:0", precision)
    got_route = est.conv0_route()
    pred = est.predict(amd.Batch(audio.cuda(), lengths, torch.zeros(2, dtype=torch.long)), None, True, _keep_hidden=True)
    est.check_finite()
    assert torch.equal(pred.lengths.cpu(), ref_len)
    conv = est.debug_fetch("conv")
    est.close()
    want = inter["conv_out"]
    if norm == "group":  # no attention mask in this family: every padded frame counts
        worst = float((conv - want).abs().max())
    else:
        worst = max(float((conv[i, :t] - want[i, :t]).abs().max()) for i, t in enumerate(ref_len.tolist()))
    print(f"[conv0 routes] {shape}: route {got_route}, conv extractor output max abs {worst:.3g}")
    assert worst < (1e-3 if precision.endswith("x3") else 6e-2), worst
    assert got_route == route


@pytest.mark.parametrize("conv_dim", [192, 1024])
def test_widths_without_a_kernel_are_refused(amd, conv_dim):
    spec = _spec(conv_dim, 10, 5, "layer")
    state = synthetic.make_state_dict(spec, seed=31)
    with pytest.raises(ValueError, match="conv_dim must be below 64 or one of 64, 128, 256, 512"):
        amd.Estimator(spec, state, "cuda:0", "f16x3")

"""On-device sinc resampling (amx_resample.hip) against the float64 restatement of the contract (tests/resample_util.py):
every source rate upstream lists down to 16 kHz plus 16 -> 8 and 16 -> 44.1 kHz within 2e-6 of each row's peak; exact
output lengths and zero tails at ragged lengths from 0 to 60 s; mixed-rate batches equal to single-row runs bit for bit;
padding that is never read; strided and batched views; graph capture; then Estimator.resample -> predict on a synthetic
model against the CPU oracle run on the restatement's audio."""
import numpy as np
import pytest
import torch

import resample_util as R

pytestmark = pytest.mark.gpu

TOL = 2e-6  # max |y - y_ref| / max |x_row|: fp32 taps and fp32 accumulation of ~15-40 products


@pytest.fixture(scope="module")
def rs():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import lib, resample

    assert lib.load() is not None
    return resample


def _audio(lengths, seed, pad_value=0.0):
    rng = np.random.default_rng(seed)
    L = max(lengths) if len(lengths) else 0
    x = np.full((len(lengths), L), pad_value, dtype=np.float32)
    for n, k in enumerate(lengths):
        x[n, :k] = (rng.standard_normal(k) * 0.3 + 0.2 * np.sin(np.arange(k) * 0.01 * (n + 1))).astype(np.float32)
    return x


def _batch(x, lengths):
    from allophant_amd.estimator import Batch

    return Batch(torch.from_numpy(x).cuda(), torch.tensor(lengths, dtype=torch.int64), torch.arange(len(lengths)))


def _check_rows(out, x, lengths, rates, new):
    y = out.audio_features.cpu().numpy()
    ref, ref_len = R.resample_batch(x, lengths, rates, new)
    assert out.lengths.tolist() == ref_len.tolist()
    assert y.shape == ref.shape
    for n, k in enumerate(ref_len):
        peak = max(float(np.abs(x[n, : lengths[n]]).max(initial=0.0)), 1e-30)
        err = float(np.abs(y[n, :k] - ref[n, :k]).max(initial=0.0))
        assert err <= TOL * peak, (n, rates[n], err, peak)
        assert not y[n, k:].any(), f"row {n}: nonzero tail"


@pytest.mark.parametrize("orig,new", [(8000, 16000), (11025, 16000), (22050, 16000), (24000, 16000), (32000, 16000),
                                      (44100, 16000), (48000, 16000), (16000, 16000), (16000, 8000), (16000, 44100)])
def test_source_rates_against_the_restatement(rs, orig, new):
    lengths = [orig * 2, orig + 123, orig // 3 + 7]
    x = _audio(lengths, seed=orig + new)
    out = rs.resample_batch(_batch(x, lengths), orig, new)
    assert out.audio_features.shape == (3, R.output_length(max(lengths), orig, new))
    assert torch.equal(out.language_ids, torch.arange(3))
    _check_rows(out, x, lengths, [orig] * 3, new)


@pytest.mark.parametrize("orig", [44100, 8000, 48000])
def test_ragged_lengths_and_zero_tails(rs, orig):
    """Lengths 0, 1, below W, an exact multiple of o, and 60 s, in one batch (torch.empty output: every tail is written)."""
    o, m, W, _, _ = R.bank(orig, 16000)
    lengths = [0, 1, W - 1, 7 * o, 60 * orig, 3 * o + 1]
    x = _audio(lengths, seed=orig)
    out = rs.resample_batch(_batch(x, lengths), orig)
    assert out.lengths.tolist() == [R.output_length(k, orig, 16000) for k in lengths]
    assert out.audio_features.shape[1] == max(out.lengths.tolist())
    _check_rows(out, x, lengths, [orig] * len(lengths), 16000)


def test_mixed_rates_equal_single_rows_bitwise(rs):
    rates = [8000, 44100, 48000, 16000, 44100, 22050]
    lengths = [8000 * 3, 44100 * 2 + 17, 48000 + 5, 16000 * 2, 999, 22050]
    x = _audio(lengths, seed=3)
    out = rs.resample_batch(_batch(x, lengths), rates)
    _check_rows(out, x, lengths, rates, 16000)
    y = out.audio_features
    for n, rate in enumerate(rates):
        single = rs.resample_batch(_batch(x[n: n + 1, : lengths[n]].copy(), [lengths[n]]), [rate])
        k = int(single.lengths[0])
        assert int(out.lengths[n]) == k
        assert torch.equal(y[n, :k], single.audio_features[0]), n
    # lengths held on the device give the same batch (one host synchronisation) and stay on the device
    dev = _batch(x, lengths)
    dev.lengths = dev.lengths.cuda()
    again = rs.resample_batch(dev, torch.tensor(rates))
    assert again.lengths.device.type == "cuda"
    assert torch.equal(again.audio_features, y) and torch.equal(again.lengths.cpu(), out.lengths)


@pytest.mark.parametrize("pad", [float("nan"), 1e30, -float("inf")])
def test_padding_is_never_read(rs, pad):
    rates = [44100, 48000, 8000]
    lengths = [44100, 30000, 7000]
    clean = rs.resample_batch(_batch(_audio(lengths, seed=9), lengths), rates)
    dirty = rs.resample_batch(_batch(_audio(lengths, seed=9, pad_value=pad), lengths), rates)
    assert torch.equal(clean.audio_features, dirty.audio_features)


def test_functional_shapes_and_strided_views(rs):
    """Leading dimensions are kept; a row-strided view is read in place, a time-strided one copied first: both right."""
    rng = np.random.default_rng(11)
    base = torch.from_numpy(rng.standard_normal((2, 3, 50000)).astype(np.float32)).cuda()
    y = rs.resample(base, 44100, 16000)
    assert y.shape == (2, 3, R.output_length(50000, 44100, 16000))
    flat = base.reshape(6, -1).cpu().numpy()
    for n in range(6):
        ref = R.resample_row(flat[n], 44100, 16000)
        assert np.abs(y.reshape(6, -1)[n].cpu().numpy() - ref).max() <= TOL * np.abs(flat[n]).max()
    wide = torch.from_numpy(rng.standard_normal((4, 40000)).astype(np.float32)).cuda()
    view = wide[:, 1000:31000]  # row stride 40000, unit time stride
    assert not view.is_contiguous()
    assert torch.equal(rs.resample(view, 48000, 16000), rs.resample(view.contiguous(), 48000, 16000))
    skip = wide[:, ::2]  # time stride 2
    assert torch.equal(rs.resample(skip, 22050, 16000), rs.resample(skip.contiguous(), 22050, 16000))
    assert rs.resample(base, 16000, 16000) is base
    with pytest.raises(TypeError):
        rs.resample(base.double(), 44100, 16000)
    batch = _batch(wide.cpu().numpy()[:, ::2].copy(), [20000, 20000, 15000, 20000])
    batch.audio_features = wide[:, ::2]
    ref = rs.resample_batch(_batch(wide.cpu().numpy()[:, ::2].copy(), [20000, 20000, 15000, 20000]), 22050)
    assert torch.equal(rs.resample_batch(batch, 22050).audio_features, ref.audio_features)


def test_module_matches_functional_and_replays_in_a_graph(rs):
    module = rs.Resample(44100, 16000).cuda()
    x = torch.randn(4, 44100 * 3, device="cuda")
    eager = module(x)
    assert torch.equal(eager, rs.resample(x, 44100, 16000))
    static_in = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        module(static_in)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = module(static_in)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, eager)
    static_in.copy_(x * 0.5)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, module(x * 0.5))


def test_estimator_resample_then_predict_against_the_oracle(rs):
    from allophant_amd import spec as S, synthetic
    from allophant_amd.estimator import Batch, Estimator
    from oracle import allophant_oracle as O

    spec = S.multitask_spec(S.tiny_encoder(2), ["syllabic", "long", "nasal"], embedding_size=16, train_phonemes=9,
                            n_features=5, n_values=3, allophone_layer=True)
    spec["shared_phones"] = 11
    state = synthetic.make_state_dict(spec, seed=1)
    tfi = synthetic.make_inventory(spec, 7, seed=1)
    est = Estimator(spec, state, "cuda:0", "f16x3")
    assert est.sample_rate == 16000
    rates = [44100, 48000, 44100]
    lengths = [44100 * 6000 // 16000, 48000 * 4100 // 16000, 44100 * 5003 // 16000]
    x = _audio(lengths, seed=21) * 0.3
    batch = Batch(torch.from_numpy(x), torch.tensor(lengths), torch.zeros(3, dtype=torch.long))
    at16 = est.resample(batch, rates)
    ref_audio, ref_len = R.resample_batch(x, lengths, rates, 16000)
    assert at16.lengths.tolist() == ref_len.tolist()
    pred = est.predict(at16, tfi)
    ref_audio = torch.from_numpy(ref_audio.astype(np.float32))
    ref_len = torch.from_numpy(ref_len)
    ref, ref_frames = O.predict(ref_audio, ref_len, state, spec, tfi, synthetic.category_offsets(spec))
    assert torch.equal(pred.lengths.cpu(), ref_frames)
    worst = 0.0
    for name, expected in ref.items():
        got = pred.outputs[name].cpu()
        valid = (torch.arange(got.shape[0]).unsqueeze(1) < ref_frames.unsqueeze(0)).unsqueeze(-1)
        worst = max(worst, ((got - expected).abs() * valid).max().item())
    assert worst < 1e-3, worst
    decoded = est.greedy_decode(pred)
    for name, expected in ref.items():
        hyps = O.greedy_ctc(expected.transpose(0, 1).contiguous(), ref_frames)
        for i, (tokens, timesteps, _score) in enumerate(hyps):
            got = decoded[name][i][0]
            assert torch.equal(got.tokens, tokens) and torch.equal(got.timesteps, timesteps), (name, i)
    est.close()

"""Long recordings on the device (amx_long.hip, Estimator.predict_long): the gather and the stitch against the NumPy restatement
of their contract (tests/longform_util.py), bit for bit, on both move widths, with sentinels around and inside every buffer and
with destination offsets past 2^31; predict_long against the window batches it stands for, against predict itself where every
recording fits a window, replayed against eager; the frame <-> sample mapping on the device's own conv features; and the
decoders and the search downstream of a stitched prediction.  Tiny models throughout."""
import ctypes as C

import numpy as np
import pytest
import torch

import longform_util as U

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
GUARD = 64
KERNELS, STRIDES = [10, 3, 3, 3, 3, 2, 2], [5, 2, 2, 2, 2, 2, 2]  # the tiny encoder's conv stack is wav2vec 2.0's
HOP, WINDOW, CONTEXT = 320, 4000, 2                               # 12 frames per window, 8 kept


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import estimator, lib

    assert lib.load() is not None
    return estimator


def _tiny_spec(kind="multitask", normalize=True):
    from allophant_amd import spec as S

    encoder = S.tiny_encoder(2)
    encoder["do_normalize"] = normalize
    attributes = ["syllabic", "long", "nasal"]
    if kind == "multitask":
        return S.multitask_spec(encoder, attributes, embedding_size=16, train_phonemes=9, n_features=5, n_values=3)
    spec = S.hierarchical_spec(encoder, attributes, embedding_size=16, train_phonemes=9, n_features=5, n_values=3)
    by_name = {c["name"]: c for c in spec["classes"]}
    by_name["long"].update(dependencies=["syllabic", S.OUTPUT], time_layer={"num_heads": 2, "positional_embeddings": True})
    S.validate(spec)
    return spec


@pytest.fixture(scope="module")
def model(amd):
    from allophant_amd import synthetic

    spec = _tiny_spec()
    est = amd.Estimator(spec, synthetic.make_state_dict(spec, seed=3), "cuda:0", "f16x3")
    yield spec, est, synthetic.make_inventory(spec, 7, seed=2)
    est.close()


def _guarded(count, shift=0, fill=SENTINEL):
    """(whole, part): a sentinel-filled device buffer and its `count` floats behind GUARD + shift floats."""
    whole = torch.full((count + 2 * GUARD + shift,), fill, dtype=torch.float32, device="cuda")
    return whole, whole[GUARD + shift: GUARD + shift + count]


def _guards_intact(whole, count, shift=0):
    host = whole.cpu()
    return bool((host[:GUARD + shift] == SENTINEL).all() and (host[GUARD + shift + count:] == SENTINEL).all())


def _bits(t):
    return t.view(torch.int32) if isinstance(t, torch.Tensor) else t.view(np.int32)


# -- gather --------------------------------------------------------------------------------------------------------------
def _gather_case(lengths, stride, shift, rng):
    """Host audio [R, stride] with a sentinel past every length, and its device copy `shift` floats off 16-byte alignment."""
    host = rng.standard_normal((len(lengths), stride)).astype(np.float32)
    for r, length in enumerate(lengths):
        host[r, length:] = 7e7
    whole = torch.empty(host.size + 4 + shift, dtype=torch.float32, device="cuda")
    device = whole[shift: shift + host.size].view(len(lengths), stride)
    device.copy_(torch.from_numpy(host))
    assert device.data_ptr() % 16 == 4 * shift
    return host, device


def _run_gather(host, device, lengths, windows, L_out, out_shift=0):
    from allophant_amd import longform

    n = len(windows)
    whole, part = _guarded(n * L_out, out_shift)
    status = torch.full((n + 2,), -77, dtype=torch.int32, device="cuda")
    longform.gather_windows(device, torch.tensor(lengths, dtype=torch.int64, device="cuda"),
                            torch.from_numpy(np.ascontiguousarray(windows)).cuda(), HOP, part.view(n, L_out), status[1:n + 1])
    want, want_status = U.gather(host, lengths, windows, HOP, L_out)
    got = part.view(n, L_out).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want)) and not (got == 7e7).any()
    assert status.tolist() == [-77] + want_status.tolist() + [-77] and _guards_intact(whole, n * L_out, out_shift)
    return want_status


@pytest.mark.parametrize("stride,audio_shift,out_shift,odd_out", [(13200, 0, 0, 0), (13200, 1, 0, 0), (13201, 0, 0, 0), (13200, 0, 0, 1),
                                                                  (13200, 0, 1, 0), (13203, 3, 2, 1)],
                         ids=["aligned", "base+1", "odd-stride", "odd-L_out", "out+1", "all"])
def test_gather_is_the_restatement_bit_for_bit(amd, stride, audio_shift, out_shift, odd_out):
    lengths = [13200, 3000, 250]  # 3.3 windows, a row below the window, nothing
    windows, frames = U.plan(lengths, WINDOW, CONTEXT, KERNELS, STRIDES)
    assert frames.tolist() == [41, 9, 0] and windows[:, U.RECORDING].tolist() == [0] * 5 + [1]
    assert windows[4].tolist() == [0, 4, 29, 34, 41, 3920]  # the right-aligned last window ends at the last sample
    host, device = _gather_case(lengths, stride, audio_shift, np.random.default_rng(stride + audio_shift))
    assert (_run_gather(host, device, lengths, windows, WINDOW + odd_out, out_shift) == 0).all()
    assert (_run_gather(host, device, lengths, windows[5:], 3000 + odd_out, out_shift) == 0).all()  # a slice maximum below the window
    assert (_run_gather(host, device, lengths, windows[3:5], 9000 + odd_out, out_shift) == 0).all()  # more than one item per row


def test_gather_malformed_rows_and_the_empty_call(amd):
    from allophant_amd import lib as L, longform

    lengths = [13200, 3000, 250]
    windows, _ = U.plan(lengths, WINDOW, CONTEXT, KERNELS, STRIDES)
    host, device = _gather_case(lengths, 13200, 0, np.random.default_rng(5))
    bad = windows[[0, 1, 2, 3, 4, 5, 0, 5]].copy()
    bad[0, U.RECORDING], bad[1, U.RECORDING], bad[2, U.START], bad[3, U.SAMPLES] = -1, 3, -1, -1
    bad[4, U.SAMPLES] = WINDOW + 4      # more than L_out
    bad[5, U.SAMPLES] = 3001            # one sample past the recording
    status = _run_gather(host, device, lengths, bad, WINDOW)
    assert status.tolist() == [-2] * 6 + [0, 0]
    bad[:, U.START] += 2 ** 30          # far outside: read nothing
    assert _run_gather(host, device, lengths, bad, WINDOW).tolist() == [-2] * 8
    empty = torch.empty(0, 6, dtype=torch.int32, device="cuda")
    longform.gather_windows(device, torch.tensor(lengths, device="cuda"), empty, HOP, torch.empty(0, WINDOW, device="cuda"),
                            torch.empty(0, dtype=torch.int32, device="cuda"))
    assert L.load().amx_long_gather(0, None, 0, None, 0, None, 0, HOP, 0, None, None, None) == L.AMX_OK
    torch.cuda.synchronize()


# -- stitch --------------------------------------------------------------------------------------------------------------
def _layout(classes, rows_src, rows_dst, misalign):
    """Offsets of consecutive blocks [rows, C] in src and dst; a block in `misalign` starts off a multiple of 4 floats in dst."""
    blocks, src_at, dst_at = [], 0, 0
    for b, c in enumerate(classes):
        if c % 4 == 0:
            src_at += -src_at % 4
            dst_at += -dst_at % 4 + (1 if b in misalign else 0)
        blocks.append((src_at, dst_at, c))
        src_at += rows_src * c
        dst_at += rows_dst * c
    return blocks, src_at, dst_at


def _run_stitch(windows, classes, src_T, R, dst_T, misalign=(), shift=0):
    from allophant_amd import longform

    n = len(windows)
    rng = np.random.default_rng(n + src_T + len(classes))
    blocks, src_size, dst_size = _layout(classes, src_T * n, dst_T * R, misalign)
    src_host = rng.standard_normal(src_size).astype(np.float32)
    whole, dst = _guarded(dst_size, shift)
    src = torch.from_numpy(src_host).cuda()
    status = torch.full((n + 2,), -77, dtype=torch.int32, device="cuda")
    longform.stitch_windows(src, src_T, torch.from_numpy(np.ascontiguousarray(windows)).cuda(), blocks, dst, R, dst_T, status[1:n + 1])
    want = np.full(dst_size, SENTINEL, dtype=np.float32)
    want_status = U.stitch([src_host[s: s + src_T * n * c].reshape(src_T, n, c) for s, _, c in blocks], windows,
                           [want[d: d + dst_T * R * c].reshape(dst_T, R, c) for _, d, c in blocks])
    got = dst.cpu().numpy()
    differ = np.flatnonzero(_bits(got) != _bits(want))
    assert differ.size == 0, (differ[:5].tolist(), got[differ[:5]], want[differ[:5]])
    assert status.tolist() == [-77] + want_status.tolist() + [-77] and _guards_intact(whole, dst_size, shift)
    return want_status, int((want != SENTINEL).sum())


CLASSES = [64, 1, 2, 3, 5, 65, 641, 64, 128]  # 64 twice: once moved 16 bytes per lane, once from a misaligned offset


def test_stitch_is_the_restatement_bit_for_bit(amd):
    lengths = [13200, 3000, 250]
    for context in (CONTEXT, 0):
        windows, frames = U.plan(lengths, WINDOW, context, KERNELS, STRIDES)
        # src_T = 14 is more than any window keeps; dst_T = 45 leaves frames beyond every recording
        status, written = _run_stitch(windows, CLASSES, 14, 3, 45, misalign=(7,))
        assert (status == 0).all() and written == int(frames.sum()) * sum(CLASSES)
    windows, _ = U.plan(lengths, WINDOW, CONTEXT, KERNELS, STRIDES)
    _run_stitch(windows, CLASSES, 14, 3, 45, misalign=(7,), shift=1)   # a misaligned destination: every block moves 4 bytes
    _run_stitch(windows[4:], [641, 8], 12, 3, 41)                       # one row
    _run_stitch(windows, list(range(1, 71)), 12, 3, 41)                 # 70 blocks: two launches
    _run_stitch(windows, [8, 3], 3000, 3, 45)                           # items that start past what a window keeps


def test_stitch_malformed_rows_write_nothing(amd):
    from allophant_amd import lib as L

    windows, _ = U.plan([13200, 3000, 250], WINDOW, CONTEXT, KERNELS, STRIDES)
    bad = windows[[0, 1, 2, 3, 4, 5, 1, 2, 3]].copy()
    bad[0, U.KEEP_LO] = bad[0, U.KEEP_HI] + 1                  # keep_lo > keep_hi
    bad[1, U.KEEP_LO] = bad[1, U.START] - 1                    # keep_lo < start
    bad[2, U.KEEP_HI] = bad[2, U.START] + 13                   # keep_hi > start + src_T
    bad[3, U.RECORDING] = 3
    bad[4, U.KEEP_HI] = 42                                     # keep_hi > dst_T
    bad[5, U.RECORDING] = -1
    bad[6, U.KEEP_HI] = bad[6, U.KEEP_LO]                      # an empty range is well-formed
    bad[7, [U.START, U.KEEP_LO, U.KEEP_HI]] = [-5, -3, 2]      # frames before the recording
    status, written = _run_stitch(bad, [5, 64], 12, 3, 41)
    assert status.tolist() == [-2] * 6 + [0, -2, 0] and written == 8 * 69
    handle = L.load()
    p = C.c_void_p(torch.empty(16, device="cuda").data_ptr())
    many = (L.AmxLongBlock * 65)(*[L.AmxLongBlock(0, 0, 1)] * 65)
    assert handle.amx_long_stitch(0, p, 1, 1, p, many, 65, p, 1, 1, p, None) == L.AMX_EINVAL


def test_stitch_with_destination_offsets_past_2_to_the_31(amd):
    """R = 64, C = 641, dst_T = 60 000: the last frames of recording 63 lie 2.46e9 floats into the block, the smallest shape at
    which a 32-bit offset goes wrong.  The 9.8 GB destination is allocated, not filled, but for a neighbourhood."""
    from allophant_amd import longform

    R, Cn, dst_T, src_T = 64, 641, 60000, 12
    dst = torch.empty(dst_T * R * Cn, dtype=torch.float32, device="cuda")
    view = dst.view(dst_T, R, Cn)
    assert ((dst_T - 1) * R + R - 1) * Cn > 2 ** 31
    view[dst_T - 40:] = SENTINEL
    windows = np.array([[63, 0, dst_T - 26, dst_T - 24, dst_T - 14, 4000], [63, 1, dst_T - 16, dst_T - 14, dst_T - 4, 4000]], dtype=np.int32)
    src_host = np.random.default_rng(63).standard_normal((src_T, 2, Cn)).astype(np.float32)
    status = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    longform.stitch_windows(torch.from_numpy(src_host).cuda().view(-1), src_T, torch.from_numpy(windows).cuda(), [(0, 0, Cn)], dst, R, dst_T,
                            status)
    want = np.full((40, R, Cn), SENTINEL, dtype=np.float32)
    shifted = windows.copy()
    shifted[:, [U.START, U.KEEP_LO, U.KEEP_HI]] -= dst_T - 40
    assert U.stitch([src_host], shifted, [want]).tolist() == [0, 0] and status.tolist() == [0, 0]
    got = view[dst_T - 40:].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want)) and (got[16:36, 63] != SENTINEL).all() and (got[:, :63] == SENTINEL).all()
    assert (got[36:] == SENTINEL).all() and (got[:16] == SENTINEL).all()
    del view, dst
    torch.cuda.empty_cache()


# -- predict_long ------------------------------------------------------------------------------------------------------------
def _recordings(lengths, seed):
    from allophant_amd import synthetic

    audio, _ = synthetic.make_audio(len(lengths), max(lengths), seed=seed)
    for r, length in enumerate(lengths):
        audio[r, length:] = 0
    return audio, torch.tensor(lengths, dtype=torch.int64)


def _expected(amd, est, tfi, audio, lengths, rows, log_probabilities):
    """What predict_long stands for, assembled on the host: the restated plan cut into slices of `rows` windows, each slice a batch
    built with torch slicing and predicted eagerly, its kept frames copied into zeros."""
    windows, frames = U.plan(lengths.tolist(), WINDOW, CONTEXT, KERNELS, STRIDES)
    T = U.frames(audio.shape[1], KERNELS, STRIDES)
    expected = None
    for lo in range(0, len(windows), rows):
        part = windows[lo: lo + rows]
        longest = int(part[:, U.SAMPLES].max())
        batch = torch.zeros(len(part), longest)
        for w, (r, _, a, _, _, samples) in enumerate(part.tolist()):
            batch[w, :samples] = audio[r, a * HOP: a * HOP + samples]
        piece = est.predict(amd.Batch(batch.cuda(), torch.from_numpy(part[:, U.SAMPLES].astype(np.int64)), torch.zeros(len(part), dtype=torch.long)),
                            tfi, log_probabilities, _no_graph=True)
        if expected is None:
            expected = {name: torch.zeros(T, len(lengths), o.shape[2]) for name, o in piece.outputs.items()}
        for name, o in piece.outputs.items():
            host = o.cpu()
            for w, (r, _, a, keep_lo, keep_hi, _) in enumerate(part.tolist()):
                expected[name][keep_lo:keep_hi, r] = host[keep_lo - a: keep_hi - a, w]
    return expected, frames


@pytest.mark.parametrize("kind,log_probabilities", [("multitask", True), ("multitask", False), ("time-layer", True)])
def test_predict_long_is_the_window_batches_it_stands_for(amd, model, kind, log_probabilities):
    from allophant_amd import synthetic

    if kind == "multitask":
        spec, est, tfi = model
    else:
        spec = _tiny_spec("time-layer")
        est, tfi = amd.Estimator(spec, synthetic.make_state_dict(spec, seed=6), "cuda:0", "f16x3"), synthetic.make_inventory(spec, 7, seed=2)
    try:
        audio, lengths = _recordings([13200, 4000, 250], seed=41)  # 3.3 windows, exactly one, none
        expected, frames = _expected(amd, est, tfi, audio, lengths, 4, log_probabilities)
        assert frames.tolist() == [41, 12, 0]  # six windows: a slice of four and one of two
        long = est.predict_long(amd.Batch(audio.cuda(), lengths, torch.zeros(3, dtype=torch.long)), tfi, log_probabilities,
                                window_seconds=WINDOW / 16000, context_seconds=0.05, batch_windows=4)
        assert long.lengths.tolist() == frames.tolist() and long._geometry == (3, 13200) and list(long.outputs) == list(expected)
        for name, want in expected.items():
            got = long.outputs[name].cpu()
            assert got.shape == want.shape and torch.equal(_bits(got), _bits(want)), name
            for r, count in enumerate(frames.tolist()):
                assert (got[count:, r] == 0).all() and (count == 0 or bool((got[:count, r] != 0).any()))
        est.synchronize()
    finally:
        if kind != "multitask":
            est.close()


def test_predict_long_of_short_recordings_is_predict(amd, model):
    spec, est, tfi = model
    audio, lengths = _recordings([3000, 2500, 1701, 399], seed=42)
    batch = amd.Batch(audio.cuda(), lengths, torch.zeros(4, dtype=torch.long))
    long = est.predict_long(batch, tfi, window_seconds=0.25, context_seconds=0.05, batch_windows=4)
    want = est.predict(amd.Batch(audio[:3].cuda(), lengths[:3], torch.zeros(3, dtype=torch.long)), tfi)
    assert long.lengths.tolist() == want.lengths.tolist() + [0]
    for name, o in want.outputs.items():
        assert torch.equal(_bits(long.outputs[name][:, :3]), _bits(o)) and (long.outputs[name][:, 3] == 0).all(), name
    # every recording at least a frame long: the flat buffer of predict itself
    long = est.predict_long(amd.Batch(audio[:3].cuda(), lengths[:3], torch.zeros(3, dtype=torch.long)), tfi, window_seconds=0.25,
                            context_seconds=0.05)
    assert torch.equal(_bits(long._flat), _bits(want._flat)) and long._geometry == want._geometry
    with pytest.raises(ValueError, match="keeps none"):
        est.predict_long(batch, tfi, window_seconds=0.25, context_seconds=0.125)
    with pytest.raises(ValueError, match="receptive field"):
        est.predict_long(batch, tfi, window_seconds=399 / 16000, context_seconds=0.0)
    nothing = amd.Batch(audio[3:, :399].cuda(), lengths[3:], torch.zeros(1, dtype=torch.long))
    with pytest.raises(ValueError, match="shorter than the receptive field"):
        est.predict_long(nothing, tfi)
    with pytest.raises(ValueError, match="shorter than the receptive field"):
        est.predict(nothing, tfi)


def test_replayed_slices_are_bitwise_the_eager_ones(amd, model):
    spec, est, tfi = model
    length = U.length_for(12 + 31 * 8, KERNELS, STRIDES)  # 32 full windows: 8 equal slices of 4
    audio, lengths = _recordings([length], seed=43)
    batch = amd.Batch(audio.cuda(), lengths, torch.zeros(1, dtype=torch.long))
    arguments = dict(window_seconds=0.25, context_seconds=0.05, batch_windows=4)
    eager = est.predict_long(batch, tfi, _no_graph=True, **arguments)
    torch.cuda.synchronize()
    _, before = est.graph_info()
    replayed = est.predict_long(batch, tfi, **arguments)
    torch.cuda.synchronize()
    assert est.graph_info()[1] - before >= 1
    assert eager.lengths.tolist() == [260] and torch.equal(_bits(replayed._flat), _bits(eager._flat))
    assert bool((eager.outputs["phoneme"] != 0).any(-1).all())  # every frame of the recording was written


def test_the_mapping_on_the_device(amd):
    """conv features of a gathered window batch against those of the whole 3-window recording at start + j: the project's 1e-3
    gate; one frame off they differ by O(1)."""
    from allophant_amd import longform, synthetic

    spec = _tiny_spec(normalize=False)
    est = amd.Estimator(spec, synthetic.make_state_dict(spec, seed=4), "cuda:0", "f16x3")
    try:
        tfi = synthetic.make_inventory(spec, 7, seed=2)
        audio, lengths = _recordings([9000], seed=8)
        plan = longform.plan_windows([9000], spec, WINDOW, CONTEXT)
        assert plan.windows[:, U.START].tolist() == [0, 8, 15] and plan.frames.tolist() == [27]
        gathered = torch.empty(3, WINDOW, device="cuda")
        status = torch.empty(3, dtype=torch.int32, device="cuda")
        longform.gather_windows(audio.cuda(), lengths.cuda(), torch.from_numpy(plan.windows).cuda(), plan.hop, gathered, status)
        assert status.tolist() == [0, 0, 0]
        est.predict(amd.Batch(gathered, torch.full((3,), WINDOW), torch.zeros(3, dtype=torch.long)), tfi, _keep_hidden=True)
        windows = est.debug_fetch("conv")
        est.predict(amd.Batch(audio.cuda(), lengths, torch.zeros(1, dtype=torch.long)), tfi, _keep_hidden=True)
        whole = est.debug_fetch("conv")[0]
        assert windows.shape[:2] == (3, 12) and whole.shape[0] == 27
        worst = max(float((windows[w] - whole[a: a + 12]).abs().max()) for w, a in enumerate([0, 8, 15]))
        shifted = max(float((windows[w, :11] - whole[a + 1: a + 12]).abs().max()) for w, a in enumerate([0, 8, 15]))
        print(f"window conv features vs the recording's: {worst:.3g} aligned, {shifted:.3g} one frame off")
        assert worst < 1e-3 and shifted > 0.5
    finally:
        est.close()


def test_decoders_and_search_take_long_predictions(amd, model):
    from oracle import allophant_oracle as O

    spec, est, tfi = model
    audio, lengths = _recordings([30000, 13200, 250], seed=44)
    long = est.predict_long(amd.Batch(audio.cuda(), lengths, torch.zeros(3, dtype=torch.long)), tfi, window_seconds=0.25,
                            context_seconds=0.05, batch_windows=4)
    frames = long.lengths.tolist()
    assert frames == [93, 41, 0]
    decoded = est.greedy_decode(long)
    for name, output in long.outputs.items():
        for n, (tokens, timesteps, _score) in enumerate(O.greedy_ctc(output.cpu().transpose(0, 1).contiguous(), long.lengths)):
            got = decoded[name][n][0]
            assert torch.equal(got.tokens, tokens) and torch.equal(got.timesteps, timesteps), (name, n)
    tokens = decoded["phoneme"][0][0].tokens.tolist()
    assert len(tokens) >= 4 and decoded["phoneme"][2][0].tokens.numel() == 0
    query = tokens[len(tokens) // 2 - 2: len(tokens) // 2 + 2]
    found = est.search(long, [query], "phoneme")
    hit = found[0][0]
    assert hit is not None and 0 <= hit.start < hit.end <= frames[0] and hit.score == 0.0
    assert found[2][0] is None
    beams = est.beam_decode(long, 4)
    assert len(beams["phoneme"]) == 3 and beams["phoneme"][0][0].tokens.numel() > 0

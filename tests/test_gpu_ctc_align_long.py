"""The long form of the on-device CTC forced alignment (amx_ctc_align_long.hip: frame blocks x state tiles with a recomputed
halo) against the restatement of the contract (tests/ctc_align_util.py), bit for bit in every output buffer, sentinels
included -- and, on rows both accept, against the one-workgroup kernel: state counts around the strips and the tile edges,
frame counts around the frame block, ragged batches, the steepest row (two states a frame across every tile edge), ties,
repeats at tile edges, -inf and NaN emissions, malformed rows, rows past the old limit through ``ctc_forced_align``, a poisoned
workspace, a side stream, the transposed view, graph capture and ``Estimator.align`` on a ``predict_long`` result."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_align_util as U

pytestmark = pytest.mark.gpu

SENTINEL_I, SENTINEL_F = -77, -12345.5
NAMES = ("paths", "frame_scores", "spans", "span_scores", "totals", "status")


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import estimator, lib

    assert lib.load() is not None
    return estimator


def _emissions(N, T, Cn, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(N, T, Cn, generator=g) * scale, dim=-1)


def _targets(rng, L, Cn, blank=0, repeat=0.2):
    """L targets among the non-blank classes; adjacent repeats with probability `repeat`."""
    out = []
    for _ in range(L):
        if out and rng.random() < repeat:
            out.append(out[-1])
        else:
            v = int(rng.integers(0, Cn - 1))
            v += v >= blank
            while out and v == out[-1]:
                v = int(rng.integers(0, Cn - 1))
                v += v >= blank
            out.append(v)
    return out


def _csr(rows):
    return np.concatenate(([0], np.cumsum([len(r) for r in rows]))).tolist(), [v for r in rows for v in r]


class _Call:
    """One amx_ctc_align_long_emissions (or, with long=False, amx_ctc_align_emissions) call on sentinel-filled buffers."""

    def __init__(self, em, lengths, offsets, ids, max_target, blank=0, long=True, poison=None):
        from allophant_amd import lib as L

        self.lib, self.handle = L, L.load()
        self.em = em  # [N, T, C] cuda view, unit class stride
        N, T, Cn = em.shape
        self.shape, self.blank, self.max_target = (N, T, Cn), blank, max_target
        self.entry = self.handle.amx_ctc_align_long_emissions if long else self.handle.amx_ctc_align_emissions
        sizer = self.handle.amx_ctc_align_long_workspace if long else self.handle.amx_ctc_align_workspace
        dev = em.device
        self.lengths = torch.tensor(lengths, dtype=torch.int32, device=dev)
        self.offsets = torch.tensor(offsets, dtype=torch.int32, device=dev)
        self.ids = torch.tensor(list(ids) + [0], dtype=torch.int32, device=dev)
        size = C.c_size_t()
        assert sizer(N, T, max_target, C.byref(size)) == L.AMX_OK
        self.size = size.value
        self.workspace = torch.empty(max(1, size.value), dtype=torch.uint8, device=dev)
        if poison is not None:
            self.workspace.fill_(poison)
        self.paths = torch.full((N, T), SENTINEL_I, dtype=torch.int32, device=dev)
        self.frame_scores = torch.full((N, T), SENTINEL_F, dtype=torch.float32, device=dev)
        self.spans = torch.full((N, max(1, max_target), 2), SENTINEL_I, dtype=torch.int32, device=dev)
        self.span_scores = torch.full((N, max(1, max_target)), SENTINEL_F, dtype=torch.float32, device=dev)
        self.totals = torch.full((N,), SENTINEL_F, dtype=torch.float32, device=dev)
        self.status = torch.full((N,), SENTINEL_I, dtype=torch.int32, device=dev)

    def reset(self):
        for t in (self.paths, self.spans, self.status):
            t.fill_(SENTINEL_I)
        for t in (self.frame_scores, self.span_scores, self.totals):
            t.fill_(SENTINEL_F)

    def run(self):
        N, T, Cn = self.shape
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        code = self.entry(
            self.em.device.index or 0, p(self.em), self.em.stride(0), self.em.stride(1), p(self.lengths), N, T, Cn, self.blank,
            p(self.offsets), p(self.ids), self.max_target, p(self.workspace), self.size, p(self.paths), p(self.frame_scores),
            p(self.spans), p(self.span_scores), p(self.totals), p(self.status),
            C.c_void_p(torch.cuda.current_stream(self.em.device).cuda_stream))
        assert code == self.lib.AMX_OK, self.handle.amx_last_error(None)
        return self

    def buffers(self):
        m = self.max_target
        return (self.paths.cpu().numpy(), self.frame_scores.cpu().numpy(), self.spans.cpu().numpy()[:, :m],
                self.span_scores.cpu().numpy()[:, :m], self.totals.cpu().numpy(), self.status.cpu().numpy())


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        differ = np.argwhere(_bits(g) != _bits(w))
        assert differ.size == 0, (what, name, differ[:5].tolist(), g[tuple(differ[0])], w[tuple(differ[0])])


def _check(em_host, lengths, rows=None, blank=0, max_target=None, em_device=None, offsets=None, ids=None, both=True):
    """The long form on `em_host` ([N, T, C] fp32 cpu tensor; `em_device` a cuda view of the same values) against the
    restatement, every buffer bit for bit; with `both`, the one-workgroup kernel too.  Returns the expected buffers."""
    if offsets is None:
        offsets, ids = _csr(rows)
    if max_target is None:
        max_target = max(len(r) for r in rows)
    em_device = em_host.cuda() if em_device is None else em_device
    want = U.expected_buffers(em_host.numpy(), lengths, offsets, ids, max_target, blank, SENTINEL_I, SENTINEL_F)
    _same(_Call(em_device, lengths, offsets, ids, max_target, blank).run().buffers(), want, "long")
    if both:
        _same(_Call(em_device, lengths, offsets, ids, max_target, blank, long=False).run().buffers(), want, "one workgroup")
    return want


def _edge_lengths():
    from allophant_amd import lib

    owned = lib.ALIGN_LONG_TILE_STATES  # S = 2L + 1 = owned - 1, owned + 1, owned + 3 and two tiles + 3
    return (0, 1, 31, 32, 33, owned // 2 - 1, owned // 2, owned // 2 + 1, owned + 1)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 129, 200, 1000, 1900])
def test_strip_and_tile_edges_on_both_paths(amd, T):
    """Every L of the list in one batch of T frames (a row with more targets than frames: -1); T around the frame block, and
    long enough for the rows at the tile edge (1000) and past two tiles (1900)."""
    lengths = _edge_lengths()
    rng = np.random.default_rng(T)
    rows = [_targets(rng, L, 11, repeat=0.05) for L in lengths]
    want = _check(_emissions(len(rows), T, 11, seed=T), [T] * len(rows), rows)
    assert want[5].tolist() == [0 if U.minimum_frames(r) <= T else -1 for r in rows]


def test_ragged_batch_on_both_paths(amd):
    """Frame lengths around the frame block inside one batch, a row of no frames (with and without targets), a row of no
    targets and a row one frame short of feasible."""
    rng = np.random.default_rng(3)
    rows = [_targets(rng, L, 8) for L in (40, 3, 0, 0, 60, 31, 100, 70, 20)]
    T = 200
    lengths = [T, 0, 0, 129, 128, 65, U.minimum_frames(rows[6]) - 1, U.minimum_frames(rows[7]), 1]
    want = _check(_emissions(len(rows), T, 8, seed=3), lengths, rows)
    assert want[5].tolist() == [0, -1, 0, 0, 0, 0, -1, 0, -1]


def _no_repeats(rng, L, Cn):
    return _targets(rng, L, Cn, repeat=0.0)


@pytest.mark.parametrize("slack", [0, 40])
def test_steepest_row(amd, slack):
    """T = L = 3000 without adjacent repeats: the only path advances two states every frame, so it crosses every tile edge at
    the speed the halo is sized for (tests/test_ctc_align_long_contract.py shows that a halo one strip short loses it); then
    the same targets with 40 frames of slack."""
    L, Cn = 3000, 9
    y = _no_repeats(np.random.default_rng(5), L, Cn)
    em = _emissions(1, L + slack, Cn, seed=5 + slack)
    want = _check(em, [L + slack], [y])
    assert want[5].tolist() == [0]
    if slack == 0:
        assert want[0][0].tolist() == y and want[2][0].tolist() == [[t, t + 1] for t in range(L)]


def test_tie_grid(amd):
    """Emissions drawn from {0, -0.25, -0.5, -1} (unnormalised): exact ties everywhere, L = 1000, T = 2500."""
    L, T = 1000, 2500
    g = torch.Generator().manual_seed(12)
    em = torch.tensor([0.0, -0.25, -0.5, -1.0])[torch.randint(0, 4, (2, T, 8), generator=g)]
    rng = np.random.default_rng(12)
    want = _check(em, [T, T - 1], [_targets(rng, L, 8, repeat=0.3), [1 + l % 2 for l in range(L)]])
    assert want[5].tolist() == [0, 0]


def test_repeats_at_tile_edges(amd):
    """Adjacent repeats placed so that the repeated target's state is the last of a tile, the first of the next, and the
    states around them: the skip is forbidden across the edge as anywhere else."""
    from allophant_amd import lib

    owned, L, Cn = lib.ALIGN_LONG_TILE_STATES, 1400, 6
    rng = np.random.default_rng(14)
    rows = []
    for shift in (0, 1):
        y = _no_repeats(rng, L, Cn)
        for edge in range(owned, 2 * L + 1, owned):
            for l in range((edge - 4) // 2 + shift, (edge + 4) // 2 + shift, 2):  # state 2l + 1 within the edge's +-4
                y[l] = y[l - 1]
        rows.append(y)
    T = max(U.minimum_frames(y) for y in rows) + 30
    want = _check(_emissions(2, T, Cn, seed=14), [T, T - 7], rows)
    assert want[5].tolist() == [0, 0]


def test_minus_infinity_emissions(amd):
    """A class that is -inf throughout and no target's; the same class among the targets (every path meets -inf: -1 and
    nothing but the status written); -inf scattered over a row."""
    T, Cn, L = 1200, 7, 500
    em = _emissions(3, T, Cn, seed=13)
    em[:2, :, 4] = -float("inf")
    g = torch.Generator().manual_seed(13)
    em[2][torch.rand(T, Cn, generator=g) < 0.1] = -float("inf")
    rng = np.random.default_rng(13)
    free = _no_repeats(rng, L, 4)  # classes 1 to 3
    blocked = list(free)
    blocked[L // 2] = 4
    want = _check(em, [T] * 3, [free, blocked, _targets(rng, 300, Cn)])
    assert want[5].tolist()[:2] == [0, -1]


def test_nan_emissions_keep_every_index_in_range(amd):
    """As the one-workgroup kernel's test: with lp[1][3] = NaN and targets 1 2 3 in six frames the path is state 5 throughout,
    targets 0 and 1 keep their `spans` untouched and get a span score of 0; then rows past a tile with NaN scattered through
    them: every output is in range or untouched."""
    em = _emissions(1, 6, 4, seed=21)
    em[0, 1, 3] = float("nan")
    paths, frame_scores, spans, span_scores, totals, status = _Call(em.cuda(), [6], [0, 3], [1, 2, 3], 3).run().buffers()
    assert status.tolist() == [0] and np.isnan(totals[0])
    assert paths[0].tolist() == [3] * 6
    assert spans[0].tolist() == [[SENTINEL_I, SENTINEL_I], [SENTINEL_I, SENTINEL_I], [0, 6]]
    assert span_scores[0, :2].tolist() == [0.0, 0.0] and np.isnan(span_scores[0, 2])

    N, T, Cn, L = 6, 1300, 6, 500
    em = _emissions(N, T, Cn, seed=22)
    g = torch.Generator().manual_seed(22)
    em[torch.rand(N, T, Cn, generator=g) < torch.tensor([0.0005, 0.003, 0.03, 0.1, 0.6, 1.0]).view(N, 1, 1)] = float("nan")
    rng = np.random.default_rng(22)
    rows = [_targets(rng, L, Cn) for _ in range(N)]
    lengths = [T, T, T - 1, T, 777, T]
    offsets, ids = _csr(rows)
    paths, frame_scores, spans, span_scores, totals, status = _Call(em.cuda(), lengths, offsets, ids, L).run().buffers()
    assert set(status.tolist()) <= {0, -1}
    for n in range(N):
        if status[n] != 0:
            assert (paths[n] == SENTINEL_I).all() and (spans[n] == SENTINEL_I).all()
            continue
        k = lengths[n]
        assert ((paths[n, :k] >= 0) & (paths[n, :k] < Cn)).all() and (paths[n, k:] == -1).all()
        assert (_bits(frame_scores[n, k:]) == _bits(np.float32(SENTINEL_F))).all()
        touched = spans[n] != SENTINEL_I
        assert ((spans[n][touched] >= 0) & (spans[n][touched] <= k)).all()
        assert (_bits(span_scores[n]) != _bits(np.float32(SENTINEL_F))).all()  # every target's sum was written


def test_malformed_rows_are_flagged_and_write_nothing(amd):
    """A target equal to the blank, a target >= C, a negative target, L > max_target and frame lengths outside [0, T]: -2 and
    sentinels everywhere, next to valid rows -- one of them past a tile -- that stay correct."""
    T, Cn, blank = 700, 6, 2
    em = _emissions(8, T, Cn, seed=15)
    rng = np.random.default_rng(15)
    good = _targets(rng, 500, Cn, blank)
    #       row: 0 ok  1 blank    2 >= C     3 ok  4 negative  5 too long                    6 length > T   7 length < 0
    rows = [good, [1, 2, 3], [1, 6, 3], [5], [0, -1], _targets(rng, 501, Cn, blank), [1], [4]]
    want = _check(em, [T, T, T, 7, T, T, T + 1, -1], rows, blank=blank, max_target=500)
    assert want[5].tolist() == [0, -2, -2, 0, -2, -2, -2, -2]
    ids = [1, 3, 4, 5, 1, 3, 4, 5]
    want = _check(em[:4], [T] * 4, blank=blank, max_target=5, offsets=[0, 4, 2, 6, 8], ids=ids)
    assert want[5].tolist() == [0, -2, 0, 0]
    want = _check(em[:3], [T] * 3, blank=blank, max_target=5, offsets=[-1, 2, 4, 3], ids=ids)
    assert want[5].tolist() == [-2, -2, -2]
    with pytest.raises(ValueError, match="row 1"):
        amd.ctc_forced_align(em[:3].cuda(), torch.tensor([T] * 3), [[1], [2], [3]], blank_index=blank, long=True)


def _same_alignment(got, want):
    if want.status != 0:
        assert got is None
        return
    assert np.array_equal(got.tokens.numpy(), want.paths) and np.array_equal(got.spans.numpy(), want.spans)
    assert np.array_equal(_bits(got.scores.numpy()), _bits(want.frame_scores))
    assert np.array_equal(_bits(got.span_scores.numpy()), _bits(want.span_scores))
    assert np.float32(got.total) == want.total


@pytest.fixture(scope="module")
def past_the_limit():
    """N = 2, L = (5000, 4500), T = 12000 with lengths (12000, 9001), C = 40, and the restatement's rows."""
    rng = np.random.default_rng(30)
    em = _emissions(2, 12000, 40, seed=30)
    lengths = [12000, 9001]
    rows = [_targets(rng, 5000, 40), _targets(rng, 4500, 40)]
    offsets, ids = _csr(rows)
    return em, lengths, rows, U.align_batch(em.numpy(), lengths, offsets, ids, 5000, fast=True)


def test_past_the_old_limit_through_ctc_forced_align(amd, past_the_limit):
    """The default ``long=None`` routes the call to the long form, since its largest row has more than 4095 targets;
    ``long=False`` keeps the refusal."""
    em, lengths, rows, want = past_the_limit
    got = amd.ctc_forced_align(em.cuda(), torch.tensor(lengths), rows)
    assert [w.status for w in want] == [0, 0]
    for g, w in zip(got, want):
        _same_alignment(g, w)
    with pytest.raises(ValueError, match="4095"):
        amd.ctc_forced_align(em.cuda(), torch.tensor(lengths), rows, long=False)


def test_poisoned_workspace_repeated_calls_and_a_side_stream(amd, past_the_limit):
    """The workspace filled with 0xFF bytes (NaN state rows, all-ones moves, bounds and flags) before the call: identical
    outputs; two calls in a row on one workspace and a call on a non-default stream too."""
    em, lengths, rows, _ = past_the_limit
    em = em[:, :3000].contiguous()
    lengths, rows = [3000, 2001], [rows[0][:1200], rows[1][:900]]
    offsets, ids = _csr(rows)
    want = U.expected_buffers(em.numpy(), lengths, offsets, ids, 1200, 0, SENTINEL_I, SENTINEL_F)
    device = em.cuda()
    call = _Call(device, lengths, offsets, ids, 1200, poison=0xFF).run()
    _same(call.buffers(), want, "poisoned")
    call.reset()
    _same(call.run().buffers(), want, "second call")
    clean = _Call(device, lengths, offsets, ids, 1200, poison=0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        clean.run()
    side.synchronize()
    _same(clean.buffers(), want, "side stream")


def test_a_workspace_that_cannot_be_allocated_names_its_bytes(amd):
    """Four rows of 2^20 frames against 262 143 targets ask for 4 x 2^37 bytes of moves, more than the device has."""
    from allophant_amd import alignment, lib

    size = C.c_size_t()
    assert lib.load().amx_ctc_align_long_workspace(4, 2 ** 20, 262143, C.byref(size)) == lib.AMX_OK and size.value > 2 ** 39
    with pytest.raises(RuntimeError, match=f"{size.value} bytes"):
        alignment.allocate(lib.load(), 4, 2 ** 20, 262143, torch.device("cuda:0"), long=True)


def test_transposed_view_is_read_in_place(amd):
    out = _emissions(1100, 3, 41, seed=11)  # [T, N, C]
    view = out.cuda().transpose(0, 1)
    assert not view.is_contiguous()
    rng = np.random.default_rng(11)
    _check(out.transpose(0, 1).contiguous(), [1100, 12, 1000], [_targets(rng, L, 41) for L in (450, 4, 420)], em_device=view)


def test_graph_capture(amd):
    """One amx_ctc_align_long_emissions call captured on a single stream and replayed twice equals the eager result bit for
    bit (the launches depend on the geometry alone)."""
    rng = np.random.default_rng(19)
    em = _emissions(3, 300, 9, seed=19).cuda()
    lengths = [300, 77, 0]
    rows = [_targets(rng, L, 9) for L in (140, 20, 0)]
    offsets, ids = _csr(rows)
    want = _Call(em, lengths, offsets, ids, 140).run().buffers()
    torch.cuda.synchronize()
    _same(want, U.expected_buffers(em.cpu().numpy(), lengths, offsets, ids, 140, 0, SENTINEL_I, SENTINEL_F), "eager")
    captured = _Call(em, lengths, offsets, ids, 140)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        captured.run()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.run()
    for _ in range(2):
        captured.reset()
        graph.replay()
        torch.cuda.synchronize()
        _same(captured.buffers(), want, "replay")


def test_through_the_estimator(amd):
    """A recording of about 5000 frames through predict_long, 4200 non-repeating targets on the phoneme output and 300 on an
    attribute output: Estimator.align (routed to amx_ctc_align_long by the phoneme row) equals the restatement on the fetched
    log-probabilities, and `segments` over ten boundaries tiles the targets' frames in order."""
    from allophant_amd import spec as S, synthetic
    from allophant_amd.alignment import segments

    spec = S.multitask_spec(S.tiny_encoder(2), ["syllabic", "long", "nasal"], embedding_size=16, train_phonemes=9, n_features=5,
                            n_values=3)
    audio, lengths = synthetic.make_audio(1, 5000 * 320, seed=8)
    est = amd.Estimator(spec, synthetic.make_state_dict(spec, seed=3), "cuda:0", "f16x3")
    try:
        pred = est.predict_long(amd.Batch(audio.cuda(), lengths, torch.zeros(1, dtype=torch.long)),
                                synthetic.make_inventory(spec, 7, seed=2))
        T = int(pred.lengths[0])
        assert 4900 <= T <= 5000
        rng = np.random.default_rng(33)
        targets = {"phoneme": [_no_repeats(rng, 4200, pred.outputs["phoneme"].shape[2])],
                   "long": [_targets(rng, 300, pred.outputs["long"].shape[2])]}
        result = est.align(pred, targets)
        assert sorted(result) == ["long", "phoneme"]
        for name, rows in targets.items():
            em = pred.outputs[name].cpu().transpose(0, 1).contiguous().numpy()
            want = U.align_row(em[0, :T], rows[0], fast=True)
            assert want.status == 0
            _same_alignment(result[name][0], want)
        with pytest.raises(ValueError, match="4095"):
            est.align(pred, targets, long=False)
        row = result["phoneme"][0]
        boundaries = [0] + sorted(rng.choice(np.arange(1, 4200), 9, replace=False).tolist()) + [4200]
        frames, means = segments(row, boundaries)
        assert frames.shape == (10, 2) and means.shape == (10,) and bool(torch.isfinite(means).all())
        assert int(frames[0, 0]) == int(row.spans[0, 0]) and int(frames[-1, 1]) == int(row.spans[-1, 1])
        assert bool((frames[:, 0] < frames[:, 1]).all()) and bool((frames[1:, 0] >= frames[:-1, 1]).all())
        for j in range(10):
            inside = row.spans[boundaries[j]:boundaries[j + 1]]
            assert int(inside.min()) == int(frames[j, 0]) and int(inside.max()) == int(frames[j, 1])
            want_mean = float(row.scores[int(frames[j, 0]):int(frames[j, 1])].to(torch.float64).mean())
            assert abs(float(means[j]) - want_mean) <= 1e-12 * abs(want_mean)
        seconds, _ = segments(row, boundaries, spec)
        assert seconds.dtype == torch.float64 and float(seconds[-1, 1]) == int(frames[-1, 1]) * 0.02
    finally:
        est.close()

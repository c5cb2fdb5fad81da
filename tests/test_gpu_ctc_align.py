"""On-device CTC forced alignment (amx_ctc_align.hip) against the restatement of the contract (tests/ctc_align_util.py),
bit for bit in every output buffer -- paths, frame_scores, spans, span_scores, totals (as fp32 bits) and status, including the
entries the contract leaves untouched (the buffers are pre-filled with sentinels): state counts around the 64-state strips
and at every strips-per-wave variant of the kernel, ragged lengths, 2 to 1025 classes and a non-zero blank, the feasibility
boundary, repeated targets, ties in every comparison, -inf emissions, the transposed view, malformed rows, NaN emissions and a long row;
then the greedy hypothesis aligned to its own argmax path, the Estimator façade, and graph capture."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_align_util as U
import edit_util as E

pytestmark = pytest.mark.gpu

SENTINEL_I, SENTINEL_F = -77, -12345.5


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
    """L targets among the non-blank classes; adjacent repeats with probability `repeat` (always, when there is one class)."""
    classes = [c for c in range(Cn) if c != blank]
    out = []
    for _ in range(L):
        if out and (len(classes) == 1 or rng.random() < repeat):
            out.append(out[-1])
        else:
            out.append(int(rng.choice([c for c in classes if not out or c != out[-1]])))
    return out


class _Call:
    """One amx_ctc_align_emissions call on sentinel-filled buffers; `run` may be repeated (graph capture)."""

    def __init__(self, em, lengths, offsets, ids, max_target, blank=0):
        from allophant_amd import lib as L

        self.lib, self.handle = L, L.load()
        self.em = em  # [N, T, C] cuda view, unit class stride
        N, T, Cn = em.shape
        self.shape, self.blank, self.max_target = (N, T, Cn), blank, max_target
        dev = em.device
        self.lengths = torch.tensor(lengths, dtype=torch.int32, device=dev)
        self.offsets = torch.tensor(offsets, dtype=torch.int32, device=dev)
        self.ids = torch.tensor(list(ids) + [0], dtype=torch.int32, device=dev)
        size = C.c_size_t()
        assert self.handle.amx_ctc_align_workspace(N, T, max_target, C.byref(size)) == L.AMX_OK
        self.size = size.value
        self.workspace = torch.empty(max(1, size.value), dtype=torch.uint8, device=dev)
        self.paths = torch.full((N, T), SENTINEL_I, dtype=torch.int32, device=dev)
        self.frame_scores = torch.full((N, T), SENTINEL_F, dtype=torch.float32, device=dev)
        self.spans = torch.full((N, max(1, max_target), 2), SENTINEL_I, dtype=torch.int32, device=dev)
        self.span_scores = torch.full((N, max(1, max_target)), SENTINEL_F, dtype=torch.float32, device=dev)
        self.totals = torch.full((N,), SENTINEL_F, dtype=torch.float32, device=dev)
        self.status = torch.full((N,), SENTINEL_I, dtype=torch.int32, device=dev)

    def run(self):
        N, T, Cn = self.shape
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        code = self.handle.amx_ctc_align_emissions(
            self.em.device.index or 0, p(self.em), self.em.stride(0), self.em.stride(1), p(self.lengths), N, T, Cn, self.blank,
            p(self.offsets), p(self.ids), self.max_target, p(self.workspace), self.size, p(self.paths), p(self.frame_scores),
            p(self.spans), p(self.span_scores), p(self.totals), p(self.status),
            C.c_void_p(torch.cuda.current_stream(self.em.device).cuda_stream))
        assert code == self.lib.AMX_OK, self.handle.amx_last_error(None)

    def buffers(self):
        m = self.max_target
        return (self.paths.cpu().numpy(), self.frame_scores.cpu().numpy(), self.spans.cpu().numpy()[:, :m],
                self.span_scores.cpu().numpy()[:, :m], self.totals.cpu().numpy(), self.status.cpu().numpy())


NAMES = ("paths", "frame_scores", "spans", "span_scores", "totals", "status")


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _check(em_host, lengths, rows, blank=0, max_target=None, em_device=None, offsets=None, ids=None):
    """Runs the kernel on `em_host` ([N, T, C] fp32 cpu tensor; `em_device` a cuda view of the same values) and compares
    every buffer with the restatement bit for bit.  Returns the status row."""
    if offsets is None:
        offsets = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).tolist()
        ids = [v for r in rows for v in r]
    if max_target is None:
        max_target = max(len(r) for r in rows)
    em_device = em_host.cuda() if em_device is None else em_device
    call = _Call(em_device, lengths, offsets, ids, max_target, blank)
    call.run()
    got = call.buffers()
    want = U.expected_buffers(em_host.numpy(), lengths, offsets, ids, max_target, blank, SENTINEL_I, SENTINEL_F)
    for name, g, w in zip(NAMES, got, want):
        differ = np.argwhere(_bits(g) != _bits(w))
        assert differ.size == 0, (name, differ[:5].tolist(), g[tuple(differ[0])], w[tuple(differ[0])])
    return want[5]


STRIP_LENGTHS = (0, 1, 31, 32, 63, 64, 100)


def test_strip_edges(amd):
    """S = 2L + 1 of 1, 3, 63, 65, 127, 129 and 201 states, each row with T = 2L + 5 frames, C = 37."""
    rng = np.random.default_rng(1)
    T = 2 * max(STRIP_LENGTHS) + 5
    em = _emissions(len(STRIP_LENGTHS), T, 37, seed=1)
    status = _check(em, [2 * L + 5 for L in STRIP_LENGTHS], [_targets(rng, L, 37) for L in STRIP_LENGTHS])
    assert (status == 0).all()


@pytest.mark.parametrize("Cn,blank", [(2, 0), (2, 1), (3, 2), (37, 5), (1025, 0), (1025, 1024)])
def test_ragged_lengths_class_counts_and_blank(amd, Cn, blank):
    T = 24
    rng = np.random.default_rng(Cn + blank)
    em = _emissions(4, T, Cn, seed=Cn + blank)
    status = _check(em, [T, 0, 1, T - 5], [_targets(rng, 6, Cn, blank), _targets(rng, 2, Cn, blank), _targets(rng, 1, Cn, blank),
                                            _targets(rng, 9, Cn, blank)], blank=blank)
    assert status.tolist() == [0, -1, 0, 0]


def test_rows_without_frames_or_targets(amd):
    em = _emissions(4, 9, 5, seed=4)
    status = _check(em, [0, 9, 0, 1], [[], [], [3], []], max_target=3)
    assert status.tolist() == [0, 0, -1, 0]
    status = _check(em, [0, 9, 1, 4], [[], [], [], []])  # max_target = 0
    assert status.tolist() == [0, 0, 0, 0]


def test_feasibility_boundary_and_repeated_targets(amd):
    """For every row T equal to targets + repeats (a single path) and one frame fewer (-1); half of the rows are runs of one
    repeated id."""
    rng = np.random.default_rng(9)
    rows, lengths = [], []
    for k, L in enumerate((1, 2, 5, 31, 32, 33, 40, 70)):
        y = [3] * L if k % 2 else _targets(rng, L, 6, repeat=0.4)
        rows += [y, y]
        lengths += [U.minimum_frames(y), U.minimum_frames(y) - 1]
    em = _emissions(len(rows), max(lengths), 6, seed=9)
    status = _check(em, lengths, rows)
    assert status.tolist() == [0, -1] * 8
    # runs of repeated ids with room to spare
    rows = [[2] * 40, [1] * 10 + [2] * 10 + [1] * 13, [4] * 64]
    status = _check(_emissions(3, 140, 5, seed=10), [140, 90, 127], rows)
    assert status.tolist() == [0, 0, 0]


def test_tie_grid(amd):
    """L = 40 (81 states, across the edge of the first strip) on emissions where comparisons tie: constant rows, on which
    every comparison between reachable states is an equality (alternating targets allow the skip, a run forbids it), and
    rows drawn from three values."""
    L, T = 40, 100
    g = torch.Generator().manual_seed(12)
    constant = torch.full((2, T, 4), -0.5)
    drawn = torch.tensor([-0.25, -0.5, -0.75])[torch.randint(0, 3, (4, T, 4), generator=g)]
    em = torch.cat([constant, drawn])
    rng = np.random.default_rng(12)
    rows = [[1 + l % 2 for l in range(L)], [2] * L] + [_targets(rng, L, 4, repeat=0.3) for _ in range(4)]
    status = _check(em, [T, T, T, T - 1, 2 * L, T], rows)
    assert (status == 0).all()


def test_minus_infinity_emissions(amd):
    """Scattered -inf (rows stay feasible or not, as the restatement says), and one row with -inf in every frame of the
    class of one of its targets (-1)."""
    T, Cn = 60, 7
    em = _emissions(5, T, Cn, seed=13)
    g = torch.Generator().manual_seed(13)
    em[:4][torch.rand(4, T, Cn, generator=g) < torch.tensor([0.05, 0.2, 0.4, 0.7]).view(4, 1, 1)] = -float("inf")
    rng = np.random.default_rng(13)
    rows = [_targets(rng, 12, Cn) for _ in range(4)] + [[1, 2, 3, 4, 5, 6]]
    em[4, :, 4] = -float("inf")
    status = _check(em, [T] * 5, rows)
    assert status[4] == -1 and 0 in status.tolist() and status.tolist().count(-1) >= 2
    # a blocked row next to the same targets unblocked
    em = _emissions(2, 20, 4, seed=14)
    em[0, :, 0] = -float("inf")  # no blank at all: the repeat cannot be separated
    status = _check(em, [20, 20], [[1, 1, 2], [1, 1, 2]])
    assert status.tolist() == [-1, 0]


def test_nan_emissions_keep_every_index_in_range(amd):
    """The result on NaN emissions is unspecified, but nothing out of range is read or written.  A NaN cell stays NaN with
    move 0, so the walk can sit on one state and never visit the lower targets: with lp[1][3] = NaN and targets 1 2 3 in six
    frames the path is state 5 throughout, targets 0 and 1 keep their `spans` untouched and get a span score of 0 (their
    bounds start as the empty span).  Then rows with NaN scattered through them: every output is in range or untouched."""
    em = _emissions(1, 6, 4, seed=21)
    em[0, 1, 3] = float("nan")
    call = _Call(em.cuda(), [6], [0, 3], [1, 2, 3], 3)
    call.run()
    paths, frame_scores, spans, span_scores, totals, status = call.buffers()
    assert status.tolist() == [0] and np.isnan(totals[0])
    assert paths[0].tolist() == [3] * 6
    assert spans[0].tolist() == [[SENTINEL_I, SENTINEL_I], [SENTINEL_I, SENTINEL_I], [0, 6]]
    assert span_scores[0, :2].tolist() == [0.0, 0.0] and np.isnan(span_scores[0, 2])

    N, T, Cn, L = 8, 150, 6, 50
    em = _emissions(N, T, Cn, seed=22)
    g = torch.Generator().manual_seed(22)
    em[torch.rand(N, T, Cn, generator=g) < torch.tensor([0.001, 0.003, 0.01, 0.03, 0.1, 0.3, 0.6, 1.0]).view(N, 1, 1)] = float("nan")
    rng = np.random.default_rng(22)
    rows = [_targets(rng, L, Cn) for _ in range(N)]
    lengths = [T, T, T - 1, T, 77, T, T, T]
    offsets = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).tolist()
    call = _Call(em.cuda(), lengths, offsets, [v for r in rows for v in r], L)
    call.run()
    paths, frame_scores, spans, span_scores, totals, status = call.buffers()
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


def test_transposed_view_is_read_in_place(amd):
    out = _emissions(30, 5, 41, seed=11)  # [T, N, C]
    view = out.cuda().transpose(0, 1)
    assert not view.is_contiguous()
    rng = np.random.default_rng(11)
    lengths = [30, 12, 0, 29, 1]
    rows = [_targets(rng, L, 41) for L in (9, 4, 0, 11, 1)]
    _check(out.transpose(0, 1).contiguous(), lengths, rows, em_device=view)
    # and through the Python entry point
    got = amd.ctc_forced_align(view, torch.tensor(lengths), rows)
    want = U.align_batch(out.transpose(0, 1).contiguous().numpy(), lengths,
                         np.concatenate(([0], np.cumsum([len(r) for r in rows]))), [v for r in rows for v in r], 11)
    for g, w in zip(got, want):
        _same_alignment(g, w)


def _same_alignment(got, want):
    if want.status != 0:
        assert got is None
        return
    assert np.array_equal(got.tokens.numpy(), want.paths) and np.array_equal(got.spans.numpy(), want.spans)
    assert np.array_equal(_bits(got.scores.numpy()), _bits(want.frame_scores))
    assert np.array_equal(_bits(got.span_scores.numpy()), _bits(want.span_scores))
    assert np.float32(got.total) == want.total


def test_malformed_rows_are_flagged_and_write_nothing(amd):
    """A target equal to the blank, a target >= C, a negative target, decreasing offsets, offsets past the id count, L >
    max_target and frame lengths outside [0, T]: -2 and sentinels everywhere, next to valid rows that stay correct."""
    T, Cn, blank = 20, 6, 2
    em = _emissions(9, T, Cn, seed=15)
    #       row: 0 ok     1 blank    2 >= C     3 ok  4 negative  5 too long        6 ok  7 length > T   8 length < 0
    rows = [[1, 3, 4], [1, 2, 3], [1, 6, 3], [5], [0, -1], [1, 3, 1, 3, 1], [3, 3], [1], [4]]
    status = _check(em, [T, T, T, 7, T, T, T, T + 1, -1], rows, blank=blank, max_target=4)
    assert status.tolist() == [0, -2, -2, 0, -2, -2, 0, -2, -2]
    # offsets: row 1 ends before it begins, row 2 starts below its predecessor's end (allowed: it is ascending itself),
    # row 3 reaches past offsets[N]
    ids = [1, 3, 4, 5, 1, 3, 4, 5]
    status = _check(em[:4], [T] * 4, None, blank=blank, max_target=4, offsets=[0, 5, 3, 9, 8], ids=ids)
    assert status.tolist() == [-2, -2, -2, -2]  # row 0 holds 5 > max_target ids
    status = _check(em[:4], [T] * 4, None, blank=blank, max_target=5, offsets=[0, 4, 2, 6, 8], ids=ids)
    assert status.tolist() == [0, -2, 0, 0]
    status = _check(em[:3], [T] * 3, None, blank=blank, max_target=5, offsets=[-1, 2, 4, 3], ids=ids)
    assert status.tolist() == [-2, -2, -2]
    with pytest.raises(ValueError, match="row 1"):
        amd.ctc_forced_align(em[:3].cuda(), torch.tensor([T] * 3), [[1], [2], [3]], blank_index=blank)


def test_long_row(amd):
    """T = 3000 with 600 targets (19 strips: every wave of the block, two strips each) next to a 17-frame row."""
    rng = np.random.default_rng(16)
    em = _emissions(2, 3000, 37, seed=16, scale=3.0)
    status = _check(em, [3000, 17], [_targets(rng, 600, 37), _targets(rng, 5, 37)])
    assert status.tolist() == [0, 0]


@pytest.mark.parametrize("L", [1023, 1024, 2047, 2048, 4095])
def test_strips_per_wave_variants(amd, L):
    """The kernel is instantiated for 1, 2, 4 and 8 strips per wave: max_target around 1024 and 2048 switches between them,
    and 4095 targets (8191 states) fill the LDS rows.  A short row shares each launch."""
    rng = np.random.default_rng(L)
    T = L + 40  # (about L / 500 adjacent repeats each need one more frame)
    em = _emissions(2, T, 5, seed=L)
    status = _check(em, [T, 40], [_targets(rng, L, 5, repeat=0.002), _targets(rng, 7, 5)])
    assert status.tolist() == [0, 0]


def test_aligning_the_greedy_hypothesis_gives_the_argmax_path(amd):
    """Independent of the restatement: the best path for the greedy hypothesis is the per-frame argmax, and its total the
    greedy score.  No row is skipped (continuous random inputs have a unique argmax in every frame)."""
    N, T, Cn = 6, 80, 13
    em = _emissions(N, T, Cn, seed=17).cuda()
    lengths = torch.tensor([T, T - 1, 33, 64, 65, 1])
    greedy = amd.greedy_ctc_decode(em, lengths)
    targets = [h[0].tokens.tolist() for h in greedy]
    got = amd.ctc_forced_align(em, lengths, targets)
    skipped = 0
    host = em.cpu()
    for n in range(N):
        k = int(lengths[n])
        top = host[n, :k].topk(2, dim=-1).values
        if bool((top[:, 0] == top[:, 1]).any()):
            skipped += 1
            continue
        assert got[n] is not None
        assert got[n].tokens.tolist() == host[n, :k].argmax(-1).tolist(), n
        assert abs(got[n].total - greedy[n][0].score) <= 1e-4 * abs(greedy[n][0].score), (n, got[n].total, greedy[n][0].score)
    assert skipped == 0
    # padded targets with lengths give the same rows
    width = max(len(t) for t in targets)
    padded = torch.tensor([t + [0] * (width - len(t)) for t in targets])
    again = amd.ctc_forced_align(em, lengths, (padded, torch.tensor([len(t) for t in targets])))
    for a, b in zip(got, again):
        assert a.tokens.tolist() == b.tokens.tolist() and a.total == b.total and a.spans.tolist() == b.spans.tolist()


def _table():
    from allophant_amd.phonetic import AttributeTable

    return AttributeTable(E.synthetic_table_text(), ["syllabic", "long", "nasal", "phoneme"])


def _assert_facade(result, pred, targets, names):
    assert list(result) == names
    lengths = [int(v) for v in pred.lengths]
    for name in names:
        em = pred.outputs[name].cpu().transpose(0, 1).contiguous().numpy()
        for n, row in enumerate(targets[name]):
            _same_alignment(result[name][n], U.align_row(em[n, :lengths[n]], row, fast=True))


@pytest.mark.parametrize("kind", ["multitask", "hierarchical"])
def test_through_the_estimator(amd, kind):
    """predict -> label_targets -> Estimator.align equals the restatement on predictions.outputs copied to the host, for
    every output, with a composition inventory and without one; align_device on earlier predictions after a later predict
    under another inventory still aligns under the first."""
    from allophant_amd import spec as S, synthetic
    from allophant_amd.alignment import label_targets
    from allophant_amd.evaluation import EvaluationMaps

    table = _table()
    attributes = ["syllabic", "long", "nasal"]
    make = S.multitask_spec if kind == "multitask" else S.hierarchical_spec
    spec = make(S.tiny_encoder(2), attributes, embedding_size=16, train_phonemes=9, n_features=5, n_values=3)
    names = S.output_names(spec)
    assert sorted(names) == sorted(attributes + ["phoneme"])
    N = 5
    audio, lengths = synthetic.make_audio(N, 12000, seed=7, ragged=True)
    inventory = ["a", "ts", "t͡ʃ", "é", "m", "aː", "i"]
    training = table.full_phonemes[:9]
    rng = np.random.default_rng(31)

    def labels_from(symbols):
        rows = [[symbols[i] for i in rng.integers(0, len(symbols), rng.integers(1, 9))] for _ in range(N)]
        rows[2] = []
        return rows

    est = amd.Estimator(spec, synthetic.make_state_dict(spec, seed=3), "cuda:0", "f16x3")
    try:
        batch = amd.Batch(audio.cuda(), lengths, torch.zeros(N, dtype=torch.long))
        first = est.predict(batch, synthetic.make_inventory(spec, len(inventory), seed=2))
        assert first.outputs["phoneme"].shape[2] == len(inventory) + 1
        first_labels = labels_from(inventory)
        first_targets = label_targets(EvaluationMaps(table, names, inventory, ["lg0"]), first_labels, ["lg0"] * N)
        result = est.align(first, first_targets)
        _assert_facade(result, first, first_targets, names)
        assert any(row is not None for row in result["phoneme"])
        seconds = next(row for row in result["phoneme"] if row is not None and len(row.spans)).seconds(spec)
        assert seconds.shape[1] == 2 and float(seconds[0, 1]) > float(seconds[0, 0]) >= 0.0

        est.set_training_inventory(synthetic.make_inventory(spec, len(training), seed=4))
        second = est.predict(batch)  # no target_feature_indices: the training inventory, another phoneme width
        assert second.outputs["phoneme"].shape[2] == len(training) + 1
        second_targets = label_targets(EvaluationMaps(table, names, training, ["lg0"]), labels_from(training))
        _assert_facade(est.align(second, second_targets), second, second_targets, names)

        aligned = est.align_device(first, {"phoneme": first_targets["phoneme"]})  # after the later predict
        assert aligned.paths.is_cuda and aligned.present == ["phoneme"] and aligned.names == names
        _assert_facade(aligned.alignments(), first, first_targets, ["phoneme"])
        absent = names.index("long")
        assert aligned.status[absent].cpu().tolist() == [0] * N  # aligned against nothing: all blank
        assert (aligned.paths[absent].cpu() <= 0).all()
        with pytest.raises(ValueError):
            est.align(first, {"nope": [[]] * N})
    finally:
        est.close()


def test_graph_capture(amd):
    """One amx_ctc_align_emissions call captured on a single stream and replayed twice equals the eager result bit for bit."""
    rng = np.random.default_rng(19)
    em = _emissions(3, 150, 9, seed=19).cuda()
    lengths = [150, 77, 0]
    rows = [_targets(rng, L, 9) for L in (70, 20, 0)]
    offsets = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).tolist()
    ids = [v for r in rows for v in r]
    eager = _Call(em, lengths, offsets, ids, 70)
    eager.run()
    torch.cuda.synchronize()
    want = eager.buffers()
    captured = _Call(em, lengths, offsets, ids, 70)
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
        for t in (captured.paths, captured.spans, captured.status):
            t.fill_(SENTINEL_I)
        for t in (captured.frame_scores, captured.span_scores, captured.totals):
            t.fill_(SENTINEL_F)
        graph.replay()
        torch.cuda.synchronize()
        for name, g, w in zip(NAMES, captured.buffers(), want):
            assert np.array_equal(_bits(g), _bits(w)), name

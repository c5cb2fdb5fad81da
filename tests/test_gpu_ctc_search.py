"""On-device CTC search (amx_ctc_search.hip) against the restatement of the contract (tests/ctc_search_util.py), bit for bit
in every output buffer -- best_scores and end_scores (as fp32 bits), best_spans, end_starts and status, including the entries
the contract leaves untouched and guard elements on both sides of every buffer (all pre-filled with sentinels): query lengths
around the 64-state strips and every strip variant in one launch, 2 to 1025 classes and a non-zero blank, frame lengths around
the feasibility boundary and the 64-frame blocks, ties in every comparison, -inf and NaN emissions, the transposed view,
malformed rows, NULL curves, repeatability and graph capture, a long row; then the Python façade and, independent of the
restatement, Estimator.search for slices of each utterance's own greedy tokens."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_search_util as U

pytestmark = pytest.mark.gpu

SENTINEL_I, SENTINEL_F = -77, -12345.5
GUARD = 64  # elements on both sides of every output buffer


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


def _query(rng, L, Cn, blank=0, repeat=0.2):
    """L ids among the non-blank classes; adjacent repeats with probability `repeat` (always, when there is one class)."""
    classes = [c for c in range(Cn) if c != blank]
    out = []
    for _ in range(L):
        if out and (len(classes) == 1 or rng.random() < repeat):
            out.append(out[-1])
        else:
            out.append(int(rng.choice([c for c in classes if not out or c != out[-1]])))
    return out


class _Guarded:
    """A sentinel-filled device buffer with GUARD sentinel elements on both sides of the part the kernel is given."""

    def __init__(self, shape, dtype, device):
        self.shape, self.count = shape, int(np.prod(shape))
        self.sentinel = SENTINEL_F if dtype == torch.float32 else SENTINEL_I
        self.whole = torch.full((self.count + 2 * GUARD,), self.sentinel, dtype=dtype, device=device)

    def pointer(self):
        return C.c_void_p(self.whole.data_ptr() + 4 * GUARD)

    def refill(self):
        self.whole.fill_(self.sentinel)

    def host(self):
        whole = self.whole.cpu().numpy()
        guards = np.concatenate((whole[:GUARD], whole[GUARD + self.count:]))
        assert (guards == guards.dtype.type(self.sentinel)).all(), "a guard element was overwritten"
        return whole[GUARD:GUARD + self.count].reshape(self.shape)


NAMES = ("best_scores", "best_spans", "status", "end_scores", "end_starts")


class _Call:
    """One amx_ctc_search_emissions call on guarded, sentinel-filled buffers; `run` may be repeated (graph capture)."""

    def __init__(self, em, lengths, offsets, ids, max_query, blank=0, curves=True):
        from allophant_amd import lib as L

        self.lib, self.handle = L, L.load()
        self.em = em  # [N, T, C] cuda view, unit class stride
        N, T, Cn = em.shape
        Q = len(offsets) - 1
        self.shape, self.Q, self.blank, self.max_query, self.curves = (N, T, Cn), Q, blank, max_query, curves
        dev = em.device
        self.lengths = torch.tensor(lengths, dtype=torch.int32, device=dev)
        self.offsets = torch.tensor(offsets, dtype=torch.int32, device=dev)
        self.ids = torch.tensor(list(ids) + [0], dtype=torch.int32, device=dev)
        size = C.c_size_t()
        assert self.handle.amx_ctc_search_workspace(N, Q, T, max_query, C.byref(size)) == L.AMX_OK
        self.size = size.value
        self.workspace = torch.empty(max(1, size.value), dtype=torch.uint8, device=dev)
        R = N * Q
        self.outputs = [_Guarded((R,), torch.float32, dev), _Guarded((R, 2), torch.int32, dev), _Guarded((R,), torch.int32, dev),
                        _Guarded((R, T), torch.float32, dev), _Guarded((R, T), torch.int32, dev)]

    def run(self, expect=None):
        N, T, Cn = self.shape
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        out = [o.pointer() for o in self.outputs]
        if not self.curves:
            out[3] = out[4] = None
        code = self.handle.amx_ctc_search_emissions(
            self.em.device.index or 0, p(self.em), self.em.stride(0), self.em.stride(1), p(self.lengths), N, T, Cn, self.blank,
            p(self.offsets), p(self.ids), self.Q, self.max_query, p(self.workspace), self.size, *out,
            C.c_void_p(torch.cuda.current_stream(self.em.device).cuda_stream))
        assert code == (self.lib.AMX_OK if expect is None else expect), self.handle.amx_last_error(None)

    def refill(self):
        for o in self.outputs:
            o.refill()

    def buffers(self):
        return tuple(o.host() for o in self.outputs)


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _compare(got, want):
    for name, g, w in zip(NAMES, got, want):
        differ = np.argwhere(_bits(g) != _bits(w))
        assert differ.size == 0, (name, differ[:5].tolist(), g[tuple(differ[0])], w[tuple(differ[0])])


def _check(em_host, lengths, queries, blank=0, max_query=None, em_device=None, offsets=None, ids=None):
    """Runs the kernel on `em_host` ([N, T, C] fp32 cpu tensor; `em_device` a cuda view of the same values) and compares
    every buffer with the restatement bit for bit.  Returns the status as [N, Q]."""
    if offsets is None:
        offsets, ids = U.pack_queries(queries)
    if max_query is None:
        max_query = max(len(q) for q in queries)
    em_device = em_host.cuda() if em_device is None else em_device
    call = _Call(em_device, lengths, offsets, ids, max_query, blank)
    call.run()
    want = U.expected_buffers(em_host.numpy(), lengths, offsets, ids, max_query, blank, SENTINEL_I, SENTINEL_F)
    _compare(call.buffers(), want)
    return want[2].reshape(em_host.shape[0], len(offsets) - 1)


STRIP_LENGTHS = (1, 2, 32, 33, 64, 65, 128, 129, 256)


def test_strip_edges_and_per_row_dispatch(amd):
    """L of 1 to 256 (1, 3, 63, 65, 127, 129, 255, 257 and 511 states) as the nine queries of one call, so that every strip
    variant runs in one launch next to the others; the 300-frame utterance cannot hold the longest query."""
    rng = np.random.default_rng(1)
    queries = [_query(rng, L, 37) for L in STRIP_LENGTHS]
    assert 300 < U.minimum_frames(queries[-1]) <= 517 and U.minimum_frames(queries[-2]) <= 300
    em = _emissions(2, 517, 37, seed=1)
    status = _check(em, [517, 300], queries)
    assert status.tolist() == [[0] * 9, [0] * 8 + [-1]]


@pytest.mark.parametrize("Cn,blank", [(2, 0), (2, 1), (3, 2), (37, 5), (1025, 1024)])
def test_class_counts_and_blank(amd, Cn, blank):
    T = 70
    rng = np.random.default_rng(Cn + blank)
    em = _emissions(4, T, Cn, seed=Cn + blank)
    queries = [_query(rng, L, Cn, blank) for L in (1, 3, 6, 2, 9)]
    status = _check(em, [T, 0, 1, T - 5], queries, blank=blank)
    assert status[1].tolist() == [-1] * 5 and status[2, 0] == 0 and (status[[0, 3]] == 0).all()


def test_frame_length_edges(amd):
    """A query with adjacent repeats at no frames, one frame, one frame too few, exactly enough and around the 64-frame
    blocks in which m is loaded and the curves are stored."""
    y = [1, 1, 2, 3, 3, 3, 4]
    need = U.minimum_frames(y)
    assert need == 10
    lengths = [0, 1, need - 1, need, 63, 64, 65, 129]
    em = _emissions(len(lengths), 130, 6, seed=3)
    status = _check(em, lengths, [y, [5], [2, 2]])
    assert status[:, 0].tolist() == [-1, -1, -1, 0, 0, 0, 0, 0] and status[:, 1].tolist() == [-1] + [0] * 7
    # exactly enough frames on sharp emissions: the only path
    lp = torch.from_numpy(U.plant(need, 6, 0, [(0, [1, 0, 1, 2, 3, 0, 3, 0, 3, 4])], filler=5))[None]
    call = _Call(lp.cuda(), [need], *U.pack_queries([y]), len(y))
    call.run()
    best_scores, best_spans, status, _, _ = call.buffers()
    assert status.tolist() == [0] and best_scores.tolist() == [0.0] and best_spans.tolist() == [[0, need]]


def test_ties_in_every_comparison(amd):
    """Dyadic emissions (multiples of 1/8, few distinct values: sums tie all the time) and one-hot-sharp emissions with
    planted and doubly planted queries, whose costs are exactly +0 along the occurrence."""
    g = torch.Generator().manual_seed(12)
    T, Cn = 100, 4
    dyadic = 0.0 - torch.randint(0, 5, (3, T, Cn), generator=g).float() / 8.0
    constant = torch.full((1, T, Cn), -0.5)
    rng = np.random.default_rng(12)
    queries = [[1], [2, 2], [1, 2, 1, 2, 1, 2], [3] * 5] + [_query(rng, L, Cn, repeat=0.3) for L in (4, 11, 40)]
    status = _check(torch.cat([dyadic, constant]), [T, T - 1, 37, T], queries)
    assert (status[0] == 0).all() and status[2, 6] == -1

    y = [1, 2, 2, 3]
    frames = [1, 1, 1, 0, 2, 2, 0, 2, 3, 3]
    rows = [U.plant(80, 6, 0, [(7, frames)], 5), U.plant(80, 6, 0, [(2, frames), (61, frames)], 5),
            U.plant(80, 6, 0, [(64 - 3, frames)], 5), U.plant(80, 6, 0, [(10, frames), (20, frames), (30, frames[:-2])], 5)]
    em = torch.from_numpy(np.stack(rows))
    call = _Call(em.cuda(), [80] * 4, *U.pack_queries([y, [5], [3, 3]]), 4)
    call.run()
    got = call.buffers()
    _compare(got, U.expected_buffers(em.numpy(), [80] * 4, *U.pack_queries([y, [5], [3, 3]]), 4, 0, SENTINEL_I, SENTINEL_F))
    best_scores, best_spans = got[0].reshape(4, 3), got[1].reshape(4, 3, 2)
    assert best_scores[:, 0].view(np.int32).tolist() == [0] * 4  # +0.0
    assert best_spans[:, 0].tolist() == [[7, 17], [61, 71], [61, 71], [20, 30]]  # the later of two wins


def test_minus_infinity_emissions(amd):
    """Scattered -inf; a class of the query that is -inf throughout (-1); and a frame that is -inf in every class in the
    middle of an otherwise perfect occurrence, which is then not found across it."""
    T, Cn = 90, 7
    em = _emissions(5, T, Cn, seed=13)
    g = torch.Generator().manual_seed(13)
    em[:4][torch.rand(4, T, Cn, generator=g) < torch.tensor([0.05, 0.2, 0.5, 0.8]).view(4, 1, 1)] = -float("inf")
    em[4, :, 4] = -float("inf")
    em[1, 40] = -float("inf")
    rng = np.random.default_rng(13)
    queries = [_query(rng, L, Cn) for L in (1, 2, 5, 12)] + [[1, 4, 2]]
    status = _check(em, [T] * 5, queries)
    assert status[4, 4] == -1 and (status[0] == 0).all() and -1 in status[3].tolist()

    y, frames = [1, 2, 3], [1, 1, 2, 2, 2, 3]
    lp = U.plant(30, 5, 0, [(9, frames)], filler=4)
    blocked = lp.copy()
    blocked[12] = -np.inf
    em = torch.from_numpy(np.stack([lp, blocked]))
    call = _Call(em.cuda(), [30, 30], *U.pack_queries([y]), 3)
    call.run()
    got = call.buffers()
    _compare(got, U.expected_buffers(em.numpy(), [30, 30], *U.pack_queries([y]), 3, 0, SENTINEL_I, SENTINEL_F))
    best_scores, best_spans, status, end_scores, _ = got
    assert status.tolist() == [0, 0] and best_scores[0] == 0.0 and best_spans[0].tolist() == [9, 15]
    start, end = best_spans[1].tolist()
    assert best_scores[1] < -20.0 and not start <= 12 < end and not np.isnan(end_scores[1]).any()
    assert end_scores[1, 12] == -np.inf  # impassable, not NaN


def test_transposed_view_is_read_in_place(amd):
    out = _emissions(70, 5, 41, seed=11)  # [T, N, C]
    view = out.cuda().transpose(0, 1)
    assert not view.is_contiguous()
    rng = np.random.default_rng(11)
    lengths = [70, 12, 0, 69, 1]
    queries = [_query(rng, L, 41) for L in (9, 4, 1, 11)]
    host = out.transpose(0, 1).contiguous()
    _check(host, lengths, queries, em_device=view)
    # and through the Python entry point
    found = amd.ctc_search(view, torch.tensor(lengths), queries, curves=True)
    want = U.search_batch(host.numpy(), lengths, *U.pack_queries(queries), 11, fast=True)
    best = found.best()
    for n in range(5):
        for q in range(4):
            row = want[n * 4 + q]
            if row.status != 0:
                assert best[n][q] is None
                continue
            assert (best[n][q].start, best[n][q].end) == row.best_span and np.float32(best[n][q].score) == row.best_score
            k = lengths[n]
            assert np.array_equal(_bits(found.end_scores[n, q, :k].cpu().numpy()), _bits(row.end_scores))


def test_malformed_rows_are_flagged_and_write_nothing(amd):
    """An empty query, an id equal to the blank, an id >= C, a negative id, L > max_query, a frame length outside [0, T] and
    descending offsets: -2 and sentinels everywhere, next to valid rows that stay correct."""
    T, Cn, blank = 20, 6, 2
    em = _emissions(3, T, Cn, seed=15)
    #          0 ok      1 empty 2 blank   3 >= C     4 ok 5 negative 6 too long       7 ok
    queries = [[1, 3, 4], [], [1, 2, 3], [1, 6, 3], [5], [0, -1], [1, 3, 1, 3, 1], [3, 3]]
    status = _check(em, [T, T + 1, -1], queries, blank=blank, max_query=4)
    assert status.tolist() == [[0, -2, -2, -2, 0, -2, -2, 0], [-2] * 8, [-2] * 8]
    # offsets: query 1 ends before it begins, query 2 starts below its predecessor's end (allowed: it ascends itself),
    # query 3 reaches past offsets[Q]
    ids = [1, 3, 4, 5, 1, 3, 4, 5]
    status = _check(em[:1], [T], None, blank=blank, max_query=5, offsets=[0, 4, 2, 6, 8], ids=ids)
    assert status.tolist() == [[0, -2, 0, 0]]
    status = _check(em[:1], [T], None, blank=blank, max_query=4, offsets=[0, 5, 3, 9, 8], ids=ids)
    assert status.tolist() == [[-2, -2, -2, -2]]
    status = _check(em[:1], [T], None, blank=blank, max_query=5, offsets=[-1, 2, 4, 3], ids=ids)
    assert status.tolist() == [[-2, -2, -2]]
    # max_query = 257 is refused on the host: nothing is written
    call = _Call(em.cuda(), [T] * 3, *U.pack_queries([[1], [3]]), 1)
    call.max_query = 257
    call.run(expect=call.lib.AMX_EINVAL)
    torch.cuda.synchronize()
    for buffer in call.buffers():
        assert (buffer == buffer.dtype.type(SENTINEL_F if buffer.dtype == np.float32 else SENTINEL_I)).all()
    with pytest.raises(ValueError, match="query 1"):
        amd.ctc_search(em.cuda(), torch.tensor([T] * 3), [[1], [2], [3]], blank_index=blank)
    with pytest.raises(ValueError, match="utterance 1"):
        amd.ctc_search(em.cuda(), torch.tensor([T, T + 1, T]), [[1]], blank_index=blank)


def test_nan_emissions_keep_every_index_in_range(amd):
    """The values on NaN emissions are unspecified, but the guards and the entries the contract leaves untouched stay intact,
    status is 0 or -1 and every span lies within the row's frames."""
    N, T, Cn = 8, 150, 6
    em = _emissions(N, T, Cn, seed=22)
    g = torch.Generator().manual_seed(22)
    em[torch.rand(N, T, Cn, generator=g) < torch.tensor([0.001, 0.003, 0.01, 0.03, 0.1, 0.3, 0.6, 1.0]).view(N, 1, 1)] = float("nan")
    rng = np.random.default_rng(22)
    queries = [_query(rng, L, Cn) for L in (1, 3, 20, 50, 70)]
    lengths = [T, T, T - 1, T, 77, T, T, T]
    call = _Call(em.cuda(), lengths, *U.pack_queries(queries), 70)
    call.run()
    best_scores, best_spans, status, end_scores, end_starts = call.buffers()  # (checks the guards)
    assert set(status.tolist()) <= {0, -1}
    for r in range(N * 5):
        k = lengths[r // 5]
        assert (_bits(end_scores[r, k:]) == _bits(np.float32(SENTINEL_F))).all() and (end_starts[r, k:] == SENTINEL_I).all()
        assert (_bits(end_scores[r, :k]) != _bits(np.float32(SENTINEL_F))).all()
        assert ((end_starts[r, :k] >= -1) & (end_starts[r, :k] < k)).all()
        if status[r] == 0:
            assert 0 <= best_spans[r, 0] < best_spans[r, 1] <= k
        else:
            assert best_spans[r].tolist() == [SENTINEL_I] * 2 and _bits(best_scores[r:r + 1])[0] == _bits(np.float32(SENTINEL_F))


def test_null_curves_repeatability_and_graph_capture(amd):
    """Without curve pointers best_* and status are bitwise those of the run with curves; two runs are bitwise equal; one
    call captured on a single stream and replayed twice equals the eager result bit for bit."""
    rng = np.random.default_rng(19)
    em = _emissions(3, 150, 9, seed=19).cuda()
    lengths = [150, 77, 0]
    queries = [_query(rng, L, 9) for L in (1, 4, 20, 40, 70)]
    offsets, ids = U.pack_queries(queries)
    eager = _Call(em, lengths, offsets, ids, 70)
    eager.run()
    torch.cuda.synchronize()
    want = eager.buffers()
    _compare(want, U.expected_buffers(em.cpu().numpy(), lengths, offsets, ids, 70, 0, SENTINEL_I, SENTINEL_F))
    eager.refill()
    eager.run()
    _compare(eager.buffers(), want)

    bare = _Call(em, lengths, offsets, ids, 70, curves=False)
    bare.run()
    got = bare.buffers()
    _compare(got[:3], want[:3])
    assert (_bits(got[3]) == _bits(np.float32(SENTINEL_F))).all() and (got[4] == SENTINEL_I).all()

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
        captured.refill()
        graph.replay()
        torch.cuda.synchronize()
        _compare(captured.buffers(), want)


def test_long_row(amd):
    """2999 frames and 8 queries up to L = 256 against the frame-at-a-time restatement."""
    rng = np.random.default_rng(16)
    em = _emissions(1, 2999, 37, seed=16, scale=3.0)
    status = _check(em, [2999], [_query(rng, L, 37) for L in (1, 3, 12, 20, 50, 100, 180, 256)])
    assert (status == 0).all()


def test_facade(amd):
    """ctc_search, Found.best() and Found.hits() on a small batch with planted occurrences."""
    y, frames = [1, 2, 3], [1, 1, 2, 3]
    rows = [U.plant(40, 5, 0, [(3, frames), (20, frames)], filler=4), U.plant(40, 5, 0, [(30, frames)], filler=4),
            U.plant(40, 5, 0, [], filler=4)]
    em = torch.from_numpy(np.stack(rows)).cuda()
    lengths = torch.tensor([40, 40, 25])
    found = amd.ctc_search(em, lengths, [y, [4], [2, 2]], curves=True)
    assert found.scores.is_cuda and found.scores.shape == (3, 3) and found.spans.shape == (3, 3, 2) and found.status.shape == (3, 3)
    assert found.end_scores.shape == found.end_starts.shape == (3, 3, 40) and found.lengths == [40, 40, 25]
    best = found.best()
    assert best[0][0] == amd.Hit(20, 24, 0.0) and best[1][0] == amd.Hit(30, 34, 0.0)
    assert best[2][0] is not None and best[2][0].score < -20 and best[2][0].end <= 25
    assert best[2][1] == amd.Hit(0, 25, 0.0)  # the filler throughout the 25 frames
    hits = found.hits(0.0)
    assert hits[0][0] == [amd.Hit(3, 7, 0.0), amd.Hit(20, 24, 0.0)] and hits[1][0] == [amd.Hit(30, 34, 0.0)] and hits[2][0] == []
    assert found.hits(0.0, max_hits=1)[0][0] == [amd.Hit(20, 24, 0.0)]
    bare = amd.ctc_search(em, lengths, [y, [4], [2, 2]])
    assert bare.end_scores is None and bare.best() == best
    with pytest.raises(ValueError, match="curves"):
        bare.hits(0.0)
    # float64 input is converted, lengths default to T, empty batches return empty results
    assert amd.ctc_search(em.double(), None, [y]).best()[1][0] == amd.Hit(30, 34, 0.0)
    assert amd.ctc_search(em, lengths, []).best() == [[], [], []] and amd.ctc_search(em[:0], lengths[:0], [y]).best() == []


def test_through_the_estimator(amd):
    """Independent of the restatement: Estimator.search for slices (3 to 6 tokens) of each utterance's own greedy tokens on
    the phoneme output finds every one with score exactly 0.0; the argmax path over the returned span collapses to the
    query and its first and last frames are the query's first and last phoneme."""
    from allophant_amd import spec as S, synthetic

    attributes = ["syllabic", "long", "nasal"]
    spec = S.multitask_spec(S.tiny_encoder(2), attributes, embedding_size=16, train_phonemes=9, n_features=5, n_values=3)
    N = 5
    audio, lengths = synthetic.make_audio(N, 12000, seed=7, ragged=True)
    inventory = ["a", "ts", "t͡ʃ", "é", "m", "aː", "i"]
    est = amd.Estimator(spec, synthetic.make_state_dict(spec, seed=3), "cuda:0", "f16x3")
    try:
        batch = amd.Batch(audio.cuda(), lengths, torch.zeros(N, dtype=torch.long))
        pred = est.predict(batch, synthetic.make_inventory(spec, len(inventory), seed=2))
        em = pred.outputs["phoneme"].cpu().transpose(0, 1)  # [N, T, C]
        frame_lengths = [int(v) for v in pred.lengths]
        rng = np.random.default_rng(5)
        queries, owner = [], []
        for n in range(N):
            tokens = U.collapse(em[n, :frame_lengths[n]].argmax(-1).tolist(), 0)
            for size in (3, 4, 5, 6):
                if len(tokens) >= size:
                    at = int(rng.integers(0, len(tokens) - size + 1))
                    queries.append(tokens[at:at + size])
                    owner.append(n)
        assert len(queries) >= N  # the tiny model's argmax path changes often enough
        found = est.search(pred, queries, "phoneme")
        assert len(found) == N and all(len(row) == len(queries) for row in found)
        for q, (query, n) in enumerate(zip(queries, owner)):
            hit = found[n][q]
            assert hit is not None and hit.score == 0.0, (n, query, hit)
            path = em[n, hit.start:hit.end].argmax(-1).tolist()
            assert U.collapse(path, 0) == query and path[0] == query[0] and path[-1] == query[-1]
            assert 0 <= hit.start < hit.end <= frame_lengths[n]
        device = est.search_device(pred, queries[:2], "phoneme", curves=True)
        assert device.scores.is_cuda and device.end_scores.shape == (N, 2, em.shape[1])
        assert device.seconds(spec).shape == (N, 2, 2)
        with pytest.raises(ValueError, match="nope"):
            est.search(pred, queries, "nope")
    finally:
        est.close()

"""On-device CTC forced alignment over label graphs (amx_ctc_align_graph.hip) against the restatement of its contract
(tests/ctc_align_graph_util.py), bit for bit in every output buffer -- paths, frame_scores, spans, span_scores, totals (as fp32
bits) and status, including the entries the contract leaves untouched (the buffers are pre-filled with sentinels and lie between
guard bands that must stay untouched) -- and, on chains, against amx_ctc_align_emissions on the same rows."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_align_graph_util as G

pytestmark = pytest.mark.gpu

SENTINEL_I, SENTINEL_F, GUARD = -77, -12345.5, 64
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


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


class _Buffers:
    """The six outputs and the workspace, each inside one allocation with GUARD sentinel elements on either side."""

    def __init__(self, N, T, width, workspace_bytes, dev):
        shapes = {"paths": (N, T), "frame_scores": (N, T), "spans": (N, max(1, width), 2), "span_scores": (N, max(1, width)),
                  "totals": (N,), "status": (N,)}
        self.whole, self.view = {}, {}
        for name, shape in list(shapes.items()) + [("workspace", (max(8, workspace_bytes) // 4,))]:
            floating = name in ("frame_scores", "span_scores", "totals")
            count = int(np.prod(shape))
            whole = torch.full((count + 2 * GUARD,), SENTINEL_F if floating else SENTINEL_I,
                               dtype=torch.float32 if floating else torch.int32, device=dev)
            self.whole[name], self.view[name] = whole, whole[GUARD:GUARD + count].view(*shape)
        self.width = width

    def pointer(self, name):
        return C.c_void_p(self.view[name].data_ptr())

    def refill(self):
        for name, whole in self.whole.items():
            whole.fill_(SENTINEL_F if whole.dtype == torch.float32 else SENTINEL_I)

    def outputs(self):
        for name, whole in self.whole.items():
            sentinel = SENTINEL_F if whole.dtype == torch.float32 else SENTINEL_I
            assert bool((whole[:GUARD] == sentinel).all()) and bool((whole[-GUARD:] == sentinel).all()), f"guard band of {name} touched"
        host = {name: self.view[name].cpu().numpy() for name in NAMES}
        return (host["paths"], host["frame_scores"], host["spans"][:, :self.width], host["span_scores"][:, :self.width],
                host["totals"], host["status"])


class _GraphCall:
    """One amx_ctc_align_graph_emissions call; `run` may be repeated (graph capture)."""

    def __init__(self, em, lengths, packed: G.Packed, max_nodes, blank=0):
        from allophant_amd import lib as L

        self.lib, self.handle, self.em, self.blank, self.max_nodes = L, L.load(), em, blank, max_nodes
        N, T, _ = em.shape
        dev = em.device
        tensor = lambda values: torch.tensor(list(values) + [0], dtype=torch.int32, device=dev)  # noqa: E731  (never empty)
        self.lengths = torch.tensor(lengths, dtype=torch.int32, device=dev)
        self.graph = [tensor(part) for part in packed]
        size = C.c_size_t()
        assert self.handle.amx_ctc_align_graph_workspace(N, T, max_nodes, C.byref(size)) == L.AMX_OK
        self.size = size.value
        self.b = _Buffers(N, T, max_nodes, size.value, dev)

    def run(self):
        N, T, Cn = self.em.shape
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        b = self.b
        code = self.handle.amx_ctc_align_graph_emissions(
            self.em.device.index or 0, p(self.em), self.em.stride(0), self.em.stride(1), p(self.lengths), N, T, Cn, self.blank,
            *(p(t) for t in self.graph), self.max_nodes, b.pointer("workspace"), self.size, b.pointer("paths"),
            b.pointer("frame_scores"), b.pointer("spans"), b.pointer("span_scores"), b.pointer("totals"), b.pointer("status"),
            C.c_void_p(torch.cuda.current_stream(self.em.device).cuda_stream))
        assert code == self.lib.AMX_OK, self.handle.amx_last_error(None)


def _chain_call(em, lengths, rows, max_target, blank=0):
    """The same rows through amx_ctc_align_emissions, on buffers of the same kind."""
    from allophant_amd import lib as L

    handle = L.load()
    N, T, Cn = em.shape
    dev = em.device
    offsets = torch.tensor(np.concatenate(([0], np.cumsum([len(r) for r in rows]))).tolist(), dtype=torch.int32, device=dev)
    ids = torch.tensor([v for r in rows for v in r] + [0], dtype=torch.int32, device=dev)
    frame_lengths = torch.tensor(lengths, dtype=torch.int32, device=dev)
    size = C.c_size_t()
    assert handle.amx_ctc_align_workspace(N, T, max_target, C.byref(size)) == L.AMX_OK
    b = _Buffers(N, T, max_target, size.value, dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    code = handle.amx_ctc_align_emissions(
        dev.index or 0, p(em), em.stride(0), em.stride(1), p(frame_lengths), N, T, Cn, blank, p(offsets), p(ids), max_target,
        b.pointer("workspace"), size.value, b.pointer("paths"), b.pointer("frame_scores"), b.pointer("spans"), b.pointer("span_scores"),
        b.pointer("totals"), b.pointer("status"), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert code == L.AMX_OK, handle.amx_last_error(None)
    return b.outputs()


def _assert_same(got, want):
    for name, g, w in zip(NAMES, got, want):
        differ = np.argwhere(_bits(g) != _bits(w))
        assert differ.size == 0, (name, differ[:5].tolist(), g[tuple(differ[0])], w[tuple(differ[0])])


def _check(em_host, lengths, graphs=None, blank=0, max_nodes=None, em_device=None, packed=None):
    """Runs the kernel on `em_host` ([N, T, C] fp32 cpu tensor; `em_device` a cuda view of the same values) and compares every
    buffer with the restatement bit for bit.  Returns the outputs."""
    packed = G.pack(graphs) if packed is None else packed
    if max_nodes is None:
        max_nodes = max(len(g.classes) for g in graphs)
    call = _GraphCall(em_host.cuda() if em_device is None else em_device, lengths, packed, max_nodes, blank)
    call.run()
    got = call.b.outputs()
    _assert_same(got, G.expected_buffers(em_host.numpy(), lengths, packed, max_nodes, blank, SENTINEL_I, SENTINEL_F))
    return got


def _targets(rng, L, Cn, blank=0, repeat=0.2):
    classes = [c for c in range(Cn) if c != blank]
    out = []
    for _ in range(L):
        out.append(out[-1] if out and rng.random() < repeat else int(rng.choice(classes)))
    return out


CHAIN_LENGTHS = (0, 1, 31, 32, 33)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_chains_equal_the_chain_kernel(amd, T):
    """L of 0, 1, 31, 32 and 33 (1, 3, 63, 65 and 67 states, around the edge of a strip), each at T frames and at a shorter
    ragged length: every output equals amx_ctc_align_emissions' bit for bit, and the restatement."""
    rng = np.random.default_rng(T)
    rows = [_targets(rng, L, 7) for L in CHAIN_LENGTHS] * 2
    lengths = [T] * len(CHAIN_LENGTHS) + [max(0, T - 1 - 7 * k) for k in range(len(CHAIN_LENGTHS))]
    em = _emissions(len(rows), T, 7, seed=T)
    em[1::2] = torch.round(em[1::2])  # integer emissions: comparisons tie
    got = _check(em, lengths, [G.chain(y) for y in rows])
    _assert_same(got, _chain_call(em.cuda(), lengths, rows, max(CHAIN_LENGTHS)))
    assert got[5][0] == 0 and (T < 33 or (got[5][:5] == 0).all())


@pytest.mark.parametrize("Cn,blank", [(2, 0), (3, 2), (37, 5)])
def test_random_dags(amd, Cn, blank):
    """In-degrees 0 .. 6, up to 150 nodes (five strips, five waves), ragged frame lengths including 0."""
    rng = np.random.default_rng(Cn)
    T = 70
    sizes = (1, 2, 9, 31, 32, 33, 64, 100, 150, 0)
    graphs = [G.random_dag(rng, L, Cn, blank) for L in sizes]
    assert {len(p) for g in graphs for p in g.preds} == set(range(7))
    lengths = [T, 3, T - 1, 40, T, 0, 64, 65, T, 5]
    got = _check(_emissions(len(sizes), T, Cn, seed=Cn), lengths, graphs, blank=blank)
    assert got[5][5] == -1 and got[5][9] == 0 and (got[5] == 0).sum() >= 6


def test_a_predecessor_in_another_waves_strip(amd):
    """A chain of 300 nodes in which node 200 is also preceded by node 3 (states 401 and 7: strips 6 and 0).  With 140 frames
    only the path through that arc fits; with 400 frames both do."""
    rng = np.random.default_rng(3)
    y = _targets(rng, 300, 9, repeat=0.0)
    g = G.chain(y)
    g.preds[200].append(3)
    got = _check(_emissions(2, 400, 9, seed=3), [140, 400], [g, g])
    assert got[5].tolist() == [0, 0]
    spans = got[2][0]
    assert (spans[4:200] == -1).all() and (spans[:4] >= 0).all() and (spans[200:] >= 0).all()


def test_same_class_predecessors(amd):
    """A predecessor with its successor's class: the direct arc is absent and the path passes the leading blank (three nodes
    of one class need five frames), also where the same-class predecessor is one of several."""
    g = G.Graph([1, 1, 1], [1, 0, 2], [[], [0], [1]])
    mixed = G.Graph([1, 2, 1, 3], [1, 1, 0, 2], [[], [], [0, 1], [2]])
    em = _emissions(4, 9, 4, seed=5)
    got = _check(em, [5, 4, 9, 9], [g, g, g, mixed])
    assert got[5].tolist() == [0, -1, 0, 0] and got[0][0].tolist()[:5] == [1, 0, 1, 0, 1]
    rng = np.random.default_rng(5)
    graphs = [G.random_dag(rng, L, 3, 0, same_class=1.0) for L in (20, 70, 90)]
    _check(_emissions(3, 150, 3, seed=6), [150, 149, 100], graphs)


def test_in_degree_and_final_limits(amd):
    """6 predecessors and 6 finals are accepted; 7 of either make the row malformed."""
    fan = lambda d: G.Graph([1 + k % 3 for k in range(d)] + [4], [1] * d + [2], [[]] * d + [list(range(d))])  # noqa: E731
    ends = lambda f: G.Graph([1] + [2 + k % 3 for k in range(f)], [1] + [2] * f, [[]] + [[0]] * f)  # noqa: E731
    got = _check(_emissions(4, 12, 5, seed=7), [12] * 4, [fan(6), fan(7), ends(6), ends(7)])
    assert got[5].tolist() == [0, -2, 0, -2]


def test_tie_grid(amd):
    """All-equal and integer-rounded emissions on slot graphs of two alternatives: the earlier candidate must win."""
    from allophant_amd.graph_alignment import TargetGraph

    rng = np.random.default_rng(8)
    slots = [[[int(rng.integers(1, 4))], [int(rng.integers(1, 4)), int(rng.integers(1, 4))]] if k % 3 == 0 else [[int(rng.integers(1, 4))]]
             for k in range(40)]
    g = G.of_target_graph(TargetGraph.from_slots(slots))
    two = G.of_target_graph(TargetGraph.from_slots([[[1], [2]]]))
    T = 120
    constant = torch.full((3, T, 4), -0.5)
    drawn = torch.round(_emissions(3, T, 4, seed=8))
    got = _check(torch.cat([constant, drawn]), [T, T - 1, 4, T, 100, 4], [g, g, two, g, g, two])
    assert (got[5] == 0).all()
    assert got[2][2, :2].tolist() == [[0, 4], [-1, -1]]  # the first final wins the tie at the end


def test_minus_infinity_emissions(amd):
    """-inf on one alternative's class leaves the other; on both, no path (-1); scattered -inf as the restatement says."""
    from allophant_amd.graph_alignment import TargetGraph

    g = G.of_target_graph(TargetGraph.from_slots([[[1]], [[2, 3], [4]], [[5]]]))
    em = _emissions(7, 30, 6, seed=9)
    em[0, :, 4] = -float("inf")
    em[1, :, 3] = -float("inf")
    em[2, :, 3] = -float("inf")
    em[2, :, 4] = -float("inf")
    gen = torch.Generator().manual_seed(9)
    em[3:][torch.rand(4, 30, 6, generator=gen) < torch.tensor([0.05, 0.3, 0.6, 0.9]).view(4, 1, 1)] = -float("inf")
    got = _check(em, [30] * 7, [g] * 7)
    assert got[5][:3].tolist() == [0, 0, -1] and got[5][6] == -1
    assert got[2][0, 3].tolist() == [-1, -1] and got[2][1, 1].tolist() == [-1, -1] and got[2][1, 3, 0] >= 0


def test_nan_emissions_leave_the_other_rows_and_the_guards_alone(amd):
    """The result on NaN emissions is unspecified; the rows next to them are what the restatement says, every index stays in
    range and no guard band is touched."""
    rng = np.random.default_rng(10)
    N, T, Cn = 6, 90, 5
    graphs = [G.random_dag(rng, 60, Cn, 0) for _ in range(N)]
    em = _emissions(N, T, Cn, seed=10)
    clean = em.clone()
    gen = torch.Generator().manual_seed(10)
    em[1::2][torch.rand(3, T, Cn, generator=gen) < torch.tensor([0.01, 0.2, 1.0]).view(3, 1, 1)] = float("nan")
    packed = G.pack(graphs)
    call = _GraphCall(em.cuda(), [T] * N, packed, 60)
    call.run()
    got = call.b.outputs()  # (checks the guard bands)
    want = G.expected_buffers(clean.numpy(), [T] * N, packed, 60, 0, SENTINEL_I, SENTINEL_F)
    for name, g, w in zip(NAMES, got, want):
        assert np.array_equal(_bits(g[0::2]), _bits(w[0::2])), name
    paths, _, spans, _, _, status = got
    for n in (1, 3, 5):
        assert status[n] in (0, -1)
        if status[n] == 0:
            assert ((paths[n] >= 0) & (paths[n] < Cn)).all() and ((spans[n] >= -1) & (spans[n] <= T)).all()


def test_malformed_rows_are_flagged_and_write_nothing(amd):
    """Every -2 condition next to valid rows that stay correct: -2 and sentinels everywhere else in the row."""
    T, Cn, blank = 20, 6, 2
    em = _emissions(12, T, Cn, seed=11)
    ok = G.Graph([1, 3, 4], [1, 0, 2], [[], [0], [0, 1]])
    graphs = [ok,
              ok._replace(classes=[1, 2, 4]),                # the blank
              ok._replace(classes=[1, 6, 4]),                # >= C
              ok._replace(classes=[-1, 3, 4]),               # negative
              ok._replace(preds=[[], [1], [0]]),             # a predecessor equal to the node
              ok._replace(preds=[[], [0], [0, 2]]),          # a predecessor above the node
              ok._replace(preds=[[], [-1], [1]]),            # a negative predecessor
              ok._replace(flags=[0, 0, 2]),                  # no initial node
              ok._replace(flags=[1, 0, 0]),                  # no final node
              G.chain([1, 3, 1, 3, 1]),                      # L > max_nodes
              ok, ok]
    got = _check(em, [T] * 10 + [T + 1, -1], graphs, blank=blank, max_nodes=4)
    assert got[5].tolist() == [0] + [-2] * 11
    # offsets: node offsets that descend or pass the node count, arc offsets that descend or pass the arc count
    packed = G.pack([ok] * 4)
    got = _check(em[:4], [T] * 4, blank=blank, max_nodes=4, packed=packed._replace(node_offsets=[0, 3, 2, 6, 12]))
    assert got[5].tolist() == [0, -2, -2, -2]  # row 2 holds 4 nodes whose arcs are another row's; row 3 six
    got = _check(em[:4], [T] * 4, blank=blank, max_nodes=4, packed=packed._replace(node_offsets=[-1, 3, 6, 9, 12]))
    assert got[5].tolist() == [-2, 0, 0, 0]
    arcs = list(packed.arc_offsets)  # [0, 0, 1, 3, 3, 4, 6, 6, 7, 9, 9, 10, 12]
    got = _check(em[:4], [T] * 4, blank=blank, max_nodes=4, packed=packed._replace(arc_offsets=arcs[:4] + [5, 4] + arcs[6:11] + [13, 12]))
    assert got[5].tolist() == [0, -2, 0, -2]
    from allophant_amd.graph_alignment import TargetGraph

    with pytest.raises(ValueError, match="row 1"):
        amd.ctc_graph_align(em[:3].cuda(), torch.tensor([T] * 3), [TargetGraph.chain(v) for v in ([1], [2], [3])], blank_index=blank)


def _skip_chain(rng, L):
    """A chain with an arc from node 50 (k - 1) to node 50 k beside the chain's own, initial at every multiple of 50 and final
    at six nodes spread over the graph: within 40 frames a path can lie in any sixth of it."""
    g = G.chain(_targets(rng, L, 5, repeat=0.002))
    for j in range(50, L, 50):
        g.preds[j].append(j - 50)
        g.flags[j] |= 1
    for k in range(1, 6):
        g.flags[min(L - 1, k * L // 6 + 7)] |= 2
    return g


@pytest.mark.parametrize("L", [1023, 1024, 2047, 2048, 4095])
def test_strips_per_wave_variants(amd, L):
    """The kernel is instantiated for 1, 2, 4 and 8 strips per wave: max_nodes around 1024 and 2048 switches between them, and
    4095 nodes (8191 states) fill the LDS rows.  T = 40, frame lengths 40 and 17."""
    rng = np.random.default_rng(L)
    g = _skip_chain(rng, L)
    got = _check(_emissions(2, 40, 5, seed=L), [40, 17], [g, g])
    assert got[5].tolist() == [0, 0]


def test_transposed_view_is_read_in_place(amd):
    from allophant_amd.graph_alignment import TargetGraph

    out = _emissions(30, 5, 11, seed=12)  # [T, N, C]
    view = out.cuda().transpose(0, 1)
    assert not view.is_contiguous()
    rng = np.random.default_rng(12)
    lengths = [30, 12, 0, 29, 1]
    slots = [[[[int(rng.integers(1, 11))], [int(rng.integers(1, 11)), int(rng.integers(1, 11))]] for _ in range(k)] for k in (5, 3, 1, 6, 1)]
    targets = [TargetGraph.from_slots(s) for s in slots]
    graphs = [G.of_target_graph(t) for t in targets]
    host = out.transpose(0, 1).contiguous()
    _check(host, lengths, graphs, em_device=view)
    # and through the Python entry point
    got = amd.ctc_graph_align(view, torch.tensor(lengths), targets)
    for n, (row, g) in enumerate(zip(got, graphs)):
        _same_alignment(row, G.align_row(host[n, :lengths[n]].numpy(), g, fast=True))


def _same_alignment(got, want):
    if want.status != 0:
        assert got is None
        return
    nodes = [j for j in range(len(want.spans)) if want.spans[j, 0] >= 0]
    assert got.nodes == nodes and got.labels == [got.graph.classes[j] for j in nodes]
    assert np.array_equal(got.tokens.numpy(), want.paths) and np.array_equal(got.spans.numpy(), want.spans[nodes])
    assert np.array_equal(_bits(got.scores.numpy()), _bits(want.frame_scores))
    assert np.array_equal(_bits(got.span_scores.numpy()), _bits(want.span_scores[nodes]))
    assert np.float32(got.total) == want.total


def test_through_the_estimator(amd):
    """predict -> greedy hypothesis -> slots with one wrong alternative at every third position -> Estimator.align_graph:
    choices() picks the hypothesis everywhere, and every output equals the restatement on predictions.outputs."""
    from allophant_amd import spec as S, synthetic
    from allophant_amd.graph_alignment import TargetGraph

    spec = S.multitask_spec(S.tiny_encoder(2), ["syllabic", "long", "nasal"], embedding_size=16, train_phonemes=9, n_features=5,
                            n_values=3)
    names = S.output_names(spec)
    N = 4
    audio, lengths = synthetic.make_audio(N, 12000, seed=7, ragged=True)
    est = amd.Estimator(spec, synthetic.make_state_dict(spec, seed=3), "cuda:0", "f16x3")
    try:
        pred = est.predict(amd.Batch(audio.cuda(), lengths, torch.zeros(N, dtype=torch.long)), synthetic.make_inventory(spec, 7, seed=2))
        greedy = est.greedy_decode(pred)
        graphs, wanted = {}, {}
        for name in ("phoneme", "nasal"):
            classes = pred.outputs[name].shape[2]
            graphs[name], wanted[name] = [], []
            for n in range(N):
                hypothesis = [int(v) for v in greedy[name][n][0].tokens.tolist()]
                if not hypothesis:
                    graphs[name].append(TargetGraph.chain([]))
                    wanted[name].append([])
                    continue
                wrong = lambda c: 1 + c % (classes - 1)  # noqa: E731  (another non-blank class)
                slots = [[[wrong(c)], [c]] if k % 3 == 0 else [[c]] for k, c in enumerate(hypothesis)]
                graphs[name].append(TargetGraph.from_slots(slots))
                wanted[name].append([1 if k % 3 == 0 else 0 for k in range(len(hypothesis))])
        assert any(len(w) > 2 for w in wanted["phoneme"])
        result = est.align_graph(pred, graphs)
        assert list(result) == [name for name in names if name in graphs]
        frames = [int(v) for v in pred.lengths]
        for name, rows in result.items():
            em = pred.outputs[name].cpu().transpose(0, 1).contiguous().numpy()
            for n, row in enumerate(rows):
                _same_alignment(row, G.align_row(em[n, :frames[n]], G.of_target_graph(graphs[name][n]), fast=True))
                assert row is not None and row.choices() == wanted[name][n]
                assert row.labels == [int(v) for v in greedy[name][n][0].tokens.tolist()]
        seconds = next(row for row in result["phoneme"] if len(row.nodes)).seconds(spec)
        assert seconds.shape[1] == 2 and float(seconds[0, 1]) > float(seconds[0, 0]) >= 0.0
        device = est.align_graph_device(pred, {"phoneme": graphs["phoneme"]})
        assert device.paths.is_cuda and device.present == ["phoneme"] and device.names == names
        assert device.status[names.index("long")].cpu().tolist() == [0] * N  # aligned against no nodes: all blank
        with pytest.raises(ValueError):
            est.align_graph(pred, {"nope": [TargetGraph.chain([])] * N})
    finally:
        est.close()


def test_graph_capture(amd):
    """One amx_ctc_align_graph_emissions call captured on a single stream and replayed twice equals the eager result bit for
    bit."""
    rng = np.random.default_rng(19)
    em = _emissions(3, 150, 9, seed=19).cuda()
    lengths = [150, 77, 0]
    packed = G.pack([G.random_dag(rng, L, 9, 0) for L in (70, 20, 0)])
    eager = _GraphCall(em, lengths, packed, 70)
    eager.run()
    torch.cuda.synchronize()
    want = eager.b.outputs()
    assert want[5].tolist()[2] == 0
    captured = _GraphCall(em, lengths, packed, 70)
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
        captured.b.refill()
        graph.replay()
        torch.cuda.synchronize()
        for name, g, w in zip(NAMES, captured.b.outputs(), want):
            assert np.array_equal(_bits(g), _bits(w)), name

"""The CTC forced alignment over label graphs without a GPU: the restatement of its contract (tests/ctc_align_graph_util.py)
against the chain aligner's restatement (bit for bit on chains) and against the maximum over every accepted sequence (bit for
bit on random DAGs), its frame-at-a-time form against the literal one, TargetGraph.from_slots against the cartesian product,
GraphAlignment.choices, and the header, exports, workspace sizes and refusals of the built library."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ctc_align_graph_util as G
import ctc_align_util as U
import edit_util as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


def _emissions(rng, T, Cn, rounded):
    lp = np.log(rng.dirichlet(np.ones(Cn), T)).astype(np.float32)
    return np.round(lp) if rounded else lp  # integer emissions: comparisons tie


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_row(got: G.Row, want, states=True):
    assert got.status == want.status
    if want.status != 0:
        return
    assert _same_bits(got.paths, want.paths) and _same_bits(got.frame_scores, want.frame_scores)
    assert _same_bits(got.spans, want.spans) and _same_bits(got.span_scores, want.span_scores)
    assert _same_bits(np.float32(got.total), np.float32(want.total))
    if states:
        assert got.states.tolist() == want.states.tolist()


@pytest.mark.parametrize("rounded", [False, True])
def test_chains_equal_the_chain_aligner_bit_for_bit(rounded):
    """Status, paths, frame scores, spans, span scores, total and the walked states, in both forms of the sweep; some rows
    have too few frames (-1) and some repeat a class."""
    rng = np.random.default_rng(5 + rounded)
    seen = set()
    for _ in range(60):
        Cn = int(rng.integers(2, 6))
        blank = int(rng.integers(0, Cn))
        L = int(rng.integers(0, 7))
        y = [int(rng.choice([c for c in range(Cn) if c != blank])) for _ in range(L)]
        T = int(rng.integers(max(0, L - 1), 2 * L + 4))
        lp = _emissions(rng, T, Cn, rounded)
        want = U.align_row(lp, y, blank)
        seen.add(want.status)
        _same_row(G.align_row(lp, G.chain(y), blank), want)
        _same_row(G.align_row(lp, G.chain(y), blank, fast=True), want)
    assert seen == {0, -1}


@pytest.mark.parametrize("rounded", [False, True])
def test_dag_totals_equal_the_best_accepted_sequence_bitwise(rounded):
    """A path's value is the same frame-order fp32 sum in either trellis, so the graph's total is the maximum of the chain
    aligner's totals over every sequence the graph accepts; and the two forms of the sweep agree in every output."""
    rng = np.random.default_rng(11 + rounded)
    aligned = 0
    for _ in range(60):
        Cn = int(rng.integers(2, 5))
        blank = int(rng.integers(0, Cn))
        g = G.random_dag(rng, int(rng.integers(1, 9)), Cn, blank)
        T = int(rng.integers(1, 12))
        lp = _emissions(rng, T, Cn, rounded)
        got = G.align_row(lp, g, blank)
        _same_row(G.align_row(lp, g, blank, fast=True), got)
        sequences = G.accepted_sequences(g)
        assert sequences
        totals = [row.total for row in (U.align_row(lp, list(s), blank) for s in sequences) if row.status == 0]
        if not totals:
            assert got.status == -1
            continue
        aligned += 1
        assert got.status == 0 and _same_bits(np.float32(got.total), np.float32(max(totals)))
        # the visited nodes spell an accepted sequence, and the path's frame-order sum is the total
        visited = [j for j in range(len(g.classes)) if got.spans[j, 0] >= 0]
        assert tuple(g.classes[j] for j in visited) in sequences
        acc = np.float32(0)
        for v in got.frame_scores:
            acc = np.float32(acc + v)
        assert acc == got.total or rounded  # (ties aside, the recurrence adds the same values in the same order)
    assert aligned > 30


def test_hand_made_rows():
    flat = np.full((4, 4), -1.0, np.float32)
    # two alternatives for one slot on flat emissions: the final nodes are compared in ascending order, the first wins
    g = G.Graph([1, 2], [3, 3], [[], []])
    row = G.align_row(flat, g)
    assert row.status == 0 and row.paths.tolist() == [1, 1, 1, 1] and row.spans.tolist() == [[0, 4], [-1, -1]]
    assert row.span_scores.tolist() == [-4.0, 0.0]
    # a same-class predecessor: the direct arc is absent, the path passes the leading blank
    g = G.Graph([1, 1], [1, 2], [[], [0]])
    row = G.align_row(flat[:3], g)
    assert row.paths.tolist() == [1, 0, 1] and G.align_row(flat[:2], g).status == -1
    assert G.candidates(g, 3) == [(0, 3), (1, 2)] and G.candidates(g, 2) == [(0, 2), (2, 1)]
    # the closing blank reads the finals in ascending node order
    g = G.Graph([1, 2, 3], [1, 2, 2], [[], [0], [0]])
    assert G.candidates(g, 6) == [(0, 6), (2, 3), (3, 5)]
    # -inf leaves one alternative
    lp = flat.copy()
    lp[:, 1] = -INF
    row = G.align_row(lp, G.Graph([1, 2], [3, 3], [[], []]))
    assert row.status == 0 and row.spans.tolist() == [[-1, -1], [0, 4]]
    lp[:, 2] = -INF
    assert G.align_row(lp, G.Graph([1, 2], [3, 3], [[], []])).status == -1
    # no nodes: all blank; no frames and no nodes: total 0
    row = G.align_row(flat, G.Graph([], [], []))
    assert row.status == 0 and row.paths.tolist() == [0] * 4 and row.total == np.float32(-4.0)
    row = G.align_row(flat[:0], G.Graph([], [], []))
    assert row.status == 0 and row.total == 0 and G.align_row(flat[:0], G.chain([1])).status == -1
    # malformed graphs
    for bad in (G.Graph([0], [3], [[]]), G.Graph([4], [3], [[]]), G.Graph([1, 2], [1, 2], [[], [1]]), G.Graph([1, 2], [1, 2], [[], [-1]]),
                G.Graph([1], [2], [[]]), G.Graph([1], [1], [[]]), G.Graph([1] * 8, [1] * 7 + [2], [[]] * 7 + [list(range(7))]),
                G.Graph([1] * 7, [3] * 7, [[]] * 7)):
        assert G.align_row(flat, bad).status == -2
    assert G.align_row(flat, G.Graph([1] * 7, [1] * 6 + [2], [[]] * 6 + [list(range(6))])).status == 0
    assert G.align_row(flat, G.Graph([1] * 6, [3] * 6, [[]] * 6)).status == 0


def test_batch_form_refuses_bad_rows():
    em = np.stack([np.full((5, 3), -1.0, np.float32)] * 4)
    packed = G.pack([G.chain([1, 2]), G.chain([1]), G.chain([2]), G.chain([1])])
    assert [r.status for r in G.align_batch(em, [5, 6, -1, 0], packed, 1)] == [-2, -2, -2, -1]
    assert [r.status for r in G.align_batch(em, [5, 5, 5, 5], packed, 2)] == [0, 0, 0, 0]
    assert [r.status for r in G.align_batch(em, [5] * 4, packed._replace(node_offsets=[0, 2, 1, 4, 5]), 2)] == [0, -2, -2, 0]
    assert [r.status for r in G.align_batch(em, [5] * 4, packed._replace(arc_offsets=[0, 0, 1, 0, 1, 1]), 2)] == [0, -2, -2, 0]
    assert [r.status for r in G.align_batch(em, [5] * 4, packed._replace(arc_offsets=[0, 0, 2, 1, 1, 1]), 2)] == [-2, -2, 0, 0]


def _random_slots(rng, classes=6):
    slots = []
    for _ in range(int(rng.integers(1, 5))):
        slot = [[int(rng.integers(1, classes)) for _ in range(int(rng.integers(0, 3)))] for _ in range(int(rng.integers(1, 4)))]
        slots.append(slot)
    return slots


def test_from_slots_accepts_the_cartesian_product():
    from allophant_amd.graph_alignment import ALIGN_GRAPH_MAX_IN, TargetGraph

    rng = np.random.default_rng(23)
    built = refused = 0
    for _ in range(300):
        slots = _random_slots(rng)
        product = sorted({tuple(v for part in parts for v in part) for parts in itertools.product(*slots)})
        try:
            graph = TargetGraph.from_slots(slots)
        except ValueError:
            refused += 1
            # only the refusals the constructor states
            assert all(any(len(a) == 0 for a in slot) for slot in slots) or sum(len(slot) for slot in slots) > ALIGN_GRAPH_MAX_IN
            continue
        built += 1
        g = G.of_target_graph(graph)
        assert not G.malformed(g, 6, 0)
        assert G.accepted_sequences(g) == product
        assert len(graph.where) == len(graph.classes) and len(graph.skips) == len(slots)
        for choice in itertools.islice(itertools.product(*[range(len(slot)) for slot in slots]), 5):
            assert graph.sequence(choice) == [v for s, k in enumerate(choice) for v in slots[s][k]]
    assert built > 150 and refused > 5


def test_from_slots_rules_and_refusals():
    from allophant_amd.graph_alignment import TargetGraph

    g = TargetGraph.from_slots([[[1, 2], [3]], [[], [4]], [[5], [6, 7]]])
    assert g.classes == [1, 2, 3, 4, 5, 6, 7]
    assert g.preds == [[], [0], [], [1, 2], [1, 2, 3], [1, 2, 3], [5]]  # slot 1 can be skipped: slot 2 sees the exits of both
    assert g.initial == [True, False, True, False, False, False, False] and g.final == [False] * 4 + [True, False, True]
    assert g.where == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 1, 0), (2, 0, 0), (2, 1, 0), (2, 1, 1)] and g.skips == [None, 0, None]
    g = TargetGraph.from_slots([[[], [1]], [[2]]])  # initial while every earlier slot can be skipped
    assert g.initial == [True, True] and g.preds == [[], [0]] and g.final == [False, True]
    assert TargetGraph.chain([3, 3, 4]) == TargetGraph.from_slots([[[3]], [[3]], [[4]]])
    assert TargetGraph.chain([]).classes == []
    with pytest.raises(ValueError, match="slot 1"):  # 7 exits enter slot 1
        TargetGraph.from_slots([[[k] for k in range(1, 8)], [[9]]])
    with pytest.raises(ValueError, match="slot 0"):  # 7 finals
        TargetGraph.from_slots([[[k] for k in range(1, 8)]])
    assert sum(TargetGraph.from_slots([[[k] for k in range(1, 7)]]).final) == 6
    with pytest.raises(ValueError, match="slot 2"):  # 4 + 3 exits reach slot 2 through the optional slot 1
        TargetGraph.from_slots([[[1], [2], [3], [4]], [[], [5], [6], [7]], [[8]]])
    with pytest.raises(ValueError, match="skipped"):
        TargetGraph.from_slots([[[], [1]], [[2], []]])
    with pytest.raises(ValueError, match="slot 0"):
        TargetGraph.from_slots([[]])
    lexicon = {"the": [[1, 2], [1, 3]], "cat": [[4, 5, 6]]}
    assert TargetGraph.from_lexicon(["the", "cat"], lexicon) == TargetGraph.from_slots([lexicon["the"], lexicon["cat"]])
    with pytest.raises(ValueError, match="dog"):
        TargetGraph.from_lexicon(["dog"], lexicon)


def test_choices_and_the_python_surface():
    import allophant_amd
    from allophant_amd import estimator, graph_alignment, lib
    from allophant_amd.graph_alignment import GraphAlignment, TargetGraph, pack_graphs

    for name in ("TargetGraph", "GraphAlignment", "GraphAligned", "ctc_graph_align", "slot_targets"):
        assert getattr(allophant_amd, name) is getattr(graph_alignment, name) is getattr(estimator, name)
        assert name in allophant_amd.__all__
    assert hasattr(estimator.Estimator, "align_graph") and hasattr(estimator.Estimator, "align_graph_device")
    assert graph_alignment.ALIGN_GRAPH_MAX_NODES == lib.ALIGN_GRAPH_MAX_NODES == 4095 and lib.ALIGN_GRAPH_MAX_IN == 6
    graph = TargetGraph.from_slots([[[1, 2], [3]], [[4], []], [[5], [6, 7]]])
    empty_i, empty_f = torch.zeros(0, dtype=torch.int32), torch.zeros(0)

    def row(nodes):
        return GraphAlignment(empty_i, empty_f, nodes, [graph.classes[j] for j in nodes], torch.zeros(len(nodes), 2, dtype=torch.int32),
                              torch.zeros(len(nodes)), 0.0, graph)

    assert row([0, 1, 3, 4]).choices() == [0, 0, 0]
    assert row([2, 5, 6]).choices() == [1, 1, 1]  # the skipped slot reports its empty alternative
    assert row([2, 3, 4]).choices() == [1, 0, 0]
    packed, starts, counts = pack_graphs([graph, TargetGraph.chain([]), TargetGraph.chain([2, 2])])
    assert packed.dtype == torch.int32 and counts == [7, 0, 2]
    node_offsets, classes, flags, arc_offsets, arcs = (packed[a:b].tolist() for a, b in zip(starts, starts[1:] + [len(packed)]))
    assert node_offsets == [0, 7, 7, 9] and classes == graph.classes + [2, 2] and flags == [1, 0, 1, 0, 2, 0, 2, 1, 2]
    assert arc_offsets == [0, 0, 1, 1, 3, 6, 9, 10, 10, 11] and arcs == [0, 1, 2, 1, 2, 3, 1, 2, 3, 5, 0, 0]
    with pytest.raises(ValueError, match="4095"):
        pack_graphs([TargetGraph.chain([1] * 4096)])
    with pytest.raises(RuntimeError, match="no CPU"):
        graph_alignment.ctc_graph_align(torch.zeros(1, 4, 3), torch.tensor([4]), [TargetGraph.chain([1])])


def test_slot_targets_and_seconds():
    from allophant_amd import spec as S
    from allophant_amd.evaluation import EvaluationMaps
    from allophant_amd.graph_alignment import GraphAlignment, TargetGraph, slot_targets
    from allophant_amd.phonetic import AttributeTable

    names = ["syllabic", "long", "nasal", "phoneme"]
    table = AttributeTable(E.synthetic_table_text(), names)
    maps = EvaluationMaps(table, names, ["a", "t", "s", "m"], ["lg0"], split_complex=True)
    symbols = [[["a"], ["m"]], [["ts"], []], [["a"]]]
    slots = slot_targets(maps, "phoneme", symbols)
    assert slots == [[[1], [4]], [[2, 3], []], [[1]]]  # "ts" is split into "t", "s"; the empty alternative stays empty
    assert slot_targets(type("Holder", (), {"maps": maps})(), 3, symbols) == slots
    with pytest.raises(ValueError, match="slot 1, alternative 0.*'q'"):
        slot_targets(maps, "phoneme", [[["a"]], [["q"]]])
    graph = TargetGraph.from_slots(slots)
    assert graph.classes == [1, 4, 2, 3, 1] and graph.preds == [[], [], [0, 1], [2], [0, 1, 3]] and graph.skips == [None, 1, None]
    spans = torch.tensor([[0, 2], [5, 6]], dtype=torch.int32)
    row = GraphAlignment(torch.zeros(6, dtype=torch.int32), torch.zeros(6), [1, 4], [4, 1], spans, torch.zeros(2), 0.0, graph)
    assert row.choices() == [1, 1, 0]
    seconds = row.seconds(dict(S.tiny_encoder(2)))
    assert seconds.dtype == torch.float64 and seconds.flatten().tolist() == pytest.approx([0.0, 0.04, 0.1, 0.12], rel=1e-12)


def _library():
    from allophant_amd import lib

    if not os.path.exists(os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)):
        pytest.skip("library not built")
    return lib, lib.load()


def test_header_declares_the_exports_and_compiles_as_c99(tmp_path):
    from allophant_amd import lib

    with open(os.path.join(ROOT, "include", "allophant_amx_align_graph.h"), encoding="utf-8") as f:
        text = f.read()
    assert re.findall(r"^int (amx_\w+)\(", text, flags=re.M) == lib.ALIGN_GRAPH_EXPORTS
    defines = dict(re.findall(r"^#define (AMX_ALIGN_GRAPH_\w+) (\d+)", text, flags=re.M))
    assert defines == {"AMX_ALIGN_GRAPH_MAX_NODES": str(lib.ALIGN_GRAPH_MAX_NODES), "AMX_ALIGN_GRAPH_MAX_IN": str(lib.ALIGN_GRAPH_MAX_IN)}
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "align_graph.c"
    src.write_text('#include "allophant_amx_align_graph.h"\nint main(void) { size_t b; return amx_ctc_align_graph_workspace(1, 1, '
                   'AMX_ALIGN_GRAPH_MAX_NODES, &b)\n'
                   '    + amx_ctc_align_graph_emissions(0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)\n'
                   '    + amx_ctc_align_graph(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    done = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_exports_workspace_and_refusals():
    lib, handle = _library()
    for symbol in lib.ALIGN_GRAPH_EXPORTS:
        assert hasattr(handle, symbol)
    size = C.c_size_t()
    for rows, T, max_nodes in ((1216, 499, 100), (1, 1, 0), (3, 64, 31), (3, 65, 32), (2, 3000, 4095), (5, 0, 7), (0, 9, 9)):
        assert handle.amx_ctc_align_graph_workspace(rows, T, max_nodes, C.byref(size)) == lib.AMX_OK
        strips, frames = (2 * max_nodes + 1 + 63) // 64, (T + 63) // 64 * 64
        assert size.value == rows * strips * frames * 32, (rows, T, max_nodes)
    assert handle.amx_ctc_align_graph_workspace(1, 2 ** 31 - 1, 4095, C.byref(size)) == lib.AMX_OK
    for bad in ((1, 1, 4096), (1, 1, -1), (-1, 1, 1), (1, -1, 1), (1, 2 ** 31, 1), (2 ** 16, 2 ** 15, 1), (2 ** 40, 2 ** 40, 1)):
        assert handle.amx_ctc_align_graph_workspace(*bad, C.byref(size)) == lib.AMX_EINVAL, bad
    assert handle.amx_ctc_align_graph_workspace(1, 1, 1, None) == lib.AMX_EINVAL

    def call(N=2, T=8, Cn=5, blank=0, max_nodes=3, null=False, workspace_bytes=1 << 20):
        p = None if null else C.c_void_p(16)  # never dereferenced: every refused call returns before any device work
        return handle.amx_ctc_align_graph_emissions(0, p, T * Cn, Cn, p, N, T, Cn, blank, p, p, p, p, p, max_nodes, p,
                                                    workspace_bytes, p, p, p, p, p, p, None)

    assert call(Cn=1) == lib.AMX_EINVAL and call(Cn=0) == lib.AMX_EINVAL
    assert call(blank=-1) == lib.AMX_EINVAL and call(blank=5) == lib.AMX_EINVAL
    assert call(max_nodes=-1) == lib.AMX_EINVAL and call(max_nodes=4096) == lib.AMX_EINVAL
    assert b"4095" in handle.amx_last_error(None)
    assert call(N=-1) == lib.AMX_EINVAL and call(T=-1) == lib.AMX_EINVAL
    assert call(N=2 ** 16, T=2 ** 15) == lib.AMX_EINVAL
    assert b"2^31" in handle.amx_last_error(None)
    assert call(null=True) == lib.AMX_EINVAL
    assert call(workspace_bytes=2 * 64 * 32 - 1) == lib.AMX_EINVAL
    assert b"workspace" in handle.amx_last_error(None) and str(2 * 64 * 32).encode() in handle.amx_last_error(None)
    assert call(N=0, null=True) == lib.AMX_OK  # nothing to align
    # the handle form refuses a null handle before anything else
    assert handle.amx_ctc_align_graph(None, None, None, 1, 1, None, None, None, None, None, 0, None, 0, None, None, None, None,
                                      None, None, None) == lib.AMX_EINVAL

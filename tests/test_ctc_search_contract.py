"""The CTC search contract without a GPU: the literal restatement (tests/ctc_search_util.py) against its frame-at-a-time form
bit for bit and against a float64 brute force over every span and path on tiny dyadic rows, planted occurrences, the status
codes of the batch form, pick_hits, the C header, the exports and host-side refusals of the built library, the Python surface
and the kernels' listing."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ctc_search_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _dyadic(rng, T, Cn, minus_inf=0.0):
    """Multiples of 1/8 in [-2, 0] (fp32 and float64 sums are exact), a share of the entries -inf."""
    lp = (0.0 - rng.integers(0, 17, (T, Cn)) / 8.0).astype(np.float32)
    if minus_inf:
        lp[rng.random((T, Cn)) < minus_inf] = -np.inf
    return lp


def _query(rng, L, Cn, blank, repeat=0.3):
    classes = [c for c in range(Cn) if c != blank]
    out = []
    for _ in range(L):
        if out and (len(classes) == 1 or rng.random() < repeat):
            out.append(out[-1])
        else:
            out.append(int(rng.choice([c for c in classes if not out or c != out[-1]])))
    return out


def _same(a: U.Row, b: U.Row):
    assert a.status == b.status and a.best_span == b.best_span
    assert (a.best_score is None) == (b.best_score is None)
    if a.best_score is not None:
        assert np.float32(a.best_score).view(np.int32) == np.float32(b.best_score).view(np.int32)
    assert np.array_equal(a.end_scores.view(np.int32), b.end_scores.view(np.int32))
    assert np.array_equal(a.end_starts, b.end_starts)


def test_fast_restatement_equals_the_literal_one_bit_for_bit():
    rng = np.random.default_rng(0)
    cases = 0
    for T, Cn, L in ((0, 3, 2), (1, 2, 1), (5, 2, 3), (40, 5, 1), (40, 5, 2), (40, 5, 9), (150, 7, 33), (150, 7, 40), (90, 3, 30)):
        for kind in range(4):
            blank = int(rng.integers(0, Cn))
            if kind == 0:
                lp = np.log(rng.dirichlet(np.ones(Cn) * 0.3, T)).astype(np.float32).reshape(T, Cn)
            elif kind == 1:
                lp = _dyadic(rng, T, Cn)
            elif kind == 2:
                lp = _dyadic(rng, T, Cn, minus_inf=0.2)
                lp[T // 2:T // 2 + 1] = -np.inf  # a frame that is -inf in every class
            else:
                lp = U.plant(T, Cn, blank, [], filler=blank)
            y = _query(rng, L, Cn, blank)
            _same(U.search_row(lp, y, blank), U.search_row(lp, y, blank, fast=True))
            cases += 1
    assert cases == 36


def test_against_brute_force_on_tiny_dyadic_rows():
    """290 rows: C 2..4, T 1..7, L 1..3, any blank, about a third with -inf entries; y = [a, a] always among them.  The best
    score is equal exactly, the reported span is an optimal one with the latest end, every end_scores[t] equals the best over
    the spans ending at t and every end_starts[t] is an optimal start for that end."""
    rng = np.random.default_rng(1)
    none = repeats = with_inf = 0
    for k in range(290):
        Cn, T, L = int(rng.integers(2, 5)), int(rng.integers(1, 8)), int(rng.integers(1, 4))
        blank = int(rng.integers(0, Cn))
        lp = _dyadic(rng, T, Cn, minus_inf=0.25 if k % 3 == 0 else 0.0)
        with_inf += bool(np.isinf(lp).any())
        a = [c for c in range(Cn) if c != blank][0]
        y = [a, a] if k % 10 == 0 else _query(rng, L, Cn, blank)
        repeats += any(u == v for u, v in zip(y, y[1:]))
        row = U.search_row(lp, y, blank)
        best, starts = U.bruteforce(lp, y, blank)
        for t in range(T):
            assert float(row.end_scores[t]) == best[t], (k, t)
            if best[t] == -INF:
                assert row.end_starts[t] == -1
            else:
                assert int(row.end_starts[t]) in starts[t], (k, t)
        top = max(best)
        if top == -INF:
            assert row.status == -1 and row.best_span is None
            none += 1
            continue
        assert row.status == 0 and float(row.best_score) == top and float(row.best_score) <= 0.0
        last = max(t for t in range(T) if best[t] == top)
        assert row.best_span[1] == last + 1 and row.best_span[0] in starts[last], k
    assert none >= 30 and repeats >= 60 and with_inf >= 60, (none, repeats, with_inf)


def test_a_repeat_passes_through_a_blank():
    lp = U.plant(6, 3, 0, [(1, [1, 1, 1, 1])], filler=2)
    assert U.search_row(lp, [1, 1]).status == 0 and U.search_row(lp, [1, 1]).best_score < -20  # pays for a blank frame
    lp = U.plant(6, 3, 0, [(1, [1, 0, 0, 1])], filler=2)
    row = U.search_row(lp, [1, 1])
    assert row.best_score == 0.0 and row.best_span == (1, 5)
    assert U.search_row(lp[:2], [1, 1]).status == -1 and U.minimum_frames([1, 1]) == 3  # two frames cannot hold the blank


def test_planted_occurrences():
    """On sharp emissions a planted query returns score 0 and exactly the planted span (the first frame of the first symbol's
    run to the last frame of the last symbol's), and the later of two plantings wins."""
    blank, filler = 0, 5
    y = [1, 2, 2, 3]
    frames = [1, 1, 1, 0, 2, 2, 0, 2, 3, 3]  # runs, an optional blank, the blank between the repeats
    for fast in (False, True):
        lp = U.plant(40, 6, blank, [(7, frames)], filler)
        row = U.search_row(lp, y, blank, fast=fast)
        assert row.status == 0 and row.best_score == 0.0 and np.signbit(row.best_score) == False  # noqa: E712
        assert row.best_span == (7, 17)
        assert (row.end_scores[[14, 15, 16]] == 0.0).tolist() == [False, True, True] and row.end_starts[15] == 7
        lp = U.plant(40, 6, blank, [(2, frames), (25, frames)], filler)
        row = U.search_row(lp, y, blank, fast=fast)
        assert row.best_score == 0.0 and row.best_span == (25, 35) and row.end_starts[11] == 2 and row.end_scores[11] == 0.0
        # the runs of the first symbol directly before the occurrence belong to it; a blank before it does not
        lp = U.plant(40, 6, blank, [(5, [0, 0]), (7, frames), (17, [0, 0])], filler)
        assert U.search_row(lp, y, blank, fast=fast).best_span == (7, 17)
        # a frame that is -inf in every class, in the middle: the occurrence is not found across it
        lp = U.plant(40, 6, blank, [(7, frames)], filler)
        lp[11] = -np.inf
        row = U.search_row(lp, y, blank, fast=fast)
        assert row.status == 0 and row.best_score < -20 and not np.isnan(row.end_scores).any()
        assert U.search_row(np.full((9, 4), -np.inf, np.float32), [1], fast=fast).status == -1


def test_batch_form_status():
    em = np.full((3, 6, 4), -1.0, np.float32)
    em[0, :, 2] = -np.inf
    offsets, ids = U.pack_queries([[1], [2, 2], [1, 2, 3, 1, 2, 3, 1]])
    rows = U.search_batch(em, [6, 2, 0], offsets, ids, max_query=7)
    assert [r.status for r in rows] == [0, -1, -1, 0, -1, -1, -1, -1, -1]  # -inf on every path; too few frames; no frames
    assert rows[1].end_scores.tolist() == [-INF] * 6 and rows[1].end_starts.tolist() == [-1] * 6
    assert rows[6].end_scores.shape == (0,)
    # malformed: L > max_query, an empty query, descending offsets, offsets past offsets[Q], frame lengths outside [0, T]
    assert [r.status for r in U.search_batch(em, [6, 7, -1], offsets, ids, max_query=6)] == [0, -1, -2, -2, -2, -2, -2, -2, -2]
    assert [r.status for r in U.search_batch(em[1:2], [6], [0, 0, 3, 2, 11, 10], list(range(1, 4)) * 4, 7)] == [-2, 0, -2, -2, -2]
    for bad in ([0], [4], [-1], [1, 0, 1]):
        assert U.search_row(em[1], bad).status == -2
    assert U.search_row(em[1], [1], blank=1).status == -2 and U.search_row(em[1], []).status == -2
    want = U.expected_buffers(em, [6, 2, 0], offsets, ids, 7, 0, -77, -5.5)
    assert want[2].tolist() == [0, -1, -1, 0, -1, -1, -1, -1, -1]
    assert want[0].tolist()[1] == -5.5 and want[1][1].tolist() == [-77, -77] and want[3][1].tolist() == [-INF] * 6
    assert want[3][3].tolist() == [-0.0] * 2 + [-5.5] * 4 and want[4][6].tolist() == [-77] * 6


def test_pick_hits():
    from allophant_amd.search import Hit, pick_hits

    scores = np.array([-INF, -1.0, -0.5, -3.0, -0.5, -2.0, -0.25, -INF], np.float32)
    starts = np.array([-1, 0, 1, 1, 3, 5, 4, -1], np.int32)
    # -0.25 first, [4, 7); then the two -0.5: the later end (frame 4, [3, 5)) overlaps, frame 2 ([1, 3)) does not
    assert pick_hits(scores, starts, 8, -0.5) == [Hit(1, 3, -0.5), Hit(4, 7, -0.25)]
    assert pick_hits(scores, starts, 8, -0.5, max_hits=1) == [Hit(4, 7, -0.25)]
    assert pick_hits(scores, starts, 8, -0.1) == [] and pick_hits(scores, starts, 0, -9.0) == []
    assert pick_hits(scores, starts, 8, -INF) == [Hit(1, 3, -0.5), Hit(4, 7, -0.25)]  # -inf frames are never candidates
    assert pick_hits(scores, starts, 6, -9.0) == [Hit(1, 3, -0.5), Hit(3, 5, -0.5), Hit(5, 6, -2.0)]  # only `length` frames
    # equal scores: the later end first
    tie = np.zeros(4, np.float32)
    assert pick_hits(tie, np.array([0, 0, 2, 2]), 4, 0.0) == [Hit(0, 2, 0.0), Hit(2, 4, 0.0)]
    assert pick_hits(torch.from_numpy(tie), torch.tensor([0, 0, 2, 2]), 4, 0.0, max_hits=1) == [Hit(2, 4, 0.0)]
    # on the restatement's curves: two plantings, both found
    frames = [1, 1, 2, 3]
    lp = U.plant(30, 5, 0, [(3, frames), (20, frames)], filler=4)
    row = U.search_row(lp, [1, 2, 3], fast=True)
    assert pick_hits(row.end_scores, row.end_starts, 30, 0.0) == [Hit(3, 7, 0.0), Hit(20, 24, 0.0)]


def _library():
    from allophant_amd import lib

    if not os.path.exists(os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)):
        pytest.skip("library not built")
    return lib, lib.load()


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "search.c"
    src.write_text('#include "allophant_amx_search.h"\nint main(void) { size_t b; return amx_ctc_search_workspace(1, 1, 1, AMX_SEARCH_MAX_QUERY, &b)\n'
                   '    + amx_ctc_search_emissions(0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    done = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_header_prototypes_are_the_exports():
    from allophant_amd import lib

    with open(os.path.join(ROOT, "include", "allophant_amx_search.h"), encoding="utf-8") as f:
        text = f.read()
    assert re.findall(r"^int (amx_\w+)\(", text, flags=re.M) == lib.SEARCH_EXPORTS
    assert int(re.search(r"#define AMX_SEARCH_MAX_QUERY (\d+)", text).group(1)) == lib.SEARCH_MAX_QUERY == 256


def test_exports_workspace_and_refusals():
    lib, handle = _library()
    for symbol in lib.SEARCH_EXPORTS:
        assert hasattr(handle, symbol)
    size = C.c_size_t()
    for N, Q, T, max_query in ((32, 1024, 499, 12), (1, 1, 1, 1), (3, 9, 64, 256), (1, 8, 2999, 256), (5, 7, 0, 7), (0, 9, 9, 9),
                               (4, 0, 2 ** 40, 3), (1, 1, 2 ** 31 - 1, 256)):
        assert handle.amx_ctc_search_workspace(N, Q, T, max_query, C.byref(size)) == lib.AMX_OK, (N, Q, T)
        assert size.value == N * T * 4, (N, Q, T)  # the frame maxima, nothing per row
    for bad in ((1, 1, 1, 0), (1, 1, 1, 257), (1, 1, 1, -1), (-1, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 2 ** 31, 1),
                (2 ** 10, 2 ** 6, 2 ** 15, 1), (2 ** 40, 2 ** 40, 2 ** 40, 1), (2 ** 16, 2 ** 15, 0, 1)):
        assert handle.amx_ctc_search_workspace(*bad, C.byref(size)) == lib.AMX_EINVAL, bad
    assert handle.amx_ctc_search_workspace(1, 1, 1, 1, None) == lib.AMX_EINVAL

    def call(N=2, T=8, Cn=5, blank=0, Q=3, max_query=3, null=False, curves=(True, True), workspace_bytes=1 << 20):
        p = None if null else C.c_void_p(16)  # never dereferenced: every refused call returns before any device work
        return handle.amx_ctc_search_emissions(0, p, T * Cn, Cn, p, N, T, Cn, blank, p, p, Q, max_query, p, workspace_bytes, p, p, p,
                                               p if curves[0] else None, p if curves[1] else None, None)

    assert call(Cn=1) == lib.AMX_EINVAL and call(Cn=0) == lib.AMX_EINVAL
    assert b"classes" in handle.amx_last_error(None)
    assert call(blank=-1) == lib.AMX_EINVAL and call(blank=5) == lib.AMX_EINVAL
    assert b"blank" in handle.amx_last_error(None)
    assert call(max_query=0) == lib.AMX_EINVAL and call(max_query=257) == lib.AMX_EINVAL
    assert b"max_query" in handle.amx_last_error(None)
    assert call(N=-1) == lib.AMX_EINVAL and call(T=-1) == lib.AMX_EINVAL and call(Q=-1) == lib.AMX_EINVAL
    assert call(N=2 ** 10, Q=2 ** 6, T=2 ** 15) == lib.AMX_EINVAL
    assert b"2^31" in handle.amx_last_error(None)
    assert call(curves=(True, False)) == lib.AMX_EINVAL and call(curves=(False, True)) == lib.AMX_EINVAL
    assert b"both" in handle.amx_last_error(None)
    assert call(null=True, curves=(False, False)) == lib.AMX_EINVAL
    assert b"null" in handle.amx_last_error(None)
    assert call(workspace_bytes=2 * 8 * 4 - 1) == lib.AMX_EINVAL
    assert b"workspace" in handle.amx_last_error(None)
    assert call(N=0, null=True, curves=(False, False)) == lib.AMX_OK and call(Q=0, null=True, curves=(False, False)) == lib.AMX_OK


def test_python_surface_without_a_gpu():
    import allophant_amd
    from allophant_amd import estimator, search

    for name in ("Found", "Hit", "ctc_search", "pick_hits", "query_targets"):
        assert getattr(allophant_amd, name) is getattr(search, name) is getattr(estimator, name)
        assert name in allophant_amd.__all__
    for method in ("search", "search_device"):
        assert hasattr(estimator.Estimator, method)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        search.ctc_search(torch.zeros(1, 4, 3), torch.tensor([4]), [[1]])
    with pytest.raises(ValueError):
        search.ctc_search(torch.zeros(4, 3), torch.tensor([4]), [[1]])
    offsets, ids = search.pack_queries([[1, 2], [3], [4, 4]], 5, 0)
    assert offsets.tolist() == [0, 2, 3, 5] and ids.tolist() == [1, 2, 3, 4, 4] and offsets.dtype == ids.dtype == torch.int32
    for bad, match in (([[1], []], "query 1"), ([[1] * 257], "256"), ([[1], [2], [0]], "query 2"), ([[5]], "query 0"), ([[-1]], "query 0")):
        with pytest.raises(ValueError, match=match):
            search.pack_queries(bad, 5, 0)


def test_host_forms():
    """Found.best(), hits() and seconds() on hand-made (CPU) buffers."""
    from allophant_amd import spec as S
    from allophant_amd.search import Found, Hit

    scores = torch.tensor([[-0.5, 9.0], [0.0, -2.0]])
    spans = torch.tensor([[[1, 3], [9, 9]], [[0, 4], [2, 3]]], dtype=torch.int32)
    status = torch.tensor([[0, -1], [0, 0]], dtype=torch.int32)
    found = Found(scores, spans, status, None, None, [4, 4])
    assert found.best() == [[Hit(1, 3, -0.5), None], [Hit(0, 4, 0.0), Hit(2, 3, -2.0)]]
    with pytest.raises(ValueError, match="curves"):
        found.hits(-1.0)
    with pytest.raises(ValueError, match="utterance 1, query 0"):
        found._replace(status=torch.tensor([[0, -1], [-2, 0]], dtype=torch.int32)).best()
    end_scores = torch.tensor([[[-INF, -1.0, -0.5, -0.5], [-INF] * 4], [[-3.0, -3.0, -3.0, 0.0], [-INF, -INF, -2.0, 7.0]]])
    end_starts = torch.tensor([[[-1, 0, 1, 3], [-1] * 4], [[0, 0, 0, 0], [-1, -1, 2, 7]]], dtype=torch.int32)
    curved = found._replace(end_scores=end_scores, end_starts=end_starts, lengths=[4, 3])
    assert curved.hits(-0.5) == [[[Hit(1, 3, -0.5), Hit(3, 4, -0.5)], []], [[], []]]  # utterance 1 has three frames
    assert curved.hits(-5.0, max_hits=1) == [[[Hit(3, 4, -0.5)], []], [[Hit(0, 3, -3.0)], [Hit(2, 3, -2.0)]]]
    spec = dict(S.tiny_encoder(2))
    seconds = found.seconds(spec)
    assert seconds.dtype == torch.float64 and seconds.shape == (2, 2, 2)
    assert seconds[0, 0].tolist() == pytest.approx(list(Hit(1, 3, -0.5).seconds(spec)), rel=1e-12)
    assert found.seconds(spec, sample_rate=8000)[0, 0, 1] == pytest.approx(2 * float(seconds[0, 0, 1]), rel=1e-12)


def test_query_targets():
    import edit_util as E
    from allophant_amd.alignment import label_targets
    from allophant_amd.evaluation import EvaluationMaps
    from allophant_amd.phonetic import AttributeTable
    from allophant_amd.search import query_targets

    table = AttributeTable(E.synthetic_table_text(), ["syllabic", "long", "nasal", "phoneme"])
    names = ["syllabic", "long", "nasal", "phoneme"]
    inventory = ["a", "ts", "t͡ʃ", "é", "m", "aː", "i"]
    maps = EvaluationMaps(table, names, inventory, ["lg0"])
    queries = [["a", "m", "i"], ["ts", "aː"], ["é"]]
    for name in names:
        assert query_targets(maps, queries, name) == label_targets(maps, queries)[name]
    assert all(v >= 1 for row in query_targets(maps, queries, "phoneme") for v in row)
    with pytest.raises(ValueError, match="nope"):
        query_targets(maps, queries, "nope")
    outside = next(p for p in table.full_phonemes if p not in inventory)
    with pytest.raises(ValueError, match="query 1") as caught:
        query_targets(maps, [["a"], [outside]], "phoneme")
    assert repr(outside) in str(caught.value)


def test_kernels_have_no_scratch_and_no_vgpr_spills(tmp_path):
    """amx_ctc_search.hip compiled for gfx950 (device ISA, -S): the pre-pass and the search kernel
    have a private segment of 0 bytes and spill no VGPR, use no LDS, and the source is plain HIP without inline assembly."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    source = os.path.join(ROOT, "allophant_amd", "csrc", "amx_ctc_search.hip")
    out = tmp_path / "amx_ctc_search.s"
    done = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(out), source],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    isa = out.read_text()
    kernels = re.findall(r"\.name:\s+(\S*ctc_search\S*kernel\S*)", isa)
    assert len(kernels) == 2, kernels
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa)]
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", isa)]
    assert private == [0] * 2 and spills == [0] * 2 and lds == [0] * 2, (private, spills, lds)
    with open(source, encoding="utf-8") as f:
        text = f.read()
    assert "asm" not in text and "__syncthreads" not in text and "atomic" not in text.lower().replace("no atomic", "")

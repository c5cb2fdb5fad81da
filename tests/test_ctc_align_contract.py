"""The CTC forced-alignment contract without a GPU: the restatement (tests/ctc_align_util.py) against brute-force
enumeration of every CTC path, the tie rule, hand-worked rows, the C header, the exports and host-side refusals of the built
library, the kernels' listing, label_targets and Alignment.seconds."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ctc_align_util as U
import edit_util as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _random_row(rng, values=None):
    T, L, Cn = int(rng.integers(1, 8)), int(rng.integers(0, 4)), int(rng.integers(2, 5))
    if values is None:
        lp = np.log(rng.dirichlet(np.ones(Cn), T)).astype(np.float32)
    else:
        lp = rng.choice(np.asarray(values, np.float32), (T, Cn))
    return lp, rng.integers(1, Cn, L).tolist()


def test_restatement_against_brute_force():
    """Random rows (T <= 7, L <= 3, C <= 4): the total agrees to 1e-4, the path is equal where the optimum is unique, and a
    row brute force finds no path for is refused with -1."""
    rng = np.random.default_rng(2024)
    unique = infeasible = 0
    for _ in range(400):
        lp, y = _random_row(rng)
        row = U.align_row(lp, y)
        best, paths = U.best_paths_bruteforce(lp, y)
        if not paths:
            assert row.status == -1 and lp.shape[0] < U.minimum_frames(y)
            infeasible += 1
            continue
        assert row.status == 0 and abs(float(row.total) - best) <= 1e-4
        assert U.collapse(row.paths.tolist(), 0) == y
        if len(paths) == 1:
            assert tuple(row.paths.tolist()) == paths[0]
            unique += 1
    assert unique > 200 and infeasible > 10


def test_frame_at_a_time_sweep_equals_the_literal_one():
    """The vectorised sweep the GPU tests use for long rows gives the literal restatement's outputs bit for bit: random,
    tie-heavy and -inf-ridden rows with repeats, up to 70 states."""
    rng = np.random.default_rng(5)
    for k in range(120):
        T, L, Cn = int(rng.integers(1, 60)), int(rng.integers(0, 35)), int(rng.integers(2, 6))
        if k % 3 == 0:
            lp = rng.choice(np.asarray((-0.25, -0.5, -0.75), np.float32), (T, Cn))
        else:
            lp = np.log(rng.dirichlet(np.ones(Cn), T)).astype(np.float32)
        if k % 4 == 0:
            lp[rng.random((T, Cn)) < 0.15] = -INF
        y = rng.integers(1, Cn, L).tolist()
        slow, fast = U.align_row(lp, y), U.align_row(lp, y, fast=True)
        assert slow.status == fast.status
        if slow.status == 0:
            for a, b in zip(slow[1:], fast[1:]):
                a, b = np.asarray(a), np.asarray(b)
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _tie_rule_path(lp, y, blank=0):
    """The path the tie rule selects, written independently of the restatement's loop: a float64 table of exact values (the
    tie-heavy emissions are multiples of 0.25, so every sum is exact) walked back preferring the smaller move."""
    T = lp.shape[0]
    S = 2 * len(y) + 1
    label = [blank if i % 2 == 0 else y[i // 2] for i in range(S)]
    a = np.full((T, S), -INF)
    a[0, 0] = lp[0, blank]
    if S > 1:
        a[0, 1] = lp[0, y[0]]

    def moves(i):
        allowed = [0] + ([1] if i >= 1 else [])
        if i % 2 == 1 and i >= 3 and y[i // 2] != y[i // 2 - 1]:
            allowed.append(2)
        return allowed

    for t in range(1, T):
        for i in range(S):
            a[t, i] = max(a[t - 1, i - m] for m in moves(i)) + lp[t, label[i]]
    e = S - 1 if (S == 1 or a[T - 1, S - 1] > a[T - 1, S - 2]) else S - 2
    total, path = a[T - 1, e], []
    for t in range(T - 1, -1, -1):
        path.append(label[e])
        if t:
            best = max(a[t - 1, e - m] for m in moves(e))
            e -= min(m for m in moves(e) if a[t - 1, e - m] == best)
    return total, tuple(reversed(path))


def test_tie_heavy_rows_follow_the_tie_rule():
    """Emissions from {-0.25, -0.5, -0.75}: the total equals the brute-force optimum exactly, and the path is among the
    optimal ones and is the one the tie rule selects."""
    rng = np.random.default_rng(7)
    tied = 0
    for _ in range(300):
        lp, y = _random_row(rng, values=(-0.25, -0.5, -0.75))
        row = U.align_row(lp, y)
        best, paths = U.best_paths_bruteforce(lp, y)
        if not paths:
            assert row.status == -1
            continue
        assert float(row.total) == best
        assert tuple(row.paths.tolist()) in paths
        assert (best, tuple(row.paths.tolist())) == _tie_rule_path(lp, y)
        tied += len(paths) > 1
    assert tied > 50  # (a guard on the generator: several paths tie for the optimum on a good share of the rows)


def test_hand_worked_tie_between_the_step_and_the_skip():
    """x1 == x2 > x0 at state 3 (the second target) in frame 2: the smaller move, 1, wins, so the path passes through the
    blank between the targets; taking x0 instead would not even be a maximum."""
    # classes (blank, a, b), targets "a b": states 0 blank, 1 a, 2 blank, 3 b, 4 blank
    lp = np.array([[-0.5, -0.25, -0.75],    # a[0] = [-0.5, -0.25, -inf, -inf, -inf]
                   [-0.25, -0.25, -0.75],   # a[1] = [-0.75, -0.5, -0.5, -1.0, -inf]
                   [-0.75, -0.75, -0.25]],  # state 3: x0 = -1.0, x1 = a[1][2] = -0.5, x2 = a[1][1] = -0.5
                  np.float32)
    row = U.align_row(lp, [1, 2])
    assert row.status == 0
    assert row.states.tolist() == [1, 2, 3] and row.paths.tolist() == [1, 0, 2]
    assert float(row.total) == -0.25 - 0.25 - 0.25
    best, paths = U.best_paths_bruteforce(lp, [1, 2])
    assert best == -0.75 and set(paths) == {(1, 0, 2), (1, 1, 2)}
    assert row.spans.tolist() == [[0, 1], [2, 3]] and row.span_scores.tolist() == [-0.25, -0.25]


def _uniform(T, Cn, value=-1.0):
    return np.full((T, Cn), value, np.float32)


def test_hand_worked_rows():
    # L = 0: every frame is blank
    row = U.align_row(np.array([[-1.0, -2.0], [-0.5, -3.0]], np.float32), [])
    assert row.status == 0 and row.paths.tolist() == [0, 0] and float(row.total) == -1.5 and row.spans.shape == (0, 2)
    empty = U.align_row(np.zeros((0, 3), np.float32), [])
    assert empty.status == 0 and float(empty.total) == 0.0 and empty.paths.shape == (0,)
    assert U.align_row(np.zeros((0, 3), np.float32), [1]).status == -1
    # a repeated target needs a blank between: three frames, one path
    row = U.align_row(_uniform(3, 2), [1, 1])
    assert row.status == 0 and row.paths.tolist() == [1, 0, 1] and row.spans.tolist() == [[0, 1], [2, 3]]
    assert U.align_row(_uniform(2, 2), [1, 1]).status == -1  # one frame below the minimum
    # T equal to the minimum for distinct targets: a single path; one below: none
    lp = np.log(np.random.default_rng(3).dirichlet(np.ones(4), 3)).astype(np.float32)
    row = U.align_row(lp, [3, 1, 2])
    assert row.paths.tolist() == [3, 1, 2] and row.spans.tolist() == [[0, 1], [1, 2], [2, 3]]
    assert float(row.total) == float(np.float32(np.float32(lp[0, 3] + lp[1, 1]) + lp[2, 2]))
    assert row.span_scores.tolist() == [float(lp[0, 3]), float(lp[1, 1]), float(lp[2, 2])]
    assert U.align_row(lp[:2], [3, 1, 2]).status == -1
    # a -inf column forces a detour: class 1 may only be taken in frame 2, whatever it scores elsewhere
    lp = np.array([[-3.0, -INF], [-3.0, -INF], [-3.0, -0.1], [-3.0, -INF]], np.float32)
    row = U.align_row(lp, [1])
    assert row.paths.tolist() == [0, 0, 1, 0] and row.spans.tolist() == [[2, 3]]
    assert row.total == np.float32(np.float32(np.float32(-6.0) + np.float32(-0.1)) + np.float32(-3.0))
    # all -inf
    assert U.align_row(np.full((4, 3), -INF, np.float32), [1]).status == -1
    assert U.align_row(np.full((4, 3), -INF, np.float32), []).status == -1
    # malformed targets
    assert U.align_row(_uniform(4, 3), [0]).status == -2 and U.align_row(_uniform(4, 3), [3]).status == -2
    assert U.align_row(_uniform(4, 3), [-1]).status == -2 and U.align_row(_uniform(4, 3), [1], blank=1).status == -2
    # span sums are added in frame order, in fp32
    lp = np.array([[-INF, 1e8], [-INF, 1.0], [-INF, -1e8]], np.float32)
    row = U.align_row(lp, [1])
    assert row.spans.tolist() == [[0, 3]] and row.span_scores.tolist() == [0.0]  # (1e8 + 1) - 1e8 in fp32


def test_batch_form_refuses_bad_rows():
    em = np.stack([_uniform(5, 3)] * 4)
    rows = U.align_batch(em, [5, 6, 5, -1], [0, 2, 1, 3, 4], [1, 2, 1, 2], max_target=1)
    assert [r.status for r in rows] == [-2, -2, -2, -2]  # L > max_target, length > T, descending offsets, length < 0
    rows = U.align_batch(em, [5, 5, 5, 0], [0, 1, 1, 3, 4], [1, 2, 1, 2], max_target=2)
    assert [r.status for r in rows] == [0, 0, 0, -1]


def _library():
    from allophant_amd import lib

    if not os.path.exists(os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)):
        pytest.skip("library not built")
    return lib, lib.load()


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "align.c"
    src.write_text('#include "allophant_amx_align.h"\nint main(void) { size_t b; return amx_ctc_align_workspace(1, 1, AMX_ALIGN_MAX_TARGET, &b)\n'
                   '    + amx_ctc_align_emissions(0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)\n'
                   '    + amx_ctc_align(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    done = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_exports_workspace_and_refusals():
    lib, handle = _library()
    for symbol in ("amx_ctc_align_workspace", "amx_ctc_align_emissions", "amx_ctc_align"):
        assert symbol in lib.ALIGN_EXPORTS and hasattr(handle, symbol)
    assert lib.ALIGN_MAX_TARGET == 4095
    size = C.c_size_t()
    for rows, T, max_target in ((1216, 499, 100), (1, 1, 0), (3, 64, 31), (3, 65, 32), (2, 3000, 4095), (5, 0, 7), (0, 9, 9)):
        assert handle.amx_ctc_align_workspace(rows, T, max_target, C.byref(size)) == lib.AMX_OK
        strips, frames = (2 * max_target + 1 + 63) // 64, (T + 63) // 64 * 64
        assert size.value == rows * strips * frames * 16, (rows, T, max_target)
    assert handle.amx_ctc_align_workspace(1, 2 ** 31 - 1, 4095, C.byref(size)) == lib.AMX_OK
    for bad in ((1, 1, 4096), (1, 1, -1), (-1, 1, 1), (1, -1, 1), (1, 2 ** 31, 1), (2 ** 16, 2 ** 15, 1), (2 ** 40, 2 ** 40, 1)):
        assert handle.amx_ctc_align_workspace(*bad, C.byref(size)) == lib.AMX_EINVAL, bad
    assert handle.amx_ctc_align_workspace(1, 1, 1, None) == lib.AMX_EINVAL

    def call(N=2, T=8, Cn=5, blank=0, max_target=3, null=False, workspace_bytes=1 << 20):
        p = None if null else C.c_void_p(16)  # never dereferenced: every refused call returns before any device work
        return handle.amx_ctc_align_emissions(0, p, T * Cn, Cn, p, N, T, Cn, blank, p, p, max_target, p, workspace_bytes,
                                              p, p, p, p, p, p, None)

    assert call(Cn=1) == lib.AMX_EINVAL and call(Cn=0) == lib.AMX_EINVAL
    assert call(blank=-1) == lib.AMX_EINVAL and call(blank=5) == lib.AMX_EINVAL
    assert call(max_target=-1) == lib.AMX_EINVAL and call(max_target=4096) == lib.AMX_EINVAL
    assert call(N=-1) == lib.AMX_EINVAL and call(T=-1) == lib.AMX_EINVAL
    assert call(N=2 ** 16, T=2 ** 15) == lib.AMX_EINVAL
    assert b"2^31" in handle.amx_last_error(None)
    assert call(null=True) == lib.AMX_EINVAL
    assert call(workspace_bytes=2 * 64 * 16 - 1) == lib.AMX_EINVAL
    assert b"workspace" in handle.amx_last_error(None)
    assert call(N=0, null=True) == lib.AMX_OK  # nothing to align
    # the handle form refuses a null handle before anything else
    assert handle.amx_ctc_align(None, None, None, 1, 1, None, None, 0, None, 0, None, None, None, None, None, None,
                                None) == lib.AMX_EINVAL


def test_python_surface_without_a_gpu():
    import allophant_amd
    from allophant_amd import alignment, estimator

    for name in ("Alignment", "Aligned", "ctc_forced_align", "label_targets"):
        assert getattr(allophant_amd, name) is getattr(alignment, name) is getattr(estimator, name)
        assert name in allophant_amd.__all__
    assert hasattr(estimator.Estimator, "align") and hasattr(estimator.Estimator, "align_device")
    with pytest.raises(RuntimeError, match="no CPU"):
        alignment.ctc_forced_align(torch.zeros(1, 4, 3), torch.tensor([4]), [[1]])
    with pytest.raises(ValueError):
        alignment.ctc_forced_align(torch.zeros(4, 3), torch.tensor([4]), [[1]])
    with pytest.raises(ValueError, match="4095"):
        alignment.pack_targets([[1] * 4096])
    offsets, ids, counts = alignment.pack_targets([[1, 2], [], [3]])
    assert offsets.tolist() == [0, 2, 2, 3] and ids.tolist() == [1, 2, 3] and counts == [2, 0, 1]
    assert offsets.dtype == ids.dtype == torch.int32


def test_kernels_have_no_scratch_and_no_vgpr_spills(tmp_path):
    """amx_ctc_align.hip compiled for gfx950 (device ISA, -S): every instantiation of the kernel has a private segment of 0
    bytes and spills no VGPR, and the source is plain HIP without inline assembly."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    source = os.path.join(ROOT, "allophant_amd", "csrc", "amx_ctc_align.hip")
    out = tmp_path / "amx_ctc_align.s"
    done = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(out), source],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    isa = out.read_text()
    kernels = re.findall(r"\.name:\s+(\S*ctc_align_kernel\S*)", isa)
    assert len(kernels) == 4, kernels
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa)]
    assert private == [0] * 4 and spills == [0] * 4, (private, spills)
    with open(source, encoding="utf-8") as f:
        text = f.read()
    assert "asm" not in text


def _maps(inventory, **options):
    from allophant_amd.evaluation import EvaluationMaps
    from allophant_amd.phonetic import AttributeTable

    table = AttributeTable(E.synthetic_table_text(), ["syllabic", "long", "nasal", "phoneme"])
    names = ["syllabic", "long", "nasal", "phoneme"]
    return table, names, EvaluationMaps(table, names, inventory, ["lg0", "lg1"], **options)


def test_label_targets_round_trips_with_hypothesis_symbols():
    from allophant_amd.alignment import label_targets
    from allophant_amd.estimator import CTCHypothesis
    from allophant_amd.phonetic import hypothesis_symbols

    inventory = ["a", "ts", "t͡ʃ", "é", "m", "aː", "i"]
    table, names, maps = _maps(inventory)
    labels = [["a", "ts", "m"], [], ["aː", "t͡ʃ", "i", "é", "aː"]]
    targets = label_targets(maps, labels, ["lg0", "lg1", "lg0"])
    assert list(targets) == names
    decoded = {name: [[CTCHypothesis(torch.tensor(row, dtype=torch.int64), [], 0.0, torch.zeros(len(row), dtype=torch.int64))]
                      for row in rows] for name, rows in targets.items()}
    symbols = hypothesis_symbols(decoded, inventory, table)
    for o, name in enumerate(names):
        for n, label in enumerate(labels):
            assert symbols[name][n][0] == maps.expand_label(o, label), (name, n)
    # contours expand as expand_label does: "aː" is "-,+" in `long`, "ts" is "-,0" in `nasal`
    long_classes = table.feature_categories("long")
    assert targets["long"][2][:2] == [long_classes.index("-") + 1, long_classes.index("+") + 1]
    assert len(targets["nasal"][0]) == 4 and len(targets["phoneme"][0]) == 3
    assert targets["phoneme"][0] == [1, 2, 5] and targets["phoneme"][1] == []
    # the same through an object holding the maps (an Evaluator)
    holder = type("Holder", (), {"maps": maps})()
    assert label_targets(holder, labels) == targets


def test_label_targets_split_segments_and_refusals():
    from allophant_amd.alignment import label_targets

    table, names, maps = _maps(["a", "t", "s", "m"], split_complex=True)
    targets = label_targets(maps, [["ts", "a"]])
    assert targets["phoneme"] == [[2, 3, 1]]  # "ts" is split into "t", "s"
    table, names, maps = _maps(["a", "t", "m"])
    with pytest.raises(ValueError, match="'phoneme'.*'s'"):
        label_targets(maps, [["a", "s"]])
    with pytest.raises(ValueError, match="lg9"):
        label_targets(maps, [["a"]], ["lg9"])
    with pytest.raises(ValueError, match="'q'"):
        label_targets(maps, [["q"]])


def test_alignment_seconds_follow_the_conv_strides():
    from allophant_amd import spec as S
    from allophant_amd.alignment import Alignment, frame_stride

    spans = torch.tensor([[0, 3], [5, 6]], dtype=torch.int32)
    row = Alignment(torch.zeros(6, dtype=torch.int32), torch.zeros(6), spans, torch.zeros(2), 0.0)
    spec = dict(S.tiny_encoder(2))
    assert frame_stride(spec) == 320
    assert row.seconds(spec).flatten().tolist() == pytest.approx([0.0, 0.06, 0.1, 0.12], rel=1e-12)
    spec["conv_stride"] = [4, 3, 2]
    assert frame_stride(spec) == 24
    assert row.seconds(spec, sample_rate=8000).flatten().tolist() == pytest.approx([0.0, 0.009, 0.015, 0.018], rel=1e-12)
    assert row.seconds(spec, sample_rate=8000).shape == (2, 2)

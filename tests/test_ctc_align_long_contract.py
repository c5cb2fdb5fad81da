"""The long form of the CTC forced alignment (amx_ctc_align_long.hip) without a GPU: exports, limits and the workspace formula
of the built library, the refusals of its entry points, pack_targets' limit, alignment.segments, the numpy emulation of the
tiled sweep (tests/ctc_align_long_util.py) against the restatement -- equal with the halo of twice the frame block, different
with one strip less -- and the kernels' listing."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ctc_align_long_util as LU
import ctc_align_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _library():
    from allophant_amd import lib

    if not os.path.exists(os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)):
        pytest.skip("library not built")
    return lib, lib.load()


def _formula(rows, T, max_target):
    """The layout include/allophant_amx_align.h states: moves, two state rows, span bounds, live flags."""
    strips, frames = (2 * max_target + 1 + 63) // 64, (T + 63) // 64 * 64
    round16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    return rows * strips * frames * 16 + rows * 2 * strips * 64 * 4 + round16(rows * max_target * 2 * 4) + round16(rows * 4)


def test_header_declares_the_long_form_and_compiles_as_c99(tmp_path):
    from allophant_amd import lib

    with open(os.path.join(ROOT, "include", "allophant_amx_align.h"), encoding="utf-8") as f:
        text = f.read()
    assert re.findall(r"^int (amx_\w+)\(", text, flags=re.M) == lib.ALIGN_EXPORTS + lib.ALIGN_LONG_EXPORTS
    defines = dict(re.findall(r"^#define (AMX_ALIGN_\w+) (\d+)", text, flags=re.M))
    assert defines == {"AMX_ALIGN_MAX_TARGET": "4095", "AMX_ALIGN_LONG_MAX_TARGET": str(lib.ALIGN_LONG_MAX_TARGET),
                       "AMX_ALIGN_LONG_FRAME_BLOCK": str(lib.ALIGN_LONG_FRAME_BLOCK),
                       "AMX_ALIGN_LONG_TILE_STATES": str(lib.ALIGN_LONG_TILE_STATES)}
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "align_long.c"
    src.write_text('#include "allophant_amx_align.h"\nint main(void) { size_t b; return amx_ctc_align_long_workspace(1, 1, '
                   'AMX_ALIGN_LONG_MAX_TARGET, &b)\n'
                   '    + amx_ctc_align_long_emissions(0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)\n'
                   '    + amx_ctc_align_long(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    done = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_exports_workspace_and_refusals():
    lib, handle = _library()
    for symbol in ("amx_ctc_align_long_workspace", "amx_ctc_align_long_emissions", "amx_ctc_align_long"):
        assert symbol in lib.ALIGN_LONG_EXPORTS and hasattr(handle, symbol)
    assert lib.ALIGN_LONG_MAX_TARGET == 262143 and lib.ALIGN_MAX_TARGET == 4095
    assert lib.ALIGN_LONG_FRAME_BLOCK == 64 and lib.ALIGN_LONG_TILE_STATES % 64 == 0
    size = C.c_size_t()
    for shape in ((1216, 499, 100), (1, 1, 0), (3, 64, 31), (3, 65, 32), (2, 3000, 4095), (2, 12000, 5000), (5, 0, 7), (0, 9, 9),
                  (1, 180000, 40000), (1, 2 ** 20, 262143)):
        assert handle.amx_ctc_align_long_workspace(*shape, C.byref(size)) == lib.AMX_OK
        assert size.value == _formula(*shape), shape
    assert handle.amx_ctc_align_long_workspace(1, 2 ** 31 - 1, 4095, C.byref(size)) == lib.AMX_OK
    for bad in ((1, 1, 262144), (1, 1, -1), (-1, 1, 1), (1, -1, 1), (1, 2 ** 31, 1), (2 ** 16, 2 ** 15, 1), (2 ** 40, 2 ** 40, 1)):
        assert handle.amx_ctc_align_long_workspace(*bad, C.byref(size)) == lib.AMX_EINVAL, bad
    assert handle.amx_ctc_align_long_workspace(1, 1, 1, None) == lib.AMX_EINVAL
    # the old entry points keep their limit
    assert handle.amx_ctc_align_workspace(1, 1, 4096, C.byref(size)) == lib.AMX_EINVAL
    assert handle.amx_ctc_align_workspace(1, 1, 4095, C.byref(size)) == lib.AMX_OK

    def call(entry=handle.amx_ctc_align_long_emissions, N=2, T=8, Cn=5, blank=0, max_target=3, null=False, workspace_bytes=1 << 20):
        p = None if null else C.c_void_p(16)  # never dereferenced: every refused call returns before any device work
        return entry(0, p, T * Cn, Cn, p, N, T, Cn, blank, p, p, max_target, p, workspace_bytes, p, p, p, p, p, p, None)

    # the matrix of tests/test_ctc_align_contract.py, with the long limit
    assert call(Cn=1) == lib.AMX_EINVAL and call(Cn=0) == lib.AMX_EINVAL
    assert call(blank=-1) == lib.AMX_EINVAL and call(blank=5) == lib.AMX_EINVAL
    assert call(max_target=-1) == lib.AMX_EINVAL and call(max_target=262144) == lib.AMX_EINVAL
    assert b"262143" in handle.amx_last_error(None)
    assert call(N=-1) == lib.AMX_EINVAL and call(T=-1) == lib.AMX_EINVAL
    assert call(N=2 ** 16, T=2 ** 15) == lib.AMX_EINVAL
    assert b"2^31" in handle.amx_last_error(None)
    assert call(null=True) == lib.AMX_EINVAL
    assert call(workspace_bytes=_formula(2, 8, 3) - 1) == lib.AMX_EINVAL
    assert b"workspace" in handle.amx_last_error(None) and str(_formula(2, 8, 3)).encode() in handle.amx_last_error(None)
    assert call(max_target=4096, workspace_bytes=_formula(2, 8, 4096) - 1) == lib.AMX_EINVAL  # accepted up to the workspace
    assert b"workspace" in handle.amx_last_error(None)
    assert call(N=0, null=True) == lib.AMX_OK  # nothing to align
    assert call(entry=handle.amx_ctc_align_emissions, max_target=4096) == lib.AMX_EINVAL
    assert b"4095" in handle.amx_last_error(None)
    # the handle forms refuse a null handle before anything else
    for entry in (handle.amx_ctc_align_long, handle.amx_ctc_align):
        assert entry(None, None, None, 1, 1, None, None, 0, None, 0, None, None, None, None, None, None, None) == lib.AMX_EINVAL


def test_python_surface_without_a_gpu():
    import allophant_amd
    from allophant_amd import alignment, estimator, lib

    assert allophant_amd.segments is alignment.segments is estimator.segments and "segments" in allophant_amd.__all__
    assert alignment.ALIGN_LONG_MAX_TARGET == lib.ALIGN_LONG_MAX_TARGET and alignment.ALIGN_MAX_TARGET == 4095
    with pytest.raises(ValueError, match="4095"):
        alignment.pack_targets([[1] * 4096])
    offsets, ids, counts = alignment.pack_targets([[1] * 4096, [2]], limit=alignment.ALIGN_LONG_MAX_TARGET)
    assert offsets.tolist() == [0, 4096, 4097] and ids.shape == (4097,) and counts == [4096, 1]
    with pytest.raises(ValueError, match="262143"):
        alignment.pack_targets([[1] * 262144], limit=alignment.ALIGN_LONG_MAX_TARGET)
    assert [alignment.use_long(n, None) for n in (0, 4095, 4096)] == [False, False, True]
    assert alignment.use_long(3, True) and not alignment.use_long(5000, False)
    for method in (estimator.Estimator.align, estimator.Estimator.align_device, alignment.ctc_forced_align):
        assert "long" in method.__code__.co_varnames
    assert "262 143" in estimator.Estimator.predict_long.__doc__ and "4095" in estimator.Estimator.predict_long.__doc__


def test_segments_of_a_hand_made_alignment():
    from allophant_amd import spec as S
    from allophant_amd.alignment import Alignment, segments

    #            frame: 0     1     2     3     4     5     6     7     8     9
    tokens = torch.tensor([0, 3, 3, 0, 4, 5, 5, 0, 0, 6], dtype=torch.int32)
    scores = torch.tensor([-1.0, -0.5, -0.25, -2.0, -0.125, -4.0, -0.5, -8.0, -16.0, -0.75])
    spans = torch.tensor([[1, 3], [4, 5], [5, 7], [9, 10]], dtype=torch.int32)
    row = Alignment(tokens, scores, spans, torch.zeros(4), float(scores.sum()))
    frames, means = segments(row, [0, 2, 3, 4])
    assert frames.dtype == torch.int32 and means.dtype == torch.float64
    assert frames.tolist() == [[1, 5], [5, 7], [9, 10]]  # the blank of frame 3 lies inside segment 0
    assert means.tolist() == [(-0.5 - 0.25 - 2.0 - 0.125) / 4, (-4.0 - 0.5) / 2, -0.75]
    # a single segment: from the first target's first frame to the last target's end
    frames, means = segments(row, [0, 4])
    assert frames.tolist() == [[1, 10]] and means.tolist() == [float(scores[1:].to(torch.float64).sum()) / 9]
    # every target its own segment, as a tensor of boundaries
    frames, means = segments(row, torch.tensor([0, 1, 2, 3, 4]))
    assert frames.tolist() == spans.tolist() and means.tolist() == [-0.375, -0.125, -2.25, -0.75]
    # seconds with a spec
    spec = dict(S.tiny_encoder(2))
    seconds, again = segments(row, [0, 2, 3, 4], spec)
    assert seconds.dtype == torch.float64 and again.tolist() == [(-0.5 - 0.25 - 2.0 - 0.125) / 4, -2.25, -0.75]
    assert seconds.flatten().tolist() == pytest.approx([0.02, 0.1, 0.1, 0.14, 0.18, 0.2], rel=1e-12)
    assert segments(row, [0, 4], spec, sample_rate=8000)[0].flatten().tolist() == pytest.approx([0.04, 0.4], rel=1e-12)
    for bad in ([1, 4], [0, 3], [0, 2, 2, 4], [0, 3, 2, 4], [0], [], [0, 5]):
        with pytest.raises(ValueError):
            segments(row, bad)


def _steepest(rng, L, Cn, slack=0):
    """L targets without adjacent repeats over L + slack frames: without slack the only path advances two states a frame."""
    y = [int(rng.integers(1, Cn))]
    while len(y) < L:
        v = int(rng.integers(1, Cn))
        if v != y[-1]:
            y.append(v)
    lp = np.log(rng.dirichlet(np.ones(Cn), L + slack)).astype(np.float32)
    return lp, y


def _halo_rows():
    rng = np.random.default_rng(41)
    steep = _steepest(rng, 3000, 9)
    tight = _steepest(rng, 1500, 9, slack=40)
    lp = np.log(rng.dirichlet(np.ones(9), 2600)).astype(np.float32)
    loose = (lp, [int(v) for v in rng.integers(1, 9, 1100)])  # (with adjacent repeats)
    return {"steepest": steep, "loose": loose, "tight": tight}


@pytest.fixture(scope="module")
def halo_rows():
    return {name: (lp, y, U._sweep_fast(lp, y, 0)) for name, (lp, y) in _halo_rows().items()}


@pytest.mark.parametrize("name", ["steepest", "loose", "tight"])
def test_tiled_sweep_with_the_full_halo_equals_the_restatement(halo_rows, name):
    """The library's cut (its tile and frame block, halo = 2 x frame block): values and moves bit for bit."""
    from allophant_amd import lib

    lp, y, (want_a, want_move) = halo_rows[name]
    F = lib.ALIGN_LONG_FRAME_BLOCK
    a, move = LU.sweep_tiled(lp, y, 0, lib.ALIGN_LONG_TILE_STATES, F, 2 * F)
    assert a.view(np.int32).tolist() == want_a.view(np.int32).tolist()
    assert np.array_equal(move, want_move)
    assert len(y) * 2 + 1 > 2 * lib.ALIGN_LONG_TILE_STATES  # (more than two tiles)


def test_a_halo_one_strip_short_shows_on_the_steepest_row(halo_rows):
    """A condition on the GPU test's input, not a measurement: on the steepest row a halo of 2F - 64 states loses the path at
    a tile edge, so a kernel with that bug cannot pass the GPU test of this row."""
    from allophant_amd import lib

    lp, y, (want_a, want_move) = halo_rows["steepest"]
    F = lib.ALIGN_LONG_FRAME_BLOCK
    want = LU.walk(want_a, want_move, y, 0)
    assert want[0] == 0 and want[1].tolist() == y
    status, paths = LU.walk(*LU.sweep_tiled(lp, y, 0, lib.ALIGN_LONG_TILE_STATES, F, 2 * F - 64), y, 0)
    assert status != 0 or paths.tolist() != y
    full = LU.walk(*LU.sweep_tiled(lp, y, 0, lib.ALIGN_LONG_TILE_STATES, F, 2 * F), y, 0)
    assert full[0] == 0 and full[1].tolist() == y


def test_kernels_have_no_scratch_and_no_vgpr_spills(tmp_path):
    """amx_ctc_align_long.hip compiled for gfx950 (device ISA, -S): each of its three kernels has a private segment of 0 bytes
    and spills no VGPR, and the source is plain HIP without inline assembly."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    source = os.path.join(ROOT, "allophant_amd", "csrc", "amx_ctc_align_long.hip")
    out = tmp_path / "amx_ctc_align_long.s"
    done = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(out), source],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    isa = out.read_text()
    kernels = re.findall(r"\.name:\s+(\S*ctc_align_long_(?:prepare|sweep|finish)\S*)", isa)
    assert len(kernels) == 3, kernels
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa)]
    assert private == [0] * 3 and spills == [0] * 3, (private, spills)
    with open(source, encoding="utf-8") as f:
        text = f.read()
    assert "asm" not in text

"""The CTC forward-backward contract without a GPU: the float64 truth (tests/ctc_score_util.py) against torch's float64 CPU
ctc_loss and its gradient on the pool, hand-worked rows, the yardsticks, the C header, the exports and host-side refusals of
the built library, the Python surface and the kernels' listing."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest
import torch

import ctc_score_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module")
def pool():
    return U.make_pool()


def test_pool_covers_what_it_should(pool):
    assert len(pool) >= 200
    Ts, Ls = [r.lp.shape[0] for r in pool], [len(r.targets) for r in pool]
    assert min(Ts) == 1 and max(Ts) == 500 and min(Ls) == 0 and max(Ls) == 100
    assert {r.lp.shape[1] for r in pool} == {2, 5, 37, 201}
    assert sum(any(a == b for a, b in zip(r.targets, r.targets[1:])) for r in pool) > 50  # repeated neighbours
    feasible = sum(r.truth.status == 0 for r in pool)
    assert feasible > 150 and len(pool) - feasible > 5
    assert all(r.truth.status in (0, -1) for r in pool)


def test_truth_equals_torch_float64(pool):
    """ll equals -ctc_loss(float64) to 1e-9 relative and is -inf exactly where torch returns inf; the class occupancy equals
    exp(lp) - grad of the float64 loss; every frame's g sums to 1."""
    for k, row in enumerate(pool):
        loss, grad = U.torch_loss_and_grad(row.lp, row.targets, torch.float64)
        assert (row.truth.status == -1) == (loss == INF), k
        assert (row.truth.ll == -INF) == (loss == INF), k
        if row.truth.status != 0:
            continue
        assert abs(-loss - row.truth.ll) <= 1e-9 * U.scale(row.truth.ll), (k, loss, row.truth.ll)
        occupancy = U.class_occupancy(row.truth, row.lp.shape[1])
        assert np.abs((row.lp.double().exp() - grad).numpy() - occupancy).max() <= 1e-9, k
        assert np.abs(row.truth.g.sum(axis=1) - 1.0).max() <= 1e-9, k
        # the sums are those of g over the odd states
        T, L = row.lp.shape[0], len(row.targets)
        assert row.truth.occupancy.shape == (L,)
        assert np.allclose(row.truth.occupancy, row.truth.g[:, 1::2].sum(axis=0), rtol=1e-12, atol=1e-300)
        assert np.allclose(row.truth.position_sums, (np.arange(T)[:, None] * row.truth.g[:, 1::2]).sum(axis=0), rtol=1e-12, atol=1e-300)


def test_yardsticks_are_those_of_an_fp32_kernel(pool):
    """A sanity check, not a constant: torch's fp32 CPU kernel is within fp32 rounding of the truth, and not exact."""
    y = U.yardsticks(pool)
    print(f"E_ll = {y.E_ll:.3e}  E_post = {y.E_post:.3e}")
    assert 1e-9 < y.E_ll < 1e-5 and 1e-9 < y.E_post < 1e-4


def test_hand_worked_rows():
    ln = math.log
    # T = 1: only the first two states can end the row
    lp = np.log(np.array([[0.5, 0.3, 0.2]]))
    row = U.score_row(lp, [])
    assert row.status == 0 and row.ll == pytest.approx(ln(0.5)) and row.g.tolist() == [[1.0]] and row.occupancy.shape == (0,)
    row = U.score_row(lp, [1])
    assert row.status == 0 and row.ll == pytest.approx(ln(0.3))  # the blank state 0 cannot end a row that has a target
    assert row.g[0] == pytest.approx([0.0, 1.0, 0.0]) and row.occupancy == pytest.approx([1.0])
    assert row.position_sums == pytest.approx([0.0]) and row.score_sums == pytest.approx([ln(0.3)])
    assert U.score_row(lp, [1, 2]).status == -1
    # L = 0: every frame is blank
    lp = np.log(np.array([[0.5, 0.5], [0.25, 0.75], [0.1, 0.9]]))
    row = U.score_row(lp, [])
    assert row.ll == pytest.approx(ln(0.5 * 0.25 * 0.1)) and row.g.tolist() == [[1.0]] * 3
    assert U.score_row(np.zeros((0, 3)), []).status == 0 and U.score_row(np.zeros((0, 3)), []).ll == 0.0
    assert U.score_row(np.zeros((0, 3)), [1]).status == -1
    # y = [k, k]: two frames cannot hold the blank between, three hold exactly one path
    uniform = np.log(np.full((3, 2), 0.5))
    assert U.score_row(uniform[:2], [1, 1]).status == -1 and U.score_row(uniform[:2], [1, 1]).ll == -INF
    row = U.score_row(uniform, [1, 1])
    assert row.status == 0 and row.ll == pytest.approx(3 * ln(0.5))
    assert row.g == pytest.approx(np.array([[0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 1, 0]], float))
    assert row.occupancy == pytest.approx([1.0, 1.0]) and row.position_sums == pytest.approx([0.0, 2.0])
    # one target in two frames: paths "a a", "a -", "- a"
    p = np.array([[0.6, 0.4], [0.7, 0.3]])
    row = U.score_row(np.log(p), [1])
    total = 0.4 * 0.3 + 0.4 * 0.7 + 0.6 * 0.3
    assert row.ll == pytest.approx(ln(total))
    assert row.occupancy == pytest.approx([(2 * 0.4 * 0.3 + 0.4 * 0.7 + 0.6 * 0.3) / total])
    assert row.position_sums == pytest.approx([(0.4 * 0.3 + 0.6 * 0.3) / total])
    assert row.score_sums == pytest.approx([((0.4 * 0.3 + 0.4 * 0.7) * ln(0.4) + (0.4 * 0.3 + 0.6 * 0.3) * ln(0.3)) / total])
    # an emission column of -inf: class 1 may only be taken in frame 2, whatever it scores elsewhere
    lp = np.array([[-3.0, -INF], [-3.0, -INF], [-3.0, -0.1], [-3.0, -INF]])
    row = U.score_row(lp, [1])
    assert row.status == 0 and row.ll == pytest.approx(-9.1)
    assert row.g == pytest.approx(np.array([[1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float))
    assert row.occupancy == pytest.approx([1.0]) and row.position_sums == pytest.approx([2.0]) and row.score_sums == pytest.approx([-0.1])
    assert not np.isnan(row.score_sums).any()  # (a term whose g is 0 counts as 0, also where e is -inf)
    lp[:, 1] = -INF
    assert U.score_row(lp, [1]).status == -1 and U.score_row(lp, []).status == 0
    assert U.score_row(np.full((4, 3), -INF), []).status == -1
    # malformed targets
    uniform = np.full((4, 3), -1.0)
    assert U.score_row(uniform, [0]).status == -2 and U.score_row(uniform, [3]).status == -2
    assert U.score_row(uniform, [-1]).status == -2 and U.score_row(uniform, [1], blank=1).status == -2


def test_batch_form_candidates_and_bad_rows():
    em = np.full((2, 5, 3), -1.0)
    rows = U.score_batch(em, [5, 3], [0, 1, 1, 3, 4], [1, 2, 1, 2], max_target=2, candidates=2)
    assert [r.status for r in rows] == [0, 0, 0, 0]
    assert rows[1].ll == pytest.approx(-5.0) and rows[3].ll == pytest.approx(U.score_row(em[1, :3], [2]).ll)
    rows = U.score_batch(em, [5, 6], [0, 3, 2, 3, 4], [1, 2, 1, 2], max_target=2, candidates=2)
    assert [r.status for r in rows] == [-2, -2, -2, -2]  # L > max_target, descending offsets, length > T (both candidates)


def test_truth_is_fast_enough_for_the_largest_row():
    rng = np.random.default_rng(0)
    lp = np.log(rng.dirichlet(np.ones(5), 4095)).astype(np.float32)
    y = (np.arange(4095) % 4 + 1).tolist()
    t0 = time.perf_counter()
    row = U.score_row(lp, y, posteriors=False)
    seconds = time.perf_counter() - t0
    assert row.status == 0 and row.occupancy.shape == (4095,) and row.occupancy.sum() == pytest.approx(4095.0)
    assert seconds < 10.0, seconds  # (about a second; the bound only catches a sweep that is no longer vectorised)


def _library():
    from allophant_amd import lib

    if not os.path.exists(os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)):
        pytest.skip("library not built")
    return lib, lib.load()


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "score.c"
    src.write_text('#include "allophant_amx_score.h"\nint main(void) { size_t b; return amx_ctc_score_workspace(1, 1, AMX_SCORE_MAX_TARGET, &b)\n'
                   '    + amx_ctc_score_emissions(0, 0, 0, 0, 0, 0, 0, 2, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)\n'
                   '    + amx_ctc_score(0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    done = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_exports_workspace_and_refusals():
    lib, handle = _library()
    for symbol in ("amx_ctc_score_workspace", "amx_ctc_score_emissions", "amx_ctc_score"):
        assert symbol in lib.SCORE_EXPORTS and hasattr(handle, symbol)
    assert lib.SCORE_MAX_TARGET == 4095 == lib.ALIGN_MAX_TARGET
    size = C.c_size_t()
    for rows, T, max_target in ((1216, 499, 388), (1, 1, 0), (3, 64, 31), (3, 65, 32), (2, 3000, 4095), (5, 0, 7), (0, 9, 9),
                                (1, 2999, 600)):
        assert handle.amx_ctc_score_workspace(rows, T, max_target, C.byref(size)) == lib.AMX_OK
        strips = (2 * max_target + 1 + 63) // 64
        assert size.value == rows * T * strips * 64 * 4, (rows, T, max_target)
    assert handle.amx_ctc_score_workspace(1, 2 ** 31 - 1, 4095, C.byref(size)) == lib.AMX_OK
    for bad in ((1, 1, 4096), (1, 1, -1), (-1, 1, 1), (1, -1, 1), (1, 2 ** 31, 1), (2 ** 16, 2 ** 15, 1), (2 ** 40, 2 ** 40, 1)):
        assert handle.amx_ctc_score_workspace(*bad, C.byref(size)) == lib.AMX_EINVAL, bad
    assert handle.amx_ctc_score_workspace(1, 1, 1, None) == lib.AMX_EINVAL

    def call(N=2, T=8, Cn=5, blank=0, candidates=1, max_target=3, null=False, posteriors=False, workspace_bytes=1 << 20):
        p = None if null else C.c_void_p(16)  # never dereferenced: every refused call returns before any device work
        return handle.amx_ctc_score_emissions(0, p, T * Cn, Cn, p, N, T, Cn, blank, candidates, p, p, max_target, p, workspace_bytes,
                                              p, p, p, p, p if posteriors else None, p, None)

    assert call(Cn=1) == lib.AMX_EINVAL and call(Cn=0) == lib.AMX_EINVAL
    assert b"classes" in handle.amx_last_error(None)
    assert call(blank=-1) == lib.AMX_EINVAL and call(blank=5) == lib.AMX_EINVAL
    assert b"blank" in handle.amx_last_error(None)
    assert call(candidates=0) == lib.AMX_EINVAL and call(candidates=-3) == lib.AMX_EINVAL
    assert b"candidates" in handle.amx_last_error(None)
    assert call(max_target=-1) == lib.AMX_EINVAL and call(max_target=4096) == lib.AMX_EINVAL
    assert b"max_target" in handle.amx_last_error(None)
    assert call(N=-1) == lib.AMX_EINVAL and call(T=-1) == lib.AMX_EINVAL
    assert call(N=2 ** 16, T=2 ** 15) == lib.AMX_EINVAL
    assert b"2^31" in handle.amx_last_error(None)
    assert call(N=2 ** 10, candidates=2 ** 6, T=2 ** 15) == lib.AMX_EINVAL  # the candidates count as rows
    assert b"2^31" in handle.amx_last_error(None)
    assert call(N=2 ** 30, candidates=2 ** 30, T=2 ** 30) == lib.AMX_EINVAL
    assert call(null=True) == lib.AMX_EINVAL
    assert b"null" in handle.amx_last_error(None)
    assert call(candidates=2, workspace_bytes=4 * 8 * 64 * 4 - 1) == lib.AMX_EINVAL  # 4 rows x 8 frames x one strip
    assert b"workspace" in handle.amx_last_error(None)
    assert call(N=0, null=True) == lib.AMX_OK  # nothing to score
    # the handle form refuses a null handle before anything else
    assert handle.amx_ctc_score(None, None, None, 1, 1, 1, None, None, 0, None, 0, None, None, None, None, None, None,
                                None) == lib.AMX_EINVAL


def test_python_surface_without_a_gpu():
    import allophant_amd
    from allophant_amd import estimator, scoring

    for name in ("Score", "Scored", "Rescored", "ctc_score"):
        assert getattr(allophant_amd, name) is getattr(scoring, name) is getattr(estimator, name)
        assert name in allophant_amd.__all__
    for method in ("score", "score_device", "rescore_device"):
        assert hasattr(estimator.Estimator, method)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scoring.ctc_score(torch.zeros(1, 4, 3), torch.tensor([4]), [[1]])
    with pytest.raises(ValueError):
        scoring.ctc_score(torch.zeros(4, 3), torch.tensor([4]), [[1]])
    with pytest.raises(ValueError, match="4095"):
        scoring.pack_targets([[1] * 4096])
    offsets, ids, counts = scoring.pack_targets([[1, 2], [], [3], [4, 4]], utterances=2, candidates=2)
    assert offsets.tolist() == [0, 2, 2, 3, 5] and ids.tolist() == [1, 2, 3, 4, 4] and counts == [2, 0, 1, 2]
    assert offsets.dtype == ids.dtype == torch.int32
    with pytest.raises(ValueError, match="3 target rows for 2 emission rows x 2 candidates"):
        scoring.pack_targets([[1], [2], [3]], utterances=2, candidates=2)
    with pytest.raises(ValueError, match="candidates"):
        scoring.pack_targets([], utterances=0, candidates=0)


def test_host_forms():
    """Scored.scores() and ctc_loss() on hand-made (CPU) buffers, and Score.seconds."""
    from allophant_amd import spec as S
    from allophant_amd.scoring import Score, Scored

    ll = torch.tensor([[-2.0, -INF], [-3.5, 7.0]])
    status = torch.tensor([[0, -1], [0, 0]], dtype=torch.int32)
    occupancy = torch.tensor([[[2.0, 1.0], [9.0, 9.0]], [[4.0, 9.0], [9.0, 9.0]]])
    scored = Scored(None, [], ll, occupancy, occupancy * 3.0, occupancy * -0.5, None, status, [6, 5], [2, 1, 1, 0])
    rows = scored.scores()
    assert rows[0][1] is None and rows[0][0].log_likelihood == -2.0 and rows[0][0].posteriors is None
    assert rows[0][0].occupancy.tolist() == [2.0, 1.0] and rows[0][0].positions.tolist() == [3.0, 3.0]
    assert rows[0][0].scores.tolist() == [-0.5, -0.5] and rows[1][0].occupancy.tolist() == [4.0] and rows[1][1].occupancy.shape == (0,)
    loss = scored.ctc_loss()
    assert loss.dtype == torch.float64 and float(loss) == 2.0 + 3.5 - 7.0
    assert float(scored.ctc_loss(zero_infinity=False)) == INF
    with pytest.raises(ValueError, match="row 1, candidate 0"):
        scored._replace(status=torch.tensor([[0, -1], [-2, 0]], dtype=torch.int32)).scores()
    named = Scored(["a", "b"], ["b"], ll.view(2, 2, 1), occupancy.view(2, 2, 1, 2), occupancy.view(2, 2, 1, 2), occupancy.view(2, 2, 1, 2),
                   None, status.view(2, 2, 1), [6, 5], [2, 1, 1, 0])
    assert list(named.scores()) == ["b"] and named.scores()["b"][0][0].log_likelihood == -3.5
    assert float(named.ctc_loss()) == 3.5 - 7.0

    row = Score(-1.0, torch.ones(2), torch.tensor([0.0, 2.5]), torch.zeros(2), None)
    spec = dict(S.tiny_encoder(2))
    assert row.seconds(spec).tolist() == pytest.approx([0.0, 0.05], rel=1e-12)
    assert row.seconds(spec, sample_rate=8000).tolist() == pytest.approx([0.0, 0.1], rel=1e-12)


def test_kernels_have_no_scratch_and_no_vgpr_spills(tmp_path):
    """amx_ctc_score.hip compiled for gfx950 (device ISA, -S): every instantiation of the kernel has a private segment of 0
    bytes and spills no VGPR, and the source is plain HIP without inline assembly."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    source = os.path.join(ROOT, "allophant_amd", "csrc", "amx_ctc_score.hip")
    out = tmp_path / "amx_ctc_score.s"
    done = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(out), source],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    isa = out.read_text()
    kernels = re.findall(r"\.name:\s+(\S*ctc_score_kernel\S*)", isa)
    assert len(kernels) == 4, kernels
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa)]
    assert private == [0] * 4 and spills == [0] * 4, (private, spills)
    with open(source, encoding="utf-8") as f:
        text = f.read()
    assert "asm" not in text

"""The one-edit-variant contract without a GPU: the float64 decomposition (tests/ctc_variants_util.py) against brute force
over every explicitly edited sequence, the C header, the exports and host-side refusals of the built library, the façade's
refusals, the math of the device-side views on hand-made tensors, and the kernels' listing."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import ctc_score_util as U
import ctc_variants_util as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _pool(count=240, seed=4711):
    """Fixed-seed rows (lp, targets, blank): T 1..12, L 0..6, C in {2, 3, 5, 9}; non-zero blanks, all-equal targets, -inf
    emission entries and rows below minimum_frames among them."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(count):
        Cn = (2, 3, 5, 9)[k % 4]
        T, L = int(rng.integers(1, 13)), int(rng.integers(0, 7))
        blank = int(rng.integers(0, Cn)) if k % 3 else 0
        classes = [c for c in range(Cn) if c != blank]
        if k % 5 == 0:
            y = [classes[0]] * L  # all equal
        else:
            y = [int(rng.choice(classes)) for _ in range(L)]  # (neighbours repeat often at these class counts)
        lp = np.log(rng.dirichlet(np.ones(Cn), T))
        if k % 4 == 1:
            lp[rng.random((T, Cn)) < 0.25] = -INF
        if k % 7 == 0 and L:
            T = max(1, U.minimum_frames(y) - int(rng.integers(0, 3)))  # at and below the feasibility boundary
            lp = lp[:T] if T <= lp.shape[0] else np.log(rng.dirichlet(np.ones(Cn), T))
        rows.append((lp, y, blank))
    return rows


def test_pool_covers_what_it_should():
    rows = _pool()
    assert {lp.shape[1] for lp, _, _ in rows} == {2, 3, 5, 9}
    assert {lp.shape[0] for lp, _, _ in rows} >= set(range(1, 13)) and {len(y) for _, y, _ in rows} == set(range(7))
    assert sum(blank != 0 for _, _, blank in rows) > 50
    assert sum(len(y) >= 2 and len(set(y)) == 1 for _, y, _ in rows) > 10
    assert sum(bool(np.isinf(lp).any()) for lp, _, _ in rows) > 30
    assert sum(lp.shape[0] < U.minimum_frames(y) for lp, y, _ in rows) > 10
    # a substitute equal to a neighbour is part of every row with L >= 2: every class is substituted at every position


def test_decomposition_equals_brute_force():
    """variants_row == score_row of every edited sequence: the same -inf cells, the finite ones within 1e-9 relative."""
    cells = infinite = 0
    worst = 0.0
    for k, (lp, y, blank) in enumerate(_pool()):
        got, want = V.variants_row(lp, y, blank), V.variants_brute(lp, y, blank)
        assert got.status == 0
        assert (got.ll == -INF) == (want.ll == -INF) and (got.ll == -INF or abs(got.ll - want.ll) <= 1e-9 * U.scale(want.ll)), k
        for name, g, w in (("sub", got.sub, want.sub), ("ins", got.ins, want.ins)):
            assert g.shape == w.shape and not np.isnan(g).any(), (k, name)
            assert np.array_equal(g == -INF, w == -INF), (k, name, y, blank)
            finite = w > -INF
            cells += int(finite.sum())
            infinite += int((~finite).sum())
            if finite.any():
                error = np.abs(g[finite] - w[finite]) / np.maximum(1.0, np.abs(w[finite]))
                worst = max(worst, float(error.max()))
                assert error.max() <= 1e-9, (k, name, float(error.max()))
        # the transcript's own symbol substituted for itself is the transcript
        for l, v in enumerate(y):
            assert (got.sub[l, v] == -INF) == (got.ll == -INF)
            assert got.ll == -INF or abs(got.sub[l, v] - got.ll) <= 1e-9 * U.scale(got.ll)
    print(f"\n{cells} finite and {infinite} -inf cells, worst relative difference {worst:.2e}")
    assert cells > 3000 and infinite > 300


def test_rows_below_minimum_frames_keep_feasible_deletions():
    lp = np.log(np.full((2, 3), 1.0 / 3))
    row = V.variants_row(lp, [1, 1])  # needs three frames
    assert row.status == 0 and row.ll == -INF
    assert row.sub[0, 0] == pytest.approx(V.variants_brute(lp, [1, 1]).sub[0, 0]) and row.sub[0, 0] > -INF  # "1" fits
    assert row.sub[0, 2] > -INF and row.sub[0, 1] == -INF and (row.ins[:, 1:] == -INF).all()
    assert V.variants_row(np.zeros((0, 3)), [1]).status == -1 and V.variants_row(lp, [0]).status == -2
    empty = V.variants_row(np.zeros((0, 3)), [], blank=1)
    assert empty.status == 0 and empty.ll == 0.0 and empty.ins.tolist() == [[-INF, 0.0, -INF]] and empty.sub.shape == (0, 3)


def _library():
    from allophant_amd import lib

    if not os.path.exists(os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)):
        pytest.skip("library not built")
    return lib, lib.load()


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "variants.c"
    src.write_text('#include "allophant_amx_variants.h"\nint main(void) { size_t b; return amx_ctc_variants_workspace(1, 1, AMX_VARIANTS_MAX_TARGET, &b)\n'
                   '    + amx_ctc_variants_emissions(0, 0, 0, 0, 0, 0, 0, AMX_VARIANTS_MAX_CLASSES, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    done = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_exports_workspace_and_refusals():
    lib, handle = _library()
    for symbol in ("amx_ctc_variants_workspace", "amx_ctc_variants_emissions"):
        assert symbol in lib.VARIANTS_EXPORTS and hasattr(handle, symbol)
    assert lib.VARIANTS_MAX_TARGET == 4095 and lib.VARIANTS_MAX_CLASSES == 65535
    size = C.c_size_t()
    for rows, T, max_target in ((32, 499, 130), (1, 1, 0), (3, 64, 31), (3, 65, 32), (2, 3000, 4095), (5, 0, 7), (0, 9, 9)):
        assert handle.amx_ctc_variants_workspace(rows, T, max_target, C.byref(size)) == lib.AMX_OK
        strips = (2 * max_target + 1 + 63) // 64
        assert size.value == 2 * rows * T * strips * 64 * 4, (rows, T, max_target)
    assert handle.amx_ctc_variants_workspace(1, 2 ** 31 - 1, 4095, C.byref(size)) == lib.AMX_OK
    assert size.value == 2 * (2 ** 31 - 1) * 8192 * 4
    for bad in ((1, 1, 4096), (1, 1, -1), (-1, 1, 1), (1, -1, 1), (1, 2 ** 31, 1), (2 ** 16, 2 ** 15, 1), (2 ** 40, 2 ** 40, 1)):
        assert handle.amx_ctc_variants_workspace(*bad, C.byref(size)) == lib.AMX_EINVAL, bad
    assert handle.amx_ctc_variants_workspace(1, 1, 1, None) == lib.AMX_EINVAL
    assert b"null" in handle.amx_last_error(None)

    def call(N=2, T=8, Cn=5, blank=0, max_target=3, null=False, workspace_bytes=1 << 20):
        p = None if null else C.c_void_p(16)  # never dereferenced: every refused call returns before any device work
        return handle.amx_ctc_variants_emissions(0, p, T * Cn, Cn, p, N, T, Cn, blank, p, p, max_target, p, workspace_bytes, p, p, p, p,
                                                 None)

    assert call(Cn=1) == lib.AMX_EINVAL and call(Cn=0) == lib.AMX_EINVAL and call(Cn=65536) == lib.AMX_EINVAL
    assert b"classes" in handle.amx_last_error(None)
    assert call(blank=-1) == lib.AMX_EINVAL and call(blank=5) == lib.AMX_EINVAL
    assert b"blank" in handle.amx_last_error(None)
    assert call(max_target=-1) == lib.AMX_EINVAL and call(max_target=4096) == lib.AMX_EINVAL
    assert b"max_target" in handle.amx_last_error(None)
    assert call(N=-1) == lib.AMX_EINVAL and call(T=-1) == lib.AMX_EINVAL
    assert call(N=2 ** 16, T=2 ** 15) == lib.AMX_EINVAL
    assert b"2^31" in handle.amx_last_error(None)
    assert call(null=True) == lib.AMX_EINVAL
    assert b"null" in handle.amx_last_error(None)
    assert call(workspace_bytes=2 * 2 * 8 * 64 * 4 - 1) == lib.AMX_EINVAL  # a and b, 2 rows x 8 frames x one strip
    assert b"workspace" in handle.amx_last_error(None)
    assert call(N=0, null=True) == lib.AMX_OK  # nothing to do


def test_facade_refusals_without_a_gpu():
    import allophant_amd
    from allophant_amd import estimator, variants

    for name in ("Variants", "Alternatives", "ctc_variants"):
        assert getattr(allophant_amd, name) is getattr(variants, name) is getattr(estimator, name)
        assert name in allophant_amd.__all__
    em = torch.zeros(2, 6, 4)
    with pytest.raises(ValueError, match="blank"):
        variants.ctc_variants(em, None, [[1, 2], [3, 0]])
    with pytest.raises(ValueError, match="blank"):
        variants.ctc_variants(em, None, [[1, 2], [3, 0]], blank=2)
    with pytest.raises(ValueError, match="outside the 4 classes"):
        variants.ctc_variants(em, None, [[1, 4], [3]])
    with pytest.raises(ValueError, match="outside the 4 classes"):
        variants.ctc_variants(em, None, [[1], [-1]])
    with pytest.raises(ValueError, match="blank_index"):
        variants.ctc_variants(em, None, [[1], [1]], blank=4)
    with pytest.raises(ValueError, match="1 target rows for 2 emission rows"):
        variants.ctc_variants(em, None, [[1]])
    with pytest.raises(ValueError, match="4095"):
        variants.ctc_variants(em, None, [[1] * 4096, []])
    with pytest.raises(ValueError):
        variants.ctc_variants(torch.zeros(6, 4), None, [[1]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        variants.ctc_variants(em, None, [[1, 2], [3]])
    # the Estimator form: one named output of the predictions
    predictions = types.SimpleNamespace(outputs={"phoneme": em.transpose(0, 1), "nasal": em.transpose(0, 1)}, lengths=torch.tensor([6, 6]))
    with pytest.raises(ValueError, match="unknown output 'voiced'"):
        estimator.Estimator.variants_device(None, predictions, [[1], [2]], "voiced")
    with pytest.raises(ValueError, match="one output"):
        estimator.Estimator.variants_device(None, predictions, {"phoneme": [[1], [2]], "nasal": [[1], [2]]}, "phoneme")
    with pytest.raises(ValueError, match="blank"):
        estimator.Estimator.variants_device(None, predictions, {"phoneme": [[1], [0]]}, "phoneme")
    with pytest.raises(ValueError, match="outside the 4 classes"):
        estimator.Estimator.variants_device(None, predictions, [[1], [7]], "phoneme")
    assert hasattr(estimator.Estimator, "variants")


def _hand_made():
    """Two rows over 4 classes (blank 0): row 0 holds y = [1, 2], row 1 y = [3] in a buffer of max_target 2."""
    from allophant_amd.variants import Variants

    ln = math.log
    ll = torch.tensor([ln(0.2), ln(0.5)])
    sub = torch.full((2, 2, 4), 123.0)  # (what lies past a row's L is never read into a result)
    sub[0, 0] = torch.tensor([ln(0.1), ln(0.2), ln(0.6), ln(0.1)])   # position 0: class 2 beats the transcript's 1 threefold
    sub[0, 1] = torch.tensor([ln(0.05), ln(0.05), ln(0.2), -INF])    # position 1: the transcript's own 2 is best
    sub[1, 0] = torch.tensor([ln(1.5), ln(0.25), ln(0.25), ln(0.5)])  # deleting y[0] = 3 is three times as probable
    ins = torch.full((2, 3, 4), 123.0)
    ins[0, 0] = torch.tensor([ln(0.2), ln(0.01), ln(0.01), ln(0.02)])
    ins[0, 1] = torch.tensor([ln(0.2), ln(0.1), ln(0.1), ln(0.4)])   # gap 1: inserting 3 doubles the likelihood
    ins[0, 2] = torch.tensor([ln(0.2), -INF, -INF, -INF])
    ins[1, 0] = torch.tensor([ln(0.5), ln(0.25), ln(0.125), ln(0.125)])
    ins[1, 1] = torch.tensor([ln(0.5), ln(0.5), -INF, -INF])         # a tie does not beat the transcript
    return Variants(ll, sub, ins, torch.tensor([0, 0], dtype=torch.int32), torch.tensor([[1, 2], [3, 0]]), torch.tensor([2, 1]), 0, [9, 9])


def test_goodness_alternatives_and_diagnose_on_hand_made_tensors():
    from allophant_amd.evaluation import Action

    ln = math.log
    v = _hand_made()
    goodness = v.goodness()
    assert goodness.shape == (2, 2) and math.isnan(float(goodness[1, 1]))
    assert goodness[0].tolist() == pytest.approx([ln(0.2 / 1.0), ln(0.2 / 0.3)], rel=1e-6)
    assert float(goodness[1, 0]) == pytest.approx(ln(0.5 / 2.5), rel=1e-6)
    free = v.insertion_free()
    assert free.shape == (2, 3) and math.isnan(float(free[1, 2]))
    assert free[0].tolist() == pytest.approx([ln(0.2 / 0.24), ln(0.2 / 0.8), 0.0], rel=1e-6, abs=1e-7)
    assert free[1, :2].tolist() == pytest.approx([ln(0.5), ln(0.5)], rel=1e-6)

    top = v.alternatives(2)
    assert top.substitution_classes.shape == (2, 2, 2) and top.insertion_log_posteriors.shape == (2, 3, 2)
    assert top.substitution_classes[0].tolist() == [[2, 1], [2, 0]] or top.substitution_classes[0].tolist() == [[2, 1], [2, 1]]
    assert top.substitution_log_posteriors[0, 0].tolist() == pytest.approx([ln(0.6), ln(0.2)], rel=1e-6)
    assert top.substitution_classes[1, 0, 0] == 0 and float(top.substitution_log_posteriors[1, 0, 0]) == pytest.approx(ln(0.6), rel=1e-6)
    assert top.insertion_classes[0, 1].tolist() == [3, 0]
    assert top.insertion_log_posteriors[0, 1].tolist() == pytest.approx([ln(0.5), ln(0.25)], rel=1e-6)
    assert torch.isnan(top.substitution_log_posteriors[1, 1]).all() and torch.isnan(top.insertion_log_posteriors[1, 2]).all()

    found = v.diagnose()
    assert [(kind, at, c) for kind, at, c, _ in found[0]] == [(Action.SUBSTITUTION, 0, 2), (Action.INSERTION, 1, 3)]
    assert [ratio for *_, ratio in found[0]] == pytest.approx([ln(3.0), ln(2.0)], rel=1e-5)
    assert [(kind, at, c) for kind, at, c, _ in found[1]] == [(Action.DELETION, 0, 3)]
    assert found[1][0][3] == pytest.approx(ln(3.0), rel=1e-5)
    assert v.diagnose(threshold=1.0) == [[(Action.SUBSTITUTION, 0, 2, pytest.approx(ln(3.0), rel=1e-5))],
                                         [(Action.DELETION, 0, 3, pytest.approx(ln(3.0), rel=1e-5))]]
    assert v.diagnose(threshold=2.0) == [[], []]
    # a transcript without a path: whatever has one beats it; a row of no frames has nothing to say; a malformed row is named
    stuck = v._replace(log_likelihood=torch.tensor([-INF, ln(0.5)]))
    kinds = [(kind, at, c) for kind, at, c, _ in stuck.diagnose()[0]]
    assert (Action.DELETION, 0, 1) in kinds and (Action.SUBSTITUTION, 1, 3) not in kinds and len(kinds) == 11
    assert v._replace(status=torch.tensor([-1, 0], dtype=torch.int32)).diagnose()[0] is None
    with pytest.raises(ValueError, match="row 1"):
        v._replace(status=torch.tensor([0, -2], dtype=torch.int32)).diagnose()


def test_kernels_have_no_scratch_and_no_vgpr_spills(tmp_path):
    """amx_ctc_variants.hip compiled for gfx950 (device ISA, -S): the four instantiations of the lattice kernel and the
    variants kernel have a private segment of 0 bytes and spill no VGPR; the variants kernel uses no LDS; the source is plain
    HIP without inline assembly."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    source = os.path.join(ROOT, "allophant_amd", "csrc", "amx_ctc_variants.hip")
    out = tmp_path / "amx_ctc_variants.s"
    done = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(out), source],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    isa = out.read_text()
    kernels = re.findall(r"\.name:\s+(\S*ctc_(?:lattice|variants)_kernel\S*)", isa)
    assert len(kernels) == 5 and sum("lattice" in k for k in kernels) == 4, kernels
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa)]
    assert private == [0] * 5 and spills == [0] * 5, (private, spills)
    lds = dict(zip(re.findall(r"\.name:\s+(\S+)", isa), (int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", isa))))
    assert [lds[k] for k in kernels if "variants" in k] == [0]
    with open(source, encoding="utf-8") as f:
        text = f.read()
    assert "asm" not in text and "atomic" not in text.replace("no atomic", "")

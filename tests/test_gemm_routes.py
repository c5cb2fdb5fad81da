"""The routing table of launch_gemm against a recording (no GPU needed: hipcc cross-compiles gfx950 here, the routing is host logic).

``tests/gemm_routes/route_dump.hip`` includes the GEMM translation unit and prints, for every product of a forward pass (four encoders,
six batch geometries, padded and packed, four precision modes, with and without split-K workspace, with and without
``g_force_generic_gemm``), the cases of ``tools/gemm_bench check``, rows on both sides of every routing threshold and operands that
each eligibility test refuses: what the public queries of ``amx_common.h`` answer, and the route (kernel, tile, LayerNorm-fold role,
whether anything is launched).  The output holds a digest per block of cases, the flagship's own products in clear text and the first
case that reached each distinct route (``route_dump full`` prints every case).  ``tests/gemm_routes/routes.txt`` is that output
recorded at the revision before ``gemm_route`` existed -- the public columns with this very program compiled against that revision's ``csrc``, the detail columns with its
``describe()`` replaced by a walk of ``launch_gemm_t``'s branch ladder -- so a routing change, intended or not, shows as a diff here.

The table depends on the CU count: 256 on an unpartitioned MI355X, and the fallback without a GPU.  Any other count legitimately
routes differently; the test then skips and names it.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HERE = os.path.join(ROOT, "tests", "gemm_routes")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("routes") / "route_dump"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", f"-I{ROOT}/include", f"-I{ROOT}/allophant_amd/csrc", "-o", str(exe),
           os.path.join(HERE, "route_dump.hip")]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, timeout=300).stdout.decode()
    cus = int(re.search(r"cus (\d+)\n$", out).group(1))
    if cus != 256:
        pytest.skip(f"the recorded table is for 256 CUs, this device has {cus}")
    return out


def test_routes_equal_the_recording_byte_for_byte(table):
    with open(os.path.join(HERE, "routes.txt"), newline="") as f:
        recorded = f.read()
    if table != recorded:
        got, want = table.splitlines(), recorded.splitlines()
        diff = [f"line {i + 1}:\n  recorded {w}\n  now      {g}" for i, (g, w) in enumerate(zip(got, want)) if g != w]
        raise AssertionError(f"{len(diff)} of {len(want)} lines differ ({len(got)} lines now):\n" + "\n".join(diff[:20]))


def test_the_table_reaches_every_kind_of_route(table):
    """So that the table cannot silently shrink to the easy cases: every kernel, tile and refusal occurs in a clear-text row (the
    table ends with the first case that reached each distinct route), and the digests stand for as many cases as were recorded."""
    rows = []
    for line in table.splitlines():
        # ... | uses_pp fuses_ln tap_minor_slice planned_splits fold_ok fixup | kernel mi ni fold dma_shape tile_bn launches
        m = re.search(r"\| \d \d \d+ (\d+) (\d) \d \| (\S+) (\d) (\d) (\d) (\d) (\d+) (\d)$", line)
        if m:
            splits, fold_ok, kernel, *rest = m.groups()
            rows.append((kernel, int(splits)) + tuple(int(v) for v in rest) + (int(fold_ok),))
    digested = sum(int(m.group(1)) for m in re.finditer(r"^digest \S+ (\d+) ", table, re.M))
    assert digested == int(re.search(r"^(\d+) cases, cus", table, re.M).group(1)) >= 14000
    have = lambda pred: any(pred(*r) for r in rows)  # noqa: E731
    for kernel in ("LN", "LN_IL", "PP", "DMA", "TILE"):
        assert have(lambda k, *_: k == kernel), kernel
    for mi in (8, 4):
        for ni in (4, 3):
            for fold in (0, 1):
                assert have(lambda k, s, m, n, f, sh, bn, l, ok: k == "PP" and (m, n, f, l) == (mi, ni, fold, 1)), (mi, ni, fold)
        assert have(lambda k, s, m, n, f, sh, bn, l, ok: k == "PP" and (m, n, f, l) == (mi, 4, 2, 1)), (mi, "producer")
    for shape in (1, 2):
        assert have(lambda k, s, m, n, f, sh, bn, l, ok: k == "DMA" and sh == shape), shape
    for width in (64, 128):
        assert have(lambda k, s, m, n, f, sh, bn, l, ok: k == "TILE" and bn == width), width
    for kernel in ("PP", "DMA", "TILE"):
        assert have(lambda k, s, m, n, f, sh, bn, l, ok: k == kernel and s > 1 and f == 0), kernel
    # refusals: a producer planned on 192-column tiles, a fold product off the ping-pong kernel, a LayerNorm shape the row-complete
    # kernel rejects
    assert have(lambda k, s, m, n, f, sh, bn, l, ok: k == "PP" and (n, f, l) == (3, 2, 0))
    assert have(lambda k, s, m, n, f, sh, bn, l, ok: k in ("DMA", "TILE") and f > 0 and l == 0)
    assert have(lambda k, s, m, n, f, sh, bn, l, ok: k in ("LN", "LN_IL") and l == 0)
    # a fold product whose plan has K chunks: reported as planned, refused by gemm_ln_fold_ok (it would launch in one piece)
    assert have(lambda k, s, m, n, f, sh, bn, l, ok: k == "PP" and f > 0 and s > 1 and ok == 0)
    assert not have(lambda k, s, m, n, f, sh, bn, l, ok: f > 0 and ok == 1 and (s > 1 or l == 0))

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

``route_dump rows <encoder> <precision> <packed> <M> [T]`` prints the products of one layer at an arbitrary row count.  With it
``test_row_edge_cases_*`` prove the case table of tests/test_gpu_stage_row_edges.py (tests/row_edge_util.py): every case's batch
has the declared row count, and every product takes the declared kernel and tile and ends the declared number of rows into it.
"""
import os
import re
import shutil
import subprocess

import pytest

from tests import row_edge_util as RE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HERE = os.path.join(ROOT, "tests", "gemm_routes")


@pytest.fixture(scope="module")
def route_dump(tmp_path_factory):
    """the compiled program: ``route_dump(*args)`` runs it and returns its output"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("routes") / "route_dump"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", f"-I{ROOT}/include", f"-I{ROOT}/allophant_amd/csrc", "-o", str(exe),
           os.path.join(HERE, "route_dump.hip")]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
    return lambda *args: subprocess.run([str(exe), *args], check=True, stdout=subprocess.PIPE, timeout=300).stdout.decode()


@pytest.fixture(scope="module")
def table(route_dump):
    out = route_dump()
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


ROW = re.compile(r"^rows \S+?-(qkv|oproj|ffn1|ffn2)(-consumer|-producer|-producer-f32)? (\S+) ws1 (\d+)x\d+x\d+ \| \d \d \d+ (\d+) (\d) \d \| "
                 r"(\S+) (\d) (\d) (\d) (\d) (\d+) (\d)$", re.M)


def layer_routes(route_dump, case, precision):
    """``route_dump rows`` for the case: whether the pass folds the LayerNorm (every fold product admitted, as ``plan_pass`` asks),
    and product -> ``RE.Route`` of the products such a pass launches"""
    out = route_dump("rows", "xlsr", precision, "1" if case.packed else "0", str(case.M), *([str(case.T)] if case.T else []))
    cus = int(re.search(r"cus (\d+)\n$", out).group(1))
    if cus != 256:
        pytest.skip(f"the case table is for 256 CUs, this device has {cus}")
    rows = {}
    for product, variant, prec, m, splits, fold_ok, kernel, mi, ni, fold, shape, bn, launches in ROW.findall(out):
        assert prec == precision and int(m) == case.M
        if kernel == "PP":
            tile = (int(mi) * 32, int(ni) * 64)
        elif kernel == "DMA":
            tile = {1: (128, 64), 2: (64, 32)}[int(shape)]
        else:
            tile = (128, int(bn))
        rows[product + variant] = (int(fold_ok), int(launches), RE.Route(kernel, *tile, case.M % tile[0], RE.ROLES[int(fold)], int(splits)))
    assert len(rows) == 9, out
    folds = all(rows[k][0] for k in ("qkv-consumer", "oproj-producer", "ffn1-consumer", "ffn2-producer", "ffn2-producer-f32"))
    taken = {"qkv": "qkv-consumer", "oproj": "oproj-producer", "ffn1": "ffn1-consumer", "ffn2": "ffn2-producer"} if folds else \
        {k: k for k in RE.PRODUCTS}
    assert all(rows[v][1] for v in taken.values()), out
    if folds:  # FFN2 with and without fp32 rows: the same route
        assert rows["ffn2-producer-f32"][2] == rows["ffn2-producer"][2], out
    return folds, {k: rows[v][2] for k, v in taken.items()}


@pytest.mark.parametrize("name,precision", RE.GPU_CASES)
def test_row_edge_case_reaches_what_it_declares(route_dump, name, precision):
    """the batch recipe gives the declared row count, and at that count every product of a layer takes the declared kernel, tile,
    LayerNorm-fold role and K chunks and ends the declared number of rows into its last row tile"""
    case = RE.CASES[name]
    frames = RE.utterance_frames(case)
    assert sum(frames) == case.M, (name, sum(frames))
    longest = max(frames)
    if case.packed:  # what ``plan_pass`` asks of a batch before it packs its rows: a tenth of the padded rows are padding
        assert case.M * 10 <= len(frames) * longest * 9 and len(case.tail) and frames[-1] == 1
        assert sum(case.tail) > max(r.tile_rows for r in case.products.values()), "the tail covers the tallest tile of the case"
    else:
        assert min(frames) == longest == case.T
    folds, routes = layer_routes(route_dump, case, precision)
    print(f"[row-edges] {name} {precision} M {case.M} fold {int(folds)}: " +
          " | ".join(f"{k} {r.kernel} {r.tile_rows}x{r.tile_cols} r{r.residue} {r.role} k{r.chunks}" for k, r in routes.items()))
    assert int(folds) == case.ln_fold
    assert routes == case.products


def test_the_row_edge_cases_cover_every_edge():
    """So that the case table cannot shrink to the easy residues: what it holds as a whole."""
    cases = list(RE.CASES.values())

    def residues(family, pred):
        return {r.residue for c in cases if c.family == family for r in c.products.values() if pred(r)}

    def product_residues(family, product, pred):
        return {c.products[product].residue for c in cases if c.family == family and pred(c.products[product])}

    listed = {1, 8, 9, 32, 33, 127, 128, 129, 255}
    for product, role in (("qkv", "consumer"), ("ffn1", "consumer"), ("oproj", "producer"), ("ffn2", "producer")):
        got = product_residues("fold256", product, lambda r: (r.kernel, r.tile_rows, r.role) == ("PP", 256, role))
        assert got == listed, (product, got)
        on_bf16 = {c.products[product].residue for c in cases if c.family == "fold256" and "bf16x3" in c.precisions}
        assert on_bf16 == {1, 129, 255}, (product, on_bf16)
    for product, role in (("qkv", "consumer"), ("oproj", "producer"), ("ffn2", "producer")):
        got = product_residues("fold128", product, lambda r: (r.kernel, r.tile_rows, r.role) == ("PP", 128, role))
        assert got == {1, 63, 64, 65, 127}, (product, got)
    assert all(c.ln_fold == 1 and c.packed == 2 for c in cases if c.family in ("fold256", "fold128"))
    plain = {1, 8, 9, 33, 63, 64, 65, 127}
    for product in ("qkv", "oproj", "ffn2"):
        got = product_residues("plain128", product, lambda r: (r.kernel, r.tile_rows, r.role) == ("PP", 128, "plain"))
        assert got == plain, (product, got)
    assert {c.products["oproj"].tile_cols for c in cases if c.family == "plain128"} == {192}  # NI = 3: generic throughout
    assert {c.products["ffn2"].chunks for c in cases if c.family == "plain128"} == {2}
    assert {c.products["oproj"].residue for c in cases if c.family == "plain128" and "bf16x3" in c.precisions} == {1, 65}
    assert all(c.ln_fold == 0 and c.packed == 2 for c in cases if c.family == "plain128")
    # both sides of every threshold, and the one product a threshold moves
    assert {c.M for c in cases if c.family == "threshold"} == {383, 384, 385, 767, 768, 769, 4095, 4096, 4097}
    assert RE.CASES["threshold/767"].products["ffn2"].kernel == "DMA" and RE.CASES["threshold/768"].products["ffn2"].kernel == "PP"
    # short products: both LDS-DMA shapes, K chunks whose slabs end inside a fix-up block and a row-norm workgroup
    assert {(r.tile_rows, r.tile_cols) for c in cases for r in c.products.values() if r.kernel == "DMA"} == {(128, 64), (64, 32)}
    short = [c for c in cases if c.family == "short"]
    assert all(c.M < 384 and set(c.precisions) == {"f16x3", "bf16x3"} for c in short)
    assert {c.products["ffn2"].chunks for c in short} == {2, 4} and all(c.products["ffn2"].kernel == "DMA" for c in short)
    assert {c.M % 64 for c in short} == {1, 63} and {c.M % 4 for c in short} == {1, 3} and {c.M % 128 for c in short} >= {1, 127}
    # T = 7, 8, 9 in the padded layout: QKV on 256-column ping-pong tiles (the fast scatter where T >= 8), and on LDS-DMA tiles
    for T in (7, 8, 9):
        kernels = {(c.products["qkv"].kernel, c.products["qkv"].tile_cols) for c in cases if c.family == "padded" and c.T == T}
        assert kernels == {("PP", 256), ("DMA", 32)}, (T, kernels)
    assert all(c.packed == 0 and c.M == c.body[1] * c.T for c in cases if c.family == "padded")
    assert residues("padded", lambda r: r.kernel == "PP") >= {6, 8, 9}

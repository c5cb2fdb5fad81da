"""The feature-weighted edit-distance contract on the host (no GPU): the forms the kernels compute (anti-diagonal matrix,
carried statistics, path codes with a walk of S + D + I records; tests/edit_weighted_util.py) against the literal restatement of
upstream's ``PropertyWeighting`` on thousands of random pairs; unit costs with an identity table against the uniform
restatements; hand-worked cases whose path differs from the uniform one; the C ABI's header, exports, refusals and compiled
ISA; and the host behaviour of ``PropertyWeighting`` / ``Evaluator(weighting=...)``."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import edit_ops_util as U
import edit_util as E
import edit_weighted_util as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, D, S = W.INSERTION, W.DELETION, W.SUBSTITUTION
COSTS = [(1.0, 1.0), (0.3, 0.7), (2.5, 0.1), (1.7, 3.3)]  # unit, non-dyadic, dear insertions, dear deletions
COSTS_ALL = COSTS + [(0.3, 1.5)]  # and insertion < 1 < deletion


def _bits(x) -> bytes:
    return np.asarray(x, dtype=np.float32).tobytes()


def _random_table(rng, alphabet):
    """1-5 feature columns over 2 values, one row duplicated when there is room: different symbols that cost 0."""
    rows = rng.integers(0, 2, (alphabet, int(rng.integers(1, 6))))
    if alphabet > 2:
        rows[alphabet - 1] = rows[0]
    return {s: rows[s] for s in range(alphabet)}


def _pair(rng, alphabet, long):
    m, n = (int(v) for v in rng.integers(0, 301 if long else 14, 2))
    a = rng.integers(0, alphabet, m).tolist()
    b = rng.integers(0, alphabet, n).tolist()
    if rng.integers(0, 3) == 0:  # a shared prefix
        p = int(rng.integers(0, min(m, n) + 1))
        b[:p] = a[:p]
    return a, b


@pytest.mark.parametrize("costs", COSTS_ALL)
def test_kernel_forms_equal_the_literal_restatement(costs):
    """5 x 900 random pairs, alphabets of 2-3 symbols (ties everywhere), tables with duplicate rows.  Short pairs (lengths
    0-13): the anti-diagonal matrix equals the cell-by-cell restatement bit for bit.  Every pair, one in nine with lengths up
    to 300 on both sides (several 64-row strips): the carried statistics and the path-code walk equal the literal walk on that
    matrix in counts, operations and cost bits; the walk stops on the diagonal (C = m - S - D, I = n - C - S hold) and records
    S + D + I <= m + n operations."""
    rng = np.random.default_rng(int(costs[0] * 10) * 100 + int(costs[1] * 10))
    longest = 0
    for q in range(900):
        alphabet = int(rng.integers(2, 4))
        table = _random_table(rng, alphabet)
        long = q % 9 == 0
        a, b = _pair(rng, alphabet, long)
        matrix = W.matrix_fast(a, b, *costs, table)
        if not long:
            assert _bits(matrix) == _bits(W.levensthein_matrix_weighted(a, b, *costs, table)), (a, b)
        operations, cost, statistics = W.walk(matrix, len(a), len(b))
        got_statistics, got_cost = W.carried_statistics(a, b, *costs, table)
        assert got_statistics == statistics and _bits(got_cost) == _bits(cost), (a, b)
        got_operations, ops_cost, ops_statistics = W.kernel_form(a, b, *costs, table)
        assert got_operations == operations and _bits(ops_cost) == _bits(cost) and ops_statistics == statistics, (a, b)
        ins, dels, subs, correct = statistics
        actions = [op[0] for op in operations]
        assert (actions.count(I), actions.count(D), actions.count(S)) == (ins, dels, subs)
        assert correct + subs + dels == len(a) and correct + subs + ins == len(b)
        assert len(operations) <= len(a) + len(b)
        # (a match may pair different symbols of equal rows: the replay equals actual up to such pairs)
        assert [tuple(table[x]) for x in U.replay(a, b, operations)] == [tuple(table[x]) for x in b]
        longest = max(longest, min(len(a), len(b)))
    assert longest > 128


def test_unit_costs_with_an_identity_table_equal_the_uniform_restatement():
    rng = np.random.default_rng(77)
    identity = {s: [s] for s in range(5)}  # one column of ids: d(a, b) = (a != b)
    for q in range(400):
        alphabet = (2, 3, 5)[q % 3]
        a, b = _pair(rng, alphabet, q % 20 == 0)
        assert W.carried_statistics(a, b, 1.0, 1.0, identity)[0] == E.levensthein_statistics_fast(a, b)
        operations, cost = U.levensthein_operations_fast(a, b)
        got, got_cost, _ = W.kernel_form(a, b, 1.0, 1.0, identity)
        assert (got, float(got_cost)) == (operations, cost)
        if q % 20:
            assert W.levensthein_statistics(a, b, 1.0, 1.0, identity) == E.levensthein_statistics(a, b)
            assert W.levensthein_operations(a, b, 1.0, 1.0, None)[0] == U.levensthein_operations(a, b)[0]
            assert _bits(W.levensthein_matrix(a, b)) == _bits(U._matrix(a, b).astype(np.float32))


# t and T share a row; d differs from t in one feature, a from t in three and from d in two
TABLE = {"t": [0, 0, 0], "T": [0, 0, 0], "d": [0, 0, 1], "a": [1, 1, 1]}
HAND_WORKED = [
    # M = [[0 1 2] [1 2 1] [2 1 2]]: (1,1) = min(1 + 1, 1 + 1, 0 + d(t,a) = 3) = 2, (1,2) = 1 + d(t,t) = 1, (2,1) = 1 + d(a,a) = 1,
    # (2,2) = min(1 + 1, 1 + 1, 2 + 3) = 2.  Walk from (2,2): above 1 is not < left 1, so insertion; the diagonal 2 > 1: insertion
    # of actual[1] -> (2,1).  There above 2, left 2, the diagonal 1 <= 2 and equal to the cost 1: a match -> (1,0); column 0:
    # deletion of expected[0] -> (0,0).  Uniform costs give two substitutions instead.
    ("ta", "at", (1.0, 1.0), [(D, 0, 0), (I, 2, 1)], 2.0, (1, 1, 0, 1), [(S, 0, 0), (S, 1, 1)]),
    # M = [[0 1 2] [1 2 1] [2 3 2]]: (2,2) = min(3 + 1, 1 + 1, 2 + 0) = 2.  From (2,2): above 1 < left 3: deletion, the diagonal
    # 2 > 1, so expected[1] is deleted -> (1,2); there above 2 is not < left 2: insertion, the diagonal 1 <= 2 and equal to the
    # cost 1: a match -> (0,1); row 0: insertion of actual[0].  Uniform costs substitute t by a at cost 1.
    ("tt", "at", (1.0, 1.0), [(I, 0, 0), (D, 1, 2)], 2.0, (1, 1, 0, 1), [(S, 0, 0)]),
    # the walk reads the matrix alone: M = [[0 1] [1 2]], (1,1) = min(2, 2, 0 + 3) = 2 is the price of a deletion and an
    # insertion, yet from (1,1) the diagonal 0 <= left 1 and differs from 2: one substitution record, at a cost of 2
    ("t", "a", (1.0, 1.0), [(S, 0, 0)], 2.0, (0, 0, 1, 0), [(S, 0, 0)]),
    # different symbols with equal rows: M[1][1] = 0 + 0, the walk never starts: a match, no record
    ("t", "T", (1.0, 1.0), [], 0.0, (0, 0, 0, 1), [(S, 0, 0)]),
    # row 0 costs 1 per insertion whatever insertion_cost is: M = [[0 1 2 3] [.5 1 1.5 2]]: (1,1) = min(.5 + .5, 1 + .5, 0 + 1),
    # (1,2) = min(1 + .5, 2 + .5, 1 + 1), (1,3) = min(1.5 + .5, 3 + .5, 2 + 0).  From (1,3) cost 2: left 1.5 (insertion), the
    # diagonal 2 > 1.5: insert actual[2] -> (1,2); left 1, the diagonal 1 <= 1 but not the cost 1.5: substitution -> (0,1);
    # row 0: insert actual[0].  Uniform costs match the final t and insert d, d.
    ("t", "ddt", (0.5, 0.5), [(I, 0, 0), (S, 0, 1), (I, 1, 2)], 2.0, (2, 0, 1, 0), [(I, 0, 0), (I, 0, 1)]),
]


@pytest.mark.parametrize("expected,actual,costs,operations,cost,statistics,uniform", HAND_WORKED)
def test_hand_worked_cases(expected, actual, costs, operations, cost, statistics, uniform):
    assert W.levensthein_operations(expected, actual, *costs, TABLE) == (operations, cost)
    assert W.levensthein_statistics(expected, actual, *costs, TABLE) == statistics
    assert W.kernel_form(expected, actual, *costs, TABLE) == (operations, cost, statistics)
    assert W.carried_statistics(expected, actual, *costs, TABLE) == (statistics, cost)
    assert U.levensthein_operations(expected, actual)[0] == uniform


def test_column_zero_is_a_repeated_addition():
    matrix = W.matrix_fast("t" * 200, "", 0.3, 0.7, TABLE)
    column = np.float32(0)
    for i in range(1, 201):
        column = np.float32(column + np.float32(0.7))
        assert matrix[i, 0] == column
    assert matrix[200, 0] != np.float32(200) * np.float32(0.7)  # not the product
    assert _bits(matrix) == _bits(W.levensthein_matrix_weighted("t" * 200, "", 0.3, 0.7, TABLE))


def _library():
    from allophant_amd import lib

    if not os.path.exists(os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)):
        pytest.skip("library not built")
    return lib, lib.load()


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "edit_weighted.c"
    src.write_text('#include "allophant_amx_edit.h"\nint main(void) { size_t b; return amx_edit_cost_table_bytes(AMX_EDIT_MAX_SYMBOLS, &b)\n'
                   '    + amx_edit_cost_table(0, 0, 1, AMX_EDIT_MAX_FEATURES, 0, 0)\n'
                   '    + amx_edit_weighted_statistics(0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1.f, 1.f, 0, 0, 0, '
                   '0, 0, 0, 0)\n'
                   '    + amx_edit_weighted_operations(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1.f, 1.f, 0, 0, 0, 0, 0, '
                   '0, 0)\n'
                   '    + amx_edit_matrix(0, 0, 0, 0, 0, 0, 0, 0, 1.f, 1.f, 0, 0, 0, 0, 0, 0, 0); }\n')
    done = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


BAD_COSTS = [(float("nan"), 1.0), (1.0, float("nan")), (float("inf"), 1.0), (1.0, float("-inf")), (0.0, 1.0), (1.0, 0.0),
             (-1.0, 1.0), (1.0, -0.5)]


def test_exports_and_refusals():
    """Every documented AMX_EINVAL returns before any device call: the pointers handed over are never dereferenced."""
    lib, handle = _library()
    for symbol in ("amx_edit_cost_table_bytes", "amx_edit_cost_table", "amx_edit_weighted_statistics",
                   "amx_edit_weighted_operations", "amx_edit_matrix"):
        assert symbol in lib.EDIT_WEIGHTED_EXPORTS and hasattr(handle, symbol)
    assert (lib.EDIT_MAX_SYMBOLS, lib.EDIT_MAX_FEATURES) == (8192, 255)
    size = C.c_size_t()
    for V in (1, 7, 3300, 8192):
        assert handle.amx_edit_cost_table_bytes(V, C.byref(size)) == lib.AMX_OK and size.value == V * V
    for V in (0, -1, 8193):
        assert handle.amx_edit_cost_table_bytes(V, C.byref(size)) == lib.AMX_EINVAL
    assert handle.amx_edit_cost_table_bytes(4, None) == lib.AMX_EINVAL
    p = C.c_void_p(16)
    for V, F, codes, table in ((0, 3, p, p), (8193, 3, p, p), (4, 256, p, p), (4, -1, p, p), (4, 3, None, p), (4, 3, p, None)):
        assert handle.amx_edit_cost_table(0, codes, V, F, table, None) == lib.AMX_EINVAL, (V, F)

    def statistics(O=1, N=1, K=1, T=4, G=1, H=1, max_expected=8, max_actual=8, costs=(1.0, 1.0), null=False,
                   workspace_bytes=1 << 20, tables=p):
        q = None if null else p
        return handle.amx_edit_weighted_statistics(0, q, 4, 4, 4, O, N, K, T, q, None, q, q, q, G, q, q, q, q, H, max_expected,
                                                   max_actual, q, workspace_bytes, costs[0], costs[1], tables, None, q, q, q, q,
                                                   None)

    def operations(O=1, N=1, T=4, G=1, H=1, max_expected=8, max_actual=8, max_ops=16, costs=(1.0, 1.0), null=False,
                   workspace_bytes=1 << 20, tables=p):
        q = None if null else p
        return handle.amx_edit_weighted_operations(0, q, 4, 4, O, N, T, q, None, q, q, q, G, q, q, q, q, H, max_expected,
                                                   max_actual, q, workspace_bytes, costs[0], costs[1], tables, None, max_ops, q, q,
                                                   q, None)

    def matrix(rows=1, max_expected=8, max_actual=8, costs=(1.0, 1.0), V=0, table=None, null=False, workspace_bytes=1 << 20):
        q = None if null else p
        return handle.amx_edit_matrix(0, q, q, q, q, rows, max_expected, max_actual, costs[0], costs[1], table, V, q,
                                      workspace_bytes, q, q, None)

    for call in (statistics, operations, matrix):
        for costs in BAD_COSTS:
            assert call(costs=costs) == lib.AMX_EINVAL, (call.__name__, costs)
        assert b"costs" in handle.amx_last_error(None)
        assert call(max_expected=65536, **({"max_ops": 1 << 20} if call is operations else {})) == lib.AMX_EINVAL
        assert call(max_actual=-1) == lib.AMX_EINVAL
        assert call(null=True) == lib.AMX_EINVAL
        assert call(workspace_bytes=16) == lib.AMX_EINVAL
        assert b"workspace" in handle.amx_last_error(None)
    for call in (statistics, operations):  # the size limits of the uniform calls
        assert call(G=0) == lib.AMX_EINVAL and call(G=3, H=2) == lib.AMX_EINVAL
        assert call(O=-1) == lib.AMX_EINVAL and call(T=-1) == lib.AMX_EINVAL
        assert call(O=65536, N=65536) == lib.AMX_EINVAL
        assert call(tables=None) == lib.AMX_EINVAL
        assert call(O=0, null=True) == lib.AMX_OK and call(N=0, null=True) == lib.AMX_OK  # nothing to score
    assert statistics(K=0) == lib.AMX_EINVAL and statistics(K=65) == lib.AMX_EINVAL
    assert operations(max_ops=15) == lib.AMX_EINVAL  # below max_expected + max_actual
    assert operations(max_ops=2 ** 31) == lib.AMX_EINVAL
    assert matrix(V=8193, table=p) == lib.AMX_EINVAL and matrix(V=-1) == lib.AMX_EINVAL
    assert matrix(V=4, table=None) == lib.AMX_EINVAL  # a table announced and not given
    assert matrix(rows=-1) == lib.AMX_EINVAL and matrix(rows=2 ** 31) == lib.AMX_EINVAL
    assert matrix(rows=0, null=True) == lib.AMX_OK


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    """amx_edit_weighted.hip compiled for gfx950 (device ISA, -S): its five kernels, each with a private segment of 0 bytes
    and no spills, no inline assembly in the source or the shared include, and the sweep's lane shift done by DPP."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    source = os.path.join(ROOT, "allophant_amd", "csrc", "amx_edit_weighted.hip")
    out = tmp_path / "amx_edit_weighted.s"
    done = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(out), source],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    isa = out.read_text()
    kernels = ("edit_cost_table_kernel", "edit_weighted_rows_kernel", "edit_weighted_select_kernel", "edit_weighted_ops_kernel",
               "edit_matrix_kernel")
    for kernel in kernels:
        assert kernel in isa
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    spills = [int(v) for v in re.findall(r"\.(?:v|s)gpr_spill_count:\s+(\d+)", isa)]
    assert private == [0] * len(kernels) and spills == [0] * (2 * len(kernels)), isa[-3000:]
    assert "wave_shr:1" in isa
    for path in (source, os.path.join(ROOT, "allophant_amd", "csrc", "amx_edit_dp.inc")):
        with open(path, encoding="utf-8") as f:
            assert "asm" not in re.sub(r"//.*", "", f.read())


def test_property_weighting_on_the_host():
    import torch

    import allophant_amd
    from allophant_amd import evaluation

    for name in ("PropertyWeighting", "levensthein_matrix"):
        assert getattr(allophant_amd, name) is getattr(evaluation, name) and name in allophant_amd.__all__
    for costs in BAD_COSTS:
        with pytest.raises(ValueError, match="finite and above 0"):
            evaluation.PropertyWeighting(*costs, TABLE)
    with pytest.raises(TypeError):
        evaluation.PropertyWeighting(1.0, 1.0, 3)
    w = evaluation.PropertyWeighting(0.3, 0.7, TABLE)
    assert np.float32(w.insertion_cost) == np.float32(0.3) and w.deletion_cost == float(np.float32(0.7))
    # a missing symbol: KeyError naming it, before any device is looked for
    for method in (w.levensthein_statistics, w.levensthein_operations, w.levensthein_matrix):
        with pytest.raises(KeyError, match="x"):
            method(["t", "x"], ["a"])
    with pytest.raises(KeyError, match="7"):
        evaluation.PropertyWeighting(1.0, 1.0, [[0, 1], [1, 1]]).levensthein_statistics([0, 7], [1])
    assert w.has("t") and not w.has("x")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU"):
            w.levensthein_statistics("ta", "at")
        with pytest.raises(RuntimeError, match="no CPU"):
            evaluation.levensthein_matrix("ta", "at")

    # codes: per column the values numbered by first appearance; float, integer and tensor rows alike
    rows = {"p": [0.5, 2.0, -1.0], "q": [0.5, 3.0, -1.0], "r": [1.5, 2.0, -1.0], "s": [0.5, 2.0, -1.0]}
    codes = evaluation.PropertyWeighting(1.0, 1.0, rows).codes(list("pqrs"))
    assert codes.dtype == np.uint8 and codes.tolist() == [[0, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 0]]
    assert codes.tolist() == W.canonical_codes(np.asarray([rows[s] for s in "pqrs"])).tolist()
    tensors = {s: torch.tensor(r) for s, r in rows.items()}
    assert evaluation.PropertyWeighting(1.0, 1.0, tensors).codes(list("pqrs")).tolist() == codes.tolist()
    integers = torch.tensor([[7, 7], [7, 9], [8, 7]])
    assert evaluation.PropertyWeighting(1.0, 1.0, integers).codes([2, 0, 1]).tolist() == [[0, 0], [1, 0], [1, 1]]
    with pytest.raises(ValueError, match="width"):
        evaluation.PropertyWeighting(1.0, 1.0, {"p": [1], "q": [1, 2]}).codes(["p", "q"])
    with pytest.raises(ValueError, match="255"):
        evaluation.PropertyWeighting(1.0, 1.0, {"p": [0] * 256}).codes(["p"])
    with pytest.raises(ValueError, match="256 distinct"):
        evaluation.PropertyWeighting(1.0, 1.0, {s: [s] for s in range(300)}).codes(list(range(300)))
    assert evaluation.PropertyWeighting(1.0, 1.0, {s: [s % 256] for s in range(300)}).codes(list(range(300))).shape == (300, 1)


def test_attribute_table_property_table():
    from allophant_amd.phonetic import AttributeTable

    table = AttributeTable(E.synthetic_table_text(), ["syllabic", "long", "nasal", "phoneme"])
    properties = table.property_table()
    assert list(properties) == table.full_phonemes
    assert all(len(row) == len(table.full_feature_names) for row in properties.values())
    assert [properties[p] for p in table.full_phonemes] == table._dense_rows(table.full_phonemes, table.full_feature_names)
    assert properties["a"] == properties["e"] and properties["a"] != properties["m"]  # a and e share every feature
    assert table.property_table(["nasal"])["m"] != table.property_table(["nasal"])["a"]
    with pytest.raises(ValueError):
        table.property_table(["nasal", "phoneme"])


def test_evaluator_refuses_symbols_the_table_lacks():
    """Construction lists every symbol of an IPA id space that the property table lacks, before any device work: the check
    lives in ``Evaluator._init_weighting`` and needs only the host maps."""
    from allophant_amd import evaluation
    from allophant_amd.phonetic import AttributeTable

    table = AttributeTable(E.synthetic_table_text(), ["syllabic", "long", "nasal", "phoneme"])
    properties = table.property_table()
    evaluator = object.__new__(evaluation.Evaluator)  # no device: the host half only
    evaluator.maps = evaluation.EvaluationMaps(table, ["nasal", "phoneme"], ["a", "ts", "m"], ["lg0"], split_complex=True)
    evaluator.device = None
    space = set(evaluator.maps.spaces[1])
    lacking = sorted(space - set(properties))
    assert lacking  # split_complex makes segments the table does not list
    with pytest.raises(ValueError) as refusal:
        evaluator._init_weighting(evaluation.PropertyWeighting(1.0, 1.0, properties))
    assert all(repr(s) in str(refusal.value) for s in lacking)
    import inspect

    assert "weighting" in inspect.signature(evaluation.Evaluator.__init__).parameters
    assert hasattr(evaluation.Evaluator, "costs")

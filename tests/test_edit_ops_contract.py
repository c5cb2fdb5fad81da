"""The edit-operations contract on the host (no GPU): the literal restatement of upstream's ``levensthein_operations``
(tests/edit_ops_util.py) on the hand-worked table, the form the kernel computes (move codes per wave step, a windowed walk
that stops after `cost` operations) against it on thousands of random pairs with its invariants, the ``UtteranceEdits`` JSON
line pinned literally, and the C ABI's header, exports, workspace sizes, refusals and compiled ISA."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import edit_ops_util as U
import edit_util as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HAND_WORKED = [
    ("abc", "ac", [(U.DELETION, 1, 1)], 1.0),
    ("aab", "ab", [(U.DELETION, 1, 1)], 1.0),  # the second a
    ("ab", "aab", [(U.INSERTION, 1, 1)], 1.0),
    ("ab", "ba", [(U.SUBSTITUTION, 0, 0), (U.SUBSTITUTION, 1, 1)], 2.0),
    ("abcd", "xbcdy", [(U.SUBSTITUTION, 0, 0), (U.INSERTION, 4, 4)], 2.0),
    ("", "xy", [(U.INSERTION, 0, 0), (U.INSERTION, 0, 1)], 2.0),
    ("abc", "", [(U.DELETION, 0, 0), (U.DELETION, 1, 0), (U.DELETION, 2, 0)], 3.0),
    ("abc", "abc", [], 0.0),
]


@pytest.mark.parametrize("expected,actual,operations,cost", HAND_WORKED)
def test_hand_worked_table(expected, actual, operations, cost):
    assert U.levensthein_operations(expected, actual) == (operations, cost)
    assert U.kernel_form(expected, actual)[:2] == (operations, cost)
    assert U.replay(list(expected), list(actual), operations) == list(actual)


def _pairs(rng, alphabet, count):
    for q in range(count):
        m, n = (int(v) for v in rng.integers(0, 141, 2))
        a = rng.integers(0, alphabet, m).tolist()
        b = rng.integers(0, alphabet, n).tolist()
        if q % 3 == 0:  # a shared prefix
            p = int(rng.integers(0, min(m, n) + 1))
            b[:p] = a[:p]
        yield a, b


@pytest.mark.parametrize("alphabet,count", [(2, 1334), (3, 1333), (5, 1333)])
def test_kernel_form_equals_the_walk(alphabet, count):
    """On 4000 random pairs (lengths 0-140, a third with shared prefixes): the kernel's form equals the literal walk; the
    operation count is the cost and at most max(m, n); the S, D, I counts are the statistics of the same walk; replaying the
    operations turns expected into actual; one window load serves at least 32 moves inside a strip."""
    rng = np.random.default_rng(alphabet)
    for a, b in _pairs(rng, alphabet, count):
        operations, cost = U.levensthein_operations(a, b)
        got, got_cost, moves, loads = U.kernel_form(a, b)
        assert (got, got_cost) == (operations, cost), (a, b)
        assert len(operations) == cost <= max(len(a), len(b))
        assert cost == E.levenshtein(a, b)
        ins, dels, subs, _ = E.levensthein_statistics(a, b)
        actions = [op[0] for op in operations]
        assert (actions.count(U.INSERTION), actions.count(U.DELETION), actions.count(U.SUBSTITUTION)) == (ins, dels, subs)
        assert U.replay(a, b, operations) == b
        assert loads <= (len(a) + 63) // 64 + moves // 32 + 1


def test_utterance_edits_json_pinned():
    from allophant_amd.evaluation import Action, UtteranceEdits, to_substitutions

    expected = ["t͡ʃ", "a", "ʃ"]
    actual = ["ts", "ɛ", "ʃ", "m"]
    operations = [(Action.SUBSTITUTION, 0, 0), (Action.SUBSTITUTION, 1, 1), (Action.INSERTION, 3, 3)]
    assert U.levensthein_operations(expected, actual) == ([tuple(map(int, op)) for op in operations], 3.0)
    edits = UtteranceEdits("lg0", "utt 7", {"phoneme": expected, "syllabic": ["+", "-"]},
                           {"phoneme": to_substitutions(expected, actual, operations),
                            "syllabic": to_substitutions(["+", "-"], ["+"], [(Action.DELETION, 1, 1)])})
    line = edits.to_json()
    assert line == ('{"language": "lg0", "utterance_id": "utt 7", "expected": {"phoneme": ["t\\u0361\\u0283", "a", "\\u0283"], '
                    '"syllabic": ["+", "-"]}, "edit_operations": {"phoneme": [[3, "t\\u0361\\u0283", "ts"], [3, "a", "\\u025b"], '
                    '[1, "", "m"]], "syllabic": [[2, "-", ""]]}}')
    assert json.loads(line) == edits.to_dict()
    back = UtteranceEdits.from_json(line)
    assert back == edits and back.to_json() == line
    assert all(isinstance(op[0], Action) for ops in back.edit_operations.values() for op in ops)
    assert Action.from_int(2) is Action.DELETION and int(Action.INSERTION) == 1
    reference = U.compute_edits("lg0", "utt 7", ["phoneme"], ["t͡ʃ", "a", "ʃ"], {"phoneme": [actual, ["x"]]}, {}, None, False)
    assert U.to_json(reference) == UtteranceEdits.from_dict(reference).to_json()


def _library():
    from allophant_amd import lib

    if not os.path.exists(os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)):
        pytest.skip("library not built")
    return lib, lib.load()


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "edit_ops.c"
    src.write_text('#include "allophant_amx_edit.h"\nint main(void) { size_t b; return amx_edit_operations_workspace(1, 1, 1, &b) '
                   '+ AMX_EDIT_INSERTION + AMX_EDIT_DELETION + AMX_EDIT_SUBSTITUTION\n    + amx_edit_operations(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, '
                   '0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    done = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_exports_workspace_and_refusals():
    lib, handle = _library()
    for symbol in ("amx_edit_operations_workspace", "amx_edit_operations"):
        assert symbol in lib.EDIT_EXPORTS and hasattr(handle, symbol)
    size = C.c_size_t()
    pad = lambda v: (v + 15) // 16 * 16  # noqa: E731
    for rows, m, n in ((10, 100, 200), (1216, 216, 499), (3, 0, 7), (1, 64, 0), (1, 65, 1)):
        assert handle.amx_edit_operations_workspace(rows, m, n, C.byref(size)) == lib.AMX_OK
        codes = (m + 63) // 64 * pad(n + 64) * 4
        assert size.value == rows * 4 * (pad(m) + pad(n) + 4 * pad(n + 1) + codes), (rows, m, n)
    assert handle.amx_edit_operations_workspace(2 ** 31 - 1, 65535, 65535, C.byref(size)) == lib.AMX_OK
    for bad in ((1, 65536, 1), (1, 1, 65536), (-1, 1, 1), (2 ** 31, 1, 1), (1, -1, 1)):
        assert handle.amx_edit_operations_workspace(*bad, C.byref(size)) == lib.AMX_EINVAL
    assert handle.amx_edit_operations_workspace(1, 1, 1, None) == lib.AMX_EINVAL

    def call(O=1, N=1, T=4, G=1, H=1, max_expected=8, max_actual=8, max_ops=8, null=False, workspace_bytes=1 << 20):
        p = None if null else C.c_void_p(16)  # never dereferenced: every refused call returns before any device work
        return handle.amx_edit_operations(0, p, 4, 4, O, N, T, p, None, p, p, p, G, p, p, p, p, H, max_expected, max_actual, p,
                                          workspace_bytes, max_ops, p, p, None)

    assert call(max_ops=7) == lib.AMX_EINVAL and call(max_actual=4, max_expected=9, max_ops=8) == lib.AMX_EINVAL
    assert call(max_ops=2 ** 31) == lib.AMX_EINVAL
    assert call(max_expected=65536, max_ops=65536) == lib.AMX_EINVAL and call(max_actual=-1) == lib.AMX_EINVAL
    assert call(G=0) == lib.AMX_EINVAL and call(G=3, H=2) == lib.AMX_EINVAL
    assert call(O=-1) == lib.AMX_EINVAL and call(T=-1) == lib.AMX_EINVAL
    assert call(O=65536, N=65536) == lib.AMX_EINVAL
    assert call(null=True) == lib.AMX_EINVAL
    assert call(workspace_bytes=16) == lib.AMX_EINVAL
    assert b"workspace" in handle.amx_last_error(None)
    assert call(O=0, null=True) == lib.AMX_OK and call(N=0, null=True) == lib.AMX_OK  # nothing to walk


def test_python_surface_without_a_gpu():
    import torch

    from allophant_amd import evaluation

    if torch.cuda.is_available():
        pytest.skip("checks the refusal without a GPU")
    with pytest.raises(RuntimeError, match="no CPU"):
        evaluation.levensthein_operations("ab", "ba")
    with pytest.raises(RuntimeError, match="no CPU"):
        evaluation.levensthein_operations_batch(["ab"], ["ba"])
    with pytest.raises(RuntimeError, match="no CPU"):
        evaluation.levensthein_substitutions(["a"], ["b"])
    assert evaluation.to_substitutions(["a", "b"], ["c"], [(3, 0, 0), (2, 1, 1)]) == [
        (evaluation.Action.SUBSTITUTION, "a", "c"), (evaluation.Action.DELETION, "b", "")]
    import allophant_amd

    for name in ("Action", "UtteranceEdits", "levensthein_operations", "levensthein_operations_batch",
                 "levensthein_substitutions", "to_substitutions"):
        assert getattr(allophant_amd, name) is getattr(evaluation, name)
        assert name in allophant_amd.__all__
    assert hasattr(evaluation.Evaluator, "operations") and hasattr(evaluation.Evaluator, "edits")


def test_kernel_has_no_scratch_and_no_spills(tmp_path):
    """amx_edit_ops.hip compiled for gfx950 (device ISA, -S): one kernel, a private segment of 0 bytes, no spills, no inline
    assembly, and the sweep's lane shift done by DPP."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    source = os.path.join(ROOT, "allophant_amd", "csrc", "amx_edit_ops.hip")
    out = tmp_path / "amx_edit_ops.s"
    done = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(out), source],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    isa = out.read_text()
    assert "edit_ops_kernel" in isa
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    spills = [int(v) for v in re.findall(r"\.(?:v|s)gpr_spill_count:\s+(\d+)", isa)]
    assert private == [0] and spills == [0, 0], isa[-3000:]
    assert "wave_shr:1" in isa
    for path in (source, os.path.join(ROOT, "allophant_amd", "csrc", "amx_edit_dp.inc")):
        with open(path, encoding="utf-8") as f:
            assert "asm" not in re.sub(r"//.*", "", f.read())

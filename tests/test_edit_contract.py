"""The evaluation contract on the host (no GPU): the literal restatement of upstream's back-trace (tests/edit_util.py) on
hand-worked pairs that each decide one rule, its invariants and the forward-carried form the kernel computes on thousands of
random pairs, fp32 error rates bit for bit against recorded upstream results, the JSON round trip with rebuilt totals, the
host map builder against the string path, and the C ABI's header, exports, limits and compiled ISA."""
import ctypes as C
import json
import math
import os
import re
import shutil
import subprocess
import unicodedata

import numpy as np
import pytest

import edit_util as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("g18_eval_baseline_ucla.json", "g18b_eval_hierarchical_commonvoice.json")


@pytest.mark.parametrize("expected,actual,stats", [
    ("acba", "bab", (1, 2, 0, 2)),  # at (4, 3) deletion and insertion tie: insertion (deletion first would give (0, 1, 2, 1))
    ("a", "ba", (1, 0, 0, 1)),      # at (1, 1) the diagonal ties the cheaper neighbour and wins (`<=`, not `<`)
    ("ab", "abx", (1, 0, 0, 2)),    # the walk stops at the zero-cost cell (2, 2): correct += 2
    ("ab", "xab", (1, 0, 0, 2)),
    ("", "abc", (3, 0, 0, 0)),      # i == 0: insertions
    ("abc", "", (0, 3, 0, 0)),      # j == 0: deletions
    ("", "", (0, 0, 0, 0)),
    ("abc", "abc", (0, 0, 0, 3)),
    ("a", "b", (0, 0, 1, 0)),
])
def test_hand_worked_rules(expected, actual, stats):
    assert E.levensthein_statistics(expected, actual) == stats
    assert E.carried_statistics(expected, actual) == stats


@pytest.mark.parametrize("alphabet", [2, 3, 4, 50])
def test_random_pairs_invariants_and_carried_form(alphabet):
    """I + D + S is the Levenshtein distance, C = m - S - D, I + C + S = n, and the forward-carried form (no matrix, no
    back-trace) and the numpy-filled matrix the GPU tests use equal the back-trace on every pair."""
    rng = np.random.default_rng(alphabet)
    for _ in range(1000):
        a = rng.integers(0, alphabet, rng.integers(0, 31)).tolist()
        b = rng.integers(0, alphabet, rng.integers(0, 31)).tolist()
        ins, dels, subs, correct = stats = E.levensthein_statistics(a, b)
        assert ins + dels + subs == E.levenshtein(a, b)
        assert correct == len(a) - subs - dels and ins + correct + subs == len(b)
        assert E.carried_statistics(a, b) == stats, (a, b)
        assert E.levensthein_statistics_fast(a, b) == stats, (a, b)


def test_word_error_rate_special_cases():
    from allophant_amd.evaluation import EditStatistics

    assert math.isnan(EditStatistics.zeros().word_error_rate())
    assert EditStatistics(3, 0, 0, 0).word_error_rate() == math.inf
    s = EditStatistics(1, 2, 3, 4)
    assert s.word_error_rate() == float(np.float32(6) / np.float32(9))
    assert s.substitution_rate() == float(np.float32(3) / np.float32(9))
    assert s.insertion_rate() == float(np.float32(1) / np.float32(9))
    assert s.deletion_rate() == float(np.float32(2) / np.float32(9))
    assert s + EditStatistics(1, 1, 1, 1) == EditStatistics(2, 3, 4, 5)
    assert EditStatistics.from_dict(s.to_dict()) == s
    with pytest.raises(ValueError):
        EditStatistics.from_dict({"insertions": 1})
    assert E.best_candidate("ab", ["xy", "ab", "ab"])[0] == 1  # equal rates: the first wins
    assert E.best_candidate("", ["a", ""]) == (-1, None)       # inf and NaN are never below inf


@pytest.mark.parametrize("fixture", FIXTURES)
def test_recorded_rates_bit_for_bit(fixture):
    """Every error rate upstream recorded comes out of its statistics bit for bit in fp32, and every total is the integer
    sum of its languages."""
    from allophant_amd.evaluation import EditStatistics, MultilingualEvaluationResults

    with open(os.path.join(GOLDEN, fixture), encoding="utf-8") as f:
        raw = json.load(f)
    count = 0
    for language, results in raw["results"].items():
        for name, stats in results["error_statistics"].items():
            s = EditStatistics.from_dict(stats)
            assert s.word_error_rate() == results["error_rates"][name], (language, name)
            assert float(E.word_error_rate(s.astuple())) == results["error_rates"][name]
            count += 1
    assert count > 80
    loaded = MultilingualEvaluationResults.from_dict(raw)
    rebuilt = loaded.with_totals()
    assert rebuilt.to_dict() == loaded.to_dict()
    assert json.loads(loaded.dumps()) == raw
    assert MultilingualEvaluationResults.loads(rebuilt.dumps()).to_dict() == raw
    assert "total" in str(loaded) and loaded.package_version == raw["package_version"]


def _table():
    from allophant_amd.phonetic import AttributeTable

    return AttributeTable(E.synthetic_table_text(), ["syllabic", "long", "nasal", "phoneme"])


@pytest.mark.parametrize("split_complex", [False, True])
@pytest.mark.parametrize("remap", [False, True])
def test_maps_against_the_string_path(split_complex, remap):
    """The host maps, expanded back to strings, equal what upstream compares: labels through contours, replacements and
    splitting; tokens through the blank offset, the per-language remap and splitting."""
    from allophant_amd.evaluation import EvaluationMaps, unicode_replacements
    from allophant_amd.phonetic import split_complex_segment

    table = _table()
    names = ["syllabic", "long", "nasal", "phoneme"]
    inventory = ["a", "ts", "t͡ʃ", "é", "m", "aː", "i"]
    decomposed = unicodedata.normalize("NFD", "é")
    replacements = unicode_replacements(table, table.full_phonemes + [decomposed])
    assert replacements == {decomposed: "é"}
    languages = ["lg0", "lg1"]
    source_maps = {"lg0": {p: p for p in inventory}, "lg1": {**{p: p for p in inventory}, "ts": "s", "a": "t͡ʃ"}} if remap else None
    maps = EvaluationMaps(table, names, inventory, languages, split_complex, source_maps, replacements)
    contours = {p: {n: table.feature_contour(p, n) for n in names[:3]} for p in table.full_phonemes}
    rng = np.random.default_rng(3)
    symbols = table.full_phonemes + [decomposed]
    for _ in range(200):
        label = [symbols[i] for i in rng.integers(0, len(symbols), rng.integers(0, 12))]
        length = rng.integers(0, 12)
        for o, name in enumerate(names):
            classes = len(inventory) if name == "phoneme" else len(table.feature_categories(name))
            tokens = rng.integers(1, classes + 1, length).tolist()
            expected = E.expected_symbols(name, label, contours, split_complex_segment, split_complex, replacements)
            assert maps.expand_label(o, label) == expected
            for h, language in enumerate(languages):
                if name == "phoneme":
                    candidate = [inventory[t - 1] for t in tokens]
                else:
                    candidate = table.feature_values(name, [t - 1 for t in tokens])
                source = source_maps[language] if remap else None
                actual = E.actual_symbols(name, candidate, split_complex_segment, split_complex, source)
                assert maps.expand_tokens(o, h, tokens) == actual
    assert maps.expand_tokens(3, 0, [0]) == []  # the blank expands to nothing
    with pytest.raises(IndexError):
        maps.expand_tokens(3, 0, [len(inventory) + 1])
    with pytest.raises(ValueError, match="Missing feature"):
        EvaluationMaps(table, ["stress"], inventory, languages)
    with pytest.raises(ValueError, match="No suitable mapping"):
        unicode_replacements(table, ["q"])


def _library():
    from allophant_amd import lib

    if not os.path.exists(os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)):
        pytest.skip("library not built")
    return lib, lib.load()


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "edit.c"
    src.write_text('#include "allophant_amx_edit.h"\nint main(void) { size_t b; return amx_edit_workspace(1, 1, 1, &b) + '
                   'AMX_EDIT_MAX_LENGTH + AMX_EDIT_MAX_CANDIDATES; }\n')
    done = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_exports_workspace_and_limits():
    lib, handle = _library()
    for symbol in lib.EDIT_EXPORTS:
        assert hasattr(handle, symbol)
    size = C.c_size_t()
    assert handle.amx_edit_workspace(10, 100, 200, C.byref(size)) == lib.AMX_OK
    pad = lambda v: (v + 15) // 16 * 16  # noqa: E731
    assert size.value == 10 * 4 * (pad(100) + pad(200) + 4 * pad(201))
    assert handle.amx_edit_workspace(1, 65535, 65535, C.byref(size)) == lib.AMX_OK
    for bad in ((1, 65536, 1), (1, 1, 65536), (-1, 1, 1), (1, -1, 1)):
        assert handle.amx_edit_workspace(*bad, C.byref(size)) == lib.AMX_EINVAL
    assert handle.amx_edit_workspace(1, 1, 1, None) == lib.AMX_EINVAL

    def call(O=1, N=1, K=1, T=4, G=1, H=1, max_expected=8, max_actual=8, null=False, workspace_bytes=1 << 20):
        p = None if null else C.c_void_p(16)  # never dereferenced: every refused call returns before any device work
        return handle.amx_edit_statistics(0, p, 4, 4, 4, O, N, K, T, p, None, p, p, p, G, p, p, p, p, H, max_expected,
                                          max_actual, p, workspace_bytes, p, p, p, None)

    assert call(K=0) == lib.AMX_EINVAL and call(K=65) == lib.AMX_EINVAL
    assert call(max_expected=65536) == lib.AMX_EINVAL and call(max_actual=65536) == lib.AMX_EINVAL
    assert call(G=0) == lib.AMX_EINVAL and call(G=3, H=2) == lib.AMX_EINVAL
    assert call(O=-1) == lib.AMX_EINVAL and call(T=-1) == lib.AMX_EINVAL
    assert call(O=65536, N=65536) == lib.AMX_EINVAL
    assert call(null=True) == lib.AMX_EINVAL
    assert call(workspace_bytes=16) == lib.AMX_EINVAL
    assert b"workspace" in handle.amx_last_error(None)
    assert call(O=0, null=True) == lib.AMX_OK and call(N=0, null=True) == lib.AMX_OK  # nothing to score


def test_python_surface_without_a_gpu():
    import torch

    from allophant_amd import evaluation

    if torch.cuda.is_available():
        pytest.skip("checks the refusal without a GPU")
    with pytest.raises(RuntimeError, match="no CPU"):
        evaluation.levensthein_statistics("ab", "ab")
    with pytest.raises(RuntimeError, match="no CPU"):
        evaluation.Evaluator(_table(), ["phoneme"], ["a"], ["lg0"])
    import allophant_amd

    for name in ("EditStatistics", "Evaluator", "EvaluationResults", "MultilingualEvaluationResults", "levensthein_statistics"):
        assert getattr(allophant_amd, name) is getattr(evaluation, name)


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    """amx_edit.hip compiled for gfx950 (device ISA, -S): both kernels with a private segment of 0 bytes and no spills, and
    the wavefront's lane shift done by DPP."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "amx_edit.s"
    done = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(out),
                           os.path.join(ROOT, "allophant_amd", "csrc", "amx_edit.hip")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    isa = out.read_text()
    assert "edit_rows_kernel" in isa and "edit_select_kernel" in isa
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    spills = [int(v) for v in re.findall(r"\.(?:v|s)gpr_spill_count:\s+(\d+)", isa)]
    assert private == [0, 0] and spills == [0, 0, 0, 0], isa[-3000:]
    assert "wave_shr:1" in isa

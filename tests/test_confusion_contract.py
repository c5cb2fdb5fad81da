"""The confusion-table contract on the host (no GPU): the restatement from upstream's records (tests/confusion_util.py)
satisfies the identities that tie it to upstream's statistics, uniform and weighted; the form the kernels compute equals it;
the C ABI's header, exports and refusals; and ``ConfusionTable`` on a hand-written table."""
import ctypes as C
import itertools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import confusion_util as CU
import edit_util as E
import edit_weighted_util as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COSTS = [(1.0, 1.0), (0.3, 0.7), (2.5, 0.1), (1.7, 3.3)]
EPS = CU.EPSILON


def _fixed_cases(alphabet):
    """Every combination of empty and non-empty, identical sequences, all-different sequences."""
    x = [s % alphabet for s in range(7)]
    cases = [([], []), ([], x), (x, []), (x, x[:4]), (x, list(x)), ([0] * 5, [1] * 5), ([0] * 3, [1] * 6), ([1] * 6, [0] * 2)]
    if alphabet >= 12:
        cases.append((list(range(6)), list(range(6, 12))))
    return cases


def _random_pairs(rng, alphabet, count):
    for _ in range(count):
        m, n = (int(v) for v in rng.integers(0, 13, 2))
        a, b = rng.integers(0, alphabet, m).tolist(), rng.integers(0, alphabet, n).tolist()
        if rng.integers(0, 3) == 0:  # a shared prefix: the walk stops early and the tail is long
            p = int(rng.integers(0, min(m, n) + 1))
            b[:p] = a[:p]
        yield a, b


def _diagonal(found):
    return sum(c for (e, a), c in found.items() if e is not EPS and a is not EPS)


@pytest.mark.parametrize("alphabet", [2, 3, 40])
def test_uniform_identities(alphabet):
    """Substitutions, deletions, insertions and matches of the events are exactly upstream's statistics of the row; the
    number of events is m + n - #diagonal; the kernels' form gives the same events."""
    rng = np.random.default_rng(alphabet)
    for a, b in itertools.chain(_fixed_cases(alphabet), _random_pairs(rng, alphabet, 400)):
        found = CU.events(a, b)
        assert CU.statistics(found) == E.levensthein_statistics(a, b), (a, b)
        assert CU.event_count(found) == len(a) + len(b) - _diagonal(found)
        assert sum(c for (e, _), c in found.items() if e is not EPS) == len(a)
        assert sum(c for (_, x), c in found.items() if x is not EPS) == len(b)
        assert CU.events(a, b, fast=True) == found
        kernel, count = CU.kernel_form(a, b)
        assert kernel == found and count == CU.event_count(found), (a, b)


def _table(rng, alphabet):
    rows = rng.integers(0, 2, (alphabet, int(rng.integers(1, 6))))
    if alphabet > 2:
        rows[alphabet - 1] = rows[0]  # two different symbols with equal rows: a pair of cost 0
    return {s: rows[s] for s in range(alphabet)}


@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("alphabet", [2, 3, 40])
def test_weighted_identities(alphabet, costs):
    """Pairs of table cost 0 sum to C and pairs of cost > 0 to S of upstream's weighted statistics; D and I as the uniform."""
    rng = np.random.default_rng(alphabet * 1000 + int(costs[0] * 10) * 100 + int(costs[1] * 10))
    seen_zero_cost_pair = False
    for q, (a, b) in enumerate(itertools.chain(_fixed_cases(alphabet), _random_pairs(rng, alphabet, 150))):
        table = _table(rng, alphabet)
        zero = lambda e, x: W.substitution_cost(table, e, x) == 0  # noqa: E731
        found = CU.weighted_events(a, b, *costs, table)
        assert CU.statistics(found, zero) == W.levensthein_statistics(a, b, *costs, table), (a, b)
        assert CU.event_count(found) == len(a) + len(b) - _diagonal(found)
        assert CU.weighted_events(a, b, *costs, table, fast=True) == found
        kernel, count = CU.kernel_form(a, b, *costs, table)
        assert kernel == found and count == CU.event_count(found), (a, b)
        seen_zero_cost_pair |= any(e is not EPS and x is not EPS and e != x and zero(e, x) for e, x in found)
    assert seen_zero_cost_pair or alphabet == 2


def _library():
    from allophant_amd import lib

    if not os.path.exists(os.path.join(ROOT, "allophant_amd", lib.LIB_NAME)):
        pytest.skip("library not built")
    return lib, lib.load()


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "edit_confusion.c"
    head = "0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0"
    src.write_text('#include "allophant_amx_edit.h"\nint main(void) { size_t b;\n'
                   '    return amx_edit_confusion_table_bytes(AMX_EDIT_CONFUSION_MAX_CAPACITY, &b)\n'
                   '    + AMX_EDIT_CONFUSION_GROUP_BITS + 2 * AMX_EDIT_CONFUSION_SYMBOL_BITS - 64 + AMX_EDIT_CONFUSION_MIN_CAPACITY\n'
                   f'    + amx_edit_confusions({head}, 0, 0, 16, 0, 0, 0)\n'
                   f'    + amx_edit_weighted_confusions({head}, 1.f, 1.f, 0, 0, 0, 0, 16, 0, 0, 0)\n'
                   '    + amx_edit_confusion_merge(0, 0, 16, 0, 16, 0, 0); }\n')
    done = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_table_bytes_exports_and_refusals():
    """The valid capacities are the powers of two from 16 to 2^28; every documented AMX_EINVAL returns before any device call:
    the pointers handed over are never dereferenced."""
    lib, handle = _library()
    for symbol in ("amx_edit_confusion_table_bytes", "amx_edit_confusions", "amx_edit_weighted_confusions",
                   "amx_edit_confusion_merge"):
        assert symbol in lib.EDIT_CONFUSION_EXPORTS and hasattr(handle, symbol)
    assert lib.EDIT_CONFUSION_GROUP_BITS + 2 * lib.EDIT_CONFUSION_SYMBOL_BITS == 64
    size = C.c_size_t()
    for exponent in range(4, 29):
        assert handle.amx_edit_confusion_table_bytes(2 ** exponent, C.byref(size)) == lib.AMX_OK
        assert size.value == 16 * 2 ** exponent
    for bad in (0, 1, 8, -16, 17, 24, 48, 1000, 2 ** 20 - 1, 2 ** 20 + 1, 3 * 2 ** 19, 2 ** 29, 2 ** 40):
        assert handle.amx_edit_confusion_table_bytes(bad, C.byref(size)) == lib.AMX_EINVAL, bad
    assert handle.amx_edit_confusion_table_bytes(16, None) == lib.AMX_EINVAL
    p = C.c_void_p(16)

    def call(O=1, N=1, K=1, T=4, G=1, H=1, max_expected=8, max_actual=8, capacity=16, null=False, workspace_bytes=1 << 20,
             costs=None):
        q = None if null else p
        head = (0, q, 4, 4, 4, O, N, K, T, q, None, q, q, q, G, q, q, q, q, H, max_expected, max_actual, q, workspace_bytes)
        tail = (None, q, capacity, q, q, None)
        if costs is None:
            return handle.amx_edit_confusions(*head, *tail)
        return handle.amx_edit_weighted_confusions(*head, costs[0], costs[1], q, None, *tail)

    for costs in (None, (1.0, 1.0)):
        for bad in (dict(O=-1), dict(K=0), dict(K=65), dict(max_expected=65536), dict(max_actual=-1), dict(G=0), dict(G=3, H=2),
                    dict(capacity=8), dict(capacity=24), dict(capacity=2 ** 29), dict(null=True), dict(workspace_bytes=16)):
            assert call(costs=costs, **bad) == lib.AMX_EINVAL, bad
        assert call(costs=costs, N=0) == lib.AMX_OK  # nothing to do
    for costs in ((float("nan"), 1.0), (1.0, float("inf")), (0.0, 1.0), (1.0, -1.0)):
        assert call(costs=costs) == lib.AMX_EINVAL
    for bad in ((None, 16, p, 16, p), (p, 16, None, 16, p), (p, 16, p, 16, None), (p, 8, C.c_void_p(4096), 16, p),
                (p, 16, C.c_void_p(4096), 48, p), (p, 16, C.c_void_p(16 + 8 * 16), 16, p)):  # (the last: overlapping tables)
        src, src_capacity, dst, dst_capacity, counters = bad
        assert handle.amx_edit_confusion_merge(0, src, src_capacity, dst, dst_capacity, counters, None) == lib.AMX_EINVAL, bad


# a hand-written table: two languages, two outputs; output "phoneme" over the synthetic table's phonemes
SYMBOLS = [["a", "e", "t", "s", "m"], ["-", "+"]]
ENTRIES = [  # (language, output, expected, actual, count), unsorted, one key twice
    (0, 0, 0, 0, 10), (0, 0, 0, 1, 3), (0, 0, 1, 0, 3), (0, 0, 2, 3, 5), (0, 0, 2, -1, 2), (0, 0, -1, 4, 4), (0, 0, 2, 2, 7),
    (0, 0, 0, 1, 1), (1, 0, 4, 4, 6), (1, 0, 4, 0, 1), (0, 1, 0, 1, 2), (0, 1, 1, 1, 9),
]


def _hand_table():
    from allophant_amd.confusion import ConfusionTable

    return ConfusionTable(["lg0", "lg1"], ["phoneme", "nasal"], SYMBOLS, *zip(*ENTRIES))


def test_confusion_table_queries():
    from allophant_amd.evaluation import EditStatistics

    t = _hand_table()
    assert len(t) == len(ENTRIES) - 1 and t.total() == sum(e[4] for e in ENTRIES)
    keys = list(zip(t.group.tolist(), t.output.tolist(), t.expected.tolist(), t.actual.tolist()))
    assert keys == sorted(keys) and keys[0] == (0, 0, -1, 4)  # canonical order, epsilon (-1) first
    assert t.pairs("lg0", "phoneme") == [("t", "s", 5), ("a", "e", 4), ("e", "a", 3)]  # substitutions by default
    assert t.pairs("lg0", "phoneme", k=1) == [("t", "s", 5)]
    assert t.pairs("lg0", "phoneme", kind="deletion") == [("t", "", 2)]
    assert t.pairs("lg0", "phoneme", kind="insertion") == [("", "m", 4)]
    assert t.pairs("lg0", "phoneme", kind="correct") == [("a", "a", 10), ("t", "t", 7)]
    everything = t.pairs("lg0", "phoneme", kind=None)
    assert len(everything) == 7 and everything[0] == ("a", "a", 10) and sum(c for _, _, c in everything) == 35
    assert t.pairs(1, 0, kind=None) == [("m", "m", 6), ("m", "a", 1)]  # by index
    assert t.pairs("lg1", "nasal", kind=None) == []
    with pytest.raises(KeyError):
        t.pairs("lg2", "phoneme")
    with pytest.raises(ValueError):
        t.pairs("lg0", "phoneme", kind="swap")
    with pytest.raises(ValueError):
        t.pairs()  # two languages: name one

    symbols, counts = t.matrix("lg0", "phoneme")
    assert symbols == ["a", "e", "t", "s", "m", ""]  # the symbols that occur, epsilon last
    expected = np.zeros((6, 6), dtype=np.int64)
    for e, a, c in ((0, 0, 10), (0, 1, 4), (1, 0, 3), (2, 3, 5), (2, 5, 2), (5, 4, 4), (2, 2, 7)):
        expected[e, a] = c
    assert counts.dtype == np.int64 and np.array_equal(counts, expected)
    symbols, counts = t.matrix("lg1", "phoneme")
    assert symbols == ["a", "m", ""] and counts.tolist() == [[0, 0, 0], [1, 6, 0], [0, 0, 0]]

    statistics = t.statistics()
    assert statistics["lg0"]["phoneme"] == EditStatistics(insertions=4, deletions=2, substitutions=12, correct=17)
    assert statistics["lg1"]["phoneme"] == EditStatistics(0, 0, 1, 6)
    assert statistics["lg0"]["nasal"] == EditStatistics(0, 0, 2, 9)
    assert statistics["lg1"]["nasal"] == EditStatistics.zeros()


def test_attribute_confusions():
    from allophant_amd.phonetic import AttributeTable

    table = AttributeTable(E.synthetic_table_text(), ["syllabic", "long", "nasal", "phoneme"])
    projected = _hand_table().attribute_confusions(table, "lg0", "phoneme")
    assert list(projected) == table.full_feature_names
    # the pairs with two phonemes: a-a 10, a-e 4, e-a 3, t-s 5, t-t 7 (a, e syllabic +; t, s syllabic -; none nasal)
    values, counts = projected["syllabic"]
    assert values == ["+", "-"] and counts.tolist() == [[17, 0], [0, 12]]
    values, counts = projected["nasal"]
    assert values == ["-"] and counts.tolist() == [[29]]
    values, counts = _hand_table().attribute_confusions(table, "lg1", "phoneme")["nasal"]  # m-m 6, m-a 1
    assert values == ["+", "-"] and counts.tolist() == [[6, 1], [0, 0]]
    with pytest.raises(ValueError):
        _hand_table().attribute_confusions(table, "lg0", "nasal")  # categories are no phonemes


def test_round_trip_and_addition():
    from allophant_amd.confusion import ConfusionTable

    t = _hand_table()
    again = ConfusionTable.loads(t.dumps())
    assert again == t and again.entries() == t.entries() and again.symbols == SYMBOLS
    assert ConfusionTable.from_dict(json.loads(json.dumps(t.to_dict()))) == t
    assert set(t.to_dict()) == {"languages", "outputs", "symbols", "entries"}
    other = ConfusionTable(["lg0", "lg1"], ["phoneme", "nasal"], SYMBOLS, [0, 1], [0, 1], [0, -1], [0, 1], [5, 2])
    both = t + other
    assert both.total() == t.total() + 7 and len(both) == len(t) + 1
    assert ("a", "a", 15) in both.pairs("lg0", "phoneme", kind="correct")
    assert both.pairs("lg1", "nasal", kind="insertion") == [("", "+", 2)]
    assert (other + t) == both
    with pytest.raises(ValueError):
        t + ConfusionTable(["lg0"], ["phoneme", "nasal"], SYMBOLS, [], [], [], [], [])
    with pytest.raises(ValueError):
        ConfusionTable(["lg0"], ["phoneme"], [["a"]], [0], [0], [1], [0], [1])  # id 1 outside the id space


def test_public_names():
    import allophant_amd
    from allophant_amd import confusion, evaluation

    for name in ("ConfusionCounts", "ConfusionTable"):
        assert getattr(allophant_amd, name) is getattr(confusion, name) and name in allophant_amd.__all__
    assert allophant_amd.levensthein_confusions_batch is evaluation.levensthein_confusions_batch
    assert callable(evaluation.PropertyWeighting.levensthein_confusions_batch)

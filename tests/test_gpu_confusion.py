"""On-device confusion tables (amx_edit_confusion.hip, amx_edit_weighted_confusion.hip) against the restatement
from upstream's records (tests/confusion_util.py).  Every count is an exact integer: no tolerance anywhere.  Direct pairs at
lengths around the 64-row strips and the 64-step code windows, one table per row; an evaluator through the maps with a beam's
chosen candidates, skipped and flagged rows; accumulation, row order and repeatability; a full table; growing and merging;
and the weighted paths, where different symbols of cost 0 are matches."""
from collections import Counter

import numpy as np
import pytest
import torch

import confusion_util as CU
import edit_util as E
import edit_weighted_util as W

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 63, 64, 65, 128, 129, 200)
WEIGHTED_LENGTHS = (0, 1, 64, 65, 129)
SYMBOL_BITS = 21


@pytest.fixture(scope="module")
def ev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import evaluation, lib

    assert lib.load() is not None
    return evaluation


def _sequences(rng, alphabet, lengths):
    expected, actual = [], []
    for m in lengths:
        for n in lengths:
            expected.append(rng.integers(0, alphabet, m).tolist())
            actual.append(rng.integers(0, alphabet, n).tolist())
    return expected, actual


def _per_row(ev, p, weights=None, capacity=2 ** 16):
    """The pairs of ``p`` with every row its own group: (ConfusionCounts, row_events list)."""
    from allophant_amd.confusion import ConfusionCounts

    N = p.tokens.shape[1]
    p.labels[N + 1:2 * N + 1] = torch.arange(N, dtype=torch.int32, device=p.labels.device)
    counts = ConfusionCounts(p.tokens.device, capacity, [str(n) for n in range(N)], ["pairs"], [p.symbols])
    row_events = counts.add_rows(p.rows()._replace(G=N), None, weights)
    return counts, row_events.reshape(N).cpu().tolist()


def _as_dict(table):
    """{(language index, output index, expected symbol, actual symbol): count} with the restatement's epsilon."""
    out = {}
    for g, o, e, a, c in table.entries():
        out[(g, o, CU.EPSILON if e < 0 else table.symbols[o][e], CU.EPSILON if a < 0 else table.symbols[o][a])] = c
    return out


def _diagonal(found):
    return sum(c for (e, a), c in found.items() if e is not CU.EPSILON and a is not CU.EPSILON)


@pytest.mark.parametrize("alphabet", [3, 500])
def test_direct_pairs_against_the_restatement(ev, alphabet):
    """All 81 combinations of the lengths, each row a group of its own, so that every row's table is compared entry by
    entry.  Alphabet 3: dense ties and hot keys; alphabet 500: many distinct keys."""
    rng = np.random.default_rng(alphabet)
    expected, actual = _sequences(rng, alphabet, LENGTHS)
    reference = [CU.events(a, b, fast=True) for a, b in zip(expected, actual)]
    counts, row_events = _per_row(ev, ev._pairs(expected, actual, torch.device("cuda", 0)))
    assert row_events == [len(a) + len(b) - _diagonal(f) for a, b, f in zip(expected, actual, reference)]
    assert row_events == [CU.event_count(f) for f in reference]
    assert counts.events() == (sum(row_events), 0)
    assert _as_dict(counts.fetch()) == CU.table_of((n, 0, f) for n, f in enumerate(reference))
    # and the public call: one table over all pairs
    table = ev.levensthein_confusions_batch(expected, actual)
    assert _as_dict(table) == CU.table_of((0, 0, f) for f in reference)
    assert table.total() == sum(row_events)


def _beam(names, tokens, counts, hyp_counts):
    from allophant_amd.estimator import BeamDecoded

    tokens = torch.tensor(tokens, dtype=torch.int64, device="cuda")
    counts = torch.tensor(counts, dtype=torch.int32, device="cuda")
    return BeamDecoded(names, tokens, torch.zeros_like(tokens), counts,
                       torch.zeros(counts.shape, dtype=torch.float64, device="cuda"),
                       torch.tensor(hyp_counts, dtype=torch.int32, device="cuda"))


def _attribute_table():
    from allophant_amd.phonetic import AttributeTable

    return AttributeTable(E.synthetic_table_text(), ["syllabic", "long", "nasal", "phoneme"])


INVENTORY = ["a", "ts", "t", "s", "m", "aː"]
LANGUAGES = ["lg0", "lg1", "lg2"]
# lg1 hears "ts" as three segments once split, lg2 remaps two phonemes: ids expand to 0 (blank), 1 and 2-3 symbols
SOURCE_MAPS = {"lg0": {p: p for p in INVENTORY}, "lg1": {**{p: p for p in INVENTORY}, "ts": "tsʃ"},
               "lg2": {**{p: p for p in INVENTORY}, "aː": "a", "m": "ts"}}


def _map_case():
    """Six utterances, K = 3, two outputs.  Utterance 0: candidate 1 is the label itself (best 1); 1: an empty label (best
    -1); 2: no candidate (hyp_counts 0); 3: a token outside the map (flagged); 4 and 5: ordinary rows of lg1 and lg2."""
    labels = [["a", "ts", "m"], [], ["t", "s"], ["m"], ["ts", "a", "ts", "aː"], ["aː", "m", "t", "a", "s"]]
    languages = ["lg0", "lg1", "lg0", "lg2", "lg1", "lg2"]
    phoneme = [[[1, 3, 5, 0], [1, 2, 5, 0], [5, 5, 0, 0]], [[1, 0, 0, 0], [2, 2, 0, 0], [0, 0, 0, 0]],
               [[3, 4, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], [[5, 0, 0, 0], [9, 1, 0, 0], [0, 0, 0, 0]],
               [[2, 1, 0, 1], [2, 1, 2, 6], [4, 0, 0, 0]], [[6, 5, 3, 1], [1, 5, 3, 1], [6, 2, 3, 1]]]
    phoneme_counts = [[3, 3, 2], [1, 2, 0], [2, 0, 0], [1, 2, 0], [4, 4, 1], [4, 4, 4]]
    hyp = [3, 2, 0, 2, 3, 3]
    nasal = [[[1, 1, 2, 0], [1, 2, 0, 0], [2, 0, 0, 0]], [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]],
             [[1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], [[2, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]],
             [[1, 3, 1, 1], [1, 1, 1, 1], [3, 0, 0, 0]], [[1, 2, 1, 1], [1, 1, 1, 1], [2, 2, 1, 1]]]
    nasal_counts = [[3, 2, 1], [1, 0, 0], [2, 0, 0], [1, 1, 0], [4, 4, 1], [4, 4, 4]]
    nasal_hyp = [3, 1, 0, 2, 3, 3]
    decoded = _beam(["phoneme", "nasal"], [phoneme, nasal], [phoneme_counts, nasal_counts], [hyp, nasal_hyp])
    return decoded, labels, languages, (phoneme, nasal), (phoneme_counts, nasal_counts), (hyp, nasal_hyp)


def _map_reference(e, labels, languages, tokens, counts, hyp):
    """The restatement through the evaluator's own host expansion: per row (best, events) of the chosen candidate, or the
    row's flag -1 / -2; and the table of the contributing rows."""
    rows, table = {}, Counter()
    for o in range(len(e.names)):
        for n, (label, language) in enumerate(zip(labels, languages)):
            g = e.languages.index(language)
            expected = e.maps.expand_label(o, label)
            try:
                candidates = [e.maps.expand_tokens(o, g, tokens[o][n][k][:counts[o][n][k]]) for k in range(hyp[o][n])]
            except IndexError:
                rows[o, n] = -2
                continue
            best, _ = E.best_candidate(expected, candidates)
            if best < 0:
                rows[o, n] = -1
                continue
            found = CU.events(expected, candidates[best])
            rows[o, n] = (best, CU.event_count(found))
            for (x, y), c in found.items():
                table[(g, o, x, y)] += c
    return rows, dict(table)


def test_through_the_maps(ev):
    decoded, labels, languages, tokens, counts, hyp = _map_case()
    e = ev.Evaluator(_attribute_table(), ["phoneme", "nasal"], INVENTORY, LANGUAGES, split_complex=True, source_maps=SOURCE_MAPS,
                     confusions=True)
    assert e.maps.H == 3 and len(e.languages) == 3
    lengths = {len(e.maps.expand_tokens(0, 1, [t])) for t in range(len(INVENTORY) + 1)}
    assert {0, 1, 3} <= lengths
    e.add(decoded, labels, languages)
    best = e.rows()[1].cpu().tolist()
    row_events = e.confusion_events().cpu().tolist()
    rows, reference = _map_reference(e, labels, languages, tokens, counts, hyp)
    assert best[0][:4] == [1, -1, -1, -2] and best[1][1] == -1 and best[1][2] == -1
    for (o, n), row in rows.items():
        if isinstance(row, tuple):
            assert (best[o][n], row_events[o][n]) == row, (o, n)
        else:
            assert best[o][n] == row and row_events[o][n] == row, (o, n)  # -1 / -2 rows: nothing added
    table = e.confusions()
    assert _as_dict(table) == reference
    assert table.statistics() == e.statistics()  # entry for entry, every language and output
    assert table.total() == sum(sum(v for v in row if v > 0) for row in row_events)
    e.reset()
    assert len(e.confusions()) == 0
    plain = ev.Evaluator(_attribute_table(), ["phoneme"], INVENTORY, LANGUAGES)
    with pytest.raises(ValueError):
        plain.confusions()


def _random_decoded(rng, N, K, T):
    tokens = rng.integers(1, len(INVENTORY) + 1, (1, N, K, T))
    counts = rng.integers(0, T + 1, (1, N, K))
    hyp = rng.integers(0, K + 1, (1, N))
    table = _attribute_table()
    labels = [[table.full_phonemes[i] for i in rng.integers(0, 11, rng.integers(0, 80))] for _ in range(N)]
    languages = [LANGUAGES[i] for i in rng.integers(0, 3, N)]
    return tokens, counts, hyp, labels, languages


def _evaluator(ev, **kwargs):
    return ev.Evaluator(_attribute_table(), ["phoneme"], INVENTORY, LANGUAGES, split_complex=True, confusions=2 ** 12, **kwargs)


def _raw(e):
    keys, counts = e._confusions[0][1].raw()
    return keys.tobytes(), counts.tobytes()


def test_accumulation_order_and_repeatability(ev):
    rng = np.random.default_rng(31)
    batches = [_random_decoded(rng, 24, 3, 90) for _ in range(2)]
    both, again = _evaluator(ev), _evaluator(ev)
    separate = []
    for tokens, counts, hyp, labels, languages in batches:
        single = _evaluator(ev)
        for e in (both, again, single):
            e.add(_beam(["phoneme"], tokens.tolist(), counts.tolist(), hyp.tolist()), labels, languages)
        separate.append(single.confusions())
    total = both.confusions()
    assert total == separate[0] + separate[1] and total.total() > 0
    assert total.statistics() == both.statistics()
    assert _raw(both) == _raw(again)  # two runs: the same table, bit for bit, once sorted by key
    permuted = _evaluator(ev)
    for tokens, counts, hyp, labels, languages in batches:
        order = rng.permutation(len(labels))
        permuted.add(_beam(["phoneme"], tokens[:, order].tolist(), counts[:, order].tolist(), hyp[:, order].tolist()),
                     [labels[i] for i in order], [languages[i] for i in order])
    assert _raw(permuted) == _raw(both)
    assert permuted.confusions() == total


def _decode(keys):
    return [(int(k) >> 2 * SYMBOL_BITS, (int(k) >> SYMBOL_BITS & (1 << SYMBOL_BITS) - 1) - 1, (int(k) & (1 << SYMBOL_BITS) - 1) - 1)
            for k in keys]


def test_full_table(ev):
    """16 slots for hundreds of distinct keys: the call returns (the probe is bounded), every event is counted as added
    or dropped, what is stored is a part of the truth, and fetch refuses to hand out a partial table."""
    rng = np.random.default_rng(4)
    expected = [rng.integers(0, 500, 60).tolist() for _ in range(8)]
    actual = [rng.integers(0, 500, 70).tolist() for _ in range(8)]
    device = torch.device("cuda", 0)
    p = ev._pairs(expected, actual, device)
    counts, row_events = ev._pair_confusions(p, device, capacity=16)
    row_events = row_events.reshape(-1).cpu().tolist()
    truth = CU.table_of((0, 0, CU.events(a, b, fast=True)) for a, b in zip(expected, actual))
    assert len(truth) > 16
    added, dropped = counts.events()
    assert added + dropped == sum(row_events) == sum(truth.values()) and dropped > 0
    keys, stored = counts.raw()
    assert len(keys) == 16 and int(stored.sum()) == added
    for (slot, e, a), c in zip(_decode(keys), stored.tolist()):
        key = (0, 0, CU.EPSILON if e < 0 else p.symbols[e], CU.EPSILON if a < 0 else p.symbols[a])
        assert slot == 1 and 0 < c <= truth[key]
    with pytest.raises(OverflowError, match=str(dropped)):
        counts.fetch()


def test_grow_and_merge(ev):
    from allophant_amd.confusion import ConfusionCounts

    device = torch.device("cuda", 0)
    rng = np.random.default_rng(6)
    first = _sequences(rng, 3, (0, 5, 64, 90))
    second = _sequences(rng, 3, (1, 33, 65))
    small, _ = ev._pair_confusions(ev._pairs(*first, device), device, capacity=64)
    before = small.fetch()
    assert 0 < len(before) <= 15
    small.grow(4096)
    assert small.capacity == 4096 and small.fetch() == before and small.events() == (before.total(), 0)

    # merge: the two batches counted apart in one id space (rows picked by hyp_counts), merged on the device
    concatenated = ev.levensthein_confusions_batch(first[0] + second[0], first[1] + second[1])
    both = ev._pairs(first[0] + second[0], first[1] + second[1], device)
    N, N1 = both.tokens.shape[1], len(first[0])

    def part(rows):
        counts = ConfusionCounts(device, 64, ["total"], ["pairs"], [both.symbols])
        present = torch.zeros(1, N, dtype=torch.int32, device=device)
        present[0, rows] = 1
        row_events = counts.add_rows(both.rows()._replace(hyp_counts=present))
        assert torch.equal(row_events[0] == -1, present[0] == 0)  # rows without a candidate
        return counts

    a, b = part(slice(0, N1)), part(slice(N1, N))
    assert a.fetch() == ev.levensthein_confusions_batch(*first) and 0 < b.fetch().total() < concatenated.total()
    a.merge(b)
    assert a.fetch() == concatenated and a.events() == (concatenated.total(), 0)

    # a merge into a table that is too small counts the drops
    wide = ev._pair_confusions(ev._pairs([rng.integers(0, 500, 100).tolist()], [rng.integers(0, 500, 100).tolist()], device),
                               device, capacity=4096)[0]
    whole = wide.fetch()
    assert len(whole) > 16
    wide.grow(16)
    added, dropped = wide.events()
    assert dropped > 0 and added + dropped == whole.total()
    with pytest.raises(OverflowError):
        wide.fetch()


WEIGHTED_TABLE = {0: [0, 1, 0], 1: [1, 1, 0], 2: [0, 1, 0], 3: [1, 0, 1]}  # 0 and 2: different symbols, equal rows


@pytest.mark.parametrize("costs", [(0.3, 0.7), (1.7, 3.3)])
def test_weighted_pairs(ev, costs):
    """All 25 combinations of the lengths under a table in which two different symbols have equal rows: every row's entries
    equal the weighted restatement, and the split of the diagonal events by table cost is the S and C of
    amx_edit_weighted_statistics."""
    rng = np.random.default_rng(int(costs[0] * 10))
    expected, actual = _sequences(rng, 4, WEIGHTED_LENGTHS)
    weighting = ev.PropertyWeighting(*costs, WEIGHTED_TABLE)
    reference = [CU.weighted_events(a, b, *costs, WEIGHTED_TABLE, fast=True) for a, b in zip(expected, actual)]
    device, p, weights = weighting._prepare(expected, actual, None)
    counts, row_events = _per_row(ev, p, weights)
    assert row_events == [CU.event_count(f) for f in reference]
    assert counts.events() == (sum(row_events), 0)
    table = counts.fetch()
    assert _as_dict(table) == CU.table_of((n, 0, f) for n, f in enumerate(reference))
    zero_cost_pairs = sum(c for (_, _, e, a), c in _as_dict(table).items()
                          if e is not CU.EPSILON and a is not CU.EPSILON and e != a and W.substitution_cost(WEIGHTED_TABLE, e, a) == 0)
    assert zero_cost_pairs > 0
    statistics = weighting.levensthein_statistics_batch(expected, actual)
    implied = table.statistics(weighting)
    for n, s in enumerate(statistics):
        assert implied[str(n)]["pairs"] == s, n
    public = weighting.levensthein_confusions_batch(expected, actual)
    assert _as_dict(public) == CU.table_of((0, 0, f) for f in reference)


def test_weighted_evaluator(ev):
    """An evaluator with a weighting keeps one accumulator per part (attribute outputs under unit costs, IPA outputs under
    the weighting) and returns one table over all outputs whose statistics are the evaluator's."""
    decoded, labels, languages, *_ = _map_case()
    table = _attribute_table()
    weighting = ev.PropertyWeighting(0.6, 0.8, table.property_table())
    sources = {language: {p: p for p in INVENTORY} for language in LANGUAGES}
    e = ev.Evaluator(table, ["nasal", "phoneme"], INVENTORY, LANGUAGES, source_maps=sources, weighting=weighting, confusions=True)
    e.add(decoded, labels, languages)
    found = e.confusions()
    assert found.names == ["nasal", "phoneme"] and found.total() > 0
    assert found.statistics(weighting)["lg0"]["phoneme"] == e.statistics()["lg0"]["phoneme"]
    for language in LANGUAGES:
        assert found.statistics()[language]["nasal"] == e.statistics()[language]["nasal"]
        assert found.statistics(weighting)[language]["phoneme"] == e.statistics()[language]["phoneme"]
    best = e.rows()[1].cpu()
    events = e.confusion_events().cpu()
    assert torch.equal(events < 0, best < 0) and torch.equal(events[best < 0], best[best < 0])

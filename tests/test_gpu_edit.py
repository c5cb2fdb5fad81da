"""On-device edit statistics (amx_edit.hip) against the literal restatement of upstream's evaluation (tests/edit_util.py):
bit-exact counts per row at lengths around the 64-row strips up to 3000 on both sides over small alphabets (ties
everywhere); the candidate choice (first of equal rates, empty labels skipped, hyp_counts, flagged tokens); totals over
several batches, repeatable bit for bit and under graph replay; and the synthetic model -> predict -> greedy and beam
decoding -> Evaluator, equal to the restatement run on hypothesis_symbols strings in every integer and fp32 rate."""
import math
import unicodedata

import numpy as np
import pytest
import torch

import edit_util as E

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 500, 3000)


@pytest.fixture(scope="module")
def ev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import evaluation, lib

    assert lib.load() is not None
    return evaluation


def _table():
    from allophant_amd.phonetic import AttributeTable

    return AttributeTable(E.synthetic_table_text(), ["syllabic", "long", "nasal", "phoneme"])


@pytest.mark.parametrize("alphabet", [2, 3])
def test_lengths_against_the_back_trace(ev, alphabet):
    rng = np.random.default_rng(alphabet)
    expected, actual = [], []
    for m in LENGTHS:
        for n in LENGTHS:
            expected.append(rng.integers(0, alphabet, m).tolist())
            actual.append(rng.integers(0, alphabet, n).tolist())
    got = ev.levensthein_statistics_batch(expected, actual)
    for a, b, stats in zip(expected, actual, got):
        assert stats.astuple() == E.levensthein_statistics_fast(a, b), (len(a), len(b))


def test_random_pairs_and_strings(ev):
    rng = np.random.default_rng(11)
    expected = [rng.integers(0, 4, rng.integers(0, 200)).tolist() for _ in range(300)]
    actual = [rng.integers(0, 4, rng.integers(0, 200)).tolist() for _ in range(300)]
    got = ev.levensthein_statistics_batch(expected, actual)
    assert [s.astuple() for s in got] == [E.levensthein_statistics_fast(a, b) for a, b in zip(expected, actual)]
    for a, b, stats in (("acba", "bab", (1, 2, 0, 2)), ("a", "ba", (1, 0, 0, 1)), ("ab", "abx", (1, 0, 0, 2)),
                        ("", "", (0, 0, 0, 0)), (["ts", "a"], ["ts", "e"], (0, 0, 1, 1))):
        assert ev.levensthein_statistics(a, b).astuple() == stats


def _beam(names, tokens, counts, hyp_counts):
    from allophant_amd.estimator import BeamDecoded

    tokens = torch.tensor(tokens, dtype=torch.int64, device="cuda")
    counts = torch.tensor(counts, dtype=torch.int32, device="cuda")
    return BeamDecoded(names, tokens, torch.zeros_like(tokens), counts,
                       torch.zeros(counts.shape, dtype=torch.float64, device="cuda"),
                       torch.tensor(hyp_counts, dtype=torch.int32, device="cuda"))


def test_candidate_choice_and_flags(ev):
    """Equal rates: the first candidate wins; an empty label: best -1 and nothing added; candidates past hyp_counts are not
    scored (-1); a token outside the map flags the row (best -2, statistics -2, nothing added)."""
    inventory = ["a", "t", "s", "m"]
    e = ev.Evaluator(_table(), ["phoneme"], inventory, ["lg0"])
    # utterance 0: label "a t"; candidates "a s" (1 sub), "m t" (1 sub, same rate), "a t" (past hyp_counts = 2)
    # utterance 1: empty label; utterance 2: label "s"; candidate 1 holds token 9 (outside the map of 5 entries)
    tokens = [[[[1, 3], [4, 2], [1, 2]], [[1, 0], [0, 0], [0, 0]], [[3, 0], [9, 0], [0, 0]]]]
    counts = [[[2, 2, 2], [1, 0, 0], [1, 1, 0]]]
    e.add(_beam(["phoneme"], tokens, counts, [[2, 1, 2]]), [["a", "t"], [], ["s"]], ["lg0"] * 3)
    statistics, best = (t.cpu().tolist() for t in e.rows())
    assert best == [[0, -1, -2]]
    assert statistics[0][0] == [[0, 0, 1, 1], [0, 0, 1, 1], [-1, -1, -1, -1]]
    assert statistics[0][1][0] == [1, 0, 0, 0] and statistics[0][1][1] == [-1] * 4
    assert statistics[0][2][0] == [0, 0, 0, 1] and statistics[0][2][1] == [-2] * 4
    assert e.totals.cpu().tolist() == [[[0, 0, 1, 1]]]
    result = e.results()
    assert result.results["lg0"].error_statistics["phoneme"] == ev.EditStatistics(0, 0, 1, 1)
    assert result.results["total"].error_rates["phoneme"] == 0.5


def _random_batch(rng, inventory, N, K, T):
    tokens = rng.integers(1, len(inventory) + 1, (1, N, K, T))
    counts = rng.integers(0, T + 1, (1, N, K))
    hyp = rng.integers(0, K + 1, (1, N))
    return tokens.tolist(), counts.tolist(), hyp.tolist()


def test_totals_repeatable_and_equal_to_the_restatement(ev):
    from allophant_amd.phonetic import split_complex_segment

    table = _table()
    inventory = ["a", "ts", "t͡ʃ", "é", "m", "aː", "i"]
    languages = ["lg0", "lg1", "lg2"]
    evaluators = [ev.Evaluator(table, ["phoneme"], inventory, languages, split_complex=True) for _ in range(2)]
    rng = np.random.default_rng(5)
    reference = {language: (0, 0, 0, 0) for language in languages}
    for _ in range(3):
        N, K, T = 24, 4, 90
        tokens, counts, hyp = _random_batch(rng, inventory, N, K, T)
        labels = [[table.full_phonemes[i] for i in rng.integers(0, 11, rng.integers(0, 80))] for _ in range(N)]
        langs = [languages[i] for i in rng.integers(0, 3, N)]
        for e in evaluators:
            e.add(_beam(["phoneme"], tokens, counts, hyp), labels, langs)
        split = lambda ps: [q for p in ps for q in split_complex_segment(p)]  # noqa: E731
        for n in range(N):
            candidates = [split([inventory[t - 1] for t in tokens[0][n][k][:counts[0][n][k]]]) for k in range(hyp[0][n])]
            _, stats = E.best_candidate(split(labels[n]), candidates)
            if stats is not None:
                reference[langs[n]] = tuple(x + y for x, y in zip(reference[langs[n]], stats))
    a, b = (e.totals.cpu() for e in evaluators)
    assert torch.equal(a, b)
    assert a[:, 0].tolist() == [list(reference[language]) for language in languages]


def test_add_replays_in_a_graph(ev):
    table = _table()
    inventory = ["a", "ts", "t͡ʃ", "é", "m", "aː", "i"]
    rng = np.random.default_rng(8)
    tokens, counts, hyp = _random_batch(rng, inventory, 16, 3, 70)
    decoded = _beam(["phoneme"], tokens, counts, hyp)
    labels = [[table.full_phonemes[i] for i in rng.integers(0, 11, rng.integers(1, 60))] for _ in range(16)]
    langs = ["lg0", "lg1"] * 8
    eager = ev.Evaluator(table, ["phoneme"], inventory, ["lg0", "lg1"])
    eager.add(decoded, labels, langs)
    eager.add(decoded, labels, langs)
    captured = ev.Evaluator(table, ["phoneme"], inventory, ["lg0", "lg1"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        captured.add(decoded, labels, langs)  # warm-up outside the capture (sizes the workspace)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    captured.reset()
    static_labels = captured.encode_labels(labels, langs)  # the labels are a static input of the graph
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.add(decoded, static_labels)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured.totals, eager.totals)
    assert torch.equal(captured.rows()[0], eager.rows()[0]) and torch.equal(captured.rows()[1], eager.rows()[1])


def _same_rate(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("beam", [False, True])
def test_synthetic_model_end_to_end(ev, beam):
    """predict -> greedy_decode_device / beam_decode_device(16, n_best=4) -> Evaluator (two languages, a remap, split
    complex segments, contour labels, an NFC replacement, an empty label) equals the restatement on hypothesis_symbols."""
    from allophant_amd import spec as S, synthetic
    from allophant_amd.estimator import Batch, Estimator
    from allophant_amd.phonetic import hypothesis_symbols, split_complex_segment

    table = _table()
    names = ["syllabic", "long", "nasal", "phoneme"]
    spec = S.multitask_spec(S.tiny_encoder(2), names[:3], embedding_size=16, train_phonemes=9, n_features=5, n_values=3)
    state = synthetic.make_state_dict(spec, seed=3)
    N = 6
    audio, lengths = synthetic.make_audio(N, 12000, seed=7, ragged=True)
    inventory = ["a", "ts", "t͡ʃ", "é", "m", "aː", "i"]
    tfi = synthetic.make_inventory(spec, len(inventory), seed=2)
    est = Estimator(spec, state, "cuda:0", "f16x3")
    try:
        pred = est.predict(Batch(audio.cuda(), lengths, torch.zeros(N, dtype=torch.long)), tfi)
        decoded = est.beam_decode_device(pred, 16, n_best=4) if beam else est.greedy_decode_device(pred)
        hosts = decoded.hypotheses()
    finally:
        est.close()
    decomposed = unicodedata.normalize("NFD", "é")
    replacements = ev.unicode_replacements(table, table.full_phonemes + [decomposed])
    languages = ["lg0", "lg1"]
    source_maps = {"lg0": {p: p for p in inventory}, "lg1": {**{p: p for p in inventory}, "ts": "s", "aː": "a"}}
    rng = np.random.default_rng(21)
    symbols = table.full_phonemes + [decomposed]
    labels = [[symbols[i] for i in rng.integers(0, len(symbols), rng.integers(5, 40))] for _ in range(N)]
    labels[2] = []
    langs = [languages[n % 2] for n in range(N)]
    e = ev.Evaluator(table, names, inventory, languages, split_complex=True, source_maps=source_maps,
                     replacements=replacements)
    e.add(decoded, labels, langs)
    got = e.results("evaluate").to_dict()

    strings = hypothesis_symbols(hosts, inventory, table)
    contours = {p: {n: table.feature_contour(p, n) for n in names[:3]} for p in table.full_phonemes}
    utterances = []
    for n in range(N):
        per_output = {}
        for name in names:
            expected = E.expected_symbols(name, labels[n], contours, split_complex_segment, True, replacements)
            candidates = [E.actual_symbols(name, c, split_complex_segment, True, source_maps[langs[n]])
                          for c in strings[name][n]]
            per_output[name] = (expected, candidates)
        utterances.append((langs[n], per_output))
    reference = E.evaluate(names, languages, utterances)
    assert list(got["results"]) == languages + ["total"]
    cells = 0
    for language, per_name in reference.items():
        for name, stats in per_name.items():
            entry = got["results"][language]
            assert tuple(entry["error_statistics"][name][k] for k in ("insertions", "deletions", "substitutions",
                                                                          "correct")) == stats, (language, name)
            assert _same_rate(entry["error_rates"][name], float(E.word_error_rate(stats))), (language, name)
            cells += sum(stats)
    assert cells > 0

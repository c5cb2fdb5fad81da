"""On-device feature-weighted edit distance (amx_edit_weighted.hip) against the restatement of upstream's ``PropertyWeighting``
(tests/edit_weighted_util.py), everything equal and the fp32 costs compared as bits: the length grid around the 64-row strips
up to 3000 on both sides under four cost pairs; matrices; unit costs with an identity table against the uniform kernels;
equal rows; flags and canaries; graph replay; and the synthetic model -> predict -> decoding -> Evaluator(weighting=...)."""
import ctypes as C
import math
import unicodedata

import numpy as np
import pytest
import torch

import edit_ops_util as U
import edit_util as E
import edit_weighted_util as W

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 500, 3000)
COSTS = [(1.0, 1.0), (0.3, 0.7), (2.5, 0.1), (1.7, 3.3)]
# alphabet 2: the symbols differ in two features; alphabet 3: symbol 2 shares symbol 0's row (different symbols at cost 0)
TABLES = {2: {0: [0, 0, 0], 1: [1, 1, 0]}, 3: {0: [0, 0], 1: [0, 1], 2: [0, 0]}}


def _bits(x) -> bytes:
    return np.asarray(x, dtype=np.float32).tobytes()


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


def _grid(rng, alphabet, lengths):
    expected, actual = [], []
    for m in lengths:
        for n in lengths:
            expected.append(rng.integers(0, alphabet, m).tolist())
            actual.append(rng.integers(0, alphabet, n).tolist())
    return expected, actual


@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("alphabet", [2, 3])
def test_lengths_against_the_restatement(ev, alphabet, costs):
    rng = np.random.default_rng(100 + alphabet)
    expected, actual = _grid(rng, alphabet, LENGTHS)
    weighting = ev.PropertyWeighting(*costs, TABLES[alphabet])
    statistics = weighting.levensthein_statistics_batch(expected, actual)
    operations = weighting.levensthein_operations_batch(expected, actual)
    for a, b, got_statistics, (got_operations, got_cost) in zip(expected, actual, statistics, operations):
        want_operations, want_cost, want_statistics = W.operations_fast(a, b, *costs, TABLES[alphabet])
        print(len(a), len(b), costs, got_statistics.astuple(), want_statistics, got_cost, float(want_cost))
        assert got_statistics.astuple() == want_statistics, (len(a), len(b))
        assert got_operations == want_operations, (len(a), len(b))
        assert _bits(got_cost) == _bits(want_cost), (len(a), len(b))


@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("alphabet", [2, 3])
def test_matrices_against_the_restatement(ev, alphabet, costs):
    rng = np.random.default_rng(200 + alphabet)
    expected, actual = _grid(rng, alphabet, LENGTHS[:8])
    weighting = ev.PropertyWeighting(*costs, TABLES[alphabet])
    for a, b, got in zip(expected, actual, weighting.levensthein_matrix_batch(expected, actual)):
        assert got.dtype == torch.float32 and got.shape == (len(a) + 1, len(b) + 1)
        assert _bits(got.cpu().numpy()) == _bits(W.matrix_fast(a, b, *costs, TABLES[alphabet])), (len(a), len(b))


def test_one_long_matrix_and_the_uniform_matrix(ev):
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 3, 500).tolist(), rng.integers(0, 3, 3000).tolist()
    got = ev.PropertyWeighting(0.3, 0.7, TABLES[3]).levensthein_matrix(a, b)
    assert _bits(got.cpu().numpy()) == _bits(W.matrix_fast(a, b, 0.3, 0.7, TABLES[3]))
    for a, b in (("abc", "ac"), ("", "xy"), ("abc", ""), ("", ""), (a[:130], b[:70])):
        got = ev.levensthein_matrix(a, b)
        assert _bits(got.cpu().numpy()) == _bits(U._matrix(a, b).astype(np.float32)), (a, b)


def _beam(names, tokens, counts, hyp_counts):
    from allophant_amd.estimator import BeamDecoded

    tokens = torch.tensor(tokens, dtype=torch.int64, device="cuda")
    counts = torch.tensor(counts, dtype=torch.int32, device="cuda")
    return BeamDecoded(names, tokens, torch.zeros_like(tokens), counts,
                       torch.zeros(counts.shape, dtype=torch.float64, device="cuda"),
                       torch.tensor(hyp_counts, dtype=torch.int32, device="cuda"))


def _random_batch(rng, inventory, N, K, T, least=0):
    tokens = rng.integers(1, len(inventory) + 1, (1, N, K, T))
    counts = rng.integers(0, T + 1, (1, N, K))
    hyp = rng.integers(least, K + 1, (1, N))
    return tokens.tolist(), counts.tolist(), hyp.tolist()


def _properties(ev, table, names, inventory, languages, **options):
    """The attribute table's property rows, plus a row for every other symbol of the IPA id spaces (split segments,
    decomposed forms): the host maps of an evaluator without weighting name them."""
    properties = dict(table.property_table())
    width = len(table.full_feature_names)
    maps = ev.EvaluationMaps(table, names, inventory, languages, **options)
    for o, name in enumerate(names):
        if name in ("phone", "phoneme"):
            for symbol in maps.spaces[o]:
                if symbol not in properties:
                    properties[symbol] = [(len(properties) + f) % 3 for f in range(width)]
    return properties


INVENTORY = ["a", "ts", "t͡ʃ", "é", "m", "aː", "i"]


def test_unit_costs_with_an_identity_table_equal_the_uniform_kernels(ev):
    table = _table()
    languages = ["lg0", "lg1", "lg2"]
    rng = np.random.default_rng(31)
    N, K, T = 40, 4, 150
    tokens, counts, hyp = _random_batch(rng, INVENTORY, N, K, T)
    decoded = _beam(["phoneme"], tokens, counts, hyp)
    labels = [[table.full_phonemes[i] for i in rng.integers(0, 11, rng.integers(0, 140))] for _ in range(N)]
    langs = [languages[i] for i in rng.integers(0, 3, N)]
    uniform = ev.Evaluator(table, ["phoneme"], INVENTORY, languages, split_complex=True)
    identity = {symbol: [i] for symbol, i in uniform.maps.spaces[0].items()}
    weighted = ev.Evaluator(table, ["phoneme"], INVENTORY, languages, split_complex=True,
                            weighting=ev.PropertyWeighting(1.0, 1.0, identity))
    uniform.add(decoded, labels, langs)
    weighted.add(decoded, labels, langs)
    assert torch.equal(weighted.rows()[0], uniform.rows()[0]) and torch.equal(weighted.rows()[1], uniform.rows()[1])
    assert torch.equal(weighted.totals, uniform.totals) and int(uniform.totals.sum()) > 0
    assert _bits(weighted.costs().cpu().numpy()) == _bits(uniform.costs().cpu().numpy())
    decoded = _beam(["phoneme"], *_random_batch(rng, INVENTORY, N, K, T, least=1))
    want_operations, want_counts = uniform.operations(decoded, labels, langs)
    got_operations, got_counts = weighted.operations(decoded, labels, langs)
    assert torch.equal(got_counts, want_counts)
    for n in range(N):
        c = int(want_counts[0, n])
        assert torch.equal(got_operations[0, n, :c], want_operations[0, n, :c]), n


def test_equal_rows_are_correct_and_the_two_calls_agree(ev):
    table = _table()
    properties = _properties(ev, table, ["phoneme"], INVENTORY, ["lg0"], split_complex=True)
    assert properties["a"] == properties["e"]
    weighting = ev.PropertyWeighting(0.3, 0.7, properties)
    assert weighting.levensthein_operations(["a", "t", "e"], ["e", "t", "a"]) == ([], 0.0)
    assert weighting.levensthein_statistics(["a", "t", "e"], ["e", "t", "a"]) == ev.EditStatistics(0, 0, 0, 3)
    rng = np.random.default_rng(9)
    N, K, T = 32, 3, 120
    decoded = _beam(["phoneme"], *_random_batch(rng, INVENTORY, N, K, T, least=1))
    labels = [[table.full_phonemes[i] for i in rng.integers(0, 11, rng.integers(0, 100))] for _ in range(N)]
    e = ev.Evaluator(table, ["phoneme"], INVENTORY, ["lg0"], split_complex=True, weighting=weighting)
    e.add(decoded, labels, ["lg0"] * N)
    operations, op_counts = e.operations(decoded, labels, ["lg0"] * N)
    statistics = e.rows()[0][0, :, 0].cpu().numpy()
    records, lengths = operations.cpu().numpy(), op_counts.cpu().numpy()
    assert _bits(e.costs()[0, :, 0].cpu().numpy()) == _bits(e._operation_costs[0].cpu().numpy())
    for n in range(N):
        actions = records[0, n, :lengths[0, n], 0]
        ins, dels, subs, _ = statistics[n]
        assert lengths[0, n] == ins + dels + subs
        assert [(actions == 1).sum(), (actions == 2).sum(), (actions == 3).sum()] == [ins, dels, subs], n


def test_flags_and_canaries(ev):
    """hyp_counts 0: -1; a token outside the map: -2; a symbol outside its cost table: -2; nothing is written past a row's
    records, into flagged rows' costs, or outside a pair's matrix."""
    from allophant_amd import evaluation, lib

    inventory = ["a", "t", "s", "m"]
    table = _table()
    weighting = ev.PropertyWeighting(0.3, 0.7, table.property_table())
    e = ev.Evaluator(table, ["phoneme"], inventory, ["lg0"], weighting=weighting)
    tokens = [[[[1, 3, 4]], [[1, 2, 0]], [[3, 9, 0]], [[2, 2, 2]]]]
    counts = [[[3], [2], [2], [3]]]
    decoded = _beam(["phoneme"], tokens, counts, [[1, 0, 1, 1]])
    labels = [["a", "t"], ["a"], ["s"], []]
    properties = table.property_table()
    want = [W.levensthein_operations(labels[n], actual, 0.3, 0.7, properties) for n, actual in ((0, ["a", "s", "m"]), (3, ["t"] * 3))]
    want_counts = [len(want[0][0]), -1, -2, len(want[1][0])]
    operations, op_counts = e.operations(decoded, labels, ["lg0"] * 4)
    assert op_counts.cpu().tolist() == [want_counts]
    assert operations.shape[2] == 5  # max_ops = max_expected 2 + T 3
    e.add(decoded, labels, ["lg0"] * 4)
    assert e.rows()[1].cpu().tolist() == [[0, -1, -2, -1]]
    costs = e.costs().cpu().numpy()
    assert _bits(costs[0, 0, 0]) == _bits(want[0][1]) and math.isnan(costs[0, 1, 0]) and math.isnan(costs[0, 2, 0])

    handle = evaluation._weighted_library()
    canary = -777
    labels_batch = e.encode_labels(labels, ["lg0"] * 4)
    O, N, T = 1, 4, 3
    tok = decoded.tokens[:, :, 0]
    cnt = decoded.counts[:, :, 0].contiguous()
    hyp = decoded.hyp_counts.contiguous()
    max_expected, max_actual = labels_batch.max_expected, T
    max_ops = max_expected + max_actual + 2  # room for canaries past the limit too
    size = C.c_size_t()
    assert handle.amx_edit_operations_workspace(O * N, max_expected, max_actual, C.byref(size)) == lib.AMX_OK
    p = evaluation._ptr
    _, label_maps, hyp_maps, weights = e._parts[0]
    space = e.maps.spaces[0]
    small = weights.descriptors.clone()
    small[0, 1] = space["s"]  # a table too small for "s" and "m": rows 0 flags, row 3 ("t" only) does not
    assert space["t"] < space["s"] < space["m"]
    for descriptors, want_row0 in ((weights.descriptors, want_counts[0]), (small, -2)):
        workspace = torch.empty(size.value, dtype=torch.uint8, device="cuda")
        records = torch.full((O, N, max_ops, 5), canary, dtype=torch.int32, device="cuda")
        record_counts = torch.full((O, N), canary, dtype=torch.int32, device="cuda")
        record_costs = torch.full((O, N), float(canary), dtype=torch.float32, device="cuda")
        code = handle.amx_edit_weighted_operations(
            0, p(tok), tok.stride(0), tok.stride(1), O, N, T, p(cnt), p(hyp), p(labels_batch.data),
            p(labels_batch.data, 2 * N + 1), p(labels_batch.data, N + 1), 1, p(e._maps), p(e._maps, e._n_offsets), p(label_maps),
            p(hyp_maps), 1, max_expected, max_actual, p(workspace), workspace.numel(), weights.insertion_cost,
            weights.deletion_cost, p(descriptors), p(weights.data), max_ops, p(records), p(record_counts), p(record_costs),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert code == lib.AMX_OK
        torch.cuda.synchronize()
        got = record_counts.cpu().tolist()[0]
        assert got == [want_row0, -1, -2, want_counts[3]]
        for n, count in enumerate(got):
            assert (records[0, n, max(count, 0):] == canary).all(), n
            assert (float(record_costs[0, n]) == canary) == (count < 0), n
    reference = want[0][0]
    rows = [[a, i, j, space[labels[0][i]] if a != W.INSERTION else -1, space[["a", "s", "m"][j]] if a != W.DELETION else -1]
            for a, i, j in reference]
    assert operations[0, 0, :len(rows)].tolist() == rows

    # the matrix: cells outside a pair's (m + 1) x (n + 1), and a flagged pair's whole matrix, stay untouched
    expected_ids = torch.tensor([0, 1, 0, 1, 1, 5], dtype=torch.int32, device="cuda")
    expected_offsets = torch.tensor([0, 2, 5, 6], dtype=torch.int32, device="cuda")
    actual_ids = torch.tensor([1, 0, 0, 1], dtype=torch.int32, device="cuda")
    actual_offsets = torch.tensor([0, 3, 4, 4], dtype=torch.int32, device="cuda")
    pair_table = weighting.cost_table(["a", "t"], torch.device("cuda", 0))
    assert pair_table.cpu().tolist() == [0, 1, 1, 0]  # a and t differ in the syllabic column alone
    matrix = torch.full((3, 4, 4), float(canary), dtype=torch.float32, device="cuda")
    status = torch.full((3,), canary, dtype=torch.int32, device="cuda")
    assert handle.amx_edit_workspace(3, 3, 3, C.byref(size)) == lib.AMX_OK
    workspace = torch.empty(size.value, dtype=torch.uint8, device="cuda")
    code = handle.amx_edit_matrix(0, p(expected_offsets), p(expected_ids), p(actual_offsets), p(actual_ids), 3, 3, 3, 0.3, 0.7,
                                  p(pair_table), 2, p(workspace), workspace.numel(), p(matrix), p(status),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code == lib.AMX_OK
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, -2]  # pair 2 holds id 5, outside the table of 2
    host = matrix.cpu().numpy()
    pairs = {0: ("at", "taa"), 1: ("att", "t")}
    for r, (a, b) in pairs.items():
        want_matrix = W.levensthein_matrix_weighted(a, b, 0.3, 0.7, properties)
        assert _bits(host[r, :len(a) + 1, :len(b) + 1]) == _bits(want_matrix)
        outside = np.ones((4, 4), dtype=bool)
        outside[:len(a) + 1, :len(b) + 1] = False
        assert (host[r][outside] == canary).all()
    assert (host[2] == canary).all()


def test_graph_replay_equals_eager(ev):
    table = _table()
    names = ["nasal", "phoneme"]  # one output scored by the uniform kernels, one by the weighted ones
    rng = np.random.default_rng(8)
    tokens = rng.integers(1, 3, (2, 16, 3, 70))
    tokens[1] = rng.integers(1, len(INVENTORY) + 1, (16, 3, 70))
    counts = rng.integers(0, 71, (2, 16, 3))
    hyp = rng.integers(1, 4, (2, 16))
    decoded = _beam(names, tokens.tolist(), counts.tolist(), hyp.tolist())
    labels = [[table.full_phonemes[i] for i in rng.integers(0, 11, rng.integers(1, 60))] for _ in range(16)]
    langs = ["lg0", "lg1"] * 8
    weighting = ev.PropertyWeighting(0.3, 0.7, _properties(ev, table, names, INVENTORY, ["lg0", "lg1"]))
    eager = ev.Evaluator(table, names, INVENTORY, ["lg0", "lg1"], weighting=weighting)
    eager.add(decoded, labels, langs)
    eager.add(decoded, labels, langs)
    eager_ops, eager_counts = eager.operations(decoded, labels, langs)
    captured = ev.Evaluator(table, names, INVENTORY, ["lg0", "lg1"], weighting=weighting)
    static_labels = captured.encode_labels(labels, langs)  # the labels are a static input of the graph
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture (sizes the workspaces)
        captured.add(decoded, static_labels)
        captured.operations(decoded, static_labels)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    captured.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.add(decoded, static_labels)
        ops, op_counts = captured.operations(decoded, static_labels)
    ops.fill_(0)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured.totals, eager.totals) and int(eager.totals.sum()) > 0
    assert torch.equal(captured.rows()[0], eager.rows()[0]) and torch.equal(captured.rows()[1], eager.rows()[1])
    assert _bits(captured.costs().cpu().numpy()) == _bits(eager.costs().cpu().numpy())
    assert _bits(captured._operation_costs.cpu().numpy()) == _bits(eager._operation_costs.cpu().numpy())
    assert torch.equal(op_counts, eager_counts)
    for o in range(2):
        for n in range(16):
            c = int(eager_counts[o, n])
            assert torch.equal(ops[o, n, :c], eager_ops[o, n, :c]), (o, n)


@pytest.mark.parametrize("variant", ["plain", "split_remap_replace"])
@pytest.mark.parametrize("beam", [False, True])
def test_synthetic_model_end_to_end(ev, beam, variant):
    """predict -> greedy_decode_device / beam_decode_device(16, n_best=4) -> Evaluator(weighting=...): add, rows, costs,
    statistics and edits equal the restatement run on hypothesis_symbols strings -- the phoneme output under the weighting,
    the attribute outputs under unit costs."""
    from allophant_amd import spec as S, synthetic
    from allophant_amd.estimator import Batch, Estimator
    from allophant_amd.phonetic import hypothesis_symbols, split_complex_segment

    table = _table()
    names = ["syllabic", "long", "nasal", "phoneme"]
    spec = S.multitask_spec(S.tiny_encoder(2), names[:3], embedding_size=16, train_phonemes=9, n_features=5, n_values=3)
    state = synthetic.make_state_dict(spec, seed=3)
    N = 6
    audio, lengths = synthetic.make_audio(N, 12000, seed=7, ragged=True)
    tfi = synthetic.make_inventory(spec, len(INVENTORY), seed=2)
    est = Estimator(spec, state, "cuda:0", "f16x3")
    try:
        pred = est.predict(Batch(audio.cuda(), lengths, torch.zeros(N, dtype=torch.long)), tfi)
        decoded = est.beam_decode_device(pred, 16, n_best=4) if beam else est.greedy_decode_device(pred)
        hosts = decoded.hypotheses()
    finally:
        est.close()
    special = variant != "plain"
    decomposed = unicodedata.normalize("NFD", "é")
    replacements = ev.unicode_replacements(table, table.full_phonemes + [decomposed]) if special else None
    languages = ["lg0", "lg1"]
    source_maps = ({"lg0": {p: p for p in INVENTORY}, "lg1": {**{p: p for p in INVENTORY}, "ts": "s", "aː": "a"}}
                   if special else None)
    rng = np.random.default_rng(21)
    symbols = table.full_phonemes + ([decomposed] if special else [])
    labels = [[symbols[i] for i in rng.integers(0, len(symbols), rng.integers(5, 40))] for _ in range(N)]
    labels[2] = []  # an empty label: every hypothesis symbol an insertion
    langs = [languages[n % 2] for n in range(N)]
    ids = [f"utt{n}" for n in range(N)]
    options = dict(split_complex=special, source_maps=source_maps, replacements=replacements)
    properties = _properties(ev, table, names, INVENTORY, languages, **options)
    costs = (0.3, 0.7)
    e = ev.Evaluator(table, names, INVENTORY, languages, weighting=ev.PropertyWeighting(*costs, properties), **options)
    e.add(decoded, labels, langs)
    statistics, best = (t.cpu().numpy() for t in e.rows())
    got_costs = e.costs().cpu().numpy()
    got_edits = e.edits(decoded, labels, langs, ids)

    strings = hypothesis_symbols(hosts, INVENTORY, table)
    contours = {p: {n: table.feature_contour(p, n) for n in names[:3]} for p in table.full_phonemes}
    totals = {language: {name: (0, 0, 0, 0) for name in names} for language in languages}
    scored = 0
    for n in range(N):
        source = source_maps[langs[n]] if special else None
        expected_sequences, edit_operations = {}, {}
        for o, name in enumerate(names):
            expected = E.expected_symbols(name, labels[n], contours, split_complex_segment, special, replacements)
            candidates = [E.actual_symbols(name, c, split_complex_segment, special, source) for c in strings[name][n]]
            lowest, chosen = math.inf, -1
            for k, actual in enumerate(candidates):
                if name == "phoneme":
                    operations, cost, stats = W.walk(W.levensthein_matrix_weighted(expected, actual, *costs, properties),
                                                     len(expected), len(actual))
                else:
                    operations, cost = U.levensthein_operations(expected, actual)
                    stats = E.levensthein_statistics(expected, actual)
                assert tuple(statistics[o, n, k]) == stats, (name, n, k)
                assert _bits(got_costs[o, n, k]) == _bits(cost), (name, n, k)
                rate = E.word_error_rate(stats)
                if rate < lowest:
                    lowest, chosen = rate, k
                if k == 0:
                    edit_operations[name] = [list(t) for t in U.to_substitutions(expected, actual, operations)]
                scored += 1
            assert best[o, n] == chosen, (name, n)
            if chosen >= 0:
                totals[langs[n]][name] = tuple(x + int(y) for x, y in zip(totals[langs[n]][name], statistics[o, n, chosen]))
            expected_sequences[name] = expected
        reference = {"language": langs[n], "utterance_id": ids[n], "expected": expected_sequences,
                     "edit_operations": edit_operations}
        assert got_edits[n].to_dict() == reference, n
    assert scored > 0
    got = e.statistics()
    for language in languages:
        for name in names:
            assert got[language][name].astuple() == totals[language][name], (language, name)

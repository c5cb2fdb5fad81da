"""On-device edit operations (amx_edit_ops.hip) against the literal restatement of upstream's ``edits``
(tests/edit_ops_util.py): record for record at lengths around the 64-row strips up to 3000 on both sides over small alphabets
(ties everywhere); the hand-worked table; per-action counts against the statistics kernel on the same rows; the -1 / -2 rows
and untouched canaries past each row's records; graph replay; and the synthetic model -> predict -> greedy and beam decoding ->
Evaluator.edits, equal to the restatement run on hypothesis_symbols strings in every record and JSON line."""
import unicodedata

import numpy as np
import pytest
import torch

import edit_ops_util as U
import edit_util as E

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 500, 3000)
HAND_WORKED = [
    ("abc", "ac", [(2, 1, 1)], 1.0),
    ("aab", "ab", [(2, 1, 1)], 1.0),
    ("ab", "aab", [(1, 1, 1)], 1.0),
    ("ab", "ba", [(3, 0, 0), (3, 1, 1)], 2.0),
    ("abcd", "xbcdy", [(3, 0, 0), (1, 4, 4)], 2.0),
    ("", "xy", [(1, 0, 0), (1, 0, 1)], 2.0),
    ("abc", "", [(2, 0, 0), (2, 1, 0), (2, 2, 0)], 3.0),
    ("abc", "abc", [], 0.0),
]


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
def test_lengths_against_the_restatement(ev, alphabet):
    rng = np.random.default_rng(100 + alphabet)
    expected, actual = [], []
    for m in LENGTHS:
        for n in LENGTHS:
            expected.append(rng.integers(0, alphabet, m).tolist())
            actual.append(rng.integers(0, alphabet, n).tolist())
    got = ev.levensthein_operations_batch(expected, actual)
    for a, b, (operations, cost) in zip(expected, actual, got):
        assert (operations, cost) == U.levensthein_operations_fast(a, b), (len(a), len(b))
        assert all(isinstance(op[0], ev.Action) for op in operations)


def test_hand_worked_table(ev):
    for expected, actual, operations, cost in HAND_WORKED:
        assert ev.levensthein_operations(expected, actual) == (operations, cost), (expected, actual)
        assert ev.levensthein_substitutions(list(expected), list(actual)) == U.to_substitutions(expected, actual, operations)


def _beam(names, tokens, counts, hyp_counts):
    from allophant_amd.estimator import BeamDecoded

    tokens = torch.tensor(tokens, dtype=torch.int64, device="cuda")
    counts = torch.tensor(counts, dtype=torch.int32, device="cuda")
    return BeamDecoded(names, tokens, torch.zeros_like(tokens), counts,
                       torch.zeros(counts.shape, dtype=torch.float64, device="cuda"),
                       torch.tensor(hyp_counts, dtype=torch.int32, device="cuda"))


def _random_batch(rng, inventory, N, K, T):
    tokens = rng.integers(1, len(inventory) + 1, (1, N, K, T))
    counts = rng.integers(0, T + 1, (1, N, K))
    hyp = rng.integers(1, K + 1, (1, N))
    return tokens.tolist(), counts.tolist(), hyp.tolist()


def test_action_counts_equal_the_statistics_kernel(ev):
    """Both kernels on one batch: the S, D and I counts of every row's operations equal candidate 0's statistics."""
    table = _table()
    inventory = ["a", "ts", "t͡ʃ", "é", "m", "aː", "i"]
    rng = np.random.default_rng(31)
    N, K, T = 40, 3, 150
    tokens, counts, hyp = _random_batch(rng, inventory, N, K, T)
    decoded = _beam(["phoneme"], tokens, counts, hyp)
    labels = [[table.full_phonemes[i] for i in rng.integers(0, 11, rng.integers(0, 140))] for _ in range(N)]
    langs = ["lg0", "lg1"] * (N // 2)
    e = ev.Evaluator(table, ["phoneme"], inventory, ["lg0", "lg1"], split_complex=True)
    e.add(decoded, labels, langs)
    operations, op_counts = e.operations(decoded, labels, langs)
    statistics = e.rows()[0][:, :, 0].cpu().numpy()  # [O, N, 4]: I, D, S, C
    records, lengths = operations.cpu().numpy(), op_counts.cpu().numpy()
    for n in range(N):
        actions = records[0, n, :lengths[0, n], 0]
        ins, dels, subs, _ = statistics[0, n]
        assert lengths[0, n] == ins + dels + subs
        assert [(actions == 1).sum(), (actions == 2).sum(), (actions == 3).sum()] == [ins, dels, subs], n


def test_flags_and_canaries(ev):
    """hyp_counts 0: -1; a token outside the map: -2; records past each row's count (and in flagged rows) stay untouched."""
    inventory = ["a", "t", "s", "m"]
    e = ev.Evaluator(_table(), ["phoneme"], inventory, ["lg0"])
    tokens = [[[[1, 3, 4]], [[1, 2, 0]], [[3, 9, 0]], [[2, 2, 2]]]]
    counts = [[[3], [2], [2], [3]]]
    decoded = _beam(["phoneme"], tokens, counts, [[1, 0, 1, 1]])
    labels = [["a", "t"], ["a"], ["s"], []]
    operations, op_counts = e.operations(decoded, labels, ["lg0"] * 4)
    assert op_counts.cpu().tolist() == [[2, -1, -2, 3]]
    assert operations.shape[2] == 3  # max_ops = max(max_expected 2, T 3)
    space = e.maps.spaces[0]
    for n, actual in ((0, ["a", "s", "m"]), (3, ["t", "t", "t"])):
        reference = U.levensthein_operations(labels[n], actual)[0]
        want = [[a, i, j, space[labels[n][i]] if a != U.INSERTION else -1, space[actual[j]] if a != U.DELETION else -1]
                for a, i, j in reference]
        assert operations[0, n, :len(want)].tolist() == want, n
    assert operations[0, 0, :2, :3].tolist() == [[U.INSERTION, 1, 1], [U.SUBSTITUTION, 1, 2]]  # the tie goes to insertion
    _assert_canaries(e, decoded, labels, -777)


def _assert_canaries(e, decoded, labels, canary):
    """The kernel writes nothing past a row's records: run it once more through the C ABI into canary-filled outputs."""
    import ctypes as C

    from allophant_amd import evaluation, lib

    handle = evaluation._library()
    labels_batch = e.encode_labels(labels, ["lg0"] * len(labels))
    O, N = 1, len(labels)
    tokens = decoded.tokens[:, :, 0]
    counts = decoded.counts[:, :, 0].contiguous()
    hyp = decoded.hyp_counts.contiguous()
    T = tokens.shape[2]
    max_expected, max_actual = labels_batch.max_expected, T
    max_ops = max(max_expected, max_actual) + 2  # room for canaries past the limit too
    size = C.c_size_t()
    assert handle.amx_edit_operations_workspace(O * N, max_expected, max_actual, C.byref(size)) == lib.AMX_OK
    workspace = torch.empty(size.value, dtype=torch.uint8, device="cuda")
    operations = torch.full((O, N, max_ops, 5), canary, dtype=torch.int32, device="cuda")
    op_counts = torch.full((O, N), canary, dtype=torch.int32, device="cuda")
    p = evaluation._ptr
    code = handle.amx_edit_operations(
        0, p(tokens), tokens.stride(0), tokens.stride(1), O, N, T, p(counts), p(hyp), p(labels_batch.data),
        p(labels_batch.data, 2 * N + 1), p(labels_batch.data, N + 1), 1, p(e._maps), p(e._maps, e._n_offsets), p(e._label_maps),
        p(e._hyp_maps), 1, max_expected, max_actual, p(workspace), workspace.numel(), max_ops, p(operations), p(op_counts),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code == lib.AMX_OK
    torch.cuda.synchronize()
    got = op_counts.cpu().tolist()[0]
    assert got == [2, -1, -2, 3]
    records = operations.cpu()
    for n, count in enumerate(got):
        assert (records[0, n, max(count, 0):] == canary).all(), n


def test_graph_replay_equals_eager(ev):
    table = _table()
    inventory = ["a", "ts", "t͡ʃ", "é", "m", "aː", "i"]
    rng = np.random.default_rng(8)
    tokens, counts, hyp = _random_batch(rng, inventory, 16, 2, 70)
    decoded = _beam(["phoneme"], tokens, counts, hyp)
    labels = [[table.full_phonemes[i] for i in rng.integers(0, 11, rng.integers(1, 60))] for _ in range(16)]
    langs = ["lg0", "lg1"] * 8
    eager = ev.Evaluator(table, ["phoneme"], inventory, ["lg0", "lg1"])
    eager_ops, eager_counts = eager.operations(decoded, labels, langs)
    captured = ev.Evaluator(table, ["phoneme"], inventory, ["lg0", "lg1"])
    static_labels = captured.encode_labels(labels, langs)  # the labels are a static input of the graph
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        captured.operations(decoded, static_labels)  # warm-up outside the capture (sizes the workspace)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops, op_counts = captured.operations(decoded, static_labels)
    ops.fill_(0)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(op_counts, eager_counts)
    for n in range(16):
        c = int(eager_counts[0, n])
        assert torch.equal(ops[0, n, :c], eager_ops[0, n, :c]), n


@pytest.mark.parametrize("variant", ["plain", "split_remap_replace"])
@pytest.mark.parametrize("beam", [False, True])
def test_synthetic_model_end_to_end(ev, beam, variant):
    """predict -> greedy_decode_device / beam_decode_device(16, n_best=4) -> Evaluator.edits equals run.py _compute_edits
    restated on hypothesis_symbols strings (first candidate), record for record and JSON line for JSON line."""
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
    special = variant != "plain"
    decomposed = unicodedata.normalize("NFD", "é")
    replacements = ev.unicode_replacements(table, table.full_phonemes + [decomposed]) if special else None
    languages = ["lg0", "lg1"]
    source_maps = ({"lg0": {p: p for p in inventory}, "lg1": {**{p: p for p in inventory}, "ts": "s", "aː": "a"}}
                   if special else None)
    rng = np.random.default_rng(21)
    symbols = table.full_phonemes + ([decomposed] if special else [])
    labels = [[symbols[i] for i in rng.integers(0, len(symbols), rng.integers(5, 40))] for _ in range(N)]
    labels[2] = []  # an empty label: every hypothesis symbol an insertion
    langs = [languages[n % 2] for n in range(N)]
    ids = [f"utt{n}" for n in range(N)]
    e = ev.Evaluator(table, names, inventory, languages, split_complex=special, source_maps=source_maps,
                     replacements=replacements)
    got = e.edits(decoded, labels, langs, ids)

    strings = hypothesis_symbols(hosts, inventory, table)
    contours = {p: {n: table.feature_contour(p, n) for n in names[:3]} for p in table.full_phonemes}
    records = 0
    assert len(got) == N
    for n in range(N):
        candidates = {name: strings[name][n] for name in names}
        source = source_maps[langs[n]] if special else None
        reference = U.compute_edits(langs[n], ids[n], names, labels[n], candidates, contours, split_complex_segment, special,
                                    replacements, source)
        assert got[n].to_dict() == reference, n
        assert got[n].to_json() == U.to_json(reference), n
        assert ev.UtteranceEdits.from_json(got[n].to_json()) == got[n]
        assert list(got[n].expected) == names and list(got[n].edit_operations) == names
        records += sum(len(v) for v in reference["edit_operations"].values())
    assert records > 0

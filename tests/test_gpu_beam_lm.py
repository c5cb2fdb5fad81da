"""On-device CTC beam search with a phonotactic language model (amx_ctc_beam_lm.hip) against the float64 restatement of the
contract (tests/ctc_beam_lm_util.py): the same tokens, timesteps and hypothesis counts, scores within 1e-9 relative (the
tolerance of test_gpu_beam.py), for beams of 1 to 64, 2 to 1025 classes, both emission modes, ragged lengths including 0, 1
and 3000 frames, per-row tables and rows without one, the transposed [T, N, C] view read in place, inputs on which the
frame threshold with the language-model term decides, forbidden transitions; bitwise identity with the decoder without a
language model at weight 0; then through Estimator.beam_decode_device, plain and under per-language inventories."""
import numpy as np
import pytest
import torch

from allophant_amd import spec as S, synthetic
from ctc_beam_lm_util import beam_search_lm
from ctc_beam_util import beam_search

pytestmark = pytest.mark.gpu

WEIGHT, BONUS = 1.3, -0.4


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import estimator, lib

    assert lib.load() is not None
    return estimator


def _emissions(N, T, C, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(N, T, C, generator=g) * scale, dim=-1)


def _table(C, seed, scale=3.0):
    """A random fp32 table at log-softmax scale: continuous values, so ties do not decide the order."""
    g = torch.Generator().manual_seed(10_000 + seed)
    return torch.log_softmax(torch.randn(C + 1, C + 1, generator=g) * scale, dim=-1)


def _lm(amd, table, blank=0):
    return amd.PhonotacticLM(table, blank)


def _assert_rows(got, em, lengths, beam, n_best, tables, weight=WEIGHT, bonus=BONUS, blank=0, exp=True, threshold=50.0):
    """``tables``: one table (or None) per row."""
    assert len(got) == em.shape[0]
    for n in range(em.shape[0]):
        table = None if tables[n] is None else tables[n].numpy()
        want = beam_search_lm(em[n].numpy(), int(lengths[n]), beam, n_best, table, weight, bonus, blank=blank, exp=exp,
                              threshold=threshold)
        hyps = got[n]
        assert len(hyps) == len(want), (n, len(hyps), len(want))
        for h, w in zip(hyps, want):
            assert h.tokens.tolist() == w.tokens, (n, h.tokens.tolist(), w.tokens)
            assert h.timesteps.tolist() == w.timesteps, n
            assert h.words == []
            assert abs(h.score - w.score) <= 1e-9 * max(1.0, abs(w.score)), (n, h.score, w.score)


def _flat(rows):
    return [[(h.tokens.tolist(), h.score, h.timesteps.tolist()) for h in hyps] for hyps in rows]


@pytest.mark.parametrize("exp", [True, False], ids=["exp", "log"])
@pytest.mark.parametrize("C", [2, 3, 37, 300])
@pytest.mark.parametrize("beam", [1, 2, 5, 16, 64])
def test_kernel_matches_restatement(amd, beam, C, exp):
    T = 24
    em = _emissions(4, T, C, seed=beam * 1000 + C + exp)
    table = _table(C, seed=beam + C)
    lengths = torch.tensor([T, 0, 1, T - 5])
    n_best = beam if beam in (5, 64) else min(beam, 3)
    got = amd.beam_ctc_decode(em.cuda(), lengths, beam, n_best, exp_emissions=exp, lm=_lm(amd, table), lm_weight=WEIGHT,
                              token_score=BONUS)
    _assert_rows(got, em, lengths, beam, n_best, [table] * 4, exp=exp)


@pytest.mark.parametrize("exp", [True, False], ids=["exp", "log"])
def test_weight_zero_is_bitwise_the_plain_decoder(amd, exp):
    for beam, C in ((1, 2), (5, 37), (16, 300), (64, 41)):
        em = _emissions(4, 24, C, seed=77 + beam).cuda()
        lengths = torch.tensor([24, 0, 1, 19])
        plain = amd.beam_ctc_decode(em, lengths, beam, min(beam, 4), exp_emissions=exp)
        fused = amd.beam_ctc_decode(em, lengths, beam, min(beam, 4), exp_emissions=exp, lm=_lm(amd, _table(C, seed=beam)),
                                    lm_weight=0.0, token_score=0.0)
        assert _flat(fused) == _flat(plain), (beam, C)


def test_rows_without_a_table_are_bitwise_the_plain_decoder(amd):
    """A mixed stack: rows 0 and 1 follow their own tables, rows 2 and 3 (index -1) are the decoder without one."""
    C = 37
    em = _emissions(4, 24, C, seed=5)
    lengths = torch.tensor([24, 20, 24, 7])
    tables = [_table(C, seed=1), _table(C, seed=2)]
    got = amd.beam_ctc_decode(em.cuda(), lengths, 16, 4, exp_emissions=False, lm=[_lm(amd, t) for t in tables],
                              lm_weight=WEIGHT, token_score=BONUS, lm_ids=[1, 0, -1, -1])
    _assert_rows(got, em, lengths, 16, 4, [tables[1], tables[0], None, None], exp=False)
    plain = amd.beam_ctc_decode(em.cuda(), lengths, 16, 4, exp_emissions=False)
    assert _flat(got[2:]) == _flat(plain[2:])
    assert _flat(got[:2]) != _flat(plain[:2])
    with pytest.raises(ValueError):
        amd.beam_ctc_decode(em.cuda(), lengths, 16, 4, lm=[_lm(amd, t) for t in tables], lm_ids=[0, 1, 2, 0])
    with pytest.raises(ValueError):
        amd.beam_ctc_decode(em.cuda(), lengths, 16, 4, lm=[_lm(amd, t) for t in tables])
    with pytest.raises(ValueError):
        amd.beam_ctc_decode(em.cuda(), lengths, 16, 4, lm=_lm(amd, _table(C + 1, seed=1)))


def test_many_classes(amd):
    """1025 classes: every prefix's list is cut from 17 wave-wide strides of the table row."""
    em = _emissions(2, 12, 1025, seed=9)
    table = _table(1025, seed=9)
    lengths = torch.tensor([12, 9])
    got = amd.beam_ctc_decode(em.cuda(), lengths, 16, 4, exp_emissions=False, lm=_lm(amd, table), lm_weight=WEIGHT,
                              token_score=BONUS)
    _assert_rows(got, em, lengths, 16, 4, [table] * 2, exp=False)


def test_long_row_and_blank_index(amd):
    """A 3000-frame row (backpointers walked over every frame, collapse in several chunks) next to a short one, with the
    blank at a non-zero index."""
    em = _emissions(2, 3000, 37, seed=7, scale=3.0)
    table = _table(37, seed=7)
    lengths = torch.tensor([3000, 17])
    got = amd.beam_ctc_decode(em.cuda(), lengths, 16, 4, blank_index=5, exp_emissions=False, lm=_lm(amd, table, blank=5),
                              lm_weight=WEIGHT, token_score=BONUS)
    _assert_rows(got, em, lengths, 16, 4, [table] * 2, blank=5, exp=False)


def test_transposed_view_is_read_in_place(amd):
    out = _emissions(30, 5, 41, seed=11).cuda()  # [T, N, C]
    table = _table(41, seed=11)
    lengths = torch.tensor([30, 12, 0, 29, 1])
    view = out.transpose(0, 1)
    assert not view.is_contiguous()
    decoder = amd.BeamCTCDecoder(["<blank>", *[f"c{i}" for i in range(40)]], 8, 3, lm=_lm(amd, table), lm_weight=WEIGHT,
                                 token_score=BONUS)
    got = decoder(view, lengths)
    _assert_rows(got, view.cpu().contiguous(), lengths, 8, 3, [table] * 5)
    assert _flat(decoder(view.contiguous(), lengths)) == _flat(got)


def _distinct(a, b):
    return [(h.tokens, round(h.score, 9), h.timesteps) for h in a] != [(h.tokens, round(h.score, 9), h.timesteps) for h in b]


def _threshold_cases():
    """Log-probability inputs, mild by themselves, on which the frame threshold decides only through the language-model
    term (a beam with room for every candidate): a table column at -60, and a table at log-softmax scale 40."""
    column = _table(3, seed=31, scale=1.0)
    column[:, 2] = -60.0
    return {"lm_column_-60": (_emissions(4, 5, 3, seed=21, scale=1.0), column),
            "lm_scale_40": (_emissions(4, 6, 3, seed=22, scale=1.0), _table(3, seed=32, scale=40.0))}


@pytest.mark.parametrize("case", ["lm_column_-60", "lm_scale_40"])
def test_frame_threshold_includes_the_language_model(amd, case):
    """Candidates more than 50 below the frame's best generated candidate, language-model term included, are dropped before
    merging: on these inputs the restatement's n-best with threshold 50 differ from those without a threshold, while the
    emissions alone (no table) give the same lists under both; the kernel gives the former."""
    em, table = _threshold_cases()[case]
    T = em.shape[1]
    lengths = torch.tensor([T] * em.shape[0])
    for n in range(em.shape[0]):
        assert _distinct(beam_search_lm(em[n].numpy(), T, 64, 64, table.numpy(), 1.0, 0.0, exp=False),
                         beam_search_lm(em[n].numpy(), T, 64, 64, table.numpy(), 1.0, 0.0, exp=False, threshold=np.inf)), n
        assert not _distinct(beam_search(em[n].numpy(), T, 64, 64, exp=False),
                             beam_search(em[n].numpy(), T, 64, 64, exp=False, threshold=np.inf)), n
    got = amd.beam_ctc_decode(em.cuda(), lengths, 64, 64, exp_emissions=False, lm=_lm(amd, table), lm_weight=1.0)
    _assert_rows(got, em, lengths, 64, 64, [table] * em.shape[0], weight=1.0, bonus=0.0, exp=False)


@pytest.mark.parametrize("weight", [1.0, 0.0])
def test_forbidden_transitions(amd, weight):
    """-inf entries: a forbidden bigram and a forbidden beginning appear in no hypothesis, at weight 0 too; a table whose
    end column is -inf leaves no hypothesis at all."""
    C = 5
    em = _emissions(3, 12, C, seed=13, scale=1.0)
    lengths = torch.tensor([12, 12, 0])
    table = _table(C, seed=13)
    table[1, 2] = -np.inf
    table[C, 3] = -np.inf
    got = amd.beam_ctc_decode(em.cuda(), lengths, 32, 32, exp_emissions=False, lm=_lm(amd, table), lm_weight=weight)
    _assert_rows(got, em, lengths, 32, 32, [table] * 3, weight=weight, bonus=0.0, exp=False)
    for hyps in got:
        for h in hyps:
            tokens = h.tokens.tolist()
            assert tokens[:1] != [3] and all((p, n) != (1, 2) for p, n in zip(tokens, tokens[1:]))
    closed = table.clone()
    closed[:, C] = -np.inf
    none = amd.beam_ctc_decode(em.cuda(), lengths, 32, 32, exp_emissions=False, lm=[_lm(amd, table), _lm(amd, closed)],
                               lm_weight=weight, lm_ids=[1, 0, 1])
    assert none[0] == [] and none[2] == [] and _flat(none[1:2]) == _flat(got[1:2])


def _model(amd, seed=3):
    spec = S.multitask_spec(S.tiny_encoder(2), ["syllabic", "long", "nasal"], embedding_size=16, train_phonemes=9, n_features=5)
    est = amd.Estimator(spec, synthetic.make_state_dict(spec, seed=seed), "cuda:0")
    tfi = synthetic.make_inventory(spec, 11, seed=seed)
    audio, lengths = synthetic.make_audio(4, 30000, seed=seed, ragged=True)
    batch = amd.Batch(audio.cuda(), lengths, torch.zeros(4, dtype=torch.long))
    return est, tfi, batch


def test_estimator_beam_decode_with_a_language_model(amd):
    """The phoneme output equals the restatement under the table; every other output is bitwise the decode without one."""
    est, tfi, batch = _model(amd)
    pred = est.predict(batch, tfi)
    C = pred.outputs[S.PHONEME].shape[2]
    tables = [_table(C, seed=41), _table(C, seed=42)]
    ids = [0, 1, -1, 0]
    plain = est.beam_decode_device(pred, 8, 3, exp_emissions=False)
    fused = est.beam_decode_device(pred, 8, 3, exp_emissions=False, lm=[_lm(amd, t) for t in tables], lm_weight=WEIGHT,
                                   token_score=BONUS, lm_ids=ids)
    assert fused.names == plain.names and fused.scores.is_cuda
    result = fused.hypotheses()
    em = pred.outputs[S.PHONEME].cpu().transpose(0, 1).contiguous()
    _assert_rows(result[S.PHONEME], em, pred.lengths, 8, 3, [None if i < 0 else tables[i] for i in ids], exp=False)
    assert _flat(result[S.PHONEME][:2]) != _flat(plain.hypotheses()[S.PHONEME][:2])
    unfused = plain.hypotheses()
    for o, name in enumerate(plain.names):
        if name != S.PHONEME:
            assert _flat(result[name]) == _flat(unfused[name]), name  # (tokens and timesteps past `counts` are not written)
            for a, b in zip(fused[3:], plain[3:]):  # counts, scores, hyp_counts
                assert torch.equal(a[o], b[o]), name
    single = est.beam_decode(pred, 8, 3, exp_emissions=False, lm=_lm(amd, tables[0]), lm_weight=WEIGHT, token_score=BONUS)
    _assert_rows(single[S.PHONEME], em, pred.lengths, 8, 3, [tables[0]] * 4, exp=False)
    with pytest.raises(ValueError):
        est.beam_decode_device(pred, 8, 3, lm=_lm(amd, _table(C + 3, seed=1)))
    est.close()


def test_estimator_beam_decode_languages_with_a_language_model(amd):
    """A two-language batch (predict_languages): each row equals the restatement over its language's columns of the
    restricted block under the table restricted to those columns, in union class ids."""
    import restrict_util as U

    e = U.EndToEnd()
    inventories = e.inventories
    languages = ["b", "c", "c", "b", "c", "b"]  # inventories of 7 and 23 phonemes
    est = amd.Estimator(e.spec, e.state, "cuda:0", "f16x3")
    batch = amd.Batch(e.audio.cuda(), e.lengths, inventories.language_ids(languages).to(torch.long))
    pred = est.predict_languages(batch, inventories)
    C = pred.outputs[S.PHONEME].shape[2]
    table = _table(C, seed=51)
    decoded = est.beam_decode(pred, 8, 3, exp_emissions=False, lm=_lm(amd, table), lm_weight=WEIGHT, token_score=BONUS)
    block = pred.outputs[S.PHONEME].cpu()  # [T, N, C]
    for n, language in enumerate(languages):
        columns = inventories.columns(language)
        index = torch.cat([columns, torch.tensor([C])])
        own = block[:, n].index_select(1, columns).contiguous()
        want = beam_search_lm(own.numpy(), int(pred.lengths[n]), 8, 3, table[index][:, index].numpy(), WEIGHT, BONUS, exp=False)
        got = decoded[S.PHONEME][n]
        assert len(got) == len(want), n
        for h, w in zip(got, want):
            assert h.tokens.tolist() == columns[torch.tensor(w.tokens, dtype=torch.int64)].tolist(), n
            assert h.timesteps.tolist() == w.timesteps, n
            assert abs(h.score - w.score) <= 1e-9 * max(1.0, abs(w.score)), (n, h.score, w.score)
    est.close()

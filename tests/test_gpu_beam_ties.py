"""The two on-device CTC beam decoders (amx_ctc_beam.hip, amx_ctc_beam_lm.hip) where equal scores decide: the tie rule of
DESIGN 9, -inf emissions, exponentials that underflow or round together, and language-model tables with equal entries.

Exact comparison with the float64 restatements (tokens, timesteps and hypothesis counts equal, scores within 1e-9 relative)
on the tied input families of tests/ctc_beam_ties_util.py: continuous random emissions with duplicated columns, so equal
scores come from the same sequence of operations.  Every case first asserts on the host that no decision rests on a
difference below 1e-6 relative and that the reversed tie rule gives other n-best, so a kernel that broke ties the other way
would fail.  Then: the two kernels are one decoder at weight 0, bitwise, on every family; both kernels against brute force
over every alignment on tiny dyadic rows (scores and sets, no tie order); the public calls on a restricted union block as
``predict_languages`` leaves it; and every call twice, bitwise equal."""
import numpy as np
import pytest
import torch

import ctc_beam_ties_util as U
from ctc_beam_lm_util import brute_force_lm
from ctc_beam_util import brute_force, search

pytestmark = pytest.mark.gpu

ALL_CASES = [c for c in U.CASES + U.LM_CASES if c.C <= 4095]  # what the kernel with a table slot takes


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import estimator, lib

    assert lib.load() is not None
    return estimator


def _flat(rows):
    return [[(h.tokens.tolist(), h.score, h.timesteps.tolist()) for h in hyps] for hyps in rows]


def _twice(call):
    """The call's result, after asserting that a second call gives bitwise the same."""
    first, second = call(), call()
    assert _flat(first) == _flat(second)
    return first


def _assert_rows(got, want_rows):
    assert len(got) == len(want_rows)
    for n, (hyps, want) in enumerate(zip(got, want_rows)):
        assert len(hyps) == len(want), (n, len(hyps), len(want))
        for h, w in zip(hyps, want):
            assert h.tokens.tolist() == w.tokens, (n, h.tokens.tolist(), w.tokens)
            assert h.timesteps.tolist() == w.timesteps, n
            assert h.words == []
            assert abs(h.score - w.score) <= 1e-9 * max(1.0, abs(w.score)), (n, h.score, w.score)


def _models(amd, tables):
    return [amd.PhonotacticLM(torch.from_numpy(np.ascontiguousarray(t)), 0) for t in tables]


def _decode(amd, case, data, em):
    lengths = torch.tensor(data.lengths)
    if not data.stack:
        return _twice(lambda: amd.beam_ctc_decode(em, lengths, case.beam, case.n_best, exp_emissions=case.exp))
    return _twice(lambda: amd.beam_ctc_decode(em, lengths, case.beam, case.n_best, exp_emissions=case.exp,
                                              lm=_models(amd, data.stack), lm_weight=data.weight, token_score=data.bonus,
                                              lm_ids=data.ids))


@pytest.mark.parametrize("case", U.CASES, ids=[c.id for c in U.CASES])
def test_kernel_matches_restatement_on_ties(amd, case):
    """Duplicated columns (the list cut inside a group at C > beam + 2), constant frames (every key of the list selection
    equal), -inf columns on both sides of beam + 2 (exact zeros that tie under EXP, never a candidate in log mode, the blank
    itself -inf in some frames), and exponentials that are one value for distinct raw emissions."""
    ref = U.check_preconditions(case)
    data = U.inputs(case)
    got = _decode(amd, case, data, torch.from_numpy(data.em).cuda())
    _assert_rows(got, ref.rows)
    if case.family.startswith("dead") and not case.exp:
        dead = set(np.flatnonzero(np.isinf(data.em[0]).all(axis=0)).tolist())
        assert dead and not any(dead & set(h.tokens.tolist()) for h in got[0])


@pytest.mark.parametrize("case", U.LM_CASES, ids=[c.id for c in U.LM_CASES])
def test_lm_kernel_matches_restatement_on_ties(amd, case):
    """Tables with equal entries: PhonotacticLM's own add-k estimate (every unseen bigram of a row equal), rows and columns
    duplicated with the emission columns, a table of one value under constant frames (every key of a prefix's selection
    equal, at C = 300 through the wave buffer), -inf inside a tied group, a tied end column, per-row tables with a row
    without one; both weight pairs."""
    ref = U.check_preconditions(case)
    data = U.inputs(case)
    got = _decode(amd, case, data, torch.from_numpy(data.em).cuda())
    _assert_rows(got, ref.rows)


@pytest.mark.parametrize("case", ALL_CASES, ids=[c.id for c in ALL_CASES])
def test_weight_zero_is_bitwise_the_plain_decoder_on_ties(amd, case):
    """On every family's emissions the kernel with a table slot is the plain decoder bit for bit: rows at index -1, weight
    0 and bonus 0 under a continuous table, and the same under a table with duplicated values."""
    data = U.inputs(case)
    em = torch.from_numpy(data.em).cuda()
    lengths = torch.tensor(data.lengths)
    plain = _flat(_twice(lambda: amd.beam_ctc_decode(em, lengths, case.beam, case.n_best, exp_emissions=case.exp)))
    rng = np.random.default_rng(case.C)
    continuous = np.log(rng.dirichlet(np.ones(case.C + 1), size=case.C + 1)).astype(np.float32)
    duplicated = np.round(continuous)  # a handful of values, many equal
    for table, ids, weight in ((continuous, [-1] * 4, 1.3), (continuous, [0] * 4, 0.0), (duplicated, [0] * 4, 0.0)):
        fused = _twice(lambda: amd.beam_ctc_decode(em, lengths, case.beam, case.n_best, exp_emissions=case.exp,
                                                   lm=_models(amd, [table]), lm_weight=weight, token_score=0.0, lm_ids=ids))
        assert _flat(fused) == plain, (ids[0], weight, table is duplicated)


def test_signed_zeros_are_one_value(amd):
    """Log-probabilities of -0.0 and 0.0 are equal values: six classes at zero, the two lowest with the sign bit set, and a
    list of beam + 2 = 4.  The rule lists classes 1 to 4 and extends by the two lowest of them, which then stay (beam
    states come first); an order by bit pattern would list 3 to 6 and begin with 3."""
    em = np.full((1, 4, 9), -3.0, dtype=np.float32)
    em[:, :, 0] = -1.0
    em[:, :, 1:3] = -0.0
    em[:, :, 3:7] = 0.0
    assert np.signbit(em[0, 0, 1]) and not np.signbit(em[0, 0, 3])
    want = [search(em[0], 4, 2, 2, exp=False)]
    assert [h.tokens for h in want[0]] == [[1], [2]]
    assert want != [search(em[0], 4, 2, 2, exp=False, reverse_ties=True)]
    lengths = torch.tensor([4])
    device = torch.from_numpy(em).cuda()
    plain = _twice(lambda: amd.beam_ctc_decode(device, lengths, 2, 2, exp_emissions=False))
    _assert_rows(plain, want)
    table = np.zeros((10, 10), dtype=np.float32)
    fused = _twice(lambda: amd.beam_ctc_decode(device, lengths, 2, 2, exp_emissions=False, lm=_models(amd, [table]),
                                               lm_weight=1.0, token_score=0.0, lm_ids=[-1]))
    assert _flat(fused) == _flat(plain)


def test_an_extension_onto_a_far_lower_beam_state_comes_first(amd):
    """``sharp_row`` at beam 4 through both kernels: the extensions onto beam states 40 below tie exactly with the
    extensions off the token list, and come first ([1], [2], [3], [4]; the other order of kinds owes [4] to [7], which
    lists of beam + 2 tokens cannot give)."""
    em = U.sharp_row()
    report = {}
    want = [search(em, 2, 4, 4, exp=False, report=report)]
    assert [h.tokens for h in want[0]] == [[1], [2], [3], [4]] and report["gap"] >= U.GAP
    assert want != [search(em, 2, 4, 4, exp=False, reverse_ties=True)]
    lengths = torch.tensor([2])
    device = torch.from_numpy(em[None]).cuda()
    plain = _twice(lambda: amd.beam_ctc_decode(device, lengths, 4, 4, exp_emissions=False))
    _assert_rows(plain, want)
    table = np.zeros((11, 11), dtype=np.float32)
    for ids in ([-1], [0]):
        fused = _twice(lambda: amd.beam_ctc_decode(device, lengths, 4, 4, exp_emissions=False, lm=_models(amd, [table]),
                                                   lm_weight=1.0, token_score=0.0, lm_ids=ids))
        _assert_rows(fused, want)


def _against_brute_force(hyps, exact, complete):
    scores = dict(exact)
    labellings = [tuple(h.tokens.tolist()) for h in hyps]
    assert len(set(labellings)) == len(labellings)
    assert all(a.score >= b.score for a, b in zip(hyps, hyps[1:]))
    for h, labelling in zip(hyps, labellings):
        want = scores[labelling]
        assert abs(h.score - want) <= 1e-9 * max(1.0, abs(want)), (labelling, h.score, want)
    if complete:
        assert set(labellings) == set(scores)


@pytest.mark.parametrize("exp", [True, False], ids=["exp", "log"])
def test_tied_rows_against_brute_force_on_the_device(amd, exp):
    """The tiny dyadic rows at beam 64 and n_best 64 through both kernels: each hypothesis has the exact score of its
    labelling (the log-sum-exp over every alignment, plus the table's terms), scores do not increase, labellings are
    distinct, and they are all of brute force's where the restatement drops nothing.  Order among equal scores is not
    asserted: mathematically equal sums are computed in different ways here."""
    for name, row in U.dyadic_rows():
        T, C = row.shape
        em = torch.from_numpy(row[None]).cuda()
        lengths = torch.tensor([T])
        report = {}
        search(row, T, 64, 64, exp=exp, report=report)
        assert report["dropped"] == 0, name
        plain = _twice(lambda: amd.beam_ctc_decode(em, lengths, 64, 64, exp_emissions=exp))
        _against_brute_force(plain[0], brute_force(row, T, exp=exp), complete=True)
        table = U.dyadic_table(C, T)
        for weight, bonus in ((1.0, 0.0), (0.5, -0.25)):
            report = {}
            search(row, T, 64, 64, table, weight, bonus, exp=exp, report=report)
            fused = _twice(lambda: amd.beam_ctc_decode(em, lengths, 64, 64, exp_emissions=exp, lm=_models(amd, [table])[0],
                                                       lm_weight=weight, token_score=bonus))
            _against_brute_force(fused[0], brute_force_lm(row, T, table, weight, bonus, exp=exp),
                                 complete=report["dropped"] == 0)


def _restated(block, lengths, beam, n_best, table=None, weight=1.0, bonus=0.0):
    """The restatement's rows on an [N, T, C] block in the default EXP mode, after the two preconditions."""
    rows, reversed_rows = [], []
    for n in range(block.shape[0]):
        a, b = {}, {}
        rows.append(search(block[n], int(lengths[n]), beam, n_best, table, weight, bonus, report=a))
        reversed_rows.append(search(block[n], int(lengths[n]), beam, n_best, table, weight, bonus, reverse_ties=True, report=b))
        assert min(a["gap"], b["gap"]) >= U.GAP, (n, a["gap"], b["gap"])
    assert rows != reversed_rows
    return rows


def test_public_decoders_on_a_restricted_union_block(amd):
    """The call a user of the reference's decoder makes after ``predict_languages``: ``beam_ctc_decode`` and
    ``BeamCTCDecoder`` (with and without a ``PhonotacticLM``) on the union block as it is, -inf outside each utterance's
    language, in the default EXP mode, where every such class adds exactly 0."""
    import restrict_util as R
    from allophant_amd import spec as S

    e = R.EndToEnd()
    # a b c c a b, inventories of 1, 7 and 23 phonemes: with one live phoneme the dead classes fill the beam of 8 and their
    # order decides the n-best; with 23 the equal unseen bigrams of the add-k table do
    languages = list(e.LANGUAGES)
    est = amd.Estimator(e.spec, e.state, "cuda:0", "f16x3")
    batch = amd.Batch(e.audio.cuda(), e.lengths, e.inventories.language_ids(languages).to(torch.long))
    pred = est.predict_languages(batch, e.inventories)
    view = pred.outputs[S.PHONEME].transpose(0, 1)
    block = view.cpu().contiguous().numpy()
    C = block.shape[2]
    assert np.isinf(block[0, 0]).any() and C > 8 + 2
    got = _twice(lambda: amd.beam_ctc_decode(view, pred.lengths, 8, 3))
    _assert_rows(got, _restated(block, pred.lengths, 8, 3))
    tokens = ["<blank>", *[f"p{i}" for i in range(1, C)]]
    assert _flat(amd.BeamCTCDecoder(tokens, 8, 3)(view, pred.lengths)) == _flat(got)
    words = [[1, 2, 3], [2, 2, 4], [4], [3, 1, 2, 3], [5, 1], [2, 3, 5, 5]]
    lm = amd.PhonotacticLM.from_sequences(words, classes=C, smoothing=1.0)
    decoder = amd.BeamCTCDecoder(tokens, 8, 3, lm=lm, lm_weight=1.3, token_score=-0.4)
    fused = _twice(lambda: decoder(view, pred.lengths))
    _assert_rows(fused, _restated(block, pred.lengths, 8, 3, lm.table.numpy(), 1.3, -0.4))
    est.close()

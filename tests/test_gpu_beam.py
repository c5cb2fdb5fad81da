"""On-device CTC beam search (amx_ctc_beam.hip) against the float64 restatement of the contract (tests/ctc_beam_util.py):
the same tokens, timesteps and hypothesis counts, scores within 1e-9 relative, for beams of 1 to 64, 2 to 1025 classes,
probability (EXP, the reference's call) and log-probability emissions, ragged lengths including 0, 1 and 3000 frames, and
the transposed [T, N, C] view read in place; inputs on which the frame and end thresholds decide the result; then through
Estimator.beam_decode on a synthetic model."""
import numpy as np
import pytest
import torch

from allophant_amd import spec as S, synthetic
from ctc_beam_util import beam_search

pytestmark = pytest.mark.gpu


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


def _assert_rows(got, em, lengths, beam, n_best, blank=0, exp=True):
    assert len(got) == em.shape[0]
    for n in range(em.shape[0]):
        want = beam_search(em[n].numpy(), int(lengths[n]), beam, n_best, blank=blank, exp=exp)
        hyps = got[n]
        assert len(hyps) == len(want), (n, len(hyps), len(want))
        for h, w in zip(hyps, want):
            assert h.tokens.tolist() == w.tokens, (n, h.tokens.tolist(), w.tokens)
            assert h.timesteps.tolist() == w.timesteps, n
            assert h.words == []
            assert abs(h.score - w.score) <= 1e-9 * max(1.0, abs(w.score)), (n, h.score, w.score)


@pytest.mark.parametrize("exp", [True, False], ids=["exp", "log"])
@pytest.mark.parametrize("C", [2, 3, 37, 1025])
@pytest.mark.parametrize("beam", [1, 2, 5, 16, 64])
def test_kernel_matches_restatement(amd, beam, C, exp):
    T = 24 if C < 1025 else 12
    em = _emissions(4, T, C, seed=beam * 1000 + C + exp)
    lengths = torch.tensor([T, 0, 1, T - 5])
    n_best = min(beam, 3) if beam != 5 else 5
    got = amd.beam_ctc_decode(em.cuda(), lengths, beam, n_best, exp_emissions=exp)
    _assert_rows(got, em, lengths, beam, n_best, exp=exp)


@pytest.mark.parametrize("exp", [True, False], ids=["exp", "log"])
def test_long_row_and_blank_index(amd, exp):
    """A 3000-frame row (backpointers walked over every frame, collapse in several chunks) next to short ones, with the
    blank at a non-zero index."""
    em = _emissions(3, 3000, 37, seed=7, scale=3.0)
    lengths = torch.tensor([3000, 17, 2999])
    got = amd.beam_ctc_decode(em.cuda(), lengths, 16, 4, blank_index=5, exp_emissions=exp)
    _assert_rows(got, em, lengths, 16, 4, blank=5, exp=exp)


def _distinct(a, b):
    return [(h.tokens, round(h.score, 9), h.timesteps) for h in a] != [(h.tokens, round(h.score, 9), h.timesteps) for h in b]


def _threshold_cases():
    """Log-probability inputs on which the frame threshold decides the result (a beam with room for every candidate):
    a column at -60, log_softmax at scale 40, and emissions offset by -20 (where a cut of max s - 50, without + max e,
    would act like a threshold of 30)."""
    column = _emissions(4, 5, 3, seed=21, scale=1.0)
    column[:, 1:4, 2] = -60.0
    return {"column_-60": (column, np.inf), "scale_40": (_emissions(4, 6, 3, seed=22, scale=40.0), np.inf),
            "offset_-20": (_emissions(4, 6, 3, seed=23, scale=8.0) - 20.0, 30.0)}


@pytest.mark.parametrize("case", ["column_-60", "scale_40", "offset_-20"])
def test_frame_threshold_is_applied(amd, case):
    """Candidates more than 50 below the frame's best (max s + max e) are dropped before merging: on these inputs the
    restatement's n-best with threshold 50 differ from those with the other threshold, and the kernel gives the former."""
    em, other = _threshold_cases()[case]
    lengths = torch.tensor([em.shape[1]] * em.shape[0])
    for n in range(em.shape[0]):
        T = em.shape[1]
        assert _distinct(beam_search(em[n].numpy(), T, 64, 64, exp=False),
                         beam_search(em[n].numpy(), T, 64, 64, exp=False, threshold=other)), n
    got = amd.beam_ctc_decode(em.cuda(), lengths, 64, 64, exp_emissions=False)
    _assert_rows(got, em, lengths, 64, 64, exp=False)


def test_end_threshold_is_applied(amd):
    """The end step cuts against the best merged state: "a" merges two paths (0 and -0.01) to 0.688, so "ca" at -49.5 (kept
    by the frame cut at -50) falls below 0.688 - 50 and is dropped; without the end cut it would be the second hypothesis."""
    em = torch.tensor([[[0.0, -0.01, -100.0, -49.5], [-100.0, 0.0, -100.0, -100.0]]])
    lengths = torch.tensor([2])
    want = beam_search(em[0].numpy(), 2, 8, 8, exp=False)
    assert [h.tokens for h in want] == [[1]]
    assert [h.tokens for h in beam_search(em[0].numpy(), 2, 8, 8, exp=False, end_threshold=np.inf)] == [[1], [3, 1]]
    got = amd.beam_ctc_decode(em.cuda(), lengths, 8, 8, exp_emissions=False)
    _assert_rows(got, em, lengths, 8, 8, exp=False)
    assert abs(got[0][0].score - np.logaddexp(0.0, np.float32(-0.01))) < 1e-12


def test_transposed_view_is_read_in_place(amd):
    """The [N, T, C] view of a [T, N, C] output (run.py:770-773) decodes like its contiguous copy."""
    out = _emissions(30, 5, 41, seed=11).cuda()  # [T, N, C]
    lengths = torch.tensor([30, 12, 0, 29, 1])
    view = out.transpose(0, 1)
    assert not view.is_contiguous()
    decoder = amd.BeamCTCDecoder(["<blank>", *[f"c{i}" for i in range(40)]], 8, 3)
    got = decoder(view, lengths)
    _assert_rows(got, view.cpu().contiguous(), lengths, 8, 3)
    again = decoder(view.contiguous(), lengths)
    for a, b in zip(got, again):
        assert [(h.tokens.tolist(), h.score, h.timesteps.tolist()) for h in a] == \
            [(h.tokens.tolist(), h.score, h.timesteps.tolist()) for h in b]


def test_limits_raise(amd):
    em = _emissions(2, 4, 3, seed=1).cuda()
    lengths = torch.tensor([4, 4])
    with pytest.raises(ValueError):
        amd.beam_ctc_decode(em, lengths, 65, 1)
    with pytest.raises(ValueError):
        amd.beam_ctc_decode(em, lengths, 4, 5)
    with pytest.raises(ValueError):
        amd.beam_ctc_decode(em[:, :, :1].contiguous(), lengths, 4, 1)
    with pytest.raises(RuntimeError):
        amd.beam_ctc_decode(em.cpu(), lengths, 4, 1)


def _model(amd, seed=3):
    spec = S.multitask_spec(S.tiny_encoder(2), ["syllabic", "long", "nasal"], embedding_size=16, train_phonemes=9, n_features=5)
    est = amd.Estimator(spec, synthetic.make_state_dict(spec, seed=seed), "cuda:0")
    tfi = synthetic.make_inventory(spec, 11, seed=seed)
    audio, lengths = synthetic.make_audio(4, 30000, seed=seed, ragged=True)
    pred = est.predict(amd.Batch(audio.cuda(), lengths, torch.zeros(4, dtype=torch.long)), tfi)
    return est, pred


@pytest.mark.parametrize("exp", [True, False], ids=["exp", "log"])
def test_estimator_beam_decode(amd, exp):
    est, pred = _model(amd)
    decoded = est.beam_decode_device(pred, 8, 3, exp_emissions=exp)
    assert decoded.tokens.is_cuda and decoded.scores.dtype == torch.float64
    result = decoded.hypotheses()
    assert list(result) == list(pred.outputs)
    for name, out in pred.outputs.items():
        em = out.cpu().transpose(0, 1).contiguous()
        _assert_rows(result[name], em, pred.lengths, 8, 3, exp=exp)
    assert est.beam_decode(pred, 8, 3, exp_emissions=exp).keys() == result.keys()
    est.close()


def test_near_one_hot_top_hypothesis_is_greedy(amd):
    """On near one-hot log-probabilities the best hypothesis is the greedy alignment.  (Not so with the reference's
    probability emissions: a sum of probabilities charges a wrong frame only about 1, so labellings with many alignments
    outweigh the greedy one; the restatement shows the same.)"""
    est, pred = _model(amd, seed=5)
    T, N = next(iter(pred.outputs.values())).shape[:2]
    for name, out in pred.outputs.items():
        C = out.shape[2]
        idx = out.argmax(-1)
        g = torch.Generator().manual_seed(C)
        logits = torch.randn(T, N, C, generator=g).cuda() + 12.0 * torch.nn.functional.one_hot(idx, C).float()
        sharp = torch.log_softmax(logits, -1)
        hyps = amd.beam_ctc_decode(sharp.transpose(0, 1), pred.lengths, 16, 1, exp_emissions=False)
        greedy_sharp = amd.greedy_ctc_decode(sharp.transpose(0, 1), pred.lengths)
        for n in range(N):
            assert hyps[n][0].tokens.tolist() == greedy_sharp[n][0].tokens.tolist(), (name, n)
            assert hyps[n][0].timesteps.tolist() == greedy_sharp[n][0].timesteps.tolist(), (name, n)
    est.close()

"""``Estimator.map_allophones`` on the MI355X (amx_allophone.hip through amx_set_allophones / amx_map_allophones): bitwise the
REAL reference's ``AllophoneMapping.map_allophones`` on tests/golden/g17_allophone_mapping.npz, bitwise the NumPy restatement
of test_allophone_mapping.py at full-size strided geometries and on ``predict`` outputs, and end to end from a restored
checkpoint within the log-prob gate with equal greedy CTC tokens."""
import json
import os

import numpy as np
import pytest
import torch

from allophant_amd import spec as S, synthetic
from test_allophone_mapping import FINFO_MIN, G17, map_allophones_np

pytestmark = pytest.mark.gpu

KEY = "_projection._layers.phoneme._allophone_layer._allophone_matrices"


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import estimator, lib

    assert lib.load() is not None
    return estimator


@pytest.fixture(scope="module")
def g17():
    return np.load(G17)


def _mapping(g17):
    return json.loads(bytes(g17["mapping_json"]).decode())


def _tiny(g17):
    spec = json.loads(bytes(g17["e2e/spec_json"]).decode())
    state = synthetic.make_state_dict(spec, seed=int(g17["e2e/seed"]))
    state[KEY] = torch.from_numpy(g17["matrices"].copy())
    return spec, state


def _bitwise(got, expected):
    torch.testing.assert_close(got.cpu(), torch.as_tensor(expected), rtol=0, atol=0, equal_nan=True)


def map_allophones_sparse(x, matrices, mask, ids):
    """The restatement without the dense [T, P+1, Q+1] temporary (same values: every column is the NaN-propagating max of its
    unmasked products and, if it has a masked entry, finfo.min); for the full-size geometries."""
    T, N, _ = x.shape
    n_lang, _, Q1 = matrices.shape
    out = np.empty((T, N, Q1), dtype=np.float32)
    for n, v in enumerate(ids):
        lang = int(v) % n_lang
        keep = ~mask[lang]
        K = max(int(keep.sum(0).max()), 1)
        p_idx = np.zeros((K, Q1), dtype=np.int64)
        valid = np.zeros((K, Q1), dtype=bool)
        for q in range(Q1):
            rows = np.nonzero(keep[:, q])[0]
            p_idx[: len(rows), q] = rows
            valid[: len(rows), q] = True
        w = matrices[lang][p_idx, np.arange(Q1)[None]]
        with np.errstate(invalid="ignore", over="ignore"):
            product = x[:, n][:, p_idx] * w[None]  # [T, K, Q1]
        start = np.where(mask[lang].any(0), FINFO_MIN, -np.inf).astype(np.float32)
        product = np.where(valid[None], product, start[None, None])
        out[:, n] = np.concatenate([np.broadcast_to(start, (T, 1, Q1)), product], axis=1).max(axis=1)
    return out


def test_sparse_restatement_is_the_dense_one(g17):
    for ids in (g17["ids"], g17["ids_float"]):
        dense = map_allophones_np(g17["inputs"], g17["matrices"], g17["mask"], ids.tolist())
        sparse = map_allophones_sparse(g17["inputs"], g17["matrices"], g17["mask"], [int(v) for v in ids.tolist()])
        np.testing.assert_array_equal(sparse, dense)


def test_g17_bitwise_the_reference(amd, g17):
    spec, state = _tiny(g17)
    est = amd.Estimator(spec, state, "cuda:0")
    est.set_allophones(_mapping(g17))
    assert est.allophone_languages == json.loads(bytes(g17["index_map_json"]).decode())
    x = torch.from_numpy(g17["inputs"]).cuda()
    for key in ("", "_float"):
        ids = torch.from_numpy(g17["ids" + key])
        out = est.map_allophones(x, ids)
        assert out.shape == (37, 6, 18) and out.dtype == torch.float32 and out.is_cuda
        _bitwise(out, g17["outputs" + key])
    # ids on the device and as a list work alike; a transposed (non-contiguous) input is read in place
    _bitwise(est.map_allophones(x, torch.from_numpy(g17["ids"]).cuda()), g17["outputs"])
    _bitwise(est.map_allophones(x, g17["ids"].tolist()), g17["outputs"])
    xt = torch.from_numpy(g17["inputs"]).transpose(0, 1).contiguous().cuda().transpose(0, 1)
    assert not xt.is_contiguous()
    _bitwise(est.map_allophones(xt, g17["ids"].tolist()), g17["outputs"])
    # a second set_allophones replaces the first
    est.set_allophones(_mapping(g17))
    _bitwise(est.map_allophones(x, g17["ids"].tolist()), g17["outputs"])
    # empty batches
    assert est.map_allophones(x[:0], g17["ids"].tolist()).shape == (0, 6, 18)
    assert est.map_allophones(x[:, :0], []).shape == (37, 0, 18)
    est.close()


def _random_mapping(n_lang, P, Q, seed):
    g = np.random.default_rng(seed)
    allophones = {}
    for lang in g.permutation(n_lang - 1):  # out of order; the last language has no entry
        per = {}
        for q in g.permutation(Q):
            k = int(g.integers(0, 6))
            if k:
                per[int(q)] = sorted(int(p) for p in g.choice(P, size=k, replace=False))
        allophones[int(lang)] = per
    return {"allophones": allophones, "languages": [f"l{i}" for i in range(n_lang)], "shared_phones": [f"p{i}" for i in range(P)]}


@pytest.mark.parametrize("P1", [1025, 4096])
def test_full_size_strided_against_the_restatement(amd, P1):
    """P+1 = 1025 / 4096 phones, Q+1 = 769 phonemes, 8 languages, 32 utterances of 10 s (499 frames), read from a
    [T, N, P+1] view of a wider flat buffer."""
    from allophant_amd.allophones import build_structure

    Q1, n_lang, T, N = 769, 8, 499, 32
    spec = S.multitask_spec(S.tiny_encoder(1), ["syllabic"], embedding_size=None, train_phonemes=Q1 - 1, allophone_layer=True)
    spec["shared_phones"] = P1 - 1
    mapping = _random_mapping(n_lang, P1 - 1, Q1 - 1, seed=P1)
    structure = build_structure(mapping, P1, Q1)
    g = torch.Generator().manual_seed(P1)
    values = structure.initialization + 0.3 * torch.randn(n_lang, P1, Q1, generator=g)
    state = synthetic.make_state_dict(spec, seed=5)
    state[KEY] = values
    est = amd.Estimator(spec, state, "cuda:0")
    est.set_allophones(mapping)
    flat = torch.randn(T * N * (P1 + 7) + 3, generator=g).log_softmax(0)
    flat[torch.randint(0, flat.numel(), (64,), generator=g)] = float("nan")
    flat[torch.randint(0, flat.numel(), (64,), generator=g)] = float("-inf")
    x_host = flat[3:].view(T, N, P1 + 7)[:, :, :P1]
    ids = torch.randint(-n_lang, n_lang, (N,), generator=g)
    x = flat.cuda()[3:].view(T, N, P1 + 7)[:, :, :P1]
    assert x.stride() == (N * (P1 + 7), P1 + 7, 1)
    out = est.map_allophones(x, ids)
    torch.cuda.synchronize()
    expected = map_allophones_sparse(x_host.numpy(), values.numpy(), structure.mask.numpy(), ids.tolist())
    _bitwise(out, expected)
    est.close()


def test_predict_then_map_equals_the_restatement(amd, g17):
    spec, state = _tiny(g17)
    est = amd.Estimator(spec, state, "cuda:0")
    audio, lengths = synthetic.make_audio(4, 8000, seed=31, ragged=True)
    batch = amd.Batch(audio.cuda(), lengths, torch.tensor([0, 2, -1, 1]))
    before = est.predict(batch)
    flat_before = before._flat.clone()
    est.set_allophones(_mapping(g17))
    pred = est.predict(batch)
    phone = pred.outputs["phone"]
    out = est.map_allophones(phone, batch.language_ids)  # the view of the flat output buffer, as it is
    expected = map_allophones_np(phone.cpu().numpy(), g17["matrices"], g17["mask"], batch.language_ids.tolist())
    _bitwise(out, expected)
    # the map leaves the forward pass alone: predictions before and after set_allophones / map_allophones are bitwise equal
    after = est.predict(batch)
    assert torch.equal(flat_before, pred._flat) and torch.equal(after._flat, flat_before)
    est.check_finite()
    est.close()


def test_restore_predict_map_decode_end_to_end(amd, g17):
    from allophant_amd.checkpoint import make_checkpoint

    spec, state = _tiny(g17)
    for keys in ("str", "int"):
        mapping = _mapping(g17)
        if keys == "int":
            mapping["allophones"] = {int(k): {int(q): v for q, v in m.items()} for k, m in mapping["allophones"].items()}
        checkpoint = make_checkpoint(spec, state, synthetic_encoder=True, indexer_state={"language_allophones": mapping})
        est, indexer = amd.Estimator.restore(checkpoint, "cuda:0")
        assert indexer is None  # no embedded table: the allophone layer is rebuilt from the mapping all the same
        assert est.allophone_languages == json.loads(bytes(g17["index_map_json"]).decode())
        audio, lengths = torch.from_numpy(g17["e2e/audio"]), torch.from_numpy(g17["e2e/lengths"])
        ids = torch.from_numpy(g17["e2e/ids"])
        pred = est.predict(amd.Batch(audio.cuda(), lengths, ids))
        frames = torch.from_numpy(g17["e2e/frame_lengths"])
        assert torch.equal(pred.lengths.cpu(), frames)
        mapped = est.map_allophones(pred.outputs["phone"], ids)
        expected = torch.from_numpy(g17["e2e/mapped"])
        valid = (torch.arange(expected.shape[0]).unsqueeze(1) < frames.unsqueeze(0)).unsqueeze(-1)
        worst = ((mapped.cpu() - expected).abs() * valid).max().item()
        assert worst < 1e-3, worst
        hyps = amd.greedy_ctc_decode(mapped.transpose(1, 0), pred.lengths)
        for i, h in enumerate(hyps):
            assert torch.equal(h[0].tokens, torch.from_numpy(g17[f"e2e/tokens/{i}"])), (keys, i)
            assert torch.equal(h[0].timesteps, torch.from_numpy(g17[f"e2e/timesteps/{i}"])), (keys, i)
        est.close()


def test_errors(amd, g17):
    spec, state = _tiny(g17)
    est = amd.Estimator(spec, state, "cuda:0")
    x = torch.from_numpy(g17["inputs"]).cuda()
    ids = g17["ids"].tolist()
    with pytest.raises(RuntimeError, match="set_allophones"):
        est.map_allophones(x, ids)
    est.set_allophones(_mapping(g17))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        est.map_allophones(x.cpu(), ids)
    with pytest.raises(ValueError, match="language ids for 6 utterances"):
        est.map_allophones(x, ids[:5])
    with pytest.raises(IndexError, match="out of bounds"):
        est.map_allophones(x, [0, 1, 2, 3, 4, 0])
    with pytest.raises(IndexError, match="out of bounds"):
        est.map_allophones(x, [0, 1, 2, 3, -5, 0])
    with pytest.raises(ValueError, match="classes"):  # a phone block of another width (a custom composition inventory)
        est.map_allophones(x[:, :, :20], ids)
    bad = _mapping(g17)
    bad["allophones"]["0"]["3"] = [23]
    with pytest.raises(ValueError, match="shared phone index"):
        est.set_allophones(bad)
    few = _mapping(g17)
    few["languages"] = few["languages"] + ["eng"]  # five languages: the trained matrices hold four
    with pytest.raises(ValueError, match="_allophone_matrices"):
        est.set_allophones(few)
    _bitwise(est.map_allophones(x, ids), g17["outputs"])  # the failed calls left the installed layer alone
    est.close()

    plain = S.multitask_spec(S.tiny_encoder(1), ["syllabic"], embedding_size=None, train_phonemes=17)
    est = amd.Estimator(plain, synthetic.make_state_dict(plain, seed=2), "cuda:0")
    message = "Can't map phones to allophones with a model without an allophone layer"
    with pytest.raises(ValueError, match=message):
        est.map_allophones(x, ids)
    with pytest.raises(ValueError, match=message):
        est.set_allophones(_mapping(g17))
    est.close()

"""Per-utterance inventories on the device: amx_restrict_outputs (amx_restrict.hip) against the float64 restatement of its
contract (tests/restrict_util.py) over class counts around the 64-column strips and the register-resident limit, in both
forms, through every layout and in place, with malformed rows; then Estimator.predict_languages against the CPU oracle run
per language, reassigned between passes, and every decoder on such predictions against its own restatement fed the
utterance's compact per-language slice."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import restrict_util as U

pytestmark = pytest.mark.gpu

GATE = 1e-3  # the project's logit gate
SENTINEL = -12345.5
T, N = 7, 5
LENGTHS = [7, 0, 3, 7, 1]
# the register-resident rows end at 512 classes: 513 and 700 take the streamed sweep
CLASSES = (2, 63, 64, 65, 129, 300, 512, 513, 700)


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import estimator, lib

    assert lib.load() is not None
    return estimator


def _members(rng, Cn):
    """Four languages: the blank only, every class, the blank and the last class, a random half."""
    return [[0], list(range(Cn)), sorted({0, Cn - 1}), sorted(rng.choice(Cn, max(1, Cn // 2), replace=False).tolist())]


def _pool(rng, Cn, ids, members):
    """randn * 8; per utterance a +30 spike on a non-member in frame 0 (the members' mass is then about e^-30 of the row's),
    -inf on a tenth of the entries, and in the last utterance's frame 0 -inf on every member."""
    src = (rng.standard_normal((T, N, Cn)) * 8).astype(np.float32)
    src[rng.random((T, N, Cn)) < 0.1] = -np.inf
    for n, l in enumerate(ids):
        rest = np.setdiff1d(np.arange(Cn), members[l])
        if rest.size:
            src[0, n, rest[0]] = 30.0 + abs(float(rng.standard_normal()) * 8)
    src[0, N - 1, members[ids[N - 1]]] = -np.inf
    return src


def _restrict(src, lengths, ids, bits, n_lang, flags, out, status):
    """One amx_restrict_outputs call on device views `src` / `out` [T, N, C] with a unit class stride."""
    from allophant_amd import lib as L

    handle = L.load()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    code = handle.amx_restrict_outputs(
        src.device.index or 0, p(src), src.stride(0), src.stride(1), src.shape[2], p(lengths), p(ids), p(bits), n_lang,
        src.shape[1], src.shape[0], flags, p(out), out.stride(0), out.stride(1), p(status),
        C.c_void_p(torch.cuda.current_stream(src.device).cuda_stream))
    assert code == L.AMX_OK, handle.amx_last_error(None)


def _device_inputs(lengths, ids, members, Cn):
    return (torch.tensor(lengths, dtype=torch.int32).cuda(), torch.tensor(ids, dtype=torch.int32).cuda(),
            torch.from_numpy(U.member_bits(members, Cn).view(np.int64)).cuda())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("ids", [[2, 0, 1, 0, 2], [3, 1, 3, 2, 0]], ids=["issue", "half"])
@pytest.mark.parametrize("Cn", CLASSES)
def test_kernel_against_the_restatement(amd, Cn, ids):
    rng = np.random.default_rng(1000 + Cn)
    members = _members(rng, Cn)
    src = _pool(rng, Cn, ids, members)
    lengths_d, ids_d, bits_d = _device_inputs(LENGTHS, ids, members, Cn)
    src_d = torch.from_numpy(src).cuda()
    got = {}
    for flags in (0, U.NORMALIZE):
        out = torch.full((T, N, Cn), SENTINEL, dtype=torch.float32).cuda()
        status = torch.full((N,), -77, dtype=torch.int32).cuda()
        _restrict(src_d, lengths_d, ids_d, bits_d, len(members), flags, out, status)
        assert status.cpu().tolist() == [0] * N
        got[flags] = out.cpu().numpy()
    assert torch.equal(src_d.cpu(), torch.from_numpy(src))  # the source is only read
    want, _ = U.restrict(src, LENGTHS, ids, members, U.NORMALIZE)
    yard = U.yardstick(src, LENGTHS, ids, members)
    finite = np.isfinite(src)
    floor = float(np.spacing(np.abs(src[finite]).max()))  # one fp32 ulp of the largest finite |input|
    device_error = yard_error = 0.0
    for n, l in enumerate(ids):
        own = np.asarray(members[l])
        rest = np.setdiff1d(np.arange(Cn), own)
        valid = slice(0, LENGTHS[n])
        for flags in (0, U.NORMALIZE):
            assert np.all(got[flags][valid, n][:, rest] == -np.inf), (n, flags)  # non-members: exactly -inf
            assert np.all(_bits(got[flags][LENGTHS[n]:, n]) == 0), (n, flags)  # past the length: exactly +0.0
        assert np.array_equal(_bits(got[0][valid, n][:, own]), _bits(src[valid, n][:, own])), n  # raw members: the input's bits
        g, w, y = got[U.NORMALIZE][valid, n][:, own], want[valid, n][:, own], yard[valid, n][:, own]
        assert not np.isnan(g).any(), n
        assert np.array_equal(g == -np.inf, w == -np.inf), n
        real = np.isfinite(w)
        if real.any():
            device_error = max(device_error, float(np.abs(g[real] - w[real]).max()))
            yard_error = max(yard_error, float(np.abs(y[real].astype(np.float64) - w[real]).max()))
    assert np.all(got[U.NORMALIZE][0, N - 1] == -np.inf)  # the row whose members are all -inf
    bound = 4.0 * max(yard_error, floor)
    print(f"\nC = {Cn}: device error {device_error:.3e}, fp32 yardstick {yard_error:.3e}, floor {floor:.3e}, "
          f"ratio to max(yardstick, floor) {device_error / max(yard_error, floor):.3f}")
    assert device_error <= bound


@pytest.mark.parametrize("Cn", [129, 600])
def test_layouts_in_place_and_repeatable(amd, Cn):
    ids = [3, 1, 3, 2, 0]
    rng = np.random.default_rng(7 + Cn)
    members = _members(rng, Cn)
    src = torch.from_numpy(_pool(rng, Cn, ids, members))
    lengths_d, ids_d, bits_d = _device_inputs(LENGTHS, ids, members, Cn)
    status = torch.empty(N, dtype=torch.int32).cuda()
    size, before = T * N * Cn, 37
    for flags in (0, U.NORMALIZE):
        def flat_pair():
            a = torch.full((size + 101,), SENTINEL, dtype=torch.float32)
            a[before:before + size] = src.reshape(-1)
            return a.cuda(), torch.full((size + 101,), SENTINEL, dtype=torch.float32).cuda()

        def block(flat):
            return flat[before:before + size].view(T, N, Cn)

        def outside(flat):
            host = flat.cpu()
            return torch.cat([host[:before], host[before + size:]])

        # a [T, N, C] block inside a larger flat buffer, out of place
        a, b = flat_pair()
        _restrict(block(a), lengths_d, ids_d, bits_d, len(members), flags, block(b), status)
        first = block(b).cpu().numpy()
        assert (outside(a) == SENTINEL).all() and (outside(b) == SENTINEL).all()
        assert torch.equal(block(a).cpu(), src)
        # the same call again
        b.fill_(SENTINEL)
        _restrict(block(a), lengths_d, ids_d, bits_d, len(members), flags, block(b), status)
        assert np.array_equal(_bits(block(b).cpu().numpy()), _bits(first))
        # through the transposed view of [N, T, C] tensors
        src_nt = src.transpose(0, 1).contiguous().cuda()
        out_nt = torch.full((N, T, Cn), SENTINEL, dtype=torch.float32).cuda()
        _restrict(src_nt.transpose(0, 1), lengths_d, ids_d, bits_d, len(members), flags, out_nt.transpose(0, 1), status)
        assert np.array_equal(_bits(out_nt.transpose(0, 1).cpu().numpy()), _bits(first))
        # in place, inside the flat buffer
        _restrict(block(a), lengths_d, ids_d, bits_d, len(members), flags, block(a), status)
        assert np.array_equal(_bits(block(a).cpu().numpy()), _bits(first))
        assert (outside(a) == SENTINEL).all()
        want, _ = U.restrict(src.numpy(), LENGTHS, ids, members, flags)
        assert np.array_equal(np.isfinite(first), np.isfinite(want))


def test_malformed_rows_write_their_status_only(amd):
    Cn = 65
    rng = np.random.default_rng(3)
    members = _members(rng, Cn)[:3]
    ids = [-1, 0, 3, 1, 2]            # 3 == n_lang
    lengths = [7, 7, 7, T + 1, 3]
    src = (rng.standard_normal((T, N, Cn)) * 8).astype(np.float32)
    lengths_d, ids_d, bits_d = _device_inputs(lengths, ids, members, Cn)
    for flags in (0, U.NORMALIZE):
        out = torch.full((T, N, Cn), SENTINEL, dtype=torch.float32).cuda()
        status = torch.full((N,), -77, dtype=torch.int32).cuda()
        _restrict(torch.from_numpy(src).cuda(), lengths_d, ids_d, bits_d, 3, flags, out, status)
        assert status.cpu().tolist() == [-2, 0, -2, -2, 0]
        got = out.cpu().numpy()
        want, want_status = U.restrict(src, lengths, ids, members, flags, out=np.full(src.shape, SENTINEL))
        assert want_status.tolist() == [-2, 0, -2, -2, 0]
        for n in (0, 2, 3):
            assert (got[:, n] == np.float32(SENTINEL)).all(), n  # the output bytes are untouched
        for n in (1, 4):
            assert np.array_equal(np.isfinite(got[:, n]), np.isfinite(want[:, n]))
            real = np.isfinite(want[:, n])
            assert np.abs(got[:, n][real] - want[:, n][real]).max() < 1e-4
            assert (got[lengths[n]:, n] == 0.0).all()


def test_graph_capture(amd):
    """One call captured on a single stream and replayed twice equals the eager result bit for bit."""
    Cn, ids = 300, [3, 1, 3, 2, 0]
    rng = np.random.default_rng(19)
    members = _members(rng, Cn)
    src = torch.from_numpy(_pool(rng, Cn, ids, members)).cuda()
    lengths_d, ids_d, bits_d = _device_inputs(LENGTHS, ids, members, Cn)
    status = torch.empty(N, dtype=torch.int32).cuda()
    eager = torch.empty(T, N, Cn, dtype=torch.float32).cuda()
    _restrict(src, lengths_d, ids_d, bits_d, 4, U.NORMALIZE, eager, status)
    torch.cuda.synchronize()
    out = torch.full((T, N, Cn), SENTINEL, dtype=torch.float32).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _restrict(src, lengths_d, ids_d, bits_d, 4, U.NORMALIZE, out, status)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _restrict(src, lengths_d, ids_d, bits_d, 4, U.NORMALIZE, out, status)
    for _ in range(2):
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(eager.cpu().numpy()))


# -- through the estimator ------------------------------------------------------------------------------------------------
ASSIGNMENT_B = ("c", "c", "b", "a", "b", "a")


class _Model:
    def __init__(self, amd):
        self.e = U.EndToEnd()
        self.inv = self.e.inventories
        self.est = amd.Estimator(self.e.spec, self.e.state, "cuda:0", "f16x3")
        self.audio = self.e.audio.cuda()

    def batch(self, amd, languages=U.EndToEnd.LANGUAGES):
        return amd.Batch(self.audio, self.e.lengths, self.inv.language_ids(languages).to(torch.long))


@pytest.fixture(scope="module")
def model(amd):
    m = _Model(amd)
    yield m
    m.est.close()


def _against_the_oracle(model, pred, languages, log_probabilities=True):
    """The composed output at each utterance's columns against O.predict under the language's own matrix (below the gate),
    -inf elsewhere, 0 past the lengths; the other outputs within the gate; the lengths equal."""
    e, inv = model.e, model.inv
    block = pred.outputs["phoneme"].cpu()
    assert block.shape[2] == inv.classes
    worst = 0.0
    for n, language in enumerate(languages):
        own, frames = e.oracle(language, log_probabilities)
        assert torch.equal(pred.lengths.cpu(), frames)
        length = int(frames[n])
        columns = inv.columns(language)
        rest = np.setdiff1d(np.arange(inv.classes), columns.numpy())
        worst = max(worst, float((block[:length, n][:, columns] - own["phoneme"][:length, n]).abs().max()))
        assert (block[:length, n][:, rest] == -math.inf).all(), n
        assert (block[length:, n] == 0.0).all(), n
        for name in own:
            if name != "phoneme":
                assert float((pred.outputs[name].cpu()[:length, n] - own[name][:length, n]).abs().max()) < GATE, (name, n)
    print(f"\ncomposed output against the per-language oracle: {worst:.3e}")
    assert worst < GATE
    return worst


def _oracle_greedy(model, languages):
    """The per-language oracle's greedy collapse per utterance (upstream's per-language ids), and its smallest top-2 margin."""
    from oracle import allophant_oracle as O

    tokens, margin = [], math.inf
    for n, language in enumerate(languages):
        own, frames = model.e.oracle(language)
        em = own["phoneme"].transpose(0, 1)
        tokens.append(O.greedy_ctc(em, frames)[n][0].tolist())
        top = em[n, :int(frames[n])].topk(2, dim=-1).values
        margin = min(margin, float((top[:, 0] - top[:, 1]).min()))
    return tokens, margin


def test_predict_languages_against_the_oracle_per_language(amd, model):
    languages = U.EndToEnd.LANGUAGES
    pred = model.est.predict_languages(model.batch(amd), model.inv)
    assert pred._languages[0].cpu().tolist() == model.inv.language_ids(languages).tolist() and pred._languages[1] is model.inv
    assert torch.equal(pred._inventory, model.inv.union_tfi)
    _against_the_oracle(model, pred, languages)
    want, margin = _oracle_greedy(model, languages)
    print(f"smallest top-2 margin of the per-language oracle: {margin:.3e}")
    assert margin > 2 * GATE  # no frame is excused
    decoded = model.est.greedy_decode(pred)["phoneme"]
    for n, language in enumerate(languages):
        assert model.inv.to_language_indices(decoded[n][0].tokens, language).tolist() == want[n], n
    # the languages by name give the same bits
    named = model.est.predict_languages(amd.Batch(model.audio, model.e.lengths, torch.zeros(6, dtype=torch.long)), model.inv,
                                        languages=list(languages))
    assert torch.equal(named._flat.view(torch.int32), pred._flat.view(torch.int32))
    # the raw-logit form
    raw = model.est.predict_languages(model.batch(amd), model.inv, log_probabilities=False)
    _against_the_oracle(model, raw, languages, log_probabilities=False)


def test_refusals(amd, model):
    from allophant_amd import spec as S, synthetic

    with pytest.raises(ValueError):
        model.est.predict_languages(model.batch(amd), model.inv, languages=["a"] * 5)
    with pytest.raises(ValueError):
        model.est.predict_languages(model.batch(amd), model.inv, languages=["a", "b", "c", "c", "a", "nope"])
    with pytest.raises(IndexError):
        model.est.predict_languages(amd.Batch(model.audio, model.e.lengths, torch.full((6,), 3)), model.inv)
    spec = S.baseline_spec(S.tiny_encoder(2), 10)
    plain = amd.Estimator(spec, synthetic.make_state_dict(spec, seed=5), "cuda:0", "f16x3")
    try:
        with pytest.raises(ValueError, match="composition"):
            plain.predict_languages(model.batch(amd), model.inv)
    finally:
        plain.close()


@pytest.mark.parametrize("no_graph", [False, True], ids=["graph", "no_graph"])
def test_language_assignment_is_per_pass(amd, model, no_graph):
    """The same batch under assignment A, then B, then A: the two A results are bitwise equal, B meets its own oracle."""
    first = model.est.predict_languages(model.batch(amd), model.inv, _no_graph=no_graph)
    second = model.est.predict_languages(model.batch(amd, ASSIGNMENT_B), model.inv, _no_graph=no_graph)
    third = model.est.predict_languages(model.batch(amd), model.inv, _no_graph=no_graph)
    assert torch.equal(first._flat.view(torch.int32), third._flat.view(torch.int32))
    assert not torch.equal(first._flat.view(torch.int32), second._flat.view(torch.int32))
    _against_the_oracle(model, second, ASSIGNMENT_B)
    want, margin = _oracle_greedy(model, ASSIGNMENT_B)
    decoded = model.est.greedy_decode(second)["phoneme"]
    if margin > 2 * GATE:
        for n, language in enumerate(ASSIGNMENT_B):
            assert model.inv.to_language_indices(decoded[n][0].tokens, language).tolist() == want[n], n


@pytest.fixture(scope="module")
def decoded_case(amd, model):
    """predict_languages predictions, their composed block on the host, each utterance's compact [T_n, P_l + 1] slice and
    targets over its members in union ids: its own greedy tokens (at most 5), or its first phoneme where it has none."""
    languages = U.EndToEnd.LANGUAGES
    pred = model.est.predict_languages(model.batch(amd), model.inv)
    block = pred.outputs["phoneme"].cpu()
    frames = [int(v) for v in pred.lengths]
    compact = [block[:frames[n], n][:, model.inv.columns(l)].contiguous().numpy() for n, l in enumerate(languages)]
    greedy = model.est.greedy_decode(pred)["phoneme"]
    targets = []
    for n, language in enumerate(languages):
        tokens = greedy[n][0].tokens.tolist()[:5]
        targets.append(tokens or [int(model.inv.columns(language)[1])])
    return pred, frames, compact, targets


def _float_bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


def test_align_score_and_search_speak_union_indices(amd, model, decoded_case):
    import ctc_align_util as A
    import ctc_score_util as SC
    import ctc_search_util as SR

    languages, inv = U.EndToEnd.LANGUAGES, model.inv
    pred, frames, compact, targets = decoded_case
    own_targets = [inv.to_language_indices(row, l) for row, l in zip(targets, languages)]
    yard = SC.yardsticks(SC.make_pool(64))

    aligned = model.est.align(pred, {"phoneme": targets})["phoneme"]
    scored = model.est.score(pred, {"phoneme": targets})["phoneme"]
    feasible = 0
    for n, language in enumerate(languages):
        want = A.align_row(compact[n], own_targets[n], fast=True)
        assert (aligned[n] is None) == (want.status != 0), n
        if want.status == 0:
            feasible += 1
            got = aligned[n]
            assert inv.to_language_indices(got.tokens, language).tolist() == want.paths.tolist(), n
            assert np.array_equal(got.spans.numpy(), want.spans)
            assert np.array_equal(_float_bits(got.scores.numpy()), _float_bits(want.frame_scores))
            assert np.array_equal(_float_bits(got.span_scores.numpy()), _float_bits(want.span_scores))
            assert np.float32(got.total) == want.total
        truth = SC.score_row(compact[n], own_targets[n], posteriors=False)
        assert (scored[n] is None) == (truth.status != 0), n
        if truth.status == 0:
            assert abs(scored[n].log_likelihood - truth.ll) <= SC.ll_bound(yard, truth.ll), n
            assert (np.abs(scored[n].occupancy.numpy() - truth.occupancy)
                    <= SC.sum_bound(yard, truth.ll, frames[n], truth.occupancy)).all(), n
    assert feasible >= 4

    queries = [row[:2] for row in targets]
    found = model.est.search(pred, queries, "phoneme")
    hits = 0
    for n, language in enumerate(languages):
        members = set(inv.columns(language).tolist())
        for q, query in enumerate(queries):
            if not set(query) <= members:
                assert found[n][q] is None, (n, q)  # a class outside the utterance's language is -inf in every frame
                continue
            want = SR.search_row(compact[n], inv.to_language_indices(query, language), fast=True)
            hit = found[n][q]
            assert (hit is None) == (want.status != 0), (n, q)
            if hit is not None:
                hits += 1
                assert (hit.start, hit.end) == tuple(want.best_span), (n, q)
                assert _float_bits(hit.score) == _float_bits(want.best_score), (n, q)
    assert hits >= len(languages)


def test_beam_decode_per_language(amd, model, decoded_case):
    from ctc_beam_util import beam_search

    languages, inv = U.EndToEnd.LANGUAGES, model.inv
    pred, frames, compact, _ = decoded_case
    decoded = model.est.beam_decode_device(pred, beam_width=8, n_best=3)
    assert decoded.tokens.is_cuda and decoded.names == list(pred.outputs)
    hypotheses = decoded.hypotheses()
    for n, language in enumerate(languages):
        want = beam_search(compact[n], frames[n], 8, 3)
        got = hypotheses["phoneme"][n]
        assert len(got) == len(want), n
        for h, w in zip(got, want):
            # (to_language_indices raises on a token outside the language: no hypothesis holds one)
            assert inv.to_language_indices(h.tokens, language).tolist() == w.tokens, n
            assert h.timesteps.tolist() == w.timesteps, n
            assert abs(h.score - w.score) <= 1e-9 * max(1.0, abs(w.score)), n
    # the other outputs are decoded as ever
    plain = model.est.predict(model.batch(amd), inv.union_tfi)
    other = model.est.beam_decode_device(plain, 8, 3).hypotheses()
    for name in decoded.names:
        if name != "phoneme":
            for got, want in zip(hypotheses[name], other[name]):
                assert [(h.tokens.tolist(), h.timesteps.tolist(), h.score) for h in got] == \
                    [(h.tokens.tolist(), h.timesteps.tolist(), h.score) for h in want], name


def test_evaluator_with_the_union_inventory(amd, model, decoded_case):
    """EditStatistics per language from one predict_languages pass and the union inventory equal those of the per-language
    loop: the whole batch predicted under each language's own matrix, its utterances' rows scored under that inventory."""
    import edit_util as E
    from allophant_amd import evaluation as ev
    from allophant_amd.phonetic import AttributeTable

    languages, inv = U.EndToEnd.LANGUAGES, model.inv
    pred = decoded_case[0]
    table = AttributeTable(E.synthetic_table_text(), ["syllabic", "long", "nasal", "phoneme"])
    known = table.full_phonemes
    union_symbols = [known[u] if u < len(known) else f"x{u}" for u in range(inv.classes - 1)]
    rng = np.random.default_rng(4)
    labels = [[known[i] for i in rng.integers(0, len(known), rng.integers(3, 12))] for _ in languages]
    names = list(inv.languages)

    union = ev.Evaluator(table, ["phoneme"], union_symbols, names)
    union.add(model.est.greedy_decode_device(pred), labels, list(languages))
    got = union.statistics()

    for language in names:
        own = [n for n, l in enumerate(languages) if l == language]
        index = torch.tensor(own, device="cuda")
        symbols = [union_symbols[c - 1] for c in inv.columns(language).tolist()[1:]]
        loop = ev.Evaluator(table, ["phoneme"], symbols, names)
        decoded = model.est.greedy_decode_device(model.est.predict(model.batch(amd), inv.tfi(language)))
        part = amd.Decoded(decoded.names, decoded.tokens.index_select(1, index), decoded.timesteps.index_select(1, index),
                           decoded.counts.index_select(1, index), decoded.scores.index_select(1, index))
        loop.add(part, [labels[n] for n in own], [language] * len(own))
        assert loop.statistics()[language]["phoneme"] == got[language]["phoneme"], language
        assert sum(got[language]["phoneme"].astuple()) > 0

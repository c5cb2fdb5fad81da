"""Every stream-ordered entry point with the host running ahead of the GPU (method and stall: tests/run_ahead_util.py).

A busy-wait holds one non-default stream while the host enqueues a whole scenario behind it; the outputs are then compared, bit
for bit, with those of the same scenario run with a synchronisation after every step, and the number of steps that returned while
the stall still held (the run-ahead depth, printed with ``-s``) is held to what the documentation promises:

  A  the handle: the pinned ring of lengths / frame counts / row offsets / conv tile lists (``PIN_SLOTS``), the range-report ring
     (``RANGE_SLOTS``), workspace growth, cached inventories;
  B  the corpus loop: ``Prefetcher`` + ``PinnedCollator`` + the ``_out`` ring, with replays, and with one ordering edge dropped
     at a time (each dropped edge must show as wrong numbers);
  C  ``predict_long``;
  D  the stateless entry points that no graph-capture test covers, each reading inputs that only arrive in stream order.
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import run_ahead_util as R
from allophant_amd import spec as S, synthetic

pytestmark = pytest.mark.gpu

PIN_SLOTS, RANGE_SLOTS = 4, 8  # amx_handle_s (amx_api.hip): pinned length slots and range-report slots of a handle
PASSES = 12                    # more than either ring


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from allophant_amd import estimator, lib

    assert lib.load() is not None
    return estimator


@pytest.fixture(scope="module")
def side(amd):
    """The one non-default stream everything here runs on."""
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(stream):
        R.calibrate()
    torch.cuda.synchronize()
    return stream


# -- group A: the handle -----------------------------------------------------------------------------------------------
def _handle_spec():
    spec = S.multitask_spec(S.tiny_encoder(2), ["syllabic", "long"], embedding_size=16, train_phonemes=9, n_features=5, n_values=3,
                            allophone_layer=True)
    spec["shared_phones"] = 11
    return spec


def _new_estimator(amd, side, spec=None, state=None, seed=21):
    """An Estimator created on `side`: a handle belongs to one stream."""
    spec = spec or _handle_spec()
    with torch.cuda.stream(side):
        est = amd.Estimator(spec, state if state is not None else synthetic.make_state_dict(spec, seed=seed), "cuda:0", "f16x3")
    return spec, est


@pytest.fixture(scope="module")
def handle(amd, side):
    spec, est = _new_estimator(amd, side)
    yield spec, est
    est.close()


def _batch(amd, audio, lengths):
    return amd.Batch(audio.cuda(), lengths, torch.zeros(len(lengths), dtype=torch.long))


def _equal_batches(amd, count, n=4, length=12000, seed=100):
    return [_batch(amd, *synthetic.make_audio(n, length, seed=seed + k)) for k in range(count)]


def _predict_step(est, batch, tfi, log=None, out=None):
    """One `predict`: the flat output buffer, and on the host the frame lengths, the output names and their shapes."""
    def step():
        pred = est.predict(batch, tfi, _out=out)
        if log is not None:
            log.append(est.pass_info())
        return [pred._flat], (pred.lengths.tolist(), [(name, tuple(o.shape)) for name, o in pred.outputs.items()])
    return step


def _same(outcome):
    assert outcome.mismatches() == [], f"passes {outcome.mismatches()} differ from the synchronous run"
    assert outcome.host_got == outcome.host_expected


def test_a1_equal_geometry_runs_pin_slots_ahead(amd, side, handle):
    """12 passes of 4 x 12000 samples, different audio in each: the bits of the synchronous run, and at least PIN_SLOTS passes
    return while the stall holds ("no synchronisation is added to the hot path", include/allophant_amx.h; the fifth pass may wait
    for slot 0's event by design)."""
    spec, est = handle
    tfi = synthetic.make_inventory(spec, 7, seed=1)
    with torch.cuda.stream(side):
        steps = [_predict_step(est, b, tfi) for b in _equal_batches(amd, PASSES)]
    outcome = R.run_ahead(side, "A1 equal geometry", steps)
    _same(outcome)
    assert outcome.depth >= PIN_SLOTS, outcome.pending


def test_a2_ragged_batches_keep_their_own_pinned_slots(amd, side, handle):
    """4 utterances padded to 32000 samples with other lengths in every pass (well over a tenth of padding: packed rows and conv
    tile lists, pinned by `pass_info` in the synchronous run).  Every pass's pinned slot holds lengths, frame counts, row offsets
    and tile lists no other pass has, so a pass that read a later pass's slot has neither the right bits nor the right lengths."""
    spec, est = handle
    tfi = synthetic.make_inventory(spec, 7, seed=1)
    g = torch.Generator().manual_seed(77)
    batches = []
    for k in range(PASSES):
        audio, _ = synthetic.make_audio(4, 32000, seed=300 + k)
        lengths = torch.randint(6000, 26000, (4,), generator=g)
        lengths[k % 4] = 32000
        for n in range(4):
            audio[n, int(lengths[n]):] = 0
        batches.append((audio, lengths))
    assert len({tuple(l.tolist()) for _, l in batches}) == PASSES
    log = []
    with torch.cuda.stream(side):
        steps = [_predict_step(est, _batch(amd, a, l), tfi, log) for a, l in batches]
    outcome = R.run_ahead(side, "A2 ragged", steps)
    assert all(info["packed"] != 0 for info in log[:PASSES]), [info["packed"] for info in log]
    _same(outcome)
    assert len({tuple(host[0]) for host in outcome.host_got}) == PASSES  # (frame lengths: every pass its own)
    assert outcome.depth >= PIN_SLOTS, outcome.pending


def test_a3_workspace_growth_never_replays_a_stale_recording(amd, side):
    """Geometries 2 x 8000, 4 x 16000, 6 x 32000 three times each in ascending order, then in descending order, on a fresh handle
    (the synchronous run on another fresh one).  `ws_get` may synchronise where it grows, so the depth is only printed; the bits
    are those of the synchronous run, the passes take the same recorded / replayed forms, and a pass in which a buffer moved is
    never the replay of a recording made before."""
    spec = _handle_spec()
    tfi = synthetic.make_inventory(spec, 7, seed=1)
    geometries = [(2, 8000), (4, 16000), (6, 32000)]
    order = [g for g in geometries for _ in range(3)] + [g for g in reversed(geometries) for _ in range(3)]
    estimators = []

    def fresh():
        _, est = _new_estimator(amd, side)
        estimators.append(est)
        with torch.cuda.stream(side):
            est._select_inventory(tfi)
            batch = {g: _batch(amd, *synthetic.make_audio(*g, seed=500 + g[0])) for g in geometries}
            out = {g: torch.empty(est._output_layout(*g)[2], dtype=torch.float32, device="cuda") for g in geometries}

        def one(g):
            def step():
                before = est.device_bytes
                pred = est.predict(batch[g], tfi, _out=out[g])
                return [pred._flat], (pred.lengths.tolist(), est.pass_info()["graph"], est.device_bytes > before)
            return step
        return [one(g) for g in order]

    try:
        outcome = R.run_ahead(side, "A3 workspace growth", fresh(), fresh())
        _same(outcome)
        modes = [host[1] for host in outcome.host_got]
        assert 2 in modes and any(host[2] for host in outcome.host_got), outcome.host_got  # (replays and growth both occurred)
        assert not any(grew and mode == 2 for _, mode, grew in outcome.host_got), outcome.host_got
        assert estimators[1].graph_info()[1] == modes.count(2)  # (`graph_info` counts the replays the passes reported, no other)
    finally:
        for est in estimators:
            est.close()


def test_a4_cached_inventories_alternate(amd, side, handle):
    """Three inventories of 5, 13 and 8 phones, installed by the synchronous run, then selected in turn a, b, c, a, ... under the
    stall: every pass comes out under its own inventory (shapes and bits), and selecting a cached inventory does not
    synchronise, so the depth is that of A1."""
    spec, est = handle
    inventories = [synthetic.make_inventory(spec, phones, seed=40 + phones) for phones in (5, 13, 8)]
    with torch.cuda.stream(side):
        steps = [_predict_step(est, b, inventories[k % 3]) for k, b in enumerate(_equal_batches(amd, PASSES, seed=700))]
    outcome = R.run_ahead(side, "A4 cached inventories", steps)
    _same(outcome)
    for k, (_, shapes) in enumerate(outcome.host_got):
        assert dict(shapes)["phoneme"][2] == (5, 13, 8)[k % 3] + 1, (k, shapes)
    assert outcome.depth >= PIN_SLOTS, outcome.pending


A5_EXPONENT = 14.125  # FFN1 x 2^14.125: between the exponents at which the two batches of A5 start to overflow (see there)


def test_a5_range_report_names_its_pass_under_run_ahead(amd, side):
    """RANGE_SLOTS + 3 passes enqueued under the stall, of which the second alone leaves the range: exactly one report arrives
    (from a later `predict` or from the final `synchronize`; which one is printed), it names that pass and counts frames of that
    pass, and no other pass is blamed.  The same sequence runs first with `synchronize()` behind every pass: there the report
    arrives right behind the offending pass, and the loop's wall time sizes the stall.

    What this does NOT reach is the wrap-and-carry branch of `range_record` (a slot still unread RANGE_SLOTS passes later): a pass
    is only issued once the pass PIN_SLOTS before it has completed (its pinned slot's event), and every `amx_forward` reads the
    completed slots first, so with PIN_SLOTS = 4 < RANGE_SLOTS = 8 no more than five slots are ever unread, however far the host
    tries to run ahead.  Measured: the report arrives from the `predict` that issues the sixth pass.

    The checkpoint is the overflowing one of test_gpu_range.py::test_activation_overflow_is_refused_not_silent (its `_scale`
    recipe on FFN1 / FFN2), but at 2^14.125 where that test has 2^16: at 2^16 every batch overflows (a LayerNorm precedes the
    FFN; measured: noise, silence, a constant, one frame, x 100 all count every frame), and a handle has one checkpoint.  Measured
    in steps of 2^0.125: the 4 x 12000 batch below overflows from 2^13.875 on (all 148 frames at 2^14.125), the 2 x 6000 batch
    only from 2^14.375 on (0 frames at 2^14.25), so each side has at least 2^0.125 = 9 % of margin, a hundred times the rounding
    differences between kernels."""
    import time

    from test_gpu_range import _scale

    spec = S.multitask_spec(S.tiny_encoder(2), ["syllabic", "long"], embedding_size=16, train_phonemes=9, n_features=5)
    tfi = synthetic.make_inventory(spec, 7, seed=1)
    state = synthetic.make_state_dict(spec, seed=8)
    _scale(state, "feed_forward.intermediate_dense", A5_EXPONENT)
    _scale(state, "feed_forward.output_dense.weight", -A5_EXPONENT, biases=False)
    _, est = _new_estimator(amd, side, spec, state)
    try:
        passes = RANGE_SLOTS + 3

        def named_in(report):
            return [(int(a), int(b)) for a, b in re.findall(r"pass #(\d+): (\d+)", report)]

        with torch.cuda.stream(side):
            good, bad = _batch(amd, *synthetic.make_audio(2, 6000, seed=6)), _batch(amd, *synthetic.make_audio(4, 12000, seed=13))
            # synchronously: the report follows the offending pass at once
            started = time.perf_counter()
            for k in range(passes):
                est.predict(bad if k == 1 else good, tfi)
                number = est.pass_info()["id"]
                if k == 1:
                    with pytest.raises(FloatingPointError) as info:
                        est.synchronize()
                    assert [n for n, _ in named_in(str(info.value))] == [number]
                else:
                    est.synchronize()
            host_ms = (time.perf_counter() - started) * 1e3
            first = est.pass_info()["id"] + 1  # the number of the first pass below
            issued, frames, pending, reports, arrived = 0, {}, [], [], None
            with R.stalled(side, R.stall_for(host_ms)) as stall:
                while issued < passes:
                    try:
                        pred = est.predict(bad if issued == 1 else good, tfi)
                    except FloatingPointError as error:  # (a refused call has enqueued nothing: it is issued again)
                        reports.append(str(error))
                        arrived = f"the predict that issues pass {issued + 1} of {passes}"
                        continue
                    frames[est.pass_info()["id"]] = int(pred.lengths.sum())
                    issued += 1
                    pending.append(stall.pending())
            try:
                est.synchronize()
            except FloatingPointError as error:
                reports.append(str(error))
                arrived = "the final synchronize"
            est.synchronize()  # nothing is left to report
        print(f"run-ahead A5 range report: depth {R.depth_of(pending)} of {passes} steps (stall {R.stall_for(host_ms):.0f} ms, "
              f"synchronous loop {host_ms:.1f} ms); the report arrived from {arrived}")
        assert sorted(frames) == list(range(first, first + passes))
        assert len(reports) == 1, reports
        named = named_in(reports[0])
        assert len(named) == 1 and named[0][0] == first + 1, (named, first)
        # frames of that pass: more than any other pass has (so they are not another pass's), at most what it has itself
        assert frames[first] < named[0][1] <= frames[first + 1], (named, frames)
        assert R.depth_of(pending) >= PIN_SLOTS, pending
    finally:
        est.close()


# -- group B: the corpus loop ------------------------------------------------------------------------------------------
BUDGET, BUCKET = 32000, 16000
PATTERN = "AAABABBBABBBABBBBB"  # the order of the batches: geometry A = (2, 16000) six times, B = (1, 32000) twelve times


@pytest.fixture(scope="module")
def corpus_model(amd, side):
    spec = S.multitask_spec(S.tiny_encoder(2), ["syllabic", "long"], embedding_size=16, train_phonemes=9, n_features=5)
    _, est = _new_estimator(amd, side, spec, synthetic.make_state_dict(spec, seed=9))
    yield est, synthetic.make_inventory(spec, 7, seed=9)
    est.close()


def _corpus():
    """24 utterances, 12 just below 1 s and 12 just below 2 s (less than a tenth of a bucketed batch is padding, so its
    recording is keyed on the geometry and later batches of the geometry replay it), and their batches in PATTERN order."""
    from allophant_amd import batching

    g = torch.Generator().manual_seed(5)
    sizes = torch.cat([torch.randint(15200, 16001, (12,), generator=g), torch.randint(30400, 32001, (12,), generator=g)]).tolist()
    corpus = [torch.randn(n, generator=g) * 0.1 for n in sizes]
    assert len(corpus) == 24 and all(2000 <= n <= 40000 for n in sizes)
    batches = list(batching.bucketed_frame_batches(batching.length_sorted_order(sizes), sizes, BUDGET, BUCKET))
    by_geometry = {"A": [b for b in batches if (len(b[0]), b[1]) == (2, 16000)], "B": [b for b in batches if (len(b[0]), b[1]) == (1, 32000)]}
    assert len(by_geometry["A"]) == 6 and len(by_geometry["B"]) == 12 and len(batches) == 18
    ordered = [by_geometry[letter].pop(0) for letter in PATTERN]
    return corpus, ordered


def _plain_steps(amd, est, tfi, corpus, batches):
    """The plain loop: collate, copy, predict."""
    def one(indices, padded_length):
        def step():
            audio = torch.zeros(len(indices), padded_length)
            for i, index in enumerate(indices):
                audio[i, : corpus[index].numel()] = corpus[index]
            batch = amd.Batch(audio.cuda(), torch.tensor([corpus[i].numel() for i in indices]), torch.zeros(len(indices), dtype=torch.long))
            batch._padded = True
            pred = est.predict(batch, tfi)
            return [pred._flat], pred.lengths.tolist()
        return step
    return [one(*b) for b in batches]


class _Unwaited:
    def synchronize(self):
        pass


def _loop_steps(est, tfi, corpus, batches, ring, modes, drop=None):
    """The loop of tools/corpus_throughput.py::run_bucketed, one step per batch: PinnedCollator(depth=2), Prefetcher(ring=ring),
    the first batch of a shape sizes a two-buffer `_out` ring and later batches of the shape write into it in turn.  `drop`
    removes one ordering edge: "wait_event" (the copy stream no longer waits for the forward pass that read the device slot) or
    "collator" (the pinned slot is refilled without waiting for the copy out of it)."""
    from allophant_amd import batching

    class Collator(batching.PinnedCollator):
        def mark_in_flight(self, batch, event):
            super().mark_in_flight(batch, _Unwaited() if drop == "collator" else event)

    class CopyStream(torch.cuda.Stream):
        def wait_event(self, event):
            if drop != "wait_event":
                super().wait_event(event)

    device = torch.device("cuda:0")
    collator = Collator(BUDGET, depth=2)
    prefetcher = batching.Prefetcher(batches, device, lambda item: collator([corpus[i] for i in item[0]], padded_length=item[1]), ring=ring)
    prefetcher._stream = CopyStream(device)
    out_ring, out_turn = {}, {}

    def step():
        batch = next(prefetcher)
        shape = tuple(batch.audio_features.shape)
        if shape not in out_ring:
            pred = est.predict(batch, tfi)
            out_ring[shape] = [torch.empty(pred._flat.numel(), dtype=torch.float32, device=device) for _ in range(2)]
        else:
            turn = out_turn.get(shape, 0)
            out_turn[shape] = turn ^ 1
            pred = est.predict(batch, tfi, _out=out_ring[shape][turn])
        modes.append(est.pass_info()["graph"])
        return [pred._flat], pred.lengths.tolist()
    return [step] * len(batches)


@pytest.mark.parametrize("ring", [2, 1, 0])
def test_b_corpus_loop_matches_the_plain_loop(amd, side, corpus_model, ring):
    """Every pass of the prefetched loop under the stall equals the plain synchronous loop's, the host gets at least two batches
    ahead (what `Prefetcher(ring=2)`'s docstring rests on), and with reused buffers (ring > 0) passes are replayed from a
    recording -- a loop that fell back to eager passes fails here.  (ring = 0 takes fresh device buffers from the allocator:
    a recording holds addresses, so it promises no replay.)"""
    est, tfi = corpus_model
    corpus, batches = _corpus()
    modes = []
    with torch.cuda.stream(side):
        plain, loop = _plain_steps(amd, est, tfi, corpus, batches), _loop_steps(est, tfi, corpus, batches, ring, modes)
    outcome = R.run_ahead(side, f"B corpus loop ring={ring}", plain, loop)
    _same(outcome)
    if ring > 0:
        assert 2 in modes, modes
    assert outcome.depth >= 2, outcome.pending


@pytest.mark.parametrize("drop", ["wait_event", "collator"])
def test_b_a_dropped_ordering_edge_shows(amd, side, corpus_model, drop):
    """Separation: the ring = 2 loop with one ordering edge removed produces wrong numbers under the stall (all buffers stay
    allocated and every access in bounds: the only effect is a pass that read another batch's audio)."""
    est, tfi = corpus_model
    corpus, batches = _corpus()
    with torch.cuda.stream(side):
        plain, loop = _plain_steps(amd, est, tfi, corpus, batches), _loop_steps(est, tfi, corpus, batches, 2, [], drop)
    outcome = R.run_ahead(side, f"B corpus loop ring=2 without {drop}", plain, loop)
    print(f"run-ahead B without {drop}: passes {outcome.mismatches()} differ")
    assert len(outcome.mismatches()) >= 1


# -- group C: predict_long ---------------------------------------------------------------------------------------------
def test_c_predict_long_under_a_stall(amd, side):
    """One recording of 32 windows and one of 5 (ten slices at batch_windows=4) in one `predict_long` call under the stall: the
    stitched outputs and lengths of the un-stalled call, bit for bit.  Each slice is a forward pass and takes one of the handle's
    PIN_SLOTS pinned slots, so such a call waits for its first slices (its docstring says so); a call of exactly PIN_SLOTS
    slices, on a handle whose earlier passes have completed, only launches, and must return with the stall pending."""
    import longform_util as U
    from test_gpu_longform import KERNELS, STRIDES, _recordings, _tiny_spec

    spec = _tiny_spec()
    _, est = _new_estimator(amd, side, spec, synthetic.make_state_dict(spec, seed=3))
    tfi = synthetic.make_inventory(spec, 7, seed=2)
    arguments = dict(window_seconds=0.25, context_seconds=0.05, batch_windows=4)
    try:
        def call(lengths, seed):
            audio, lengths = _recordings(lengths, seed)
            with torch.cuda.stream(side):
                batch = _batch(amd, audio, lengths)

            def step():
                long = est.predict_long(batch, tfi, **arguments)
                return [long._flat], long.lengths.tolist()
            return step

        many = call([U.length_for(12 + 31 * 8, KERNELS, STRIDES), 13200], 43)
        few = call([13200, 13200, 13200, 4000], 44)  # 5 + 5 + 5 + 1 windows: four slices, one per pinned slot
        with torch.cuda.stream(side):
            many(), few()  # warm-up: the workspace, the pinned ring and the recordings of the slices
        outcome = R.run_ahead(side, "C predict_long, 10 slices", [many])
        _same(outcome)
        assert outcome.host_got[0] == [260, 41]
        outcome = R.run_ahead(side, "C predict_long, 4 slices", [few])
        _same(outcome)
        assert outcome.depth == 1, "predict_long of PIN_SLOTS slices waited for the device"
    finally:
        est.close()


# -- group D: stateless entry points no graph-capture test covers ------------------------------------------------------
def _sentinel(t):
    if t.is_floating_point():
        return torch.full_like(t, float("nan"))
    return torch.full_like(t, 255 if t.dtype == torch.uint8 else -1)


def _stream_pointer():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stateless(side, label, real, make_outputs, call):
    """`call(inputs, outputs)` makes the entry point's call on the current stream and returns its code; `real` are ALL its device
    inputs, `make_outputs()` fresh initialised outputs.  The plain call on the default stream gives the expectation.  Then every
    input buffer of a second call holds a sentinel (NaN, -1) until device-to-device copies, enqueued on `side` behind the
    busy-wait, bring the real inputs: the call must return AMX_OK with the stall still pending, and its outputs must be the
    plain call's, bit for bit -- a read on the host, on the null stream or ahead of the stream sees sentinels."""
    want = make_outputs()
    assert call(real, want) == 0
    torch.cuda.synchronize()
    inputs = {name: _sentinel(t) for name, t in real.items()}
    got = make_outputs()
    torch.cuda.synchronize()
    with torch.cuda.stream(side), R.stalled(side) as stall:
        for name, t in real.items():
            inputs[name].copy_(t)
        code = call(inputs, got)
        pending = stall.pending()
    print(f"run-ahead D {label}: depth {int(pending)} of 1 step")
    assert code == 0, (label, code)
    assert pending, f"{label} waited for the device"
    return want, got


def _assert_bitwise(want, got):
    assert list(want) == list(got)
    for name in want:
        assert torch.equal(R._words(want[name]), R._words(got[name])), name


def _emissions():
    """3 rows, T = 40, C = 9: log-probabilities and frame lengths (a full row, a partial one, a short one)."""
    g = torch.Generator().manual_seed(11)
    return {"emissions": torch.randn(3, 40, 9, generator=g).log_softmax(-1).cuda(),
            "lengths": torch.tensor([40, 25, 7], dtype=torch.int32).cuda()}


def test_d_greedy_ctc_emissions(amd, side):
    from allophant_amd import lib as L

    lib = L.load()
    outputs = lambda: {"tokens": torch.zeros(3, 40, dtype=torch.int64, device="cuda"), "timesteps": torch.zeros(3, 40, dtype=torch.int64, device="cuda"),  # noqa: E731
                       "counts": torch.full((3,), -7, dtype=torch.int32, device="cuda"), "scores": torch.zeros(3, device="cuda")}

    def call(i, o):
        return lib.amx_greedy_ctc_emissions(0, _ptr(i["emissions"]), 40 * 9, 9, _ptr(i["lengths"]), 3, 40, 9, 0, _ptr(o["tokens"]),
                                            _ptr(o["timesteps"]), _ptr(o["counts"]), _ptr(o["scores"]), _stream_pointer())
    want, got = _stateless(side, "amx_greedy_ctc_emissions", _emissions(), outputs, call)
    _assert_bitwise(want, got)
    assert want["counts"].tolist() != [-7] * 3 and int(want["counts"].max()) > 0


@pytest.mark.parametrize("fused", [False, True], ids=["amx_beam_ctc_emissions", "amx_beam_ctc_lm_emissions"])
def test_d_beam_ctc_emissions(amd, side, fused):
    from allophant_amd import lib as L

    lib = L.load()
    beam, n_best, size = 4, 2, C.c_size_t()
    assert (lib.amx_beam_ctc_lm_workspace if fused else lib.amx_beam_ctc_workspace)(beam, 3, 40, C.byref(size)) == 0
    real = _emissions()
    if fused:
        g = torch.Generator().manual_seed(12)
        real["lm"] = torch.randn(2, 10, 10, generator=g).log_softmax(-1).cuda()
        real["lm_index"] = torch.tensor([1, -1, 0], dtype=torch.int32).cuda()
    outputs = lambda: {"tokens": torch.zeros(3, n_best, 40, dtype=torch.int64, device="cuda"),  # noqa: E731
                       "timesteps": torch.zeros(3, n_best, 40, dtype=torch.int64, device="cuda"),
                       "counts": torch.full((3, n_best), -7, dtype=torch.int32, device="cuda"),
                       "scores": torch.zeros(3, n_best, dtype=torch.float64, device="cuda"),
                       "hyp_counts": torch.full((3,), -7, dtype=torch.int32, device="cuda"),
                       "workspace": torch.zeros(max(1, size.value), dtype=torch.uint8, device="cuda")}

    def call(i, o):
        head = (0, _ptr(i["emissions"]), 40 * 9, 9, _ptr(i["lengths"]), 3, 40, 9, 0, beam, n_best, 0)
        tail = (_ptr(o["workspace"]), size.value, _ptr(o["tokens"]), _ptr(o["timesteps"]), _ptr(o["counts"]), _ptr(o["scores"]),
                _ptr(o["hyp_counts"]), _stream_pointer())
        if fused:
            return lib.amx_beam_ctc_lm_emissions(*head, _ptr(i["lm"]), 2, _ptr(i["lm_index"]), 0.7, -0.1, *tail)
        return lib.amx_beam_ctc_emissions(*head, *tail)
    want, got = _stateless(side, "amx_beam_ctc_lm_emissions" if fused else "amx_beam_ctc_emissions", real, outputs, call)
    want.pop("workspace"), got.pop("workspace")
    _assert_bitwise(want, got)
    assert want["hyp_counts"].tolist() == [n_best] * 3


def test_d_map_allophones(amd, side):
    from test_gpu_allophones import _mapping, _tiny

    from test_allophone_mapping import G17

    g17 = np.load(G17)
    spec, state = _tiny(g17)
    _, est = _new_estimator(amd, side, spec, state)
    try:
        est.set_allophones(_mapping(g17))
        n_lang = est._allophone_shape[0]
        real = {"x": torch.from_numpy(g17["inputs"]).cuda(),
                "ids": torch.tensor([int(v) % n_lang for v in g17["ids"].tolist()], dtype=torch.int32).cuda()}
        T, N, _ = real["x"].shape
        outputs = lambda: {"out": torch.zeros(T, N, est._allophone_shape[2], device="cuda")}  # noqa: E731

        def call(i, o):
            return est._lib.amx_map_allophones(est._handle, _ptr(i["x"]), i["x"].stride(0), i["x"].stride(1), _ptr(i["ids"]), N, T,
                                               _ptr(o["out"]), _stream_pointer())
        want, got = _stateless(side, "amx_map_allophones", real, outputs, call)
        _assert_bitwise(want, got)
        torch.testing.assert_close(want["out"].cpu(), torch.from_numpy(g17["outputs"]), rtol=0, atol=0, equal_nan=True)
    finally:
        est.close()


def _sorted_table(table):
    """A confusion table's occupied slots by key: slot positions depend on the order of arrival, the (key, count) set does not."""
    host = table.cpu()
    host = host[host[:, 0] != 0]
    return host[host[:, 0].argsort()]


def _confusion_case(ev):
    from test_gpu_edit_workspace import ALPHABET, BEST, COSTS, TABLE, _rows, _sequences

    expected, candidates = _sequences(np.random.default_rng(16017), 16, 17)
    rows = _rows(ev, expected, candidates, 16, 17)
    device = rows.tokens.device
    weighting = ev.PropertyWeighting(*COSTS, TABLE)
    weights = ev._Weights(weighting.insertion_cost, weighting.deletion_cost, torch.tensor([[0, ALPHABET]], dtype=torch.int64, device=device),
                          weighting.cost_table(list(range(ALPHABET)), device))
    return rows, torch.tensor([BEST], dtype=torch.int32, device=device), weights, ALPHABET


@pytest.mark.parametrize("weighted", [False, True], ids=["amx_edit_confusions", "amx_edit_weighted_confusions"])
def test_d_edit_confusions(amd, side, weighted):
    from allophant_amd import evaluation as ev
    from allophant_amd.confusion import ConfusionCounts

    rows, best, weights, alphabet = _confusion_case(ev)
    real = {"tokens": rows.tokens, "counts": rows.counts, "labels": rows.labels, "maps": rows.maps, "label_maps": rows.label_maps,
            "hyp_maps": rows.hyp_maps.clone(), "best": best}
    if weighted:
        real.update(descriptors=weights.descriptors, data=weights.data)
    workspace = rows.workspace(True)
    accumulators = []

    def outputs():
        accumulators.append(ConfusionCounts(rows.tokens.device, 4096, ["total"], ["pairs"], [list(range(alphabet))]))
        accumulators[-1]._workspace = torch.empty_like(workspace)
        return {"accumulator": len(accumulators) - 1}

    def call(i, o):
        these = rows._replace(tokens=i["tokens"], counts=i["counts"], labels=i["labels"], maps=i["maps"], label_maps=i["label_maps"],
                              hyp_maps=i["hyp_maps"])
        w = ev._Weights(weights.insertion_cost, weights.deletion_cost, i["descriptors"], i["data"]) if weighted else None
        o["row_events"] = accumulators[o["accumulator"]].add_rows(these, i["best"], w)  # (raises unless the call returned AMX_OK)
        return 0
    want, got = _stateless(side, "amx_edit_weighted_confusions" if weighted else "amx_edit_confusions", real, outputs, call)
    a, b = accumulators[want["accumulator"]], accumulators[got["accumulator"]]
    assert torch.equal(want["row_events"], got["row_events"]) and int(want["row_events"].min()) > 0
    assert torch.equal(a.counters, b.counters) and int(a.counters[0]) == int(want["row_events"].sum())
    assert torch.equal(_sorted_table(a.table), _sorted_table(b.table))


def test_d_edit_confusion_merge(amd, side):
    from allophant_amd import evaluation as ev
    from allophant_amd.confusion import ConfusionCounts

    rows, best, _, alphabet = _confusion_case(ev)
    source = ConfusionCounts(rows.tokens.device, 4096, ["total"], ["pairs"], [list(range(alphabet))])
    source.add_rows(rows, best)
    torch.cuda.synchronize()
    accumulators = []

    def outputs():
        accumulators.append(ConfusionCounts(rows.tokens.device, 8192, ["total"], ["pairs"], [list(range(alphabet))]))
        return {"accumulator": len(accumulators) - 1}

    def call(i, o):
        accumulators[o["accumulator"]]._merge_from(i["table"])  # (raises unless the call returned AMX_OK)
        return 0
    want, got = _stateless(side, "amx_edit_confusion_merge", {"table": source.table}, outputs, call)
    a, b = accumulators[want["accumulator"]], accumulators[got["accumulator"]]
    assert torch.equal(a.counters, b.counters) and torch.equal(a.counters, source.counters) and int(a.counters[0]) > 0
    assert torch.equal(_sorted_table(a.table), _sorted_table(b.table)) and torch.equal(_sorted_table(a.table), _sorted_table(source.table))


def test_d_edit_cost_table(amd, side):
    from allophant_amd import lib as L
    from test_gpu_edit_workspace import TABLE

    lib = L.load()
    codes = np.asarray([TABLE[symbol] for symbol in sorted(TABLE)], dtype=np.uint8)  # [V, F] feature codes
    V, F = codes.shape
    outputs = lambda: {"table": torch.full((V, V), 0xA5, dtype=torch.uint8, device="cuda")}  # noqa: E731

    def call(i, o):
        return lib.amx_edit_cost_table(0, _ptr(i["codes"]), V, F, _ptr(o["table"]), _stream_pointer())
    want, got = _stateless(side, "amx_edit_cost_table", {"codes": torch.from_numpy(codes).cuda()}, outputs, call)
    _assert_bitwise(want, got)
    differing = (codes[:, None, :] != codes[None, :, :]).sum(-1).astype(np.uint8)  # the contract: differing feature columns
    assert np.array_equal(want["table"].cpu().numpy(), differing) and differing.max() > 0


def test_d_edit_matrix(amd, side):
    """The small case of test_gpu_edit_weighted.py: three pairs over a table of two symbols, the third with an id outside it."""
    from allophant_amd import lib as L

    lib = L.load()
    i32 = lambda values: torch.tensor(values, dtype=torch.int32, device="cuda")  # noqa: E731
    real = {"expected_offsets": i32([0, 2, 5, 6]), "expected_ids": i32([0, 1, 0, 1, 1, 5]), "actual_offsets": i32([0, 3, 4, 4]),
            "actual_ids": i32([1, 0, 0, 1]), "table": torch.tensor([0, 1, 1, 0], dtype=torch.uint8, device="cuda")}
    size = C.c_size_t()
    assert lib.amx_edit_workspace(3, 3, 3, C.byref(size)) == 0
    outputs = lambda: {"matrix": torch.full((3, 4, 4), -5.5, device="cuda"), "status": torch.full((3,), -77, dtype=torch.int32, device="cuda"),  # noqa: E731
                       "workspace": torch.zeros(size.value, dtype=torch.uint8, device="cuda")}

    def call(i, o):
        return lib.amx_edit_matrix(0, _ptr(i["expected_offsets"]), _ptr(i["expected_ids"]), _ptr(i["actual_offsets"]), _ptr(i["actual_ids"]),
                                   3, 3, 3, 0.3, 0.7, _ptr(i["table"]), 2, _ptr(o["workspace"]), size.value, _ptr(o["matrix"]),
                                   _ptr(o["status"]), _stream_pointer())
    want, got = _stateless(side, "amx_edit_matrix", real, outputs, call)
    want.pop("workspace"), got.pop("workspace")
    _assert_bitwise(want, got)
    assert want["status"].tolist() == [0, 0, -2]
    first = want["matrix"][0].cpu()
    assert first[0].tolist() == [0.0, 1.0, 2.0, 3.0] and bool((first[3] == -5.5).all()) and bool((want["matrix"][2] == -5.5).all())


def _long_case():
    import longform_util as U
    from test_gpu_longform import CONTEXT, KERNELS, STRIDES, WINDOW

    lengths = [13200, 3000]
    windows, frames = U.plan(lengths, WINDOW, CONTEXT, KERNELS, STRIDES)
    assert frames.tolist() == [41, 9] and len(windows) == 6
    return lengths, windows, U


def test_d_long_gather(amd, side):
    from allophant_amd import longform
    from test_gpu_longform import HOP, WINDOW

    lengths, windows, U = _long_case()
    host = np.random.default_rng(3).standard_normal((2, 13200)).astype(np.float32)
    real = {"audio": torch.from_numpy(host).cuda(), "lengths": torch.tensor(lengths, dtype=torch.int64).cuda(),
            "windows": torch.from_numpy(np.ascontiguousarray(windows)).cuda()}
    outputs = lambda: {"batch": torch.full((6, WINDOW), -5.5, device="cuda"), "status": torch.full((6,), -77, dtype=torch.int32, device="cuda")}  # noqa: E731

    def call(i, o):
        longform.gather_windows(i["audio"], i["lengths"], i["windows"], HOP, o["batch"], o["status"])  # (raises unless AMX_OK)
        return 0
    want, got = _stateless(side, "amx_long_gather", real, outputs, call)
    _assert_bitwise(want, got)
    reference, status = U.gather(host, lengths, windows, HOP, WINDOW)
    assert np.array_equal(want["batch"].cpu().numpy().view(np.int32), reference.view(np.int32)) and want["status"].tolist() == status.tolist()


def test_d_long_stitch(amd, side):
    from allophant_amd import longform

    _, windows, _ = _long_case()
    src_T, n, classes, R_, dst_T = 12, 6, 5, 2, 41
    g = torch.Generator().manual_seed(4)
    real = {"src": torch.randn(src_T * n * classes, generator=g).cuda(), "windows": torch.from_numpy(np.ascontiguousarray(windows)).cuda()}
    outputs = lambda: {"dst": torch.full((dst_T * R_ * classes,), -5.5, device="cuda"), "status": torch.full((n,), -77, dtype=torch.int32, device="cuda")}  # noqa: E731

    def call(i, o):
        longform.stitch_windows(i["src"], src_T, i["windows"], [(0, 0, classes)], o["dst"], R_, dst_T, o["status"])  # (raises unless AMX_OK)
        return 0
    want, got = _stateless(side, "amx_long_stitch", real, outputs, call)
    _assert_bitwise(want, got)
    assert want["status"].tolist() == [0] * n
    written = want["dst"].view(dst_T, R_, classes) != -5.5
    assert bool(written[:, 0].all()) and bool(written[:9, 1].all()) and not bool(written[9:, 1].any())

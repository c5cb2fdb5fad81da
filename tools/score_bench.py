"""Times the on-device CTC forward-backward scoring (amx_ctc_score.hip) and sets no threshold:

  * every output of the benchmark's config 2 -- 32 x 10 s utterances, each (output, utterance) row scored against its own
    greedy tokens -- through ``Estimator.score_device`` (with its allocations and target upload) and through
    ``amx_ctc_score`` on prepared buffers, with and without ``posteriors``, beside ``amx_ctc_align`` on the same rows and
    buffers of its own;
  * one 60 s row with 600 targets through ``amx_ctc_score_emissions`` and ``amx_ctc_align_emissions`` on prepared buffers;
  * ``Estimator.rescore_device`` of beam 16 / n_best 4 on the config-2 outputs;
  * ``torch.nn.functional.ctc_loss`` (fp32, forward only) on the host CPU for the same config-2 rows and the long row, the
    outputs already on the host.

Prints one JSON line per measurement.  The device times are HIP events around whole calls; ``amx_ctc_score`` and
``amx_ctc_align`` include the frame-length upload and its host synchronisation.

    python tools/score_bench.py [--utterances 32] [--seconds 10] [--iters 5]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from allophant_amd import alignment, lib as L, scoring, synthetic  # noqa: E402
from allophant_amd.estimator import Batch, Estimator  # noqa: E402
from bench import build_spec  # noqa: E402


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--phones", type=int, default=27)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    lib = L.load()
    device = torch.device("cuda:0")
    spec = build_spec(phones=args.phones)
    est = Estimator(spec, synthetic.make_state_dict(spec, seed=0), "cuda:0")
    tfi = synthetic.make_inventory(spec, args.phones, seed=0)
    audio, lengths = synthetic.make_audio(args.utterances, int(args.seconds * 16000), seed=1234)
    batch = Batch(audio.cuda(), lengths, torch.zeros(args.utterances, dtype=torch.long))
    pred = est.predict(batch, tfi)
    names = list(pred.outputs)
    T, N = next(iter(pred.outputs.values())).shape[:2]
    O = len(names)
    decoded = est.greedy_decode_device(pred)
    tokens, counts = decoded.tokens.cpu(), decoded.counts.cpu()
    targets = {name: [tokens[o, n, :int(counts[o, n])].tolist() for n in range(N)] for o, name in enumerate(names)}
    flat_rows = [row for name in names for row in targets[name]]
    max_target = max(len(row) for row in flat_rows)
    print(json.dumps({"case": "config2", "utterances": N, "frames": T, "outputs": O, "rows": O * N, "max_target": max_target,
                      "mean_target": round(float(np.mean([len(row) for row in flat_rows])), 1)}))

    scored = est.score_device(pred, targets)
    status = scored.status.cpu()
    facade_ms = timed(lambda: est.score_device(pred, targets), args.iters)
    offsets, ids, _ = scoring.pack_targets(flat_rows)
    meta = torch.cat([offsets, ids, torch.zeros(1, dtype=torch.int32)]).cuda()
    frame_lengths = pred.lengths.detach().to("cpu", torch.int64).contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    out_ptr, fl_ptr = C.c_void_p(pred._flat.data_ptr()), C.cast(frame_lengths.data_ptr(), C.POINTER(C.c_int64))
    offsets_ptr, ids_ptr = C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 4 * (O * N + 1))

    def score_call(b):
        def call():
            code = lib.amx_ctc_score(est._handle, out_ptr, fl_ptr, N, pred._geometry[1], 1, offsets_ptr, ids_ptr, max_target,
                                     *b.pointers(), C.c_void_p(stream))
            assert code == L.AMX_OK, lib.amx_last_error(est._handle)
        return call

    plain = scoring.allocate(lib, O * N, T, max_target, device)
    score_ms = timed(score_call(plain), args.iters)
    assert torch.equal(plain.log_likelihood.view(O, N, 1), scored.log_likelihood)
    workspace_mb = plain.size / 2 ** 20
    del plain
    full = scoring.allocate(lib, O * N, T, max_target, device, posteriors=True)
    posteriors_ms = timed(score_call(full), args.iters)
    posteriors_mb = full.posteriors.numel() * 4 / 2 ** 20
    del full

    ab = alignment.allocate(lib, O * N, T, max_target, device)

    def align_call():
        code = lib.amx_ctc_align(est._handle, out_ptr, fl_ptr, N, pred._geometry[1], offsets_ptr, ids_ptr, max_target, *ab.pointers(),
                                 C.c_void_p(stream))
        assert code == L.AMX_OK, lib.amx_last_error(est._handle)

    align_ms = timed(align_call, args.iters)
    above = bool((scored.log_likelihood.view(O, N)[status.view(O, N) == 0]
                  >= ab.totals.view(O, N)[status.view(O, N) == 0] - 1e-3).all())  # the sum over paths holds the best path
    del ab
    print(json.dumps({"case": "config2_all_outputs", "rows": O * N, "frames": T, "scored_rows": int((status == 0).sum()),
                      "workspace_mb": round(workspace_mb, 1), "posteriors_mb": round(posteriors_mb, 1),
                      "score_device_ms": round(facade_ms, 3), "amx_ctc_score_ms": round(score_ms, 3),
                      "amx_ctc_score_with_posteriors_ms": round(posteriors_ms, 3), "amx_ctc_align_ms": round(align_ms, 3),
                      "ll_at_least_best_path": above}))

    # exact rescoring of an n-best list
    beam = est.beam_decode_device(pred, 16, 4)
    beam_ms = timed(lambda: est.beam_decode_device(pred, 16, 4), args.iters)
    rescored = est.rescore_device(pred, beam)
    rescore_ms = timed(lambda: est.rescore_device(pred, beam), args.iters)
    present = torch.isfinite(rescored.log_likelihood)
    print(json.dumps({"case": "rescore_beam16_nbest4", "rows": O * N * 4, "hypotheses": int(beam.hyp_counts.sum()),
                      "with_a_path": int(present.sum()), "beam16_decode_ms": round(beam_ms, 3), "rescore_device_ms": round(rescore_ms, 3)}))

    # torch's CPU ctc_loss on the same rows (the outputs are copied to the host first, which is not timed)
    host = {name: pred.outputs[name].cpu() for name in names}
    frames = torch.tensor([int(v) for v in frame_lengths])
    cpu_ms, worst = 0.0, 0.0
    F.ctc_loss(host[names[0]][:8], torch.ones(N, 1, dtype=torch.long), torch.full((N,), 8), torch.ones(N, dtype=torch.long))  # warm-up
    for o, name in enumerate(names):
        width = max(1, max(len(row) for row in targets[name]))
        padded = torch.tensor([row + [0] * (width - len(row)) for row in targets[name]], dtype=torch.long)
        sizes = torch.tensor([len(row) for row in targets[name]])
        t0 = time.perf_counter()
        loss = F.ctc_loss(host[name], padded, frames, sizes, blank=0, reduction="none", zero_infinity=False)
        cpu_ms += (time.perf_counter() - t0) * 1e3
        ll = scored.log_likelihood[o, :, 0].cpu()
        ok = status[o, :, 0] == 0
        worst = max(worst, float(((-loss[ok] - ll[ok]).abs() / ll[ok].abs().clamp_min(1.0)).max()) if bool(ok.any()) else 0.0)
    print(json.dumps({"case": "torch_cpu_ctc_loss", "rows": O * N, "threads": torch.get_num_threads(), "forward_ms": round(cpu_ms, 1),
                      "worst_relative_difference_to_device_ll": float(f"{worst:.3e}")}))
    est.close()

    # one 60 s row (50 frames a second) with 600 targets
    frames_long, classes, count = 60 * 50 - 1, 64, 600
    g = torch.Generator().manual_seed(0)
    em = torch.log_softmax(torch.randn(1, frames_long, classes, generator=g) * 3.0, -1).cuda()
    rng = np.random.default_rng(0)
    row = []
    while len(row) < count:
        v = int(rng.integers(1, classes))
        if not row or v != row[-1]:
            row.append(v)
    offsets, ids, _ = scoring.pack_targets([row])
    meta = torch.cat([offsets, ids]).cuda()
    lengths_dev = torch.tensor([frames_long], dtype=torch.int32).cuda()
    common = (C.c_void_p(em.data_ptr()), em.stride(0), em.stride(1), C.c_void_p(lengths_dev.data_ptr()), 1, frames_long, classes, 0)
    targets_ptr = (C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 8), count)
    results = {}
    for label, with_posteriors in (("amx_ctc_score_emissions_ms", False), ("amx_ctc_score_emissions_with_posteriors_ms", True)):
        sb = scoring.allocate(lib, 1, frames_long, count, device, posteriors=with_posteriors)

        def long_score():
            code = lib.amx_ctc_score_emissions(0, *common, 1, *targets_ptr, *sb.pointers(), C.c_void_p(stream))
            assert code == L.AMX_OK, lib.amx_last_error(None)

        results[label] = round(timed(long_score, args.iters), 3)
        assert int(sb.status.cpu()[0]) == 0
        long_ll, workspace_long = float(sb.log_likelihood.cpu()[0]), sb.size
    lb = alignment.allocate(lib, 1, frames_long, count, device)

    def long_align():
        code = lib.amx_ctc_align_emissions(0, *common, *targets_ptr, *lb.pointers(), C.c_void_p(stream))
        assert code == L.AMX_OK, lib.amx_last_error(None)

    long_align_ms = timed(long_align, args.iters)
    em_host = em[0].cpu().unsqueeze(1)
    t0 = time.perf_counter()
    loss = F.ctc_loss(em_host, torch.tensor([row]), torch.tensor([frames_long]), torch.tensor([count]), blank=0,
                      reduction="none")
    cpu_long_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"case": "long_row", "frames": frames_long, "targets": count, "classes": classes,
                      "workspace_mb": round(workspace_long / 2 ** 20, 1), **results, "amx_ctc_align_emissions_ms": round(long_align_ms, 3),
                      "torch_cpu_ctc_loss_ms": round(cpu_long_ms, 1), "log_likelihood": round(long_ll, 3),
                      "torch_cpu_log_likelihood": round(-float(loss[0]), 3), "best_path_total": round(float(lb.totals.cpu()[0]), 3)}))


if __name__ == "__main__":
    main()

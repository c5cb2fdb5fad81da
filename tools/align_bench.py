"""Times the on-device CTC forced alignment (amx_ctc_align.hip) and sets no threshold:

  * every output of the benchmark's config 2 -- 32 x 10 s utterances, each (output, utterance) row aligned against its own
    greedy tokens -- through ``Estimator.align_device`` (with its allocations and target upload) and through
    ``amx_ctc_align`` on prepared buffers, beside the prediction step and the greedy and beam decoders on the same outputs
    (as ``tools/beam_bench.py`` times them);
  * one 60 s row with 600 targets through ``amx_ctc_align_emissions`` on prepared buffers;
  * the host restatement (``tests/ctc_align_util.py``, the frame-at-a-time numpy sweep) on a sample of config-2 rows.

Prints one JSON line per measurement.  The device times are HIP events around whole calls; ``amx_ctc_align`` includes the
frame-length upload and its host synchronisation.  Run it under ``rocprofv3 --kernel-trace --stats`` for the kernel's own
time: ctc_align_kernel runs ``2 * (iters + 1) + 1`` times on config 2, then ``iters + 1`` times on the long row.

    python tools/align_bench.py [--utterances 32] [--seconds 10] [--iters 5] [--host-rows 8]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from allophant_amd import alignment, lib as L, synthetic  # noqa: E402
from allophant_amd.estimator import Batch, Estimator  # noqa: E402
from bench import build_spec  # noqa: E402
import ctc_align_util as U  # noqa: E402


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
    ap.add_argument("--host-rows", type=int, default=8)
    args = ap.parse_args()
    lib = L.load()
    spec = build_spec(phones=args.phones)
    est = Estimator(spec, synthetic.make_state_dict(spec, seed=0), "cuda:0")
    tfi = synthetic.make_inventory(spec, args.phones, seed=0)
    audio, lengths = synthetic.make_audio(args.utterances, int(args.seconds * 16000), seed=1234)
    batch = Batch(audio.cuda(), lengths, torch.zeros(args.utterances, dtype=torch.long))
    pred = est.predict(batch, tfi)
    names = list(pred.outputs)
    T, N = next(iter(pred.outputs.values())).shape[:2]
    O = len(names)
    step_ms = timed(lambda: est.predict(batch, tfi), args.iters)
    greedy_ms = timed(lambda: est.greedy_decode_device(pred), args.iters)
    beam_ms = timed(lambda: est.beam_decode_device(pred, 16, 4), args.iters)
    decoded = est.greedy_decode_device(pred)
    tokens, counts = decoded.tokens.cpu(), decoded.counts.cpu()
    targets = {name: [tokens[o, n, :int(counts[o, n])].tolist() for n in range(N)] for o, name in enumerate(names)}
    max_target = max(len(row) for rows in targets.values() for row in rows)
    mean_target = float(np.mean([len(row) for rows in targets.values() for row in rows]))
    print(json.dumps({"case": "config2", "utterances": N, "frames": T, "outputs": O, "rows": O * N, "max_target": max_target,
                      "mean_target": round(mean_target, 1), "predict_step_ms": round(step_ms, 3),
                      "greedy_decode_ms": round(greedy_ms, 4), "beam16_decode_ms": round(beam_ms, 3)}))

    aligned = est.align_device(pred, targets)
    status = aligned.status.cpu()
    facade_ms = timed(lambda: est.align_device(pred, targets), args.iters)
    offsets, ids, _ = alignment.pack_targets([row for name in names for row in targets[name]])
    meta = torch.cat([offsets, ids, torch.zeros(1, dtype=torch.int32)]).cuda()
    b = alignment.allocate(lib, O * N, T, max_target, torch.device("cuda:0"))
    frame_lengths = pred.lengths.detach().to("cpu", torch.int64).contiguous()
    stream = torch.cuda.current_stream().cuda_stream

    def direct():
        code = lib.amx_ctc_align(est._handle, C.c_void_p(pred._flat.data_ptr()), C.cast(frame_lengths.data_ptr(), C.POINTER(C.c_int64)),
                                 N, pred._geometry[1], C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 4 * (O * N + 1)),
                                 max_target, *b.pointers(), C.c_void_p(stream))
        assert code == L.AMX_OK, lib.amx_last_error(est._handle)

    direct_ms = timed(direct, args.iters)
    assert torch.equal(b.paths.view(O, N, T), aligned.paths) and torch.equal(b.totals.view(O, N), aligned.totals)
    print(json.dumps({"case": "config2_all_outputs", "rows": O * N, "frames": T, "aligned_rows": int((status == 0).sum()),
                      "workspace_mb": round(b.size / 2 ** 20, 1), "align_device_ms": round(facade_ms, 3),
                      "amx_ctc_align_ms": round(direct_ms, 3)}))

    # the host restatement on a sample of rows (the outputs are copied to the host first, which is not timed)
    sample = [(o, n) for o in range(0, O, max(1, O // args.host_rows)) for n in (0,)][:args.host_rows]
    host_ms = []
    for o, n in sample:
        em = pred.outputs[names[o]][:, n].cpu().numpy()
        t0 = time.perf_counter()
        row = U.align_row(em[:int(frame_lengths[n])], targets[names[o]][n], fast=True)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        assert row.status == int(status[o, n]) and (row.status != 0 or np.array_equal(row.paths, aligned.paths[o, n].cpu().numpy()[:len(row.paths)]))
    print(json.dumps({"case": "host_restatement", "rows": len(sample), "ms_per_row": round(float(np.mean(host_ms)), 3),
                      "ms_for_all_rows_at_that_rate": round(float(np.mean(host_ms)) * O * N, 1)}))
    est.close()

    # one 60 s row (50 frames a second) with 600 targets
    frames, classes, count = 60 * 50 - 1, 64, 600
    g = torch.Generator().manual_seed(0)
    em = torch.log_softmax(torch.randn(1, frames, classes, generator=g) * 3.0, -1).cuda()
    rng = np.random.default_rng(0)
    row = []
    while len(row) < count:
        v = int(rng.integers(1, classes))
        if not row or v != row[-1]:
            row.append(v)
    offsets, ids, _ = alignment.pack_targets([row])
    meta = torch.cat([offsets, ids]).cuda()
    lengths_dev = torch.tensor([frames], dtype=torch.int32).cuda()
    lb = alignment.allocate(lib, 1, frames, count, torch.device("cuda:0"))

    def long_row():
        code = lib.amx_ctc_align_emissions(0, C.c_void_p(em.data_ptr()), em.stride(0), em.stride(1), C.c_void_p(lengths_dev.data_ptr()),
                                           1, frames, classes, 0, C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 8), count,
                                           *lb.pointers(), C.c_void_p(stream))
        assert code == L.AMX_OK, lib.amx_last_error(None)

    long_ms = timed(long_row, args.iters)
    t0 = time.perf_counter()
    want = U.align_row(em[0].cpu().numpy(), row, fast=True)
    host_long_ms = (time.perf_counter() - t0) * 1e3
    assert int(lb.status.cpu()[0]) == 0 and np.array_equal(lb.paths.cpu().numpy()[0], want.paths)
    print(json.dumps({"case": "long_row", "frames": frames, "targets": count, "classes": classes,
                      "amx_ctc_align_emissions_ms": round(long_ms, 3), "host_restatement_ms": round(host_long_ms, 1)}))


if __name__ == "__main__":
    main()

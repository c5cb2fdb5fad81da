"""Times the on-device CTC beam search (amx_ctc_beam.hip) at the geometry of the benchmark's config 2 -- 32 x 10 s
utterances, every output of the multitask model decoded (Estimator.beam_decode_device) -- and on one 1025-class head
(beam_ctc_decode on [32, 499, 1025] log-probabilities), at beams of 4, 16 and 64, beside the prediction step and the greedy
decoder on the same outputs.  Prints one JSON line per measurement.  The times are HIP events around whole Python calls:
they include the output and workspace allocations and the host synchronisation in ``amx_beam_ctc`` (config 2) or the copies
to the host and the ``CTCHypothesis`` objects (head_1025).  Run it under ``rocprofv3 --kernel-trace`` for the kernels' own
times: each case issues its kernel ``iters + 1`` times, config 2 cases (beam_ctc_kernel) first, in the order printed.

    python tools/beam_bench.py [--utterances 32] [--seconds 10] [--beams 4 16 64] [--iters 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from allophant_amd import synthetic  # noqa: E402
from allophant_amd.estimator import Batch, Estimator, beam_ctc_decode  # noqa: E402
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
    ap.add_argument("--beams", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    spec = build_spec(phones=args.phones)
    est = Estimator(spec, synthetic.make_state_dict(spec, seed=0), "cuda:0")
    tfi = synthetic.make_inventory(spec, args.phones, seed=0)
    audio, lengths = synthetic.make_audio(args.utterances, int(args.seconds * 16000), seed=1234)
    batch = Batch(audio.cuda(), lengths, torch.zeros(args.utterances, dtype=torch.long))
    pred = est.predict(batch, tfi)
    T, N = next(iter(pred.outputs.values())).shape[:2]
    classes = {name: out.shape[2] for name, out in pred.outputs.items()}
    step_ms = timed(lambda: est.predict(batch, tfi), args.iters)
    greedy_ms = timed(lambda: est.greedy_decode_device(pred), args.iters)
    print(json.dumps({"case": "config2", "utterances": N, "frames": T, "outputs": len(classes), "max_classes": max(classes.values()),
                      "predict_step_ms": round(step_ms, 3), "greedy_decode_ms": round(greedy_ms, 4)}))
    for beam in args.beams:
        ms = timed(lambda: est.beam_decode_device(pred, beam, min(beam, 4)), args.iters)
        print(json.dumps({"case": "config2_all_outputs", "beam": beam, "n_best": min(beam, 4), "rows": N * len(classes),
                          "beam_decode_ms": round(ms, 3)}))
    est.close()
    g = torch.Generator().manual_seed(0)
    em = torch.log_softmax(torch.randn(N, T, 1025, generator=g) * 3.0, -1).cuda()
    frames = torch.full((N,), T, dtype=torch.int32)
    for beam in args.beams:
        for exp in (True, False):
            ms = timed(lambda: beam_ctc_decode(em, frames, beam, min(beam, 4), exp_emissions=exp), args.iters)
            print(json.dumps({"case": "head_1025", "beam": beam, "n_best": min(beam, 4), "emissions": "exp" if exp else "log",
                              "rows": N, "frames": T, "beam_decode_ms": round(ms, 3)}))


if __name__ == "__main__":
    main()

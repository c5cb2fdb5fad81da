"""Times the on-device sinc resampler (amx_resample.hip) at the geometry of the benchmark's config 2 -- 32 x 10 s utterances --
from each source rate upstream lists (Common Voice 8 / 24 / 32 / 44.1 / 48 kHz, plus 11.025 and 22.05 kHz) to 16 kHz; then
``Estimator.resample`` + ``predict`` against ``predict`` alone on the config-2 model (44.1 kHz input); then the host path a
user has without this package: the same bank applied per utterance by ``torch.nn.functional.conv1d`` on the CPU, upstream's
formulation (full [m, 2W + o] kernel, stride o), at 16 threads.  Prints one JSON line per measurement.

``launch_ms`` is HIP events around the ``amx_resample`` call alone (descriptors already on the device): kernel time plus one
launch.  ``batch_ms`` is the whole ``resample_batch`` call (bank lookup, descriptor copy to the device, launch).
``effective_GBps`` = (bytes read + bytes written) / launch_ms with bytes = 4 x (input samples + output samples).  Run it
under ``rocprofv3 --kernel-trace --stats`` (``--gpu-only``) for the kernel's own time: each rate issues ``resample_kernel``
``2 * iters + 3`` times, in the order printed.

    python tools/resample_bench.py [--utterances 32] [--seconds 10] [--iters 20] [--gpu-only]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from allophant_amd import resample as RS, synthetic  # noqa: E402
from allophant_amd.estimator import Batch, Estimator  # noqa: E402

RATES = [8000, 11025, 22050, 24000, 32000, 44100, 48000]


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


def source_batch(rate, utterances, seconds, device="cuda"):
    g = torch.Generator().manual_seed(rate)
    n = int(seconds * rate)
    audio = torch.randn(utterances, n, generator=g) * 0.1
    return Batch(audio.to(device), torch.full((utterances,), n, dtype=torch.int64), torch.zeros(utterances, dtype=torch.long))


def conv1d_bank(rate, new=16000):
    """Upstream's kernel layout, [m, 1, 2W + o], filled from the library's bank (the dropped taps are zero)."""
    geometry, bank, phases = RS.host_bank(rate, new)
    full = torch.zeros(geometry.m, 1, 2 * geometry.width + geometry.o)
    for j in range(geometry.m):
        first, count = int(phases[0, j]), int(phases[1, j])
        full[j, 0, first: first + count] = bank[:count, j]
    return geometry, full


def host_resample(x, geometry, kernel):
    """torchaudio's _apply_sinc_resample_kernel restated: pad (W, W + o), conv1d stride o, interleave the phases."""
    n = x.shape[-1]
    padded = torch.nn.functional.pad(x[None, None], (geometry.width, geometry.width + geometry.o))
    y = torch.nn.functional.conv1d(padded, kernel, stride=geometry.o)
    return y.transpose(1, 2).reshape(-1)[: -(-geometry.m * n // geometry.o)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--gpu-only", action="store_true", help="only the kernel cases (for a rocprofv3 run)")
    args = ap.parse_args()
    N = args.utterances
    for rate in RATES:
        batch = source_batch(rate, N, args.seconds)
        out = RS.resample_batch(batch, rate)
        entry = RS._device_bank(rate, 16000, 6, 0.99, batch.audio_features.device)
        lengths = batch.lengths.cuda()
        rows = entry.row_dev.expand(N, 6).contiguous()
        L_out = out.audio_features.shape[1]
        launch = lambda: RS._launch(batch.audio_features, lengths, rows, entry.bank, entry.phases, entry.geometry.window,  # noqa: E731
                                    L_out)
        launch_ms = timed(launch, args.iters)
        batch_ms = timed(lambda: RS.resample_batch(batch, rate), args.iters)
        nbytes = 4 * (batch.audio_features.numel() + out.audio_features.numel())
        g = entry.geometry
        print(json.dumps({"case": "kernel", "rate": rate, "o": g.o, "m": g.m, "W": g.width, "taps": g.taps,
                          "utterances": N, "seconds": args.seconds, "in_samples": batch.audio_features.numel(),
                          "out_samples": out.audio_features.numel(), "fma": out.audio_features.numel() * g.taps,
                          "launch_ms": round(launch_ms, 4), "batch_ms": round(batch_ms, 4),
                          "effective_GBps": round(nbytes / launch_ms / 1e6, 1)}), flush=True)
    if args.gpu_only:
        return

    from bench import build_spec

    spec = build_spec(phones=27)
    est = Estimator(spec, synthetic.make_state_dict(spec, seed=0), "cuda:0")
    tfi = synthetic.make_inventory(spec, 27, seed=0)
    src = source_batch(44100, N, args.seconds)
    at16 = est.resample(src, 44100)
    predict_ms = timed(lambda: est.predict(at16, tfi), 5)
    both_ms = timed(lambda: est.predict(est.resample(src, 44100), tfi), 5)
    print(json.dumps({"case": "estimator", "rate": 44100, "utterances": N, "seconds": args.seconds,
                      "predict_ms": round(predict_ms, 3), "resample_plus_predict_ms": round(both_ms, 3),
                      "resample_share": round((both_ms - predict_ms) / both_ms, 4)}), flush=True)
    est.close()

    torch.set_num_threads(args.host_threads)
    for rate in (44100, 48000, 8000):
        geometry, kernel = conv1d_bank(rate)
        audio = source_batch(rate, N, args.seconds, device="cpu").audio_features
        host_resample(audio[0], geometry, kernel)  # warm-up
        t0 = time.perf_counter()
        for n in range(N):
            host_resample(audio[n], geometry, kernel)
        host_ms = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"case": "host_conv1d", "rate": rate, "utterances": N, "seconds": args.seconds,
                          "threads": torch.get_num_threads(), "taps_per_phase": kernel.shape[-1], "host_ms": round(host_ms, 2)}),
              flush=True)


if __name__ == "__main__":
    main()

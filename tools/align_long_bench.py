"""Times the long form of the on-device CTC forced alignment (amx_ctc_align_long.hip) and sets no threshold:

  * (a) the largest row both paths accept -- 4095 non-repeating random targets over 20 480 frames, as many classes as the
    phoneme output of the benchmark's config 2 -- through ``amx_ctc_align_emissions`` (one workgroup) and through
    ``amx_ctc_align_long_emissions`` on prepared buffers, and whether every output buffer is equal;
  * (b) one recording of each ``--seconds`` (600 and 3600) through ``Estimator.predict_long`` of the config-2 model, its phoneme
    output aligned against round(T / 5) random non-repeating targets, beside the ``predict_long`` that produced the emissions.

The alignment time is split three ways.  ``host_enqueue_ms`` is the wall time of the call, which returns once its
2 + ceil(T / 64) launches are enqueued.  ``device_ms`` is HIP events around the call.  ``sweep_ms`` is HIP events around the
same call on a copy of the emissions whose last frame is -inf in every class: the prepare launch and every sweep launch do
the same work (-inf is an ordinary value), and the finish launch finds no alignment and returns at once; ``finish_ms`` is the
difference.  Prints one JSON line per measurement.

    python tools/align_long_bench.py [--seconds 600 3600] [--iters 3] [--phones 27]
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

from allophant_amd import alignment, lib as L, synthetic  # noqa: E402
from allophant_amd.estimator import Batch, Estimator  # noqa: E402
from bench import build_spec  # noqa: E402


def timed(fn, iters):
    """(device ms by events, host ms until the call returns), each a mean over `iters` calls after one warm-up."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    device = host = 0.0
    for _ in range(iters):
        start.record()
        t0 = time.perf_counter()
        fn()
        host += (time.perf_counter() - t0) * 1e3
        stop.record()
        torch.cuda.synchronize()
        device += start.elapsed_time(stop)
    return device / iters, host / iters


def non_repeating(rng, count, classes):
    draws = rng.integers(1, classes, count)
    for k in range(1, count):
        while draws[k] == draws[k - 1]:
            draws[k] = rng.integers(1, classes)
    return draws.tolist()


class Row:
    """One row [1, T, C] (any strides, unit class stride) and its targets on prepared buffers, for either entry point."""

    def __init__(self, lib, em, frames, targets, long):
        self.lib, self.em, self.frames, self.count = lib, em, frames, len(targets)
        offsets, ids, _ = alignment.pack_targets([targets], limit=alignment.ALIGN_LONG_MAX_TARGET)
        self.meta = torch.cat([offsets, ids]).cuda()
        self.lengths = torch.tensor([frames], dtype=torch.int32).cuda()
        self.b = alignment.allocate(lib, 1, em.shape[1], self.count, em.device, long)
        self.entry = lib.amx_ctc_align_long_emissions if long else lib.amx_ctc_align_emissions
        self.stream = torch.cuda.current_stream().cuda_stream

    def __call__(self, em=None):
        em = self.em if em is None else em
        code = self.entry(0, C.c_void_p(em.data_ptr()), em.stride(0), em.stride(1), C.c_void_p(self.lengths.data_ptr()), 1,
                          em.shape[1], em.shape[2], 0, C.c_void_p(self.meta.data_ptr()), C.c_void_p(self.meta.data_ptr() + 8),
                          self.count, *self.b.pointers(), C.c_void_p(self.stream))
        assert code == L.AMX_OK, self.lib.amx_last_error(None)

    def outputs(self):
        b = self.b
        return [t.clone() for t in (b.paths, b.frame_scores, b.spans, b.span_scores, b.totals, b.status)]


def split(row, iters):
    """The three parts of a long-form call on `row`, and the outputs of the full call."""
    device_ms, host_ms = timed(row, iters)
    outputs = row.outputs()
    assert int(outputs[5][0]) == 0, "the row has no alignment"
    blocked = row.em.clone()
    blocked[0, row.frames - 1] = -float("inf")
    sweep_ms, _ = timed(lambda: row(blocked), iters)
    assert int(row.b.status.cpu()[0]) == -1
    return {"host_enqueue_ms": round(host_ms, 3), "device_ms": round(device_ms, 3), "sweep_ms": round(sweep_ms, 3),
            "finish_ms": round(device_ms - sweep_ms, 3), "launches": 2 + (row.em.shape[1] + 63) // 64,
            "workspace_mb": round(row.b.size / 2 ** 20, 1)}, outputs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, nargs="*", default=[600.0, 3600.0])
    ap.add_argument("--phones", type=int, default=27)
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    lib = L.load()
    rng = np.random.default_rng(0)

    # (a) the largest row both paths accept
    frames, classes, count = 20480, args.phones + 1, alignment.ALIGN_MAX_TARGET
    g = torch.Generator().manual_seed(0)
    em = torch.log_softmax(torch.randn(1, frames, classes, generator=g) * 3.0, -1).cuda()
    targets = non_repeating(rng, count, classes)
    old = Row(lib, em, frames, targets, long=False)
    old_ms, old_host_ms = timed(old, args.iters)
    parts, new_outputs = split(Row(lib, em, frames, targets, long=True), args.iters)
    old()
    equal = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                for a, b in zip(old.outputs(), new_outputs))
    print(json.dumps({"case": "both_paths", "frames": frames, "targets": count, "classes": classes,
                      "amx_ctc_align_emissions_ms": round(old_ms, 3), "amx_ctc_align_emissions_host_ms": round(old_host_ms, 3),
                      "amx_ctc_align_long_emissions": parts, "outputs_equal": equal}), flush=True)
    del old, em

    # (b) whole recordings through predict_long
    if not args.seconds:
        return
    spec = build_spec(phones=args.phones)
    est = Estimator(spec, synthetic.make_state_dict(spec, seed=0), "cuda:0")
    tfi = synthetic.make_inventory(spec, args.phones, seed=0)
    for seconds in args.seconds:
        audio, lengths = synthetic.make_audio(1, int(seconds * 16000), seed=1234)
        batch = Batch(audio.cuda(), lengths, torch.zeros(1, dtype=torch.long))
        pred = est.predict_long(batch, tfi)
        torch.cuda.synchronize()
        predict_ms, _ = timed(lambda: est.predict_long(batch, tfi), max(1, args.iters - 1))
        frames = int(pred.lengths[0])
        em = pred.outputs["phoneme"].transpose(0, 1)  # [1, T, C], read in place
        targets = non_repeating(rng, round(frames / 5), em.shape[2])
        parts, outputs = split(Row(lib, em, frames, targets, long=True), args.iters)
        print(json.dumps({"case": "recording", "seconds": seconds, "frames": frames, "targets": len(targets), "classes": em.shape[2],
                          "predict_long_ms": round(predict_ms, 1), "amx_ctc_align_long_emissions": parts,
                          "total": round(float(outputs[4][0]), 1)}), flush=True)
        del pred, em, batch
        torch.cuda.empty_cache()
    est.close()


if __name__ == "__main__":
    main()

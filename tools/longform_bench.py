"""Times ``Estimator.predict_long`` on long recordings at XLS-R shape (the composition model of BASELINE config 2, bench.py) with
10 s windows, 1 s of context and 32-row slices, and the two launches of its own -- ``amx_long_gather`` and ``amx_long_stitch`` --
against the same copies written with torch indexing on the same machine.  Prints one JSON line per part:

  * ``recording``: per duration (default 600 s and 3 600 s, one recording each) the time of one ``predict_long`` call ended by a
    synchronise (median of ``--iters`` calls after a warm-up call), audio seconds per second, and the graphs recorded and
    replayed by the timed calls (``graph_info``);
  * ``slice``: one full slice (32 windows of 10 s) of the longest recording: the forward pass alone on the gathered batch, the
    gather and the stitch alone, each as launched by ``predict_long``, and the same two copies as torch indexing (the windows as
    ``as_strided`` + ``copy_``, the outputs as one slice assignment per window and block); medians of ``--iters`` samples after
    warm-up with the 10th and 90th percentiles, the five alternating, a sample being a burst of launches between two events
    (10 for the copies, 2 for the torch stitch, 1 for the forward pass); the share of gather plus
    stitch in gather + forward + stitch; bytes moved and the rate, to set beside the copy rate of tools/hbm_bw_probe.hip;
  * ``seams`` (information only, the weights are procedural): on 1 x 60 s, the largest difference between the long-form and the
    single-pass log-probabilities over all frames of the recording, and the share of frames with the same greedy class.

    python tools/longform_bench.py [--seconds 600 3600] [--iters 20] [--precision f16x3]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from allophant_amd import longform, spec as S, synthetic  # noqa: E402
from allophant_amd.estimator import Batch, Estimator  # noqa: E402

WINDOW_SECONDS, CONTEXT_SECONDS, ROWS = 10.0, 1.0, 32


def timed(fn, burst=1):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(burst):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / burst


def summary(samples):
    ordered = sorted(samples)
    pick = lambda q: ordered[min(len(ordered) - 1, int(q * len(ordered)))]  # noqa: E731
    return {"median_ms": round(statistics.median(ordered), 4), "p10_ms": round(pick(0.1), 4), "p90_ms": round(pick(0.9), 4)}


def recording(seconds, seed):
    audio, lengths = synthetic.make_audio(1, int(seconds * 16000), seed=seed)
    return Batch(audio.cuda(), lengths, torch.zeros(1, dtype=torch.long))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, nargs="+", default=[600.0, 3600.0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--precision", default="f16x3")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU path and no CPU timing")
    spec = S.multitask_spec(S.xlsr_300m_encoder(), allophone_layer=True)
    spec["shared_phones"] = 80
    est = Estimator(spec, synthetic.make_state_dict(spec, seed=0), "cuda:0", args.precision)
    tfi = synthetic.make_inventory(spec, 27, seed=0)
    arguments = dict(window_seconds=WINDOW_SECONDS, context_seconds=CONTEXT_SECONDS, batch_windows=ROWS)
    window = int(WINDOW_SECONDS * est.sample_rate)
    context = int(CONTEXT_SECONDS * est.sample_rate) // math.prod(spec["conv_stride"])

    batch = None
    for seconds in args.seconds:
        batch = recording(seconds, seed=int(seconds))
        est.predict_long(batch, tfi, **arguments)  # warm-up: workspace, the first recordings
        torch.cuda.synchronize()
        captures, replays = est.graph_info()
        samples = [timed(lambda: est.predict_long(batch, tfi, **arguments)) for _ in range(args.iters)]
        after = est.graph_info()
        plan = longform.plan_windows(batch.lengths.tolist(), spec, window, context)
        total = summary(samples)
        print(json.dumps({"part": "recording", "seconds": seconds, "windows": len(plan), "slices": -(-len(plan) // ROWS),
                          "frames": int(plan.frames[0]), "precision": args.precision, "iters": args.iters, "predict_long": total,
                          "audio_seconds_per_second": round(seconds / (total["median_ms"] * 1e-3), 1),
                          "graphs_recorded": after[0] - captures, "passes_replayed": after[1] - replays}), flush=True)

    # one full slice of the last recording: the first ROWS windows
    audio, lengths = batch.audio_features, batch.lengths.cuda()
    plan = longform.plan_windows(batch.lengths.tolist(), spec, window, context)
    if len(plan) < ROWS:
        raise SystemExit("the last recording is shorter than one full slice")
    rows = plan.windows[:ROWS]
    windows = torch.from_numpy(rows).cuda()
    gathered = torch.empty(ROWS, window, device="cuda")
    status = torch.empty(ROWS, dtype=torch.int32, device="cuda")
    part = Batch(gathered, torch.full((ROWS,), window), torch.zeros(ROWS, dtype=torch.long))
    longform.gather_windows(audio, lengths, windows, plan.hop, gathered, status)
    piece = est.predict(part, tfi)
    window_out = piece._flat
    descs, T, total_floats = est._output_layout(1, audio.shape[1])
    flat = torch.zeros(total_floats, device="cuda")
    where = {d.name.decode(): (d.offset, d.classes) for d in descs}
    blocks = sorted({(o.storage_offset(), where[name][0], o.shape[2]) for name, o in piece.outputs.items()})
    src_T = next(iter(piece.outputs.values())).shape[0]
    src_views = [window_out[s: s + src_T * ROWS * c].view(src_T, ROWS, c) for s, _, c in blocks]
    dst_views = [flat[d: d + T * c].view(T, 1, c) for _, d, c in blocks]
    step = int(rows[1, longform.START] - rows[0, longform.START]) * plan.hop

    def forward():
        est.predict(part, tfi, _out=window_out)

    def gather():
        longform.gather_windows(audio, lengths, windows, plan.hop, gathered, status)

    def stitch():
        longform.stitch_windows(window_out, src_T, windows, blocks, flat, 1, T, status)

    def torch_gather():
        gathered.copy_(audio[0].as_strided((ROWS, window), (step, 1), int(rows[0, longform.START]) * plan.hop))

    def torch_stitch():
        for w, (_, _, a, keep_lo, keep_hi, _) in enumerate(rows.tolist()):
            for src, dst in zip(src_views, dst_views):
                dst[keep_lo:keep_hi, 0] = src[keep_lo - a: keep_hi - a, w]

    want_audio, want_flat = gathered.clone(), None
    stitch()
    want_flat = flat.clone()
    flat.zero_(), torch_stitch(), torch_gather()
    assert torch.equal(flat, want_flat) and torch.equal(gathered, want_audio)  # the yardstick makes the same copies
    parts = (("forward", forward, 1), ("gather", gather, 10), ("torch_gather", torch_gather, 10), ("stitch", stitch, 10),
             ("torch_stitch", torch_stitch, 2))
    for _, fn, _ in parts:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name, _, _ in parts}
    for _ in range(args.iters):  # alternating: a kernel and its yardstick see the same neighbours on the machine
        for name, fn, burst in parts:
            samples[name].append(timed(fn, burst))
    results = {name: summary(values) for name, values in samples.items()}
    kept = int((rows[:, longform.KEEP_HI] - rows[:, longform.KEEP_LO]).sum())
    moved = {"gather": 2 * 4 * ROWS * window, "stitch": 2 * 4 * kept * sum(c for _, _, c in blocks)}
    ours = results["gather"]["median_ms"] + results["stitch"]["median_ms"]
    print(json.dumps({"part": "slice", "rows": ROWS, "window_samples": window, "blocks": len(blocks), "kept_frames": kept,
                      "torch_copies_per_slice": 1 + ROWS * len(blocks), **results,
                      "gather_plus_stitch_share": round(ours / (ours + results["forward"]["median_ms"]), 5),
                      "bytes_moved": moved,
                      "gather_gb_s": round(moved["gather"] / (results["gather"]["median_ms"] * 1e-3) / 1e9, 1),
                      "stitch_gb_s": round(moved["stitch"] / (results["stitch"]["median_ms"] * 1e-3) / 1e9, 1),
                      "torch_over_kernel": {"gather": round(results["torch_gather"]["median_ms"] / results["gather"]["median_ms"], 2),
                                            "stitch": round(results["torch_stitch"]["median_ms"] / results["stitch"]["median_ms"], 2)}}),
          flush=True)

    # the seams, as information: 1 x 60 s in windows against one pass over the whole minute
    minute = recording(60.0, seed=60)
    if int(est._lib.amx_max_utterances(est._handle, minute.audio_features.shape[1])) >= 1:
        long = est.predict_long(minute, tfi, **arguments)
        single = est.predict(minute, tfi)
        frames = int(single.lengths[0])
        worst = max(float((long.outputs[k][:frames] - single.outputs[k][:frames]).abs().max()) for k in single.outputs)
        same = float((long.outputs["phoneme"][:frames].argmax(-1) == single.outputs["phoneme"][:frames].argmax(-1)).float().mean())
        print(json.dumps({"part": "seams", "seconds": 60.0, "frames": frames, "max_abs_log_probability_difference": round(worst, 4),
                          "frames_with_equal_greedy_class": round(same, 4)}), flush=True)
    est.close()


if __name__ == "__main__":
    main()

"""Times a mixed-language batch of a composition model two ways: (a) the per-language loop as it has to be written without
``predict_languages`` (split the batch by language, one ``predict`` under each language's own inventory, greedy decoding of
each part) and (b) one ``predict_languages`` call under the union inventory plus one greedy decoding; and (c) the restriction
alone (``amx_restrict_outputs`` in place on the composed block of such a pass).  The model is the XLS-R composition model of
BASELINE config 2 (bench.py), the batch 32 x 10 s spread over 8 languages of different inventory sizes, 4 utterances each.

(a) and (b) alternate in one loop, every iteration timed on its own with device events and ended by a synchronise; the line
reports medians with the 10th and 90th percentiles.  Prints one JSON line.  For the kernels' own times (``restrict_kernel``
beside ``logsoftmax_out_kernel`` of the same pass) run it under ``rocprofv3 --kernel-trace --stats`` with ``--iters 5 --no-graph``.

    python tools/mixed_language_bench.py [--utterances 32] [--seconds 10] [--iters 30] [--warmup 5] [--no-graph]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from allophant_amd import lib as L, spec as S, synthetic  # noqa: E402
from allophant_amd.estimator import Batch, Estimator  # noqa: E402
from allophant_amd.inventories import LanguageInventories  # noqa: E402

SIZES = (12, 20, 27, 35, 44, 52, 64, 80)  # phonemes per language ('es' has 27)


def build_inventories(spec, sizes):
    rows = synthetic.make_inventory(spec, 400, seed=0).tolist()
    pool = torch.tensor(list(dict.fromkeys(tuple(r) for r in rows)), dtype=torch.int64)
    g = torch.Generator().manual_seed(1)
    return LanguageInventories.from_matrices(
        {f"lg{i}": pool[torch.randperm(pool.shape[0], generator=g)[:size].sort().values] for i, size in enumerate(sizes)})


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def summary(samples):
    ordered = sorted(samples)
    pick = lambda q: ordered[min(len(ordered) - 1, int(q * len(ordered)))]  # noqa: E731
    return {"median_ms": round(statistics.median(ordered), 4), "p10_ms": round(pick(0.1), 4), "p90_ms": round(pick(0.9), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--no-graph", action="store_true", help="enqueue every pass launch by launch (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU path and no CPU timing")
    N = args.utterances
    spec = S.multitask_spec(S.xlsr_300m_encoder(), allophone_layer=True)
    spec["shared_phones"] = 80
    state = synthetic.make_state_dict(spec, seed=0)
    inventories = build_inventories(spec, SIZES)
    names = inventories.languages
    languages = [names[n * len(names) // N] for n in range(N)]  # consecutive utterances share a language
    audio, lengths = synthetic.make_audio(N, int(args.seconds * 16000), seed=0)
    audio = audio.cuda()
    est = Estimator(spec, state, "cuda:0", args.precision)
    whole = Batch(audio, lengths, inventories.language_ids(languages).to(torch.long))
    parts = []
    for language in names:
        own = [n for n, l in enumerate(languages) if l == language]
        parts.append((inventories.tfi(language), Batch(audio[own].contiguous(), lengths[own], torch.zeros(len(own), dtype=torch.long))))

    def loop():
        return [est.greedy_decode_device(est.predict(part, tfi, _no_graph=args.no_graph)) for tfi, part in parts]

    def one_call():
        return est.greedy_decode_device(est.predict_languages(whole, inventories, _no_graph=args.no_graph))

    for _ in range(args.warmup):
        loop(), one_call()
    torch.cuda.synchronize()
    loop_ms, call_ms = [], []
    for _ in range(args.iters):  # alternating: both see the same neighbours on the machine
        loop_ms.append(timed(loop))
        call_ms.append(timed(one_call))

    # the decoded tokens agree: the union pass restricted is the per-language pass
    together = one_call()
    o = together.names.index("phoneme")
    counts, tokens = together.counts[o].cpu(), together.tokens[o].cpu()
    equal = 0
    for (_, part), language, decoded in zip(parts, names, loop()):
        own = [n for n, l in enumerate(languages) if l == language]
        for row, n in enumerate(own):
            k = int(decoded.counts[o, row])
            mapped = inventories.to_language_indices(tokens[n, :int(counts[n])], language)
            equal += int(counts[n]) == k and torch.equal(mapped, decoded.tokens[o, row, :k].cpu())

    # (c) the restriction alone, in place on the composed block of one pass
    pred = est.predict_languages(whole, inventories)
    block = pred.outputs["phoneme"]
    T, _, classes = block.shape
    meta = torch.cat([pred.lengths.to(torch.int32), pred._languages[0].cpu()]).cuda()
    status = torch.empty(N, dtype=torch.int32, device="cuda")
    bits = inventories.device_bits(block.device)
    handle = L.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def restriction():
        code = handle.amx_restrict_outputs(0, C.c_void_p(block.data_ptr()), block.stride(0), block.stride(1), classes,
                                           C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 4 * N), C.c_void_p(bits.data_ptr()),
                                           len(names), N, T, L.RESTRICT_NORMALIZE, C.c_void_p(block.data_ptr()), block.stride(0),
                                           block.stride(1), C.c_void_p(status.data_ptr()), stream)
        assert code == L.AMX_OK

    for _ in range(args.warmup):
        restriction()
    torch.cuda.synchronize()
    burst = 20  # launches per sample: one launch is shorter than the events' resolution
    restrict_ms = [timed(lambda: [restriction() for _ in range(burst)]) / burst for _ in range(args.iters)]
    moved = 2 * 4 * T * N * classes
    a, b, c = summary(loop_ms), summary(call_ms), summary(restrict_ms)
    print(json.dumps({
        "utterances": N, "seconds": args.seconds, "languages": len(names), "inventory_sizes": list(SIZES), "union_classes": classes,
        "frames": T, "precision": args.precision, "iters": args.iters, "warmup": args.warmup,
        "a_per_language_loop": a, "b_predict_languages": b, "loop_over_one_call": round(a["median_ms"] / b["median_ms"], 3),
        "c_restriction_back_to_back": c, "c_bytes_moved": moved,
        "c_effective_gb_s": round(moved / (c["median_ms"] * 1e-3) / 1e9, 1),
        "utterances_with_equal_greedy_tokens": equal}))
    est.close()


if __name__ == "__main__":
    main()

"""Times the on-device CTC scoring of every one-edit variant (amx_ctc_variants.hip) and sets no threshold:

  * the phoneme output of the benchmark's config 2 -- 32 x 10 s utterances, each against its own greedy tokens -- through
    ``Estimator.variants_device`` (with its allocations and target upload) and through ``amx_ctc_variants_emissions`` on
    prepared buffers;
  * the two launches of that call apart (the lattice kernel and the variants kernel), from the device times that
    ``torch.profiler`` records for one call (``null`` where the profiler gives none; ``rocprofv3 --kernel-trace --stats`` on
    this tool gives the same);
  * ``amx_ctc_score_emissions`` on the same rows, one forward-backward pass, for scale;
  * for one utterance the brute force this replaces: ``amx_ctc_score_emissions`` with every edited sequence as a candidate
    row, how many there are, and how far its log-likelihoods lie from the variants' cells.

Prints one JSON line per measurement and appends them to ``--log`` (``profiles/ctc_variants.log``).  The device times are
HIP events around whole calls.

    python tools/variants_bench.py [--utterances 32] [--seconds 10] [--iters 5]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from allophant_amd import lib as L, scoring, synthetic  # noqa: E402
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


def kernel_times(fn):
    """Device microseconds of the lattice and the variants kernel of one call, or (None, None)."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        found = {"lattice": 0.0, "variants": 0.0}
        for item in prof.key_averages():
            for key in found:
                if f"ctc_{key}_kernel" in item.key:
                    found[key] += float(item.self_device_time_total)
        return (found["lattice"] or None, found["variants"] or None)
    except Exception as error:  # noqa: BLE001  (a profiler that is not there is no reason to lose the other lines)
        print(f"torch.profiler gave no kernel times: {error}", file=sys.stderr)
        return None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--phones", type=int, default=27)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "ctc_variants.log"))
    args = ap.parse_args()
    lines = []

    def report(**fields):
        lines.append(json.dumps(fields))
        print(lines[-1], flush=True)

    lib = L.load()
    device = torch.device("cuda:0")
    spec = build_spec(phones=args.phones)
    est = Estimator(spec, synthetic.make_state_dict(spec, seed=0), "cuda:0")
    tfi = synthetic.make_inventory(spec, args.phones, seed=0)
    audio, lengths = synthetic.make_audio(args.utterances, int(args.seconds * 16000), seed=1234)
    pred = est.predict(Batch(audio.cuda(), lengths, torch.zeros(args.utterances, dtype=torch.long)), tfi)
    names = list(pred.outputs)
    o = names.index("phoneme")
    em = pred.outputs["phoneme"].transpose(0, 1)  # [N, T, C], read in place
    N, T, Cn = em.shape
    decoded = est.greedy_decode_device(pred)
    tokens, counts = decoded.tokens.cpu(), decoded.counts.cpu()
    rows = [tokens[o, n, :int(counts[o, n])].tolist() for n in range(N)]
    max_target = max(len(row) for row in rows)
    cells = sum((2 * len(row) + 1) * Cn for row in rows)
    report(case="config2_phoneme", utterances=N, frames=T, classes=Cn, max_target=max_target,
           mean_target=round(float(np.mean([len(row) for row in rows])), 1), variant_cells=cells)

    variants = est.variants_device(pred, rows, "phoneme")
    assert variants.status.cpu().tolist() == [0] * N
    facade_ms = timed(lambda: est.variants_device(pred, rows, "phoneme"), args.iters)

    offsets, ids, _ = scoring.pack_targets(rows)
    meta = torch.cat([offsets, ids, torch.zeros(1, dtype=torch.int32)]).cuda()
    frame_lengths = pred.lengths.detach().to(device, torch.int32).contiguous()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    common = (0, p(em), em.stride(0), em.stride(1), p(frame_lengths), N, T, Cn, 0)
    size = C.c_size_t()
    L.check(lib, None, lib.amx_ctc_variants_workspace(N, T, max_target, C.byref(size)))
    workspace = torch.empty(max(1, size.value), dtype=torch.uint8, device=device)
    ll = torch.empty(N, device=device)
    sub, ins = torch.empty(N, max_target, Cn, device=device), torch.empty(N, max_target + 1, Cn, device=device)
    status = torch.empty(N, dtype=torch.int32, device=device)

    def variants_call():
        code = lib.amx_ctc_variants_emissions(*common, p(meta), C.c_void_p(meta.data_ptr() + 4 * (N + 1)), max_target, p(workspace),
                                              size.value, p(ll), p(sub), p(ins), p(status), stream)
        assert code == L.AMX_OK, lib.amx_last_error(None)

    call_ms = timed(variants_call, args.iters)
    assert torch.equal(ll, variants.log_likelihood)
    lattice_us, variants_us = kernel_times(variants_call)

    sb = scoring.allocate(lib, N, T, max_target, device)

    def score_call():
        code = lib.amx_ctc_score_emissions(*common, 1, p(meta), C.c_void_p(meta.data_ptr() + 4 * (N + 1)), max_target, *sb.pointers(),
                                           stream)
        assert code == L.AMX_OK, lib.amx_last_error(None)

    score_ms = timed(score_call, args.iters)
    report(case="config2_phoneme_variants", rows=N, frames=T, classes=Cn, workspace_mb=round(size.value / 2 ** 20, 1),
           variants_device_ms=round(facade_ms, 3), amx_ctc_variants_emissions_ms=round(call_ms, 3),
           lattice_kernel_ms=None if lattice_us is None else round(lattice_us / 1e3, 3),
           variants_kernel_ms=None if variants_us is None else round(variants_us / 1e3, 3),
           amx_ctc_score_emissions_ms=round(score_ms, 3), variants_over_one_scoring_pass=round(call_ms / score_ms, 2))
    del sb

    # the brute force, for the utterance with the most targets: every edited sequence as a candidate row of one scoring call
    n = int(np.argmax([len(row) for row in rows]))
    y = rows[n]
    edited, where = [list(y)], [("ins", 0, 0)]
    for l in range(len(y)):
        edited.append(y[:l] + y[l + 1:])
        where.append(("sub", l, 0))
        for c in range(1, Cn):
            edited.append(y[:l] + [c] + y[l + 1:])
            where.append(("sub", l, c))
    for q in range(len(y) + 1):
        for c in range(1, Cn):
            edited.append(y[:q] + [c] + y[q:])
            where.append(("ins", q, c))
    G = len(edited)
    one = em[n:n + 1]
    offsets, ids, edited_counts = scoring.pack_targets(edited, 1, G)
    brute_meta = torch.cat([offsets, ids, torch.zeros(1, dtype=torch.int32)]).cuda()
    width = max(edited_counts)
    bb = scoring.allocate(lib, G, T, width, device)
    one_length = frame_lengths[n:n + 1].contiguous()

    def brute_call():
        code = lib.amx_ctc_score_emissions(0, p(one), one.stride(0), one.stride(1), p(one_length), 1, T, Cn, 0, G, p(brute_meta),
                                           C.c_void_p(brute_meta.data_ptr() + 4 * (G + 1)), width, *bb.pointers(), stream)
        assert code == L.AMX_OK, lib.amx_last_error(None)

    brute_ms = timed(brute_call, args.iters)
    one_offsets, one_ids, _ = scoring.pack_targets([y])
    one_meta = torch.cat([one_offsets, one_ids, torch.zeros(1, dtype=torch.int32)]).cuda()

    def one_call():
        code = lib.amx_ctc_variants_emissions(0, p(one), one.stride(0), one.stride(1), p(one_length), 1, T, Cn, 0, p(one_meta),
                                              C.c_void_p(one_meta.data_ptr() + 8), len(y), p(workspace), size.value, p(ll), p(sub),
                                              p(ins), p(status), stream)
        assert code == L.AMX_OK, lib.amx_last_error(None)

    one_ms = timed(one_call, args.iters)
    brute_ll = bb.log_likelihood.cpu()
    got_sub, got_ins = sub.view(-1)[:len(y) * Cn].view(len(y), Cn).cpu(), ins.view(-1)[:(len(y) + 1) * Cn].view(len(y) + 1, Cn).cpu()
    worst = 0.0
    for g, (kind, at, c) in enumerate(where):
        cell, want = float((got_sub if kind == "sub" else got_ins)[at, c]), float(brute_ll[g])
        if want == float("-inf") or cell == float("-inf"):
            assert want == cell, (kind, at, c, cell, want)
        else:
            worst = max(worst, abs(cell - want) / max(1.0, abs(want)))
    report(case="one_utterance_against_brute_force", utterance=n, frames=int(one_length[0]), targets=len(y), classes=Cn,
           edited_sequences=G, brute_force_workspace_mb=round(bb.size / 2 ** 20, 1), brute_force_amx_ctc_score_emissions_ms=round(brute_ms, 3),
           amx_ctc_variants_emissions_ms=round(one_ms, 3), brute_force_over_variants=round(brute_ms / one_ms, 1),
           worst_relative_difference=float(f"{worst:.3e}"))
    est.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a", encoding="utf-8") as f:
        f.write("".join(line + "\n" for line in lines))


if __name__ == "__main__":
    main()

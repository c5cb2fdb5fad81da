"""Times the on-device CTC forced alignment over label graphs (amx_ctc_align_graph.hip) against the chain aligner
(amx_ctc_align.hip) and sets no threshold.  The rows are the phoneme output of the benchmark's config 2 (32 x 10 s utterances)
against each utterance's greedy tokens; both kernels read the same ``[N, T, C]`` view through their ``_emissions`` entry points,
on prepared buffers, in the same process:

  * chain comparison: the greedy tokens as chain graphs through ``amx_ctc_align_graph_emissions`` beside the same rows
    through ``amx_ctc_align_emissions`` (every output must agree bit for bit);
  * enumeration comparison: ``--positions`` (8) positions of each row get a second alternative; one graph call beside
    ``amx_ctc_align_emissions`` over the 2 ** positions enumerated sequences per row (one call of N rows per combination,
    which is what a caller without the graph aligner must do).  The graph's totals must equal the best enumerated totals
    bit for bit.

A timing is HIP events around ``--iters`` back-to-back calls after a warm-up; the two sides alternate ``--repeats`` times and
the median is reported with the smallest and largest repeat.  Prints one JSON line per comparison.

    python tools/align_graph_bench.py [--utterances 32] [--seconds 10] [--iters 20] [--repeats 7] [--positions 8]
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

from allophant_amd import alignment, graph_alignment, lib as L, synthetic  # noqa: E402
from allophant_amd.estimator import Batch, Estimator  # noqa: E402
from allophant_amd.graph_alignment import TargetGraph  # noqa: E402
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


def alternate(first, second, iters, repeats):
    """Per side the median, the smallest and the largest of `repeats` timings, taken alternately."""
    a, b = [], []
    for _ in range(repeats):
        a.append(timed(first, iters))
        b.append(timed(second, iters))
    summary = lambda v: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}  # noqa: E731
    return summary(a), summary(b), statistics.median(a) / statistics.median(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--phones", type=int, default=27)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--positions", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("align_graph_bench needs an MI355X: there is no CPU path to time")
    lib = L.load()
    device = torch.device("cuda:0")
    spec = build_spec(phones=args.phones)
    est = Estimator(spec, synthetic.make_state_dict(spec, seed=0), "cuda:0")
    audio, lengths = synthetic.make_audio(args.utterances, int(args.seconds * 16000), seed=1234)
    pred = est.predict(Batch(audio.cuda(), lengths, torch.zeros(args.utterances, dtype=torch.long)),
                       synthetic.make_inventory(spec, args.phones, seed=0))
    em = pred.outputs["phoneme"].transpose(0, 1)  # [N, T, C], read in place
    N, T, Cn = em.shape
    decoded = est.greedy_decode_device(pred)
    o = list(pred.outputs).index("phoneme")
    tokens, counts = decoded.tokens[o].cpu(), decoded.counts[o].cpu()
    targets = [tokens[n, :int(counts[n])].tolist() for n in range(N)]
    frame_lengths = pred.lengths.detach().to(device=device, dtype=torch.int32).contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def chain_call(rows, buffers, totals=None, status=None):
        offsets, ids, row_counts = alignment.pack_targets(rows)
        meta = torch.cat([offsets, ids, torch.zeros(1, dtype=torch.int32)]).to(device)
        width = buffers.spans.shape[1]
        assert max(row_counts) <= width
        pointers = list(buffers.pointers())
        if totals is not None:
            pointers[6], pointers[7] = p(totals), p(status)

        def call():
            code = lib.amx_ctc_align_emissions(0, p(em), em.stride(0), em.stride(1), p(frame_lengths), N, T, Cn, 0, p(meta),
                                               C.c_void_p(meta.data_ptr() + 4 * (N + 1)), width, *pointers, C.c_void_p(stream))
            assert code == L.AMX_OK, lib.amx_last_error(None)
        return call, meta

    def graph_call(graphs, buffers):
        packed, starts, node_counts = graph_alignment.pack_graphs(graphs)
        meta = packed.to(device)
        width = buffers.spans.shape[1]
        assert max(node_counts) <= width

        def call():
            code = lib.amx_ctc_align_graph_emissions(0, p(em), em.stride(0), em.stride(1), p(frame_lengths), N, T, Cn, 0,
                                                     *graph_alignment.graph_pointers(meta, starts), width, *buffers.pointers(),
                                                     C.c_void_p(stream))
            assert code == L.AMX_OK, lib.amx_last_error(None)
        return call, meta

    # ---- chains: the same rows through both kernels
    max_target = max(len(row) for row in targets)
    chain_buffers = alignment.allocate(lib, N, T, max_target, device)
    graph_buffers = graph_alignment.allocate(lib, N, T, max_target, device)
    for b in (chain_buffers, graph_buffers):
        b.paths.fill_(-7), b.spans.fill_(-7), b.status.fill_(-7)  # (what a call leaves untouched compares equal)
        b.frame_scores.fill_(-7.0), b.span_scores.fill_(-7.0), b.totals.fill_(-7.0)
    chains, keep_a = chain_call(targets, chain_buffers)
    graphs, keep_b = graph_call([TargetGraph.chain(row) for row in targets], graph_buffers)
    chains(), graphs()
    torch.cuda.synchronize()
    for name in ("paths", "frame_scores", "spans", "span_scores", "totals", "status"):
        assert torch.equal(getattr(chain_buffers, name), getattr(graph_buffers, name)), name
    graph_ms, chain_ms, ratio = alternate(graphs, chains, args.iters, args.repeats)
    print(json.dumps({"case": "chain_comparison", "rows": N, "frames": T, "classes": Cn, "max_target": max_target,
                      "mean_target": round(sum(len(r) for r in targets) / N, 1), "outputs_equal_bitwise": True,
                      "amx_ctc_align_graph": graph_ms, "amx_ctc_align": chain_ms, "graph_over_chain": round(ratio, 3),
                      "graph_workspace_mb": round(graph_buffers.size / 2 ** 20, 1),
                      "chain_workspace_mb": round(chain_buffers.size / 2 ** 20, 1)}))

    # ---- enumeration: `positions` two-way choices per row, one graph call against 2 ** positions chain calls
    K = args.positions
    other = lambda c: 1 + c % (Cn - 1)  # noqa: E731  (another non-blank class)
    chosen = [sorted({(2 * k + 1) * len(row) // (2 * K) for k in range(K)}) if row else [] for row in targets]
    slot_graphs = [TargetGraph.from_slots([[[c], [other(c)]] if j in chosen[n] else [[c]] for j, c in enumerate(row)]) if row
                   else TargetGraph.chain([]) for n, row in enumerate(targets)]
    combos = 2 ** K
    enumerated = []
    for g in range(combos):
        rows = []
        for n, row in enumerate(targets):
            taken = list(row)
            for bit, j in enumerate(chosen[n]):
                if (g >> bit) & 1:
                    taken[j] = other(row[j])
            rows.append(taken)
        enumerated.append(rows)
    width = max(len(g.classes) for g in slot_graphs)
    slot_buffers = graph_alignment.allocate(lib, N, T, width, device)
    all_totals = torch.full((combos, N), float("-inf"), dtype=torch.float32, device=device)
    all_status = torch.empty(combos, N, dtype=torch.int32, device=device)
    calls = [chain_call(rows, chain_buffers, all_totals[g], all_status[g]) for g, rows in enumerate(enumerated)]

    def enumerate_all():  # (the paths and spans of every combination land in the same buffers; the totals and status are kept)
        for call, _ in calls:
            call()

    one_graph, keep_c = graph_call(slot_graphs, slot_buffers)
    one_graph(), enumerate_all()
    torch.cuda.synchronize()
    best = torch.where(all_status == 0, all_totals, torch.full_like(all_totals, float("-inf"))).max(dim=0).values
    aligned = slot_buffers.status == 0
    assert bool(aligned.any()) and torch.equal(slot_buffers.totals[aligned].view(torch.int32), best[aligned].view(torch.int32))
    assert bool((best[~aligned] == float("-inf")).all())
    graph_ms, enum_ms, ratio = alternate(one_graph, enumerate_all, max(1, args.iters // 10), args.repeats)
    print(json.dumps({"case": "enumeration_comparison", "rows": N, "frames": T, "choices_per_row": K, "sequences_per_row": combos,
                      "graph_nodes_max": width, "totals_equal_bitwise": True, "amx_ctc_align_graph_one_call": graph_ms,
                      "amx_ctc_align_enumerated": enum_ms, "graph_over_enumeration": round(ratio, 5),
                      "graph_is_faster": graph_ms["max_ms"] < enum_ms["min_ms"]}))
    est.close()


if __name__ == "__main__":
    main()

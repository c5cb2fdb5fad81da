"""Times the feature-weighted edit kernels (amx_edit_weighted.hip) against the uniform ones on the same rows in the same run,
at the geometry of the benchmark's config 2 (the rows, labels and decoding of tools/edit_bench.py: 32 x 10 s utterances, every
output of the synthetic multitask model, greedy and beam 16 / n_best 4), with an attribute table of PHOIBLE's size (3300
phonemes by default, so the IPA outputs gather from a pairwise table of about 10 MB).  Every output gets a cost table -- the
IPA outputs the table's property rows, the attribute outputs one column of category ids -- so that every row of the weighted
launch pays the gather.  Prints one JSON line per measurement: HIP events around the C calls (statistics: score + select;
operations: candidate 0), uniform then weighted, and the one-off build of the cost tables next to the prediction step.  Run it
under ``rocprofv3 --kernel-trace --stats`` for the kernels' own times: edit_rows_kernel / edit_weighted_rows_kernel and
edit_ops_kernel / edit_weighted_ops_kernel get ``iters + 1`` dispatches per case, greedy first.

    python tools/edit_weighted_bench.py [--utterances 32] [--seconds 10] [--label-length 150] [--table-phonemes 3300] [--iters 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from allophant_amd import evaluation, synthetic  # noqa: E402
from allophant_amd.estimator import Batch, Estimator  # noqa: E402
from allophant_amd.evaluation import Evaluator, PropertyWeighting  # noqa: E402
from allophant_amd.phonetic import IPA_LAYERS, AttributeTable  # noqa: E402
from bench import build_spec  # noqa: E402
from edit_bench import synthetic_table, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--phones", type=int, default=27)
    ap.add_argument("--label-length", type=int, default=150)
    ap.add_argument("--table-phonemes", type=int, default=3300)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--insertion-cost", type=float, default=0.3)
    ap.add_argument("--deletion-cost", type=float, default=0.7)
    args = ap.parse_args()
    spec = build_spec(phones=args.phones)
    est = Estimator(spec, synthetic.make_state_dict(spec, seed=0), "cuda:0")
    tfi = synthetic.make_inventory(spec, args.phones, seed=0)
    audio, lengths = synthetic.make_audio(args.utterances, int(args.seconds * 16000), seed=1234)
    batch = Batch(audio.cuda(), lengths, torch.zeros(args.utterances, dtype=torch.long))
    pred = est.predict(batch, tfi)
    names = list(pred.outputs)
    step_ms = timed(lambda: est.predict(batch, tfi), 5)
    greedy = est.greedy_decode_device(pred)
    beam = est.beam_decode_device(pred, 16, n_best=4)
    torch.cuda.synchronize()
    est.close()

    features = [n for n in names if n not in IPA_LAYERS]
    phonemes = [f"p{k}" for k in range(max(args.phones, args.table_phonemes))]
    table = AttributeTable(synthetic_table(features, phonemes), names)
    inventory = phonemes[:args.phones]
    languages = ["lg0", "lg1"]
    rng = np.random.default_rng(7)
    N, O, G = args.utterances, len(names), len(languages)
    labels = [[phonemes[i] for i in rng.integers(0, len(phonemes), int(rng.integers(args.label_length - 20,
                                                                                     args.label_length + 21)))]
              for _ in range(N)]
    langs = [languages[n % 2] for n in range(N)]
    ev = Evaluator(table, names, inventory, languages)
    static = ev.encode_labels(labels, langs)
    device = ev.device

    # one cost table per output, in the order of its id space
    properties = table.property_table()
    weightings = [PropertyWeighting(args.insertion_cost, args.deletion_cost,
                                    properties if name in IPA_LAYERS else {s: [i] for s, i in ev.maps.spaces[o].items()})
                  for o, name in enumerate(names)]
    build = lambda: [w.cost_table(list(ev.maps.spaces[o]), device) for o, w in enumerate(weightings)]  # noqa: E731
    tables = build()
    build_ms = timed(build, 3)
    descriptors, first = [], 0
    for o, t in enumerate(tables):
        descriptors.append((first, len(ev.maps.spaces[o])))
        first += t.numel()
    weights = evaluation._Weights(weightings[0].insertion_cost, weightings[0].deletion_cost,
                                  torch.tensor(descriptors, dtype=torch.int64, device=device), torch.cat(tables))
    torch.cuda.synchronize()
    print(json.dumps({"case": "config2", "utterances": N, "outputs": O, "rows": N * O, "predict_step_ms": round(step_ms, 3),
                      "max_expected": static.max_expected, "table_phonemes": len(phonemes), "features": len(features),
                      "largest_table_symbols": max(v for _, v in descriptors), "cost_table_bytes": first,
                      "cost_tables_build_ms": round(build_ms, 3), "costs": [weights.insertion_cost, weights.deletion_cost]}))

    totals = torch.zeros(G, O, 4, dtype=torch.int64, device=device)
    for case, decoded in (("greedy", greedy), ("beam16_nbest4", beam)):
        tokens, counts = decoded.tokens, decoded.counts
        if tokens.dim() == 3:
            tokens, counts = tokens.unsqueeze(2), counts.unsqueeze(2)
        rows = ev._edit_rows(decoded, tokens, counts, static, None)
        max_actual = rows.max_actual
        workspace = [None]

        def statistics(w):
            out = evaluation._run(rows, workspace[0], totals, w)
            workspace[0] = out[2]
            return out

        uniform_ms = timed(lambda: statistics(None), args.iters)
        weighted_ms = timed(lambda: statistics(weights), args.iters)
        same = torch.equal(statistics(None)[0], statistics(weights)[0])
        candidate0 = rows.first()
        ops_workspace = [None]

        def operations(w):
            out = evaluation._run_operations(candidate0, ops_workspace[0], w)
            ops_workspace[0] = out[2]
            return out

        uniform_ops_ms = timed(lambda: operations(None), args.iters)
        weighted_ops_ms = timed(lambda: operations(weights), args.iters)
        records = operations(weights)[1]
        print(json.dumps({"case": case, "scored_rows": int((statistics(weights)[0][..., 0] >= 0).sum()),
                          "max_actual": max_actual, "statistics_ms_uniform": round(uniform_ms, 4),
                          "statistics_ms_weighted": round(weighted_ms, 4), "statistics_equal_to_uniform": same,
                          "operations_ms_uniform": round(uniform_ops_ms, 4), "operations_ms_weighted": round(weighted_ops_ms, 4),
                          "weighted_records": int(records.clamp(min=0).sum())}))


if __name__ == "__main__":
    main()

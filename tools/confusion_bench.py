"""Times the on-device confusion tables (amx_edit_confusion.hip, ``Evaluator(confusions=True)``) on the rows of
tools/edit_ops_bench.py: the benchmark's config 2 (32 x 10 s utterances, every output of the synthetic multitask model, 1216
(output, utterance) rows) against synthetic labels of about 150 phonemes, for greedy hypotheses and for the candidate that the
statistics chose from beam 16 / n_best 4.  Prints one JSON line per case:

  confusions_ms   HIP events around whole ``amx_edit_confusions`` calls (labels uploaded, ``best`` already computed), each call
                  adding the batch to the same table again, as a corpus would
  operations_ms   the same around ``Evaluator.operations`` (amx_edit_operations) on the same rows
  add_ms / add_with_confusions_ms   ``Evaluator.add`` without and with the confusion call behind it
  todays_route_ms the route without this kernel, wall time: ``Evaluator.operations``, the records fetched to the host, and
                  ``numpy.unique`` over (language, output, expected id, actual id) of every record.  It follows candidate 0 and
                  has no matches, so it is not the same table: it is what could be had before
  the table's occupancy (distinct keys / slots), events per batch, and ``fetch`` + decode time

    python tools/confusion_bench.py [--utterances 32] [--seconds 10] [--label-length 150] [--iters 20] [--capacity 1048576]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from allophant_amd import synthetic  # noqa: E402
from allophant_amd.estimator import Batch, Estimator  # noqa: E402
from allophant_amd.evaluation import Evaluator  # noqa: E402
from allophant_amd.phonetic import IPA_LAYERS, AttributeTable  # noqa: E402
from bench import build_spec  # noqa: E402
from edit_bench import synthetic_table, timed  # noqa: E402


def todays_route(ev, decoded, static, groups):
    """operations -> host -> numpy.unique: the table of candidate 0's operations (no matches)."""
    operations, counts = ev.operations(decoded, static)
    records, lengths = operations.cpu().numpy(), counts.cpu().numpy()
    O, N, max_ops, _ = records.shape
    valid = np.arange(max_ops)[None, None, :] < lengths[:, :, None]
    o, n, _ = np.nonzero(valid)
    picked = records[valid]
    keys = np.stack([groups[n], o, picked[:, 3], picked[:, 4]], axis=1)
    return np.unique(keys, axis=0, return_counts=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--phones", type=int, default=27)
    ap.add_argument("--label-length", type=int, default=150)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=2 ** 20)
    args = ap.parse_args()
    spec = build_spec(phones=args.phones)
    est = Estimator(spec, synthetic.make_state_dict(spec, seed=0), "cuda:0")
    tfi = synthetic.make_inventory(spec, args.phones, seed=0)
    audio, lengths = synthetic.make_audio(args.utterances, int(args.seconds * 16000), seed=1234)
    batch = Batch(audio.cuda(), lengths, torch.zeros(args.utterances, dtype=torch.long))
    pred = est.predict(batch, tfi)
    names = list(pred.outputs)
    greedy = est.greedy_decode_device(pred)
    beam = est.beam_decode_device(pred, 16, n_best=4)
    torch.cuda.synchronize()
    est.close()

    features = [n for n in names if n not in IPA_LAYERS]
    phonemes = [f"p{k}" for k in range(max(args.phones, 40))]
    table = AttributeTable(synthetic_table(features, phonemes), names)
    inventory = phonemes[:args.phones]
    languages = ["lg0", "lg1"]
    rng = np.random.default_rng(7)
    N = args.utterances
    labels = [[phonemes[i] for i in rng.integers(0, len(phonemes), int(rng.integers(args.label_length - 20,
                                                                                     args.label_length + 21)))]
              for _ in range(N)]
    langs = [languages[n % 2] for n in range(N)]
    groups = np.asarray([n % 2 for n in range(N)])
    print(json.dumps({"case": "config2", "utterances": N, "outputs": len(names), "rows": N * len(names),
                      "capacity": args.capacity}))

    for case, decoded in (("greedy", greedy), ("beam16_nbest4_chosen", beam)):
        plain = Evaluator(table, names, inventory, languages)
        ev = Evaluator(table, names, inventory, languages, confusions=args.capacity)
        static = ev.encode_labels(labels, langs)
        torch.cuda.synchronize()
        add_ms = timed(lambda: plain.add(decoded, static), args.iters)
        add_both_ms = timed(lambda: ev.add(decoded, static), args.iters)
        ops_ms = timed(lambda: ev.operations(decoded, static), args.iters)
        # the confusion call alone, on the rows and the `best` of the last add
        ev.reset()
        counts = ev._confusions[0][1]
        tokens, token_counts = decoded.tokens, decoded.counts
        if tokens.dim() == 3:
            tokens, token_counts = tokens.unsqueeze(2), token_counts.unsqueeze(2)
        rows = ev._edit_rows(decoded, tokens, token_counts, static, None)
        best = ev.rows()[1]
        call = lambda: counts.add_rows(rows, best)  # noqa: E731
        confusions_ms = timed(call, args.iters)
        row_events = call().cpu().numpy()
        added, dropped = counts.events()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        found = counts.fetch()
        fetch_s = time.perf_counter() - t0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keys, _ = todays_route(ev, decoded, static, groups)
        route_s = time.perf_counter() - t0
        print(json.dumps({"case": case, "rows": int(row_events.size), "rows_contributing": int((row_events >= 0).sum()),
                          "events_per_batch": int(row_events[row_events >= 0].sum()), "events_added": added,
                          "events_dropped": dropped, "distinct_keys": len(found),
                          "occupancy": round(len(found) / args.capacity, 6),
                          "confusions_ms": round(confusions_ms, 4), "operations_ms": round(ops_ms, 4),
                          "add_ms": round(add_ms, 4), "add_with_confusions_ms": round(add_both_ms, 4),
                          "fetch_ms": round(fetch_s * 1e3, 2), "todays_route_ms": round(route_s * 1e3, 1),
                          "todays_route_keys_no_matches": int(len(keys))}))


if __name__ == "__main__":
    main()

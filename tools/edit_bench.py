"""Times the on-device edit statistics (amx_edit.hip, Evaluator.add) at the geometry of the benchmark's config 2: 32 x 10 s
utterances, every output of the synthetic multitask model (1216 (output, utterance) rows), against synthetic labels of about
150 phonemes per utterance, for greedy hypotheses and for beam 16 / n_best 4.  The attribute table is synthetic too (every
model feature, three categories, one contour cell in eight).  Prints one JSON line per measurement with the expanded lengths
next to the times: the cost scales with m x n, and a random-weight model emits much longer hypotheses than a trained one.
The times are HIP events around whole ``Evaluator.add`` calls (labels pre-uploaded, and with host encoding + upload); run it
under ``rocprofv3 --kernel-trace --stats`` for the kernels' own times (edit_rows_kernel, edit_select_kernel: ``iters + 1``
dispatches per case, greedy first).  The last line is the literal Python restatement of upstream's back-trace
(tests/edit_util.py) on a sample of the same rows, scaled to the batch: a Python restatement, not upstream's Rust.

    python tools/edit_bench.py [--utterances 32] [--seconds 10] [--label-length 150] [--iters 20] [--host-rows 24]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from allophant_amd import synthetic  # noqa: E402
from allophant_amd.estimator import Batch, Estimator  # noqa: E402
from allophant_amd.evaluation import Evaluator  # noqa: E402
from allophant_amd.phonetic import IPA_LAYERS, AttributeTable  # noqa: E402
from bench import build_spec  # noqa: E402
import edit_util as E  # noqa: E402


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


def synthetic_table(features, phonemes, seed=0):
    rng = np.random.default_rng(seed)
    header = "InventoryID,Glottocode,ISO6393,LanguageName,SpecificDialect,GlyphID,Phoneme,Allophones,Marginal,SegmentClass,Source,tone,"
    lines = [header + ",".join(features)]
    values = ["+", "-", "0"]
    for k, p in enumerate(phonemes):
        cells = []
        for f in range(len(features)):
            cell = values[(k + f) % 3] if k < 3 else values[rng.integers(0, 3)]  # every category present in every column
            if rng.random() < 0.125:
                cell += "," + values[rng.integers(0, 3)]
            cells.append(f'"{cell}"')
        lines.append(f"1,glot,xxx,Language,,G{k},{p},{p},FALSE,segment,src,0," + ",".join(cells))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--phones", type=int, default=27)
    ap.add_argument("--label-length", type=int, default=150)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-rows", type=int, default=24)
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
    ev = Evaluator(table, names, inventory, languages)
    static = ev.encode_labels(labels, langs)
    torch.cuda.synchronize()
    print(json.dumps({"case": "config2", "utterances": N, "outputs": len(names), "rows": N * len(names),
                      "predict_step_ms": round(step_ms, 3), "max_expected": static.max_expected}))

    expanded = [sum(len(table.feature_contour(p, name)) if name not in IPA_LAYERS else 1 for p in label)
                for name in names for label in labels]
    for case, decoded in (("greedy", greedy), ("beam16_nbest4", beam)):
        kernel_ms = timed(lambda: ev.add(decoded, static), args.iters)
        with_labels_ms = timed(lambda: ev.add(decoded, labels, langs), args.iters)
        counts = decoded.counts.reshape(len(names) * N, -1).cpu().numpy().astype(np.int64)
        present = (decoded.hyp_counts.reshape(-1).cpu().numpy() if hasattr(decoded, "hyp_counts")
                   else np.ones(len(names) * N, dtype=np.int64))
        m = np.asarray(expanded, dtype=np.int64)
        scored = [(m[r], counts[r, k]) for r in range(len(m)) for k in range(int(present[r]))]
        cells = np.asarray([a * b for a, b in scored], dtype=np.int64)
        print(json.dumps({"case": case, "scored_rows": len(scored), "mean_expected": round(float(m.mean()), 1),
                          "mean_actual": round(float(np.mean([b for _, b in scored])), 1),
                          "max_actual": int(max(b for _, b in scored)), "mean_cells_per_row": int(cells.mean()),
                          "total_cells": int(cells.sum()), "add_ms_labels_uploaded": round(kernel_ms, 4),
                          "add_ms_with_label_encoding": round(with_labels_ms, 4)}))

    # the literal Python restatement on a sample of the greedy rows, scaled to the batch
    tokens = greedy.tokens.cpu().numpy()
    gcounts = greedy.counts.cpu().numpy()
    sample = rng.choice(len(names) * N, size=min(args.host_rows, len(names) * N), replace=False)
    pairs = []
    for r in sample:
        o, n = divmod(int(r), N)
        a = ev.maps.expand_label(o, labels[n])
        b = ev.maps.expand_tokens(o, 0, tokens[o, n, :gcounts[o, n]])
        pairs.append((a, b))
    t0 = time.perf_counter()
    for a, b in pairs:
        E.levensthein_statistics(a, b)
    host_s = time.perf_counter() - t0
    sample_cells = sum(len(a) * len(b) for a, b in pairs)
    print(json.dumps({"case": "host_python_restatement_greedy", "sampled_rows": len(pairs), "sampled_cells": sample_cells,
                      "ns_per_cell": round(host_s / max(1, sample_cells) * 1e9, 1),
                      "batch_estimate_s": round(host_s / len(pairs) * len(names) * N, 2)}))


if __name__ == "__main__":
    main()

"""Times the on-device edit operations (amx_edit_ops.hip, Evaluator.operations / Evaluator.edits) at the geometry of the
benchmark's config 2: 32 x 10 s utterances, every output of the synthetic multitask model (1216 (output, utterance) rows),
against synthetic labels of about 150 phonemes per utterance (the tables and labels of tools/edit_bench.py), for greedy
hypotheses and for the first candidate of beam 16 / n_best 4.  Prints one JSON line per measurement: HIP events around whole
``Evaluator.operations`` calls (labels pre-uploaded), the wall time of ``Evaluator.edits`` (one host synchronisation, the
records as ``UtteranceEdits``) plus ``to_json`` of every record, and the workspace size.  Run it under
``rocprofv3 --kernel-trace --stats`` for the kernel's own time (edit_ops_kernel: ``iters + 3`` dispatches per case, greedy
first; edit_rows_kernel: ``iters + 1`` per case, for comparison: the same rows for greedy, all four candidates for beam).  The last line is the literal Python
restatement of upstream's ``levensthein_operations`` + ``to_substitutions`` (tests/edit_ops_util.py) on a sample of the same
rows, scaled to the batch: a Python restatement, not upstream's Rust.

    python tools/edit_ops_bench.py [--utterances 32] [--seconds 10] [--label-length 150] [--iters 20] [--host-rows 24]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from allophant_amd import lib, synthetic  # noqa: E402
from allophant_amd.estimator import Batch, Estimator  # noqa: E402
from allophant_amd.evaluation import Evaluator  # noqa: E402
from allophant_amd.phonetic import IPA_LAYERS, AttributeTable  # noqa: E402
from bench import build_spec  # noqa: E402
from edit_bench import synthetic_table, timed  # noqa: E402
import edit_ops_util as U  # noqa: E402


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
    ids = [f"utt{n}" for n in range(N)]
    ev = Evaluator(table, names, inventory, languages)
    static = ev.encode_labels(labels, langs)
    torch.cuda.synchronize()
    print(json.dumps({"case": "config2", "utterances": N, "outputs": len(names), "rows": N * len(names),
                      "predict_step_ms": round(step_ms, 3), "max_expected": static.max_expected}))

    for case, decoded in (("greedy", greedy), ("beam16_nbest4_first", beam)):
        ev.add(decoded, static)  # the statistics kernel on the same rows (its time is in the kernel trace)
        for _ in range(args.iters):
            ev.add(decoded, static)
        ops_ms = timed(lambda: ev.operations(decoded, static), args.iters)
        T = decoded.tokens.shape[-1]
        max_actual = min(T * ev.maps.hyp_fanout, lib.EDIT_MAX_LENGTH)
        size = C.c_size_t()
        lib.load().amx_edit_operations_workspace(N * len(names), static.max_expected, max_actual, C.byref(size))
        _, counts = ev.operations(decoded, static)
        cost = counts.cpu().numpy()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        edits = ev.edits(decoded, labels, langs, ids)
        edits_s = time.perf_counter() - t0
        lines = [e.to_json() for e in edits]
        total_s = time.perf_counter() - t0
        print(json.dumps({"case": case, "rows": int(cost.size), "operations": int(cost.sum()), "mean_cost": round(float(cost.mean()), 1),
                          "max_cost": int(cost.max()), "max_actual": max_actual, "workspace_mb": round(size.value / 1e6, 1),
                          "operations_ms_labels_uploaded": round(ops_ms, 4), "edits_ms": round(edits_s * 1e3, 1),
                          "edits_plus_to_json_ms": round(total_s * 1e3, 1), "json_bytes": sum(map(len, lines))}))

    # the literal Python restatement on a sample of the greedy rows, scaled to the batch
    tokens = greedy.tokens.cpu().numpy()
    gcounts = greedy.counts.cpu().numpy()
    sample = rng.choice(len(names) * N, size=min(args.host_rows, len(names) * N), replace=False)
    pairs = []
    for r in sample:
        o, n = divmod(int(r), N)
        pairs.append((ev.maps.expand_label(o, labels[n]), ev.maps.expand_tokens(o, 0, tokens[o, n, :gcounts[o, n]])))
    t0 = time.perf_counter()
    for a, b in pairs:
        U.levensthein_substitutions(a, b)
    host_s = time.perf_counter() - t0
    sample_cells = sum(len(a) * len(b) for a, b in pairs)
    print(json.dumps({"case": "host_python_restatement_greedy", "sampled_rows": len(pairs), "sampled_cells": sample_cells,
                      "ns_per_cell": round(host_s / max(1, sample_cells) * 1e9, 1),
                      "batch_estimate_s": round(host_s / len(pairs) * len(names) * N, 2)}))


if __name__ == "__main__":
    main()

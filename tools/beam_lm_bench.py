"""Times the CTC beam search with a phonotactic language model (amx_ctc_beam_lm.hip) beside the decoder without one
(amx_ctc_beam.hip) on the same rows: the phoneme output of the benchmark's config 2 (32 x 10 s utterances, its [T, N, C]
block read in place) at beam 16 / n_best 4, under three decoders -- the existing kernel, the language-model kernel at
weight 0, and the language-model kernel under a random bigram -- and one 60 s row (2999 frames of random log-probabilities
over the same classes).  Prints one JSON line per measurement with the ratio to the existing kernel.  The times are HIP
events around the device calls (``_beam_ctc_rows``: allocations and one launch, no copy to the host).

    python tools/beam_lm_bench.py [--utterances 32] [--seconds 10] [--beam 16] [--n-best 4] [--iters 10]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from allophant_amd import spec as S, synthetic  # noqa: E402
from allophant_amd.estimator import Batch, Estimator, _beam_ctc_rows  # noqa: E402
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


def measure(case, emissions, lengths, beam, n_best, iters):
    N, T, C = emissions.shape
    g = torch.Generator().manual_seed(C)
    table = torch.log_softmax(torch.randn(1, C + 1, C + 1, generator=g) * 3.0, -1).cuda()
    ids = torch.zeros(N, dtype=torch.int32)
    for exp in (True, False):
        plain = timed(lambda: _beam_ctc_rows(emissions, lengths, beam, n_best, 0, exp), iters)
        zero = timed(lambda: _beam_ctc_rows(emissions, lengths, beam, n_best, 0, exp, (table, ids, 0.0, 0.0)), iters)
        fused = timed(lambda: _beam_ctc_rows(emissions, lengths, beam, n_best, 0, exp, (table, ids, 1.0, 0.0)), iters)
        print(json.dumps({"case": case, "rows": N, "frames": T, "classes": C, "beam": beam, "n_best": n_best,
                          "emissions": "exp" if exp else "log", "plain_ms": round(plain, 3), "lm_weight0_ms": round(zero, 3),
                          "lm_bigram_ms": round(fused, 3), "ratio_weight0": round(zero / plain, 2),
                          "ratio_bigram": round(fused / plain, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--phones", type=int, default=27)
    ap.add_argument("--beam", type=int, default=16)
    ap.add_argument("--n-best", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    spec = build_spec(phones=args.phones)
    est = Estimator(spec, synthetic.make_state_dict(spec, seed=0), "cuda:0")
    tfi = synthetic.make_inventory(spec, args.phones, seed=0)
    audio, lengths = synthetic.make_audio(args.utterances, int(args.seconds * 16000), seed=1234)
    pred = est.predict(Batch(audio.cuda(), lengths, torch.zeros(args.utterances, dtype=torch.long)), tfi)
    block = pred.outputs[S.PHONEME]  # [T, N, C]
    measure("config2_phoneme", block.transpose(0, 1), pred.lengths, args.beam, args.n_best, args.iters)
    C = block.shape[2]
    est.close()
    g = torch.Generator().manual_seed(0)
    long_row = torch.log_softmax(torch.randn(1, 2999, C, generator=g) * 3.0, -1).cuda()
    measure("row_60s", long_row, torch.tensor([2999]), args.beam, args.n_best, args.iters)


if __name__ == "__main__":
    main()

"""Times ``Estimator.map_allophones`` (amx_allophone.hip) at the size of a 10 s batch of an allophone-layer model, and the
reference's algorithm (``AllophoneMapping.map_allophones``: per utterance the dense [T, P+1, Q+1] product, masked fill, max)
restated in torch on the same GPU.  Prints one JSON line; run it under ``rocprofv3 --kernel-trace --stats`` for the kernel's
own time.

    python tools/allophone_bench.py [--utterances 32] [--frames 499] [--phones 1025] [--phonemes 769] [--languages 8]
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
from allophant_amd.allophones import build_structure  # noqa: E402
from allophant_amd.estimator import ALLOPHONE_MATRICES_KEY, Estimator  # noqa: E402


def reference_algorithm(x, matrices, mask, ids):
    out = torch.empty(*x.shape[:2], matrices.shape[2], device=x.device)
    for n, lang in enumerate(ids):
        product = (x[:, n].unsqueeze(-1) * matrices[lang].unsqueeze(0)).masked_fill_(mask[lang].unsqueeze(0), torch.finfo(torch.float32).min)
        out[:, n] = product.max(1).values
    return out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--frames", type=int, default=499)
    ap.add_argument("--phones", type=int, default=1025)
    ap.add_argument("--phonemes", type=int, default=769)
    ap.add_argument("--languages", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    N, T, P1, Q1, L = args.utterances, args.frames, args.phones, args.phonemes, args.languages
    g = torch.Generator().manual_seed(0)
    allophones = {}
    for lang in range(L):
        per = {}
        for q in range(Q1 - 1):
            k = int(torch.randint(0, 6, (1,), generator=g))
            if k:
                per[q] = torch.randperm(P1 - 1, generator=g)[:k].tolist()
        allophones[lang] = per
    mapping = {"allophones": allophones, "languages": [f"l{i}" for i in range(L)], "shared_phones": [str(i) for i in range(P1 - 1)]}
    structure = build_structure(mapping, P1, Q1)
    values = structure.initialization + 0.3 * torch.randn(L, P1, Q1, generator=g)
    spec = S.multitask_spec(S.tiny_encoder(1), ["syllabic"], embedding_size=None, train_phonemes=Q1 - 1, allophone_layer=True)
    spec["shared_phones"] = P1 - 1
    state = synthetic.make_state_dict(spec, seed=1)
    state[ALLOPHONE_MATRICES_KEY] = values
    est = Estimator(spec, state, "cuda:0")
    est.set_allophones(mapping)
    x = torch.randn(T, N, P1, generator=g).log_softmax(-1).cuda()
    ids = [n % L for n in range(N)]
    ms = timed(lambda: est.map_allophones(x, ids), args.iters)
    matrices, mask = values.cuda(), structure.mask.cuda()
    ref_ms = timed(lambda: reference_algorithm(x, matrices, mask, ids), 3)
    same = torch.equal(torch.nan_to_num(est.map_allophones(x, ids)), torch.nan_to_num(reference_algorithm(x, matrices, mask, ids)))
    moved = 4 * (T * N * (P1 + Q1))
    print(json.dumps({"utterances": N, "frames": T, "phones": P1, "phonemes": Q1, "languages": L,
                      "map_allophones_ms": round(ms, 4), "bytes_moved": moved, "effective_tb_s": round(moved / (ms * 1e-3) / 1e12, 3),
                      "torch_reference_ms": round(ref_ms, 3), "bitwise_equal": same}))
    est.close()


if __name__ == "__main__":
    main()

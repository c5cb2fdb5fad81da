"""Times the on-device CTC search (amx_ctc_search.hip) and sets no threshold:

  * the phoneme output of the benchmark's config 2 -- 32 x 10 s utterances -- searched for Q in {1, 64, 1024} queries of 3 to
    12 phonemes, drawn from slices of the batch's own greedy tokens, through ``amx_ctc_search_emissions`` on prepared
    buffers, with and without the curves, and through ``Estimator.search_device`` (with its allocations and query upload);
  * ``amx_ctc_align_emissions`` on the 32 phoneme rows against their greedy tokens from the same build, and the numpy restatement
    (``tests/ctc_search_util.py``, the frame-at-a-time sweep) per row, beside them;
  * one 60 s row (2999 frames) with a 256-phoneme query.

Prints one JSON line per measurement and writes the same lines to ``--log`` (``profiles/ctc_search.log``).  The device times are HIP events around whole calls (the pre-pass and the search
kernel together).  Run it under ``rocprofv3 --kernel-trace --stats`` for the kernels' own times.

    python tools/search_bench.py [--utterances 32] [--seconds 10] [--iters 5] [--host-rows 8] [--log profiles/ctc_search.log]
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

from allophant_amd import alignment, lib as L, search, synthetic  # noqa: E402
from allophant_amd.estimator import Batch, Estimator  # noqa: E402
from bench import build_spec  # noqa: E402
import ctc_search_util as U  # noqa: E402


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


class Prepared:
    """The buffers of one amx_ctc_search_emissions call."""

    def __init__(self, lib, em, lengths, queries, curves):
        self.lib, self.em = lib, em
        N, T, self.classes = em.shape
        self.N, self.T, self.Q = N, T, len(queries)
        dev = em.device
        offsets, ids = search.pack_queries(queries, self.classes, 0)
        self.meta = torch.cat([offsets, ids]).to(dev)
        self.lengths = lengths.to(device=dev, dtype=torch.int32)
        self.max_query = max(len(q) for q in queries)
        size = C.c_size_t()
        assert lib.amx_ctc_search_workspace(N, self.Q, T, self.max_query, C.byref(size)) == L.AMX_OK
        self.size = size.value
        self.workspace = torch.empty(max(1, size.value), dtype=torch.uint8, device=dev)
        self.scores = torch.empty(N, self.Q, dtype=torch.float32, device=dev)
        self.spans = torch.empty(N, self.Q, 2, dtype=torch.int32, device=dev)
        self.status = torch.empty(N, self.Q, dtype=torch.int32, device=dev)
        self.end_scores = torch.empty(N, self.Q, T, dtype=torch.float32, device=dev) if curves else None
        self.end_starts = torch.empty(N, self.Q, T, dtype=torch.int32, device=dev) if curves else None
        self.stream = torch.cuda.current_stream().cuda_stream

    def __call__(self):
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        code = self.lib.amx_ctc_search_emissions(
            0, p(self.em), self.em.stride(0), self.em.stride(1), p(self.lengths), self.N, self.T, self.classes, 0, p(self.meta),
            C.c_void_p(self.meta.data_ptr() + 4 * (self.Q + 1)), self.Q, self.max_query, p(self.workspace), self.size,
            p(self.scores), p(self.spans), p(self.status), p(self.end_scores), p(self.end_starts), C.c_void_p(self.stream))
        assert code == L.AMX_OK, self.lib.amx_last_error(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--phones", type=int, default=27)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=8)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "ctc_search.log"))
    args = ap.parse_args()
    log = open(args.log, "w", encoding="utf-8")

    def report(**fields):
        line = json.dumps(fields)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    report(case="run", device=torch.cuda.get_device_name(0), boxes=1, iters=args.iters,
           command="python tools/search_bench.py " + " ".join(sys.argv[1:]))
    lib = L.load()
    spec = build_spec(phones=args.phones)
    est = Estimator(spec, synthetic.make_state_dict(spec, seed=0), "cuda:0")
    tfi = synthetic.make_inventory(spec, args.phones, seed=0)
    audio, lengths = synthetic.make_audio(args.utterances, int(args.seconds * 16000), seed=1234)
    batch = Batch(audio.cuda(), lengths, torch.zeros(args.utterances, dtype=torch.long))
    pred = est.predict(batch, tfi)
    names = list(pred.outputs)
    o = names.index("phoneme")
    view = pred.outputs["phoneme"].transpose(0, 1)  # [N, T, C], read in place
    N, T, classes = view.shape
    decoded = est.greedy_decode_device(pred)
    tokens, counts = decoded.tokens.cpu(), decoded.counts.cpu()
    greedy = [tokens[o, n, :int(counts[o, n])].tolist() for n in range(N)]
    rng = np.random.default_rng(0)

    def draw(count):
        out = []
        while len(out) < count:
            row = greedy[int(rng.integers(0, N))]
            size = int(rng.integers(3, 13))
            if len(row) >= size:
                at = int(rng.integers(0, len(row) - size + 1))
                out.append(row[at:at + size])
        return out

    report(**{"case": "config2_phoneme", "utterances": N, "frames": T, "classes": classes,
                      "mean_greedy_tokens": round(float(np.mean([len(r) for r in greedy])), 1)})
    host = view.cpu().numpy()
    frame_lengths = [int(v) for v in pred.lengths]
    for Q in (1, 64, 1024):
        queries = draw(Q)
        bare, curved = Prepared(lib, view, pred.lengths, queries, False), Prepared(lib, view, pred.lengths, queries, True)
        bare_ms, curves_ms = timed(bare, args.iters), timed(curved, args.iters)
        facade_ms = timed(lambda: est.search_device(pred, queries, "phoneme"), args.iters)
        status = bare.status.cpu()
        ok = bare.status == 0  # (the entries of the other rows are not written)
        assert torch.equal(bare.status, curved.status) and torch.equal(bare.scores[ok], curved.scores[ok])
        assert torch.equal(bare.spans[ok], curved.spans[ok])
        found, exact = int((status == 0).sum()), int(((status == 0) & (bare.scores.cpu() == 0.0)).sum())
        # the numpy restatement on a sample of rows (the output is copied to the host first, which is not timed)
        host_ms = []
        for k in range(min(args.host_rows, Q)):
            n = k % N
            t0 = time.perf_counter()
            row = U.search_row(host[n, :frame_lengths[n]], queries[k], fast=True)
            host_ms.append((time.perf_counter() - t0) * 1e3)
            assert row.status == int(status[n, k])
            assert row.status != 0 or (np.float32(row.best_score) == bare.scores[n, k].cpu().numpy() and list(row.best_span) == bare.spans[n, k].tolist())
        report(**{"case": "config2_search", "queries": Q, "rows": N * Q, "frames": T, "found_rows": found,
                          "score_0_rows": exact, "amx_ctc_search_emissions_ms": round(bare_ms, 4),
                          "with_curves_ms": round(curves_ms, 4), "search_device_ms": round(facade_ms, 3),
                          "curves_mb": round(N * Q * T * 8 / 2 ** 20, 1), "host_restatement_ms_per_row": round(float(np.mean(host_ms)), 3),
                          "host_ms_for_all_rows_at_that_rate": round(float(np.mean(host_ms)) * N * Q, 1)})

    # amx_ctc_align_emissions on the 32 phoneme rows against their greedy tokens, from the same build
    max_target = max(len(r) for r in greedy)
    stream = torch.cuda.current_stream().cuda_stream
    phoneme = view.contiguous()
    p_offsets, p_ids, _ = alignment.pack_targets(greedy)
    p_meta = torch.cat([p_offsets, p_ids, torch.zeros(1, dtype=torch.int32)]).cuda()
    pb = alignment.allocate(lib, N, T, max_target, torch.device("cuda:0"))
    lengths_dev = pred.lengths.to(device="cuda", dtype=torch.int32)

    def align_phoneme():
        code = lib.amx_ctc_align_emissions(0, C.c_void_p(phoneme.data_ptr()), phoneme.stride(0), phoneme.stride(1),
                                           C.c_void_p(lengths_dev.data_ptr()), N, T, classes, 0, C.c_void_p(p_meta.data_ptr()),
                                           C.c_void_p(p_meta.data_ptr() + 4 * (N + 1)), max_target, *pb.pointers(), C.c_void_p(stream))
        assert code == L.AMX_OK, lib.amx_last_error(None)

    report(**{"case": "config2_align_beside", "phoneme_rows": N, "max_target": max_target,
                      "amx_ctc_align_emissions_ms": round(timed(align_phoneme, args.iters), 4)})
    est.close()

    # one 60 s row (50 frames a second) with a 256-phoneme query
    frames, wide, count = 60 * 50 - 1, 64, 256
    g = torch.Generator().manual_seed(0)
    em = torch.log_softmax(torch.randn(1, frames, wide, generator=g) * 3.0, -1).cuda()
    query = []
    while len(query) < count:
        v = int(rng.integers(1, wide))
        if not query or v != query[-1]:
            query.append(v)
    one = torch.tensor([frames])
    bare, curved = Prepared(lib, em, one, [query], False), Prepared(lib, em, one, [query], True)
    bare_ms, curves_ms = timed(bare, args.iters), timed(curved, args.iters)
    t0 = time.perf_counter()
    want = U.search_row(em[0].cpu().numpy(), query, fast=True)
    host_long_ms = (time.perf_counter() - t0) * 1e3
    assert int(bare.status.cpu()[0, 0]) == want.status == 0 and np.float32(want.best_score) == bare.scores.cpu().numpy()[0, 0]
    assert np.array_equal(curved.end_scores.cpu().numpy()[0, 0].view(np.int32), want.end_scores.view(np.int32))
    report(**{"case": "long_row", "frames": frames, "query": count, "classes": wide,
                      "amx_ctc_search_emissions_ms": round(bare_ms, 4), "with_curves_ms": round(curves_ms, 4),
                      "host_restatement_ms": round(host_long_ms, 1)})


if __name__ == "__main__":
    main()

"""On-device timing of the attention adapters (``adapter_attn_dim``: the fine-tuned MMS encoders).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iallophant_amd/csrc -Iinclude -o build/attn_adapter_probe tools/attn_adapter_probe.hip \
          -Lallophant_amd -lallophant_amx -Wl,-rpath,'$ORIGIN/../allophant_amd'
    python tools/attn_adapter_bench.py [--batch 32] [--seconds 10] [--layers 4] [--dim 16] [--precision f16x3] [--steps 10]

Two measurements, for ``batch`` utterances of ``seconds`` at XLS-R 1B width (hidden 1280):

1. kernels (``build/attn_adapter_probe``, a child process): the adapter launch with the next layer's planes, the last layer's
   (no planes), and ``launch_rownorm`` with unit gamma on the same rows -- the launch at the top of the next layer that an
   adapter model does not issue.  By bytes the adapter (4 read + 4 written back + planes) should stay near 1.5 x the row pass
   (4 read + planes).
2. the whole ``predict`` step of a ``layers``-layer model with and without adapters (HIP events around ``steps`` steps after a
   warm-up), and the per-class kernel time of both (``AMX_FLAG_TIMING``).  The model without adapters folds its LayerNorms at this
   geometry (``ln_fold`` 1) and the adapter model does not, so the difference is the adapters PLUS the row passes the fold saves.

Prints one JSON line per measurement.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PROBE = os.path.join(ROOT, "build", "attn_adapter_probe")


def kernels(rows, hidden, dim, precision, iterations):
    from allophant_amd import lib

    if not os.path.exists(PROBE):
        raise SystemExit(f"{PROBE} not found: build it first (the hipcc line in this file's docstring)")
    out = subprocess.run([PROBE, str(rows), str(hidden), str(dim), str(lib.PRECISIONS[precision]), str(iterations)], check=True,
                         capture_output=True, text=True, timeout=300).stdout
    return json.loads(out.strip().splitlines()[-1])


def steps(args, dim):
    import torch

    from allophant_amd import spec as S, synthetic
    from allophant_amd.estimator import Batch, Estimator

    encoder = dict(S.xlsr_1b_encoder(), layers=args.layers)
    if dim:
        encoder["adapter_attn_dim"] = dim
    spec = S.multitask_spec(encoder, ["syllabic", "long"])
    state = synthetic.make_state_dict(spec, seed=0)
    tfi = synthetic.make_inventory(spec, 27, seed=0)
    audio, lengths = synthetic.make_audio(args.batch, int(args.seconds * 16000), seed=1234)
    est = Estimator(spec, state, "cuda:0", args.precision)
    try:
        batch = Batch(audio.cuda(), lengths, torch.zeros(args.batch, dtype=torch.long))
        pred = est.predict(batch, tfi)
        for _ in range(args.warmup):
            pred = est.predict(batch, tfi, _out=pred._flat)
        info = est.pass_info()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        begin.record()
        for _ in range(args.steps):
            pred = est.predict(batch, tfi, _out=pred._flat)
        end.record()
        torch.cuda.synchronize()
        step_ms = begin.elapsed_time(end) / args.steps
        est.timing_fetch()
        for _ in range(args.steps):
            est.predict(batch, tfi, _timing=True, _out=pred._flat)
        classes = {k: (round(ms / args.steps, 4), n // args.steps) for k, (ms, n) in est.timing_fetch().items() if n}
        est.check_finite()
    finally:
        est.close()
    return {"adapter_dim": dim, "layers": args.layers, "batch": args.batch, "seconds": args.seconds, "precision": args.precision,
            "rows": info["rows"], "ln_fold": info["ln_fold"], "graph": info["graph"], "step_ms": round(step_ms, 4),
            "kernel_ms_and_launches_per_step": classes}


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--batch", type=int, default=32)
    parser.add_argument("--seconds", type=float, default=10.0)
    parser.add_argument("--layers", type=int, default=4)
    parser.add_argument("--dim", type=int, default=16)
    parser.add_argument("--precision", default="f16x3")
    parser.add_argument("--steps", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--iterations", type=int, default=50, help="launches per kernel measurement")
    args = parser.parse_args()
    from allophant_amd import spec as S

    encoder = S.xlsr_1b_encoder()
    frames = S.frame_lengths([int(args.seconds * 16000)], encoder)[0]
    # (the probe runs as a child process before this one touches the device)
    print(json.dumps({"kernels": kernels(args.batch * frames, encoder["hidden"], args.dim, args.precision, args.iterations)}), flush=True)
    with_adapters = steps(args, args.dim)
    print(json.dumps({"step_with_adapters": with_adapters}), flush=True)
    without = steps(args, 0)
    print(json.dumps({"step_without_adapters": without}), flush=True)
    print(json.dumps({"adapters_cost_ms_per_layer": round((with_adapters["step_ms"] - without["step_ms"]) / args.layers, 4)}))


if __name__ == "__main__":
    main()

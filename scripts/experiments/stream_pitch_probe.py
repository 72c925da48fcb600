"""What per-frame pitch control costs a streaming tick (BASELINE config 5: 64 streams, the 80 ms schedule 6 / 6 / 7 / 6 / 7).

Measures the steady tick of the canonical SPEECH model -- device time (HIP events around the tick's launches, copies
included) and host-inclusive time, p50 / p99 -- in four set-ups on the same build:

    none     no stream ever uses control: the tick passes none of the control arguments (the launch sequence of bench.py)
    scale    every stream pushes a transposition contour: + f0_control_kernel, + 2 x (64, window) floats in the staged upload
    frames   every stream is opened with f0="frames" and pushes a contour too (the F0-net still runs: the driver always
             passes a mask, so that the ring's F0 lane stays whole)
    mixed    half the streams as in "frames", the other half without any control

Every set-up runs in a child process of its own under its own time limit; the first one that fails or runs out of time ends
the probe.  The parent never touches the GPU.

    python scripts/experiments/stream_pitch_probe.py [--steps 200] [--streams 64] [--timeout 240]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
MODES = ("none", "scale", "frames", "mixed")
SCHEDULE = (6, 6, 7, 6, 7)


def measure(mode, n_streams, steps, warmup):
    import torch
    from bench import build_engine, synthetic_batch
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    cfg, raw, wt, dims, eng = build_engine("SPEECH")
    syn = StreamingSynthesizer(eng, chunk_frames=list(SCHEDULE))
    syn.time_device = True
    steps = steps // len(SCHEDULE) * len(SCHEDULE)
    lead = 6 * len(SCHEDULE)                     # left context, one period recorded, one captured, three to settle (bench.py)
    n_ticks = lead + warmup + steps
    total = sum(SCHEDULE[ii % len(SCHEDULE)] for ii in range(n_ticks + 1)) + syn.right + 8
    rng = np.random.default_rng(7)
    for sid in range(n_streams):
        frames = mode == "frames" or (mode == "mixed" and sid % 2 == 0)
        scaled = mode == "scale" or frames
        syn.open(sid, f0="frames" if frames else "net")
        mm, nn = synthetic_batch(np.random.default_rng(1000 + sid), 1, total, dims.steps_per_frame)
        tt = np.arange(total)
        syn.push(sid, mm[0], nn[0],
                 f0=(180.0 + 40.0 * np.sin(2.0 * np.pi * tt / 57.0 + sid)).astype(np.float32) if frames else None,
                 transposition=(1.0 + 0.06 * np.sin(2.0 * np.pi * tt / 9.0 + sid)).astype(np.float32) if scaled else None)
    dev_ms, host_ms = [], []
    for tick in range(n_ticks):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        res = syn.tick()
        torch.cuda.synchronize()
        assert len(res) == n_streams
        if tick >= lead + warmup:
            host_ms.append((time.perf_counter() - t1) * 1e3)
            dev_ms.append(syn.last_tick_device_ms)
    return {"mode": mode, "streams": n_streams, "ticks": steps, "ticks_replayed_as_graph": int(syn.graph_ticks),
            "control_arguments_passed": bool(syn._control),
            "tick_ms_device_p50": float(np.percentile(dev_ms, 50)), "tick_ms_device_p99": float(np.percentile(dev_ms, 99)),
            "tick_ms_host_inclusive_p50": float(np.percentile(host_ms, 50)),
            "tick_ms_host_inclusive_p99": float(np.percentile(host_ms, 99))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per set-up")
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.child, args.streams, args.steps, args.warmup)), flush=True)
        return 0
    lines = []
    for mode in args.modes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--steps", str(args.steps), "--warmup",
               str(args.warmup), "--streams", str(args.streams)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"stream_pitch_probe: set-up {mode!r} ran out of its {args.timeout} s; stopping", file=sys.stderr)
            return 1
        if res.returncode != 0:
            print(f"stream_pitch_probe: set-up {mode!r} failed ({res.returncode}); stopping\n{res.stderr[-2000:]}", file=sys.stderr)
            return 1
        line = res.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

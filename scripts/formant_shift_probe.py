#!/usr/bin/env python3
"""What the formant shift costs on the device: the 16 x 10 s step and the 64-stream tick of the 80 ms
schedule on the canonical SPEECH model, in three variants --

    parent    a built tree of the commit before the formant shift (--parent-tree DIR; left out when none is given)
    plain     this tree, no factor anywhere: the launch sequence of the parent, so it has to time like the parent
    formant   this tree, a factor on every frame of every item / stream (one more launch per forward)

Every variant runs in a fresh child process of its own (one engine, one HIP context at a time; this parent never touches
the GPU), and the variants alternate: ROUNDS times parent, plain, formant.  A child times the step between two HIP events
per call and the tick with the streaming driver's own device timer, after warming both up, and prints one JSON line.  The
parent of the children gathers the medians of every round: the spread of a variant between its rounds is the run-to-run
spread of this probe, against which the difference between parent and plain is to be read.  The formant child also times
the kernel alone (mbxe_warp_envelope on the step's shape).  Writes the result as JSON (--out) and prints it.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULE = (6, 6, 7, 6, 7)


def percentiles(values):
    return {"p50": float(np.percentile(values, 50)), "p10": float(np.percentile(values, 10)),
            "p90": float(np.percentile(values, 90)), "n": len(values)}


def synthetic_batch(rng, batch, frames, steps_per_frame):
    mell = np.log(np.exp(rng.normal(-5.0, 2.0, size=(batch, frames, 80))) + 1e-5)
    return (np.clip(mell, -11.5, 2.0).astype(np.float32), rng.normal(size=(batch, frames * steps_per_frame)).astype(np.float32))


def factor_rows(rng, batch, frames):
    """per-frame factors between 0.8 and 1.25 that change with every frame"""
    phase = rng.uniform(size=(batch, 1))
    return (1.0 + 0.22 * np.sin(2.0 * np.pi * (np.arange(frames)[None, :] / 17.0 + phase))).astype(np.float32)


def child(args):
    """One variant in this process, from the tree args.root: {"step_ms": [...], "tick_ms": [...], ...} as one JSON line."""
    sys.path.insert(0, args.root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("formant_shift_probe.py: no GPU available; a timing taken without one says nothing")
    from mbexwn_vocoder_amd.config import ModelDims, canonical_config
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    from mbexwn_vocoder_amd.tables import WaveTables
    from mbexwn_vocoder_amd.weights import synthetic_weights
    shifted = args.child == "formant"
    cfg = canonical_config("SPEECH")
    dims = ModelDims(cfg)
    eng = MBExWNEngine(cfg, synthetic_weights(cfg, seed=1234),
                       WaveTables(sample_rate=dims.pulse_rate, **cfg["mbexwn_config"]["wavetable_config"]))
    dev, stream = eng.device, torch.cuda.current_stream(eng.device)
    rng = np.random.default_rng(0)
    result = {"variant": args.child, "device": torch.cuda.get_device_name(0)}

    def timed(fn, warmup, iters):
        out = []
        for it in range(warmup + iters):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record(stream)
            fn()
            ev1.record(stream)
            ev1.synchronize()
            if it >= warmup:
                out.append(ev0.elapsed_time(ev1))
        return out

    # the step: 16 items of 800 frames
    B, T = args.items, args.frames
    mel, noise = (torch.as_tensor(xx).to(dev) for xx in synthetic_batch(rng, B, T, dims.steps_per_frame))
    extra = {"formant": torch.as_tensor(factor_rows(rng, B, T)).to(dev)} if shifted else {}
    audio = torch.empty((B, T * dims.hop_size), dtype=torch.float32, device=dev)
    result["step_ms"] = timed(lambda: eng.forward(mel, noise=noise, out=audio, **extra), args.warmup, args.iters)
    result["step_checksum"] = float(audio.double().abs().sum().item())
    if shifted:
        result["kernel_alone_ms"] = timed(lambda: eng.warp_envelope(mel, extra["formant"]), args.warmup, args.iters)
    # the tick: 64 streams through the 80 ms schedule, steady ticks replayed as graphs
    syn = StreamingSynthesizer(eng, chunk_frames=SCHEDULE)
    syn.time_device = True
    lead = 6 * len(SCHEDULE)
    n_ticks = lead + args.tick_warmup + args.ticks
    total = sum(SCHEDULE[ii % len(SCHEDULE)] for ii in range(n_ticks + 1)) + syn.right + 8
    for sid in range(args.streams):
        mm, nn = synthetic_batch(np.random.default_rng(1000 + sid), 1, total, dims.steps_per_frame)
        more = {"formant": factor_rows(np.random.default_rng(2000 + sid), 1, total)[0]} if shifted else {}
        syn.open(sid)
        syn.push(sid, mm[0], nn[0], **more)
    ticks = []
    for tick in range(n_ticks):
        torch.cuda.synchronize()
        res = syn.tick()
        torch.cuda.synchronize()
        assert len(res) == args.streams
        if tick >= lead + args.tick_warmup:
            ticks.append(syn.last_tick_device_ms)
    result["tick_ms"] = ticks
    result["ticks_replayed_as_graph"] = int(syn.graph_ticks)
    result["tick_checksum"] = float(sum(float(np.abs(res[sid]).sum()) for sid in sorted(res)))
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-tree", default=None, help="a built tree of the parent commit (none: the parent is not measured)")
    ap.add_argument("--rounds", type=int, default=3, help="times the variants alternate")
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=10, help="untimed steps of a child")
    ap.add_argument("--iters", type=int, default=40, help="timed steps of a child")
    ap.add_argument("--tick-warmup", dest="tick_warmup", type=int, default=10)
    ap.add_argument("--ticks", type=int, default=100, help="timed ticks of a child")
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    ap.add_argument("--child", default=None, choices=["parent", "plain", "formant"], help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    variants = ([("parent", os.path.abspath(args.parent_tree))] if args.parent_tree else []) + [("plain", HERE), ("formant", HERE)]
    sizes = ["--items", args.items, "--frames", args.frames, "--streams", args.streams, "--warmup", args.warmup, "--iters",
             args.iters, "--tick-warmup", args.tick_warmup, "--ticks", args.ticks]
    runs = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, root in variants:                       # alternating: every variant sees the same state of the machine
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--root", root,
                                  *[str(ss) for ss in sizes]], capture_output=True, text=True, timeout=900)
            if res.returncode != 0:
                raise SystemExit(f"formant_shift_probe.py: the {name} child failed:\n{res.stderr[-3000:]}")
            runs[name].append(json.loads(res.stdout.strip().splitlines()[-1]))
    result = {"device": runs["plain"][0]["device"], "step": f"{args.items} x {args.frames} frames", "tick":
              f"{args.streams} streams, schedule {list(SCHEDULE)}", "rounds": args.rounds, "variants": {}}
    for name, rr in runs.items():
        entry = {"ticks_replayed_as_graph": [one["ticks_replayed_as_graph"] for one in rr]}
        for key in ("step_ms", "tick_ms", "kernel_alone_ms"):
            if key in rr[0]:
                entry[key] = percentiles([vv for one in rr for vv in one[key]])
                entry[key]["p50_of_each_round"] = [float(np.percentile(one[key], 50)) for one in rr]
        entry["step_checksum"], entry["tick_checksum"] = rr[0]["step_checksum"], rr[0]["tick_checksum"]
        assert all(one["step_checksum"] == rr[0]["step_checksum"] and one["tick_checksum"] == rr[0]["tick_checksum"] for one in rr)
        result["variants"][name] = entry
    if "parent" in runs:                                     # no factor: the parent's bits
        for key in ("step_checksum", "tick_checksum"):
            assert result["variants"]["plain"][key] == result["variants"]["parent"][key], key
        result["plain_has_the_parents_checksums"] = True
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

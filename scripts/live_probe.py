#!/usr/bin/env python3
"""What the live path costs per tick: 64 streams of the canonical SPEECH model at the 80 ms schedule.

Two legs in one process, each after a time-based warm-up:

  synthesis  a StreamingSynthesizer alone, its mel frames resident on the host (bench.py's config 5): host-inclusive time of a
             steady tick and the device time of its launches
  live       a LiveResynthesizer fed 80 ms of audio per stream and tick: device time of the two analysis launches
             (mbxl_ring_append + mbxl_mel_frames, HIP events around them), host-inclusive time of the whole live tick
             (analysis tick, scale_mel, hand-over, synthesis tick), and the time of the 64 push_audio calls in front of it

With ``--input-rate R`` a third leg follows in the same process: the live leg again with every stream opened at R Hz (80 ms of
audio at R per push), so that the device time of the analysis launches -- now mbxl_ring_append into the input store,
mbxr_resample_rings, mbxl_mel_frames -- and the host-inclusive live tick stand next to the figures without resampling.

With ``--output-rate R`` a further leg follows: the live leg with every stream opened with ``output_rate=R`` (at the input rate
of ``--input-rate``, when given), so that the device time of the output stage's launches -- mbxl_ring_append from the
synthesizer's buffer, mbxo_resample_emit -- and the host-inclusive live tick stand next to the tick without an output rate.

With ``--limiter`` a last leg follows: that leg again (with the output rate, when given) with every stream opened with
``peak_limit=-1.0``, so that the device time of the limiter's launches -- mbxl_ring_append from the buffer of the stage in
front of it, mbxd_limit_emit -- and the host-inclusive live tick stand next to the tick without a limiter.

Prints one JSON line.  ``--synthesis-only`` runs the first leg alone; with ``--root DIR`` the package is imported from another
checkout (the parent commit, for the comparison of the synthesis tick), which needs nothing of the live path.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

SCHEDULE = (6, 6, 7, 6, 7)


def percentiles(values):
    return {"p50": float(np.percentile(values, 50)), "p10": float(np.percentile(values, 10)),
            "p90": float(np.percentile(values, 90)), "p99": float(np.percentile(values, 99)), "n": len(values)}


def synthetic_mel(rng, frames, channels, spf):
    mell = np.log(np.exp(rng.normal(-5.0, 2.0, size=(frames, channels))) + 1e-5)
    return np.clip(mell, -11.5, 2.0).astype(np.float32), rng.normal(size=frames * spf).astype(np.float32)


def synthesis_leg(torch, inv, streams, warm_seconds, ticks):
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    dims = inv.model.dims
    syn = StreamingSynthesizer(inv.model, chunk_frames=SCHEDULE)
    syn.time_device = True
    lead = 6 * len(SCHEDULE)
    # the frames arrive in blocks of 100 ticks' worth, pushed outside the timed section (the same block again and again: what
    # the frames hold does not change what a tick costs)
    block_ticks = 100
    block_frames = block_ticks * sum(SCHEDULE) // len(SCHEDULE) + sum(SCHEDULE)
    blocks = [synthetic_mel(np.random.default_rng(sid), block_frames, dims.mel_channels, dims.steps_per_frame)
              for sid in range(streams)]
    for sid in range(streams):
        syn.open(sid)

    def feed():
        for sid in range(streams):
            syn.push(sid, *blocks[sid])

    feed()
    feed()
    host_ms, dev_ms, done, warm_ticks = [], [], 0, 0
    t_start = time.perf_counter()
    while len(host_ms) < ticks:
        if done % block_ticks == 0:
            feed()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = syn.tick()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        assert len(res) == streams
        done += 1
        if done > lead and t1 - t_start >= warm_seconds and syn.last_tick_replayed:
            host_ms.append((t1 - t0) * 1e3)
            dev_ms.append(syn.last_tick_device_ms)
        else:
            warm_ticks += 1
            assert warm_ticks < 50000, "the ticks never became steady"
    return {"tick_ms_host_inclusive": percentiles(host_ms), "tick_ms_device": percentiles(dev_ms), "warmup_ticks": warm_ticks,
            "graph_ticks": int(syn.graph_ticks)}


def live_leg(torch, inv, streams, warm_seconds, ticks, input_rate=None, output_rate=None, limiter=False):
    from mbexwn_vocoder_amd.live import LiveResynthesizer
    live = LiveResynthesizer(inv, chunk_frames=SCHEDULE)
    live.analyzer.time_device = True
    live.synthesizer.time_device = True
    if output_rate:
        live.output.time_device = True
    if limiter:
        live.limiter.time_device = True
    rate = int(input_rate or inv.srate)
    per_tick = int(round(0.080 * rate))
    rng = np.random.default_rng(99)
    tt = np.arange(50 * per_tick) / rate
    sounds = [(0.3 * np.sin(2 * np.pi * (90.0 + 3 * sid) * tt) + 0.05 * rng.normal(size=tt.size)).astype(np.float32)
              for sid in range(streams)]
    rates = {"sample_rate": input_rate} if input_rate else {}
    if output_rate:
        rates["output_rate"] = output_rate
    if limiter:
        rates["peak_limit"] = -1.0
    for sid in range(streams):
        live.open(sid, seed=sid, **rates)
    allocations = out_allocations = lim_allocations = None
    tick_ms, push_ms, analysis_ms, syn_dev_ms, output_ms, limiter_ms, replayed, pos, warm_ticks = [], [], [], [], [], [], 0, 0, 0
    t_start = time.perf_counter()
    while len(tick_ms) < ticks:
        t0 = time.perf_counter()
        for sid in range(streams):                                   # the sounds repeat: the streams never end
            live.push_audio(sid, sounds[sid][pos:pos + per_tick])
        pos = (pos + per_tick) % sounds[0].size
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        res = live.tick()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        steady = len(res) == streams and live.synthesizer.last_tick_replayed
        if steady and t2 - t_start >= warm_seconds:
            if allocations is None:
                allocations = live.analyzer.device_allocations
                out_allocations = live.output.device_allocations if output_rate else 0
                lim_allocations = live.limiter.device_allocations if limiter else 0
            if output_rate:
                output_ms.append(live.output.last_tick_device_ms)
            if limiter:
                limiter_ms.append(live.limiter.last_tick_device_ms)
            tick_ms.append((t2 - t1) * 1e3)
            push_ms.append((t1 - t0) * 1e3)
            analysis_ms.append(live.analyzer.last_tick_device_ms)
            syn_dev_ms.append(live.synthesizer.last_tick_device_ms)
            replayed += 1
        else:
            warm_ticks += 1
            assert warm_ticks < 20000, "the live ticks never became steady"
    return {"live_tick_ms_host_inclusive": percentiles(tick_ms), "push_audio_ms_all_streams": percentiles(push_ms),
            "analysis_launches_ms_device": percentiles(analysis_ms), "synthesis_ms_device_inside": percentiles(syn_dev_ms),
            "warmup_ticks": warm_ticks,
            "lookahead_ms": live.lookahead_ms_for(input_rate) if input_rate else live.lookahead_ms,
            "analyzer_device_allocations_during_timed_ticks": live.analyzer.device_allocations - allocations,
            "ring_samples": live.analyzer.ring_samples,
            **({"input_rate": input_rate, "input_ring_samples": live.analyzer.input_ring_samples} if input_rate else {}),
            **({"output_rate": output_rate, "output_stage_launches_ms_device": percentiles(output_ms),
                "output_lookahead_ms": live.lookahead_ms_for(input_rate or None, output_rate) - live.lookahead_ms_for(input_rate or None),
                "output_device_allocations_during_timed_ticks": live.output.device_allocations - out_allocations,
                "output_ring_samples": live.output.ring_samples, "samples_per_stream_and_tick": int(next(iter(res.values())).size)}
               if output_rate else {}),
            **({"peak_limit": -1.0, "limiter_launches_ms_device": percentiles(limiter_ms),
                "limiter_device_allocations_during_timed_ticks": live.limiter.device_allocations - lim_allocations,
                "limiter_ring_samples": live.limiter.ring_samples} if limiter else {})}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--warm-seconds", type=float, default=3.0, help="each leg warms up at least this long before it is timed")
    ap.add_argument("--ticks", type=int, default=300, help="timed steady ticks per leg")
    ap.add_argument("--synthesis-only", action="store_true")
    ap.add_argument("--input-rate", type=int, default=0, metavar="R",
                    help="also run the live leg with every stream opened at R Hz (resampled on the device)")
    ap.add_argument("--output-rate", type=int, default=0, metavar="R",
                    help="also run the live leg with every stream opened with output_rate=R (resampled on the device on the way "
                         "out)")
    ap.add_argument("--limiter", action="store_true",
                    help="also run the live leg (with the output rate, when given) with every stream opened with peak_limit=-1.0")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to import mbexwn_vocoder_amd from (default: this one)")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("live_probe.py: no GPU available; a timing taken without one says nothing")
    from mbexwn_vocoder_amd.mel_inverter import MELInverter, create_synthetic_model_dir
    with tempfile.TemporaryDirectory() as tmp:
        inv = MELInverter(create_synthetic_model_dir(os.path.join(tmp, "speech"), "SPEECH"))
    out = {"label": args.label, "root": os.path.abspath(args.root), "streams": args.streams, "schedule": list(SCHEDULE),
           "device": torch.cuda.get_device_name(0)}
    out["synthesis"] = synthesis_leg(torch, inv, args.streams, args.warm_seconds, args.ticks)
    if not args.synthesis_only:
        out["live"] = live_leg(torch, inv, args.streams, args.warm_seconds, args.ticks)
        if args.input_rate and args.input_rate != int(inv.srate):
            out["live_resampled"] = live_leg(torch, inv, args.streams, args.warm_seconds, args.ticks, args.input_rate)
        if args.output_rate and args.output_rate != int(inv.srate):
            out["live_output"] = live_leg(torch, inv, args.streams, args.warm_seconds, args.ticks, args.input_rate or None,
                                          args.output_rate)
        if args.limiter:
            out_rate = args.output_rate if args.output_rate != int(inv.srate) else 0
            out["live_limited"] = live_leg(torch, inv, args.streams, args.warm_seconds, args.ticks, args.input_rate or None,
                                           out_rate or None, limiter=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
